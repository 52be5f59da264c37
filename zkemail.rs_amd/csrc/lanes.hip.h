// lanes.hip.h — the two whole-wave DPP shifts, the one cross-lane move the RSA wave routine (rsa.hip.h: the low words of
// a Montgomery step) and the e-mail front end (bytes.hip.h, mime.hip.h, canon.hip.h: the neighbouring byte) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zke {

// value of lane+1 (lane 63 gets 0): v_mov_b32_dpp wave_shl:1 bound_ctrl:0
__device__ __forceinline__ uint32_t lane_up(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x130 /*wave_shl:1*/, 0xf, 0xf, false);
}
// value of lane-1 (lane 0 gets 0): wave_shr:1
__device__ __forceinline__ uint32_t lane_down(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
}

}  // namespace zke
