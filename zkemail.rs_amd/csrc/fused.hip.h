// fused.hip.h — the hash / modexp stage of a batch as ONE launch.
//
// A batch's SHA-256 launch is a few long dependency chains (a 4 KB body = 65 dependent compressions: 137 us whatever
// the batch size) that leave most of the chip idle, and the RSA modular exponentiation of the same e-mails does not
// depend on any hash — only the final EMSA compare does (call site core/src/email.rs:31-33: cfdkim computes bh, the
// header hash and the signature check one after the other; nothing orders the arithmetic inside).  One stream runs
// its kernels in order, so the two can only overlap inside one launch: workgroups [0, g_sha) are SHA-256 groups
// (two waves each: sha256_pair_group, sha256_ring_group or sha256_twin_group, one kernel per routine below; stage_plan.hip.h
// says which a batch takes and how many workgroups each role gets), the rest are RSA roles — one signature per wave for keys whose
// Montgomery constants are not cached yet (it fills the cache) or that the lane-group kernels do not take, four / eight
// lanes per signature (rsa_group_wave<4>, <8> and <8, 9>) for everything the front end routed there.  RSA leaves EM's shape verdict and its
// digest bytes in EmailMeta; verdict_kernel joins them with the hashes.  The batch's chain becomes
// front end -> max(SHA-256, RSA) -> verdict instead of front end -> SHA-256 -> RSA.
#pragma once
#include "rsa_quad.hip.h"
#include "stage_plan.hip.h"      // the layout of the SHA-256 groups (sha_stage_kind) and the plan the host fills StageArgs from

namespace zke {

struct StageArgs {
  const ShaJob* sha; uint32_t n_sha;       // 4 * n_pad messages, kind-major
  const RsaJob* rsa; uint32_t n;           // one job per e-mail
  EmailMeta* meta;
  KeyCacheEntry* cache;
  uint8_t* em_out;                         // parity intermediates (nullptr in production)
  const uint32_t* wave_count;              // the front end's list of jobs for the one-signature-per-wave routine (the keys
  const uint32_t* wave_list;               // not cached yet, other exponents ...); nullptr: no list, job = 2 b + wave
  uint32_t g_sha, g_wave, g_quad, g_oct;   // workgroups per role, in this order; blockDim = 128 (two waves)
  uint32_t g_oct9;                         // ... then the eight-lane role for moduli <= 2048 bits (a launch has it or g_quad, never both)
  const uint32_t* order; uint32_t n_pad;   // length buckets of the body / header-preimage hashes (BatchDev::order), or nullptr
  uint32_t twin_kinds;                     // bit k: kind k is hashed by sha256_twin_group in groups of 32 (launches with `order` only)
  uint32_t debug_skip_rsa;
};

template <int G, int L> constexpr uint32_t group_lds_dwords() { return (64 / G) * (G * L + 4); }      // per wave: rsa_group_wave's Llimb
constexpr uint32_t QUAD_LDS_DWORDS = group_lds_dwords<4, QL>(), OCT_LDS_DWORDS = group_lds_dwords<8, QL>(), OCT9_LDS_DWORDS = group_lds_dwords<8, QL9>();

// Waves per SIMD of the hash / modexp launch.  The kernel needs 153 registers (the SHA-256 pair routine's), which would let
// three waves share a SIMD; ZKE_STAGE_WAVES is both the least the compiler must allow AND the most the hardware may place
// (amdgpu_waves_per_eu(min, max): the register count is raised to what max waves leave each other), so that the occupancy
// is chosen here and not by whatever the register allocation happens to come to.  2 or 3; the A/B is profiles/limb29_bench_ab.txt.
#ifndef ZKE_STAGE_WAVES
#define ZKE_STAGE_WAVES 2
#endif
// RING: the SHA-256 groups run sha256_ring_group (two K+W buffers: the launch then carries sha256_ring_lds_bytes of LDS, and the
// RSA roles, whose workgroups are two waves as well, borrow the front of it as before).  TWIN (with RING): the kinds of
// A.twin_kinds run sha256_twin_group — the ring's LDS, 32 messages per group —, the other kinds the ring.
template <int T, bool RING, bool TWIN = false>
__device__ __forceinline__ void hash_modexp_body(const StageArgs& A, uint8_t* lds_raw) {
  static_assert(sha256_pair_lds_bytes<T>() >= 2 * 4 * QUAD_LDS_DWORDS && sha256_pair_lds_bytes<T>() >= 2 * 4 * OCT_LDS_DWORDS &&
                sha256_pair_lds_bytes<T>() >= 2 * 4 * OCT9_LDS_DWORDS,
                "the RSA roles borrow the launch's LDS");
  uint32_t b = blockIdx.x;
  if (b < A.g_sha) {
    if (!A.order) {
      if (RING) sha256_ring_group<T>(A.sha, A.n_sha, b, lds_raw); else sha256_pair_group<T>(A.sha, A.n_sha, b, lds_raw);
      return;
    }
    // kind-major job list: groups [k gpk, (k + 1) gpk) hash kind k; bodies and header preimages by length class
    const uint32_t twin_kinds = TWIN ? A.twin_kinds : 0u;
    uint32_t gk = b;
    const uint32_t kind = sha_stage_kind(A.n_pad, twin_kinds, gk);
    const ShaOrder so{kind < 2 ? A.order + sha_order_cnt(kind) : nullptr, kind < 2 ? A.order + sha_order_key(kind, A.n_pad) : nullptr, A.n};
    if (TWIN && (twin_kinds >> kind & 1u)) sha256_twin_group<T>(A.sha + (size_t)kind * A.n_pad, A.n_pad, gk, lds_raw, &so);
    else if (RING) sha256_ring_group<T>(A.sha + (size_t)kind * A.n_pad, A.n_pad, gk, lds_raw, &so);
    else sha256_pair_group<T>(A.sha + (size_t)kind * A.n_pad, A.n_pad, gk, lds_raw, &so);
    return;
  }
  b -= A.g_sha;
  const uint32_t wave = threadIdx.x >> 6;
  if (b < A.g_wave) {
    if (A.wave_list) {
      // Once a batch's keys are cached this list is empty and the role's workgroups leave at once — that is why they are
      // few and loop (a workgroup that only looks and leaves still has to be given LDS and registers on a full chip first).
      const uint32_t cnt = *A.wave_count;
      for (uint32_t t = 2 * b + wave; t < cnt; t += 2 * A.g_wave)
        rsa_wave_any(A.rsa, A.wave_list[t], nullptr, 0, nullptr, A.em_out, A.cache, A.meta, A.debug_skip_rsa);
    } else {
      const uint32_t job = 2 * b + wave;
      if (job < A.n) rsa_wave_any(A.rsa, job, nullptr, 0, nullptr, A.em_out, A.cache, A.meta, A.debug_skip_rsa);
    }
    return;
  }
  b -= A.g_wave;
  uint32_t* lds = reinterpret_cast<uint32_t*>(lds_raw);
  if (b < A.g_quad) {
    if (!A.debug_skip_rsa) rsa_group_wave<4>(A.rsa, A.n, (2 * b + wave) * 16, lds + wave * QUAD_LDS_DWORDS, nullptr, 0, nullptr, A.em_out, A.cache, A.meta);
    return;
  }
  b -= A.g_quad;
  if (b < A.g_oct) {
    if (!A.debug_skip_rsa) rsa_group_wave<8>(A.rsa, A.n, (2 * b + wave) * 8, lds + wave * OCT_LDS_DWORDS, nullptr, 0, nullptr, A.em_out, A.cache, A.meta);
    return;
  }
  b -= A.g_oct;
  if (!A.debug_skip_rsa) rsa_group_wave<8, QL9>(A.rsa, A.n, (2 * b + wave) * 8, lds + wave * OCT9_LDS_DWORDS, nullptr, 0, nullptr, A.em_out, A.cache, A.meta);
}

template <int T>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(ZKE_STAGE_WAVES, ZKE_STAGE_WAVES))) void hash_modexp_kernel(StageArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  hash_modexp_body<T, false>(A, lds_raw);
}
template <int T>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(ZKE_STAGE_WAVES, ZKE_STAGE_WAVES))) void hash_modexp_ring_kernel(StageArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  hash_modexp_body<T, true>(A, lds_raw);
}
template <int T>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(ZKE_STAGE_WAVES, ZKE_STAGE_WAVES))) void hash_modexp_twin_kernel(StageArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  hash_modexp_body<T, true, true>(A, lds_raw);
}

}  // namespace zke
