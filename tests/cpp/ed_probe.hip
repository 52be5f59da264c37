// ed_probe — runs a tape of cases through the device routines of zkemail.rs_amd/csrc/ed25519.hip.h, one routine per case,
// and writes every result back.  Test infrastructure: compiled from the product header with the engine's flags, not part of
// the library.  tests/ed_field_cases.py writes the tape and holds the expectations; tests/test_gpu_ed_field.py runs this once.
//
//   ed_probe <tape-in> <results-out>        exit status: 0 done, 1 bad tape / file error, 2 HIP error
//
// Tape (little-endian 32-bit words):
//   header, 16 words:  [0] 0x42504445 "EDPB"   [1] n records   [2] IN_WORDS (80)   [3] OUT_WORDS (40)
//                      [4 + 2f], [5 + 2f]  first record and record count of family f = 0..3   [12..15] zero
//   n records of IN_WORDS words:   [0] op   [1] aux   [2..79] operands, packed in the order given below
//                      (a field element is 8 words, least significant first; a point is X, Y, Z, T; bytes are packed
//                       little-endian into words, so the record read as bytes is the byte string itself)
//   Records of one family are contiguous; every family is ONE launch over its slice.
// Results:
//   header, 4 words:   [0] 0x52504445 "EDPR"   [1] n   [2] OUT_WORDS   [3] zero
//   n records of OUT_WORDS words:  [0] flag (a bool result, else 0)   [1..39] result words, zero where unused
//
//   family 0, field, one case per lane
//      1 fe_add a b -> fe      2 fe_sub a b -> fe      3 fe_mul a b -> fe (the call)     4 fe_sq a -> fe (the call)
//      5 fe_mul_i a b -> fe    6 fe_sq_i a -> fe       7 fe_canon a -> fe                8 fe_is_zero a -> flag
//      9 fe_eq a b -> flag    10 fe_is_neg a -> flag  11 fe_neg a -> fe                 12 fe_invert a -> fe
//     13 fe_pow22523 a -> fe  14 fe_from_bytes 32 bytes -> fe
//   family 1, scalars and hash, one case per lane
//     20 sc_lt_L s[8] -> flag          21 sc_reduce512 h[16] -> 8 words
//     22 sha512_ram R[32 B] A[32 B] M[32 B], aux = mlen -> 16 words
//   family 2, points, one case per lane
//     30 ge_decompress 32 bytes -> flag, X Y Z T     31 ge_compress P -> 8 words     32 ge_is_small_order P -> flag
//     33 ge_add P Q -> point         34 ge_dbl P -> point         35 ge_add_cached P Q t2d -> point
//   family 3, quad formulas: 16 cases per 64-lane block, lane (threadIdx.x & 3) holds coordinate X, Y, Z or T and
//   writes its own eight result words, as in ed25519_verify_quad
//     40 q_table P -> the four level-1 factors    41 q_dbl P -> point    42 q_add P Q -> point, against q_table(Q)
#include <cstdint>
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>

#include "ed25519.hip.h"

namespace {

constexpr uint32_t IN_WORDS = 80, OUT_WORDS = 40, TAPE_MAGIC = 0x42504445u, RES_MAGIC = 0x52504445u, HEADER_WORDS = 16;
constexpr uint32_t MAX_RECORDS = 1u << 20;

using zke::Fe;
using zke::Ge;

__device__ __forceinline__ Fe ld_fe(const uint32_t* p) {
  Fe r;
#pragma unroll
  for (int j = 0; j < 8; j++) r.v[j] = p[j];
  return r;
}
__device__ __forceinline__ void st_fe(uint32_t* p, const Fe& a) {
#pragma unroll
  for (int j = 0; j < 8; j++) p[j] = a.v[j];
}
__device__ __forceinline__ Ge ld_ge(const uint32_t* p) { return Ge{ld_fe(p), ld_fe(p + 8), ld_fe(p + 16), ld_fe(p + 24)}; }
__device__ __forceinline__ void st_ge(uint32_t* p, const Ge& a) { st_fe(p, a.X); st_fe(p + 8, a.Y); st_fe(p + 16, a.Z); st_fe(p + 24, a.T); }

__global__ __launch_bounds__(64) void probe_field(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* a = in + (size_t)i * IN_WORDS + 2;
  uint32_t* o = out + (size_t)i * OUT_WORDS;
  const Fe x = ld_fe(a), y = ld_fe(a + 8);
  switch (a[-2]) {
    case 1: st_fe(o + 1, zke::fe_add(x, y)); break;
    case 2: st_fe(o + 1, zke::fe_sub(x, y)); break;
    case 3: st_fe(o + 1, zke::fe_mul(x, y)); break;
    case 4: st_fe(o + 1, zke::fe_sq(x)); break;
    case 5: st_fe(o + 1, zke::fe_mul_i(x, y)); break;
    case 6: st_fe(o + 1, zke::fe_sq_i(x)); break;
    case 7: st_fe(o + 1, zke::fe_canon(x)); break;
    case 8: o[0] = zke::fe_is_zero(x); break;
    case 9: o[0] = zke::fe_eq(x, y); break;
    case 10: o[0] = zke::fe_is_neg(x); break;
    case 11: st_fe(o + 1, zke::fe_neg(x)); break;
    case 12: st_fe(o + 1, zke::fe_invert(x)); break;
    case 13: st_fe(o + 1, zke::fe_pow22523(x)); break;
    case 14: st_fe(o + 1, zke::fe_from_bytes((const uint8_t*)a)); break;
    default: break;
  }
}

__global__ __launch_bounds__(64) void probe_scalar(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* a = in + (size_t)i * IN_WORDS + 2;
  uint32_t* o = out + (size_t)i * OUT_WORDS;
  switch (a[-2]) {
    case 20: {
      uint32_t s[8];
      for (int j = 0; j < 8; j++) s[j] = a[j];
      o[0] = zke::sc_lt_L(s);
      break;
    }
    case 21: {
      uint32_t h[16], r[8];
      for (int j = 0; j < 16; j++) h[j] = a[j];
      zke::sc_reduce512(r, h);
      for (int j = 0; j < 8; j++) o[1 + j] = r[j];
      break;
    }
    case 22: {
      uint32_t mlen = a[-1], h[16];
      if (mlen > 32) mlen = 32;                   // the operand field holds 32 message bytes
      const uint8_t* b = (const uint8_t*)a;
      zke::sha512_ram(h, b, b + 32, b + 64, mlen);
      for (int j = 0; j < 16; j++) o[1 + j] = h[j];
      break;
    }
    default: break;
  }
}

__global__ __launch_bounds__(64) void probe_point(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* a = in + (size_t)i * IN_WORDS + 2;
  uint32_t* o = out + (size_t)i * OUT_WORDS;
  switch (a[-2]) {
    case 30: {
      Ge p;
      o[0] = zke::ge_decompress(p, (const uint8_t*)a);
      st_ge(o + 1, p);
      break;
    }
    case 31: {
      uint32_t e[8];
      zke::ge_compress(e, ld_ge(a));
      for (int j = 0; j < 8; j++) o[1 + j] = e[j];
      break;
    }
    case 32: o[0] = zke::ge_is_small_order(ld_ge(a)); break;
    case 33: st_ge(o + 1, zke::ge_add(ld_ge(a), ld_ge(a + 32))); break;
    case 34: st_ge(o + 1, zke::ge_dbl(ld_ge(a))); break;
    case 35: st_ge(o + 1, zke::ge_add_cached(ld_ge(a), ld_ge(a + 32), ld_fe(a + 64))); break;
    default: break;
  }
}

// the op is the same in the four lanes of a quad (they read the same record), so the quad moves stay inside one branch
__global__ __launch_bounds__(64) void probe_quad(const uint32_t* in, uint32_t* out, uint32_t n) {
  uint32_t i = blockIdx.x * 16 + (threadIdx.x >> 2);
  const bool live = i < n;
  if (!live) i = n - 1;                           // whole quads stay in step; the result is dropped (n >= 1: see main)
  const uint32_t q = threadIdx.x & 3u;
  const uint32_t* a = in + (size_t)i * IN_WORDS + 2;
  uint32_t* o = out + (size_t)i * OUT_WORDS + 1 + 8 * q;
  Fe r = zke::fe_small(0);
  switch (a[-2]) {
    case 40: r = zke::q_table(ld_ge(a), q); break;
    case 41: r = zke::q_dbl(ld_fe(a + 8 * q), q); break;
    case 42: r = zke::q_add(ld_fe(a + 8 * q), zke::q_table(ld_ge(a + 32), q), q); break;
    default: break;
  }
  if (live) st_fe(o, r);
}

bool hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  fprintf(stderr, "ed_probe: %s: %s\n", what, hipGetErrorString(e));
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ed_probe <tape-in> <results-out>\n"); return 1; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "ed_probe: cannot read %s\n", argv[1]); return 1; }
  uint32_t hd[HEADER_WORDS];
  if (fread(hd, 4, HEADER_WORDS, f) != HEADER_WORDS || hd[0] != TAPE_MAGIC || hd[2] != IN_WORDS || hd[3] != OUT_WORDS ||
      hd[1] == 0 || hd[1] > MAX_RECORDS) {
    fprintf(stderr, "ed_probe: bad tape header\n"); fclose(f); return 1;
  }
  const uint32_t n = hd[1];
  for (int k = 0; k < 4; k++)                     // every family's slice lies inside the tape
    if (hd[4 + 2 * k] > n || hd[5 + 2 * k] > n - hd[4 + 2 * k]) { fprintf(stderr, "ed_probe: family %d out of range\n", k); fclose(f); return 1; }
  std::vector<uint32_t> tape((size_t)n * IN_WORDS), res((size_t)n * OUT_WORDS);
  const bool whole = fread(tape.data(), 4, tape.size(), f) == tape.size();
  fclose(f);
  if (!whole) { fprintf(stderr, "ed_probe: short tape\n"); return 1; }

  uint32_t *din = nullptr, *dout = nullptr;
  if (!hip_ok(hipMalloc(&din, tape.size() * 4), "hipMalloc") || !hip_ok(hipMalloc(&dout, res.size() * 4), "hipMalloc")) return 2;
  if (!hip_ok(hipMemset(dout, 0, res.size() * 4), "hipMemset")) return 2;
  if (!hip_ok(hipMemcpy(din, tape.data(), tape.size() * 4, hipMemcpyHostToDevice), "upload")) return 2;
  using Kernel = void (*)(const uint32_t*, uint32_t*, uint32_t);
  const Kernel kernels[4] = {probe_field, probe_scalar, probe_point, probe_quad};
  const uint32_t per_block[4] = {64, 64, 64, 16};
  for (int k = 0; k < 4; k++) {
    const uint32_t first = hd[4 + 2 * k], cnt = hd[5 + 2 * k];
    if (!cnt) continue;
    hipLaunchKernelGGL(kernels[k], dim3((cnt + per_block[k] - 1) / per_block[k]), dim3(64), 0, 0,
                       din + (size_t)first * IN_WORDS, dout + (size_t)first * OUT_WORDS, cnt);
    if (!hip_ok(hipGetLastError(), "launch")) return 2;
  }
  if (!hip_ok(hipDeviceSynchronize(), "run")) return 2;
  if (!hip_ok(hipMemcpy(res.data(), dout, res.size() * 4, hipMemcpyDeviceToHost), "copy back")) return 2;
  hipFree(din); hipFree(dout);

  FILE* g = fopen(argv[2], "wb");
  const uint32_t rh[4] = {RES_MAGIC, n, OUT_WORDS, 0};
  if (!g || fwrite(rh, 4, 4, g) != 4 || fwrite(res.data(), 4, res.size(), g) != res.size() || fclose(g) != 0) {
    fprintf(stderr, "ed_probe: cannot write %s\n", argv[2]); return 1;
  }
  return 0;
}
