// utf8_lossy.hip.h — String::from_utf8_lossy (helpers/src/regex.rs:35; the rule is core::str::Utf8Chunks'): a byte string as the
// UTF-8 text the reference turns a capture into.  Every maximal prefix of a well-formed sequence (Unicode Table 3-7) that is not
// itself well-formed becomes one U+FFFD (EF BF BD); so does every byte no sequence covers — a stray continuation byte, C0, C1,
// F5..FF — and a sequence the end of the string cuts short.  Well-formed bytes are copied.  Python's bytes.decode("utf-8",
// "replace").encode() writes the same bytes (tests/test_utf8_lossy_sanitizers.py, tests/test_gpu_utf8_lossy.py).
//
// Two forms of the two routines (the repaired length; the repaired bytes):
//   * utf8_lossy_len / utf8_lossy_write: plain C++, one byte after the other, no HIP call — the CPU tier
//     (tests/cpp/utf8_lossy_fuzz.cpp defines ZKE_UTF8_LOSSY_SCALAR_ONLY and sees nothing else of this file) and host callers.
//   * u8l_wave<WRITE>: one string by one wavefront, a lane per byte, 64 bytes a step.  A lead byte is never a continuation byte and
//     a sequence covers continuation bytes only, so every lead starts a chunk of the serial walk whatever lies in front of it, and
//     what becomes of byte j is decided by the bytes j - 3 .. j + 3 alone:
//       ASCII                        copied (width 1)
//       lead C2..F4                  cover = the bytes of the maximal well-formed prefix it starts (u8l_cover); the whole sequence:
//                                    copied (1), else the lane writes the chunk's U+FFFD (3)
//       continuation 80..BF          the nearest non-continuation byte at most three in front, if it is a lead whose cover reaches
//                                    j, owns it: copied (1) when that sequence is whole, dropped into the lead's U+FFFD (0) when
//                                    not; with no such lead: U+FFFD (3)
//       C0, C1, F5..FF               U+FFFD (3)
//     Widths are 0, 1 or 3, so the wave's exclusive scan is two ballots and two popcounts (ones + 3 * threes), no shuffle; the
//     running offset is a scalar.  The neighbours are plain byte loads (the lane's own and at most six beside it, all in cache lines
//     the step loads anyway); `n` bounds every one of them, so nothing outside src[0, n) is read — not the next string's first byte
//     either — and a sequence that straddles two steps is seen whole by the lanes on both sides.
// The kernels of zke_utf8_lossy_batch follow: lengths and flags, one block's scan, the bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(ZKE_UTF8_LOSSY_SCALAR_ONLY)
#include <hip/hip_runtime.h>
#define ZKE_U8L_HD __host__ __device__
#else
#define ZKE_U8L_HD
#endif

namespace zke {

constexpr uint32_t U8L_END = 0x100;      // "no byte here": beyond the end (or in front of the start) of the string

// the length of the sequence lead byte c announces (2 .. 4); 0: c is no lead byte
ZKE_U8L_HD inline uint32_t u8l_need(uint32_t c) {
  return c >= 0xC2 && c <= 0xDF ? 2u : c >= 0xE0 && c <= 0xEF ? 3u : c >= 0xF0 && c <= 0xF4 ? 4u : 0u;
}
ZKE_U8L_HD inline bool u8l_cont(uint32_t b) { return (b & ~0x3Fu) == 0x80; }
// Table 3-7's second byte: 80..BF but E0 A0..BF, ED 80..9F, F0 90..BF, F4 80..8F
ZKE_U8L_HD inline bool u8l_second(uint32_t c, uint32_t b) {
  const uint32_t lo = c == 0xE0 ? 0xA0u : c == 0xF0 ? 0x90u : 0x80u, hi = c == 0xED ? 0x9Fu : c == 0xF4 ? 0x8Fu : 0xBFu;
  return b >= lo && b <= hi;
}
// Bytes of the maximal well-formed prefix that lead c (need = u8l_need(c) != 0) starts, b1 .. b3 the bytes behind it (U8L_END
// beyond the string): `need` when the sequence is whole, else the length of the chunk one U+FFFD stands for.
ZKE_U8L_HD inline uint32_t u8l_cover(uint32_t c, uint32_t need, uint32_t b1, uint32_t b2, uint32_t b3) {
  if (!u8l_second(c, b1)) return 1;
  if (need == 2 || !u8l_cont(b2)) return 2;
  if (need == 3 || !u8l_cont(b3)) return 3;
  return 4;
}

// The serial walk.  dst == nullptr: the length alone; else dst holds utf8_lossy_len(src, n) bytes.  Returns the repaired length.
inline size_t utf8_lossy_serial(const uint8_t* src, size_t n, uint8_t* dst) {
  size_t o = 0;
  for (size_t i = 0; i < n;) {
    const uint32_t c = src[i];
    const uint32_t need = u8l_need(c);
    uint32_t take = 1;
    bool whole = c < 0x80;
    if (need) {
      take = u8l_cover(c, need, i + 1 < n ? src[i + 1] : U8L_END, i + 2 < n ? src[i + 2] : U8L_END, i + 3 < n ? src[i + 3] : U8L_END);
      whole = take == need;
    }
    if (whole) {
      if (dst) for (uint32_t k = 0; k < take; k++) dst[o + k] = src[i + k];
      o += take;
    } else {
      if (dst) { dst[o] = 0xEF; dst[o + 1] = 0xBF; dst[o + 2] = 0xBD; }
      o += 3;
    }
    i += take;
  }
  return o;
}
inline size_t utf8_lossy_len(const uint8_t* src, size_t n) { return utf8_lossy_serial(src, n, nullptr); }
inline size_t utf8_lossy_write(const uint8_t* src, size_t n, uint8_t* dst) { return utf8_lossy_serial(src, n, dst); }

#if defined(__HIPCC__) && !defined(ZKE_UTF8_LOSSY_SCALAR_ONLY)

// What byte j of src[0, n) puts out: 1 (itself), 3 (a U+FFFD) or 0 (its lead's U+FFFD stands for it).  c: the byte (j < n).
__device__ __forceinline__ uint32_t u8l_width(const uint8_t* src, uint32_t n, uint32_t j, uint32_t c) {
  auto at = [&](uint32_t k) -> uint32_t { return k < n ? (uint32_t)src[k] : U8L_END; };      // (j - d wraps to "beyond the end": n < 2^32 - 3)
  if (c < 0x80) return 1;
  if (const uint32_t need = u8l_need(c)) return u8l_cover(c, need, at(j + 1), at(j + 2), at(j + 3)) == need ? 1u : 3u;
  if (!u8l_cont(c)) return 3;
#pragma unroll
  for (uint32_t d = 1; d <= 3; d++) {
    const uint32_t p = at(j - d);
    if (u8l_cont(p)) continue;
    const uint32_t need = u8l_need(p);
    if (need > d) {
      const uint32_t cov = u8l_cover(p, need, at(j - d + 1), at(j - d + 2), at(j - d + 3));
      if (cov > d) return cov == need ? 1u : 0u;
    }
    break;
  }
  return 3;
}

// src[0, n) repaired by one wavefront (wave-uniform arguments; lane = the lane's number): returns the repaired length, `changed`:
// some byte was replaced.  WRITE: the bytes go to dst[0, that length).
template <bool WRITE>
__device__ __forceinline__ uint32_t u8l_wave(const uint8_t* __restrict__ src, uint32_t n, uint8_t* __restrict__ dst, uint32_t lane, bool& changed) {
  uint32_t o = 0;
  changed = false;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t j = base + lane;
    uint32_t c = 0, w = 0;
    if (j < n) { c = src[j]; w = u8l_width(src, n, j, c); }
    const uint64_t m1 = __ballot(w == 1), m3 = __ballot(w == 3);
    if (WRITE) {
      uint8_t* to = dst + o + (uint32_t)__builtin_popcountll(m1 & below) + 3u * (uint32_t)__builtin_popcountll(m3 & below);
      if (w == 1) to[0] = (uint8_t)c;
      else if (w == 3) { to[0] = 0xEF; to[1] = 0xBF; to[2] = 0xBD; }
    }
    o += (uint32_t)__builtin_popcountll(m1) + 3u * (uint32_t)__builtin_popcountll(m3);
    changed = changed || m3 != 0;
  }
  return o;
}

// ---- zke_utf8_lossy_batch: string i = blob[off[i] - off[0] .. off[i + 1] - off[0]).  Three launches on one stream:
//   utf8_lossy_len_kernel     a wave per string (the host bounds the grid, each wave loops): out_off[i] = its repaired length, flags[i]
//   utf8_lossy_scan_kernel    ONE block: out_off becomes the exclusive scan, out_off[n] the total (the host keeps it below 2^32)
//   utf8_lossy_write_kernel   a wave per string: its bytes at out_off[i] — unless the string would end beyond `cap`
struct Utf8LossyArgs {
  uint32_t n;
  const uint8_t* blob; const uint64_t* off;
  uint32_t* out_off;          // [n + 1]
  uint8_t* out; uint64_t cap; // the repaired blob and its capacity
  uint8_t* flags;             // [n] bit 0: the string was changed
};

__global__ __launch_bounds__(64) void utf8_lossy_len_kernel(Utf8LossyArgs A) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t off0 = A.off[0];
  for (uint32_t i = blockIdx.x; i < A.n; i += gridDim.x) {
    bool changed;
    const uint32_t len = u8l_wave<false>(A.blob + (A.off[i] - off0), (uint32_t)(A.off[i + 1] - A.off[i]), nullptr, lane, changed);
    if (lane == 0) { A.out_off[i] = len; A.flags[i] = changed ? 1 : 0; }
  }
}

__global__ __launch_bounds__(1024) void utf8_lossy_scan_kernel(Utf8LossyArgs A) {
  __shared__ uint64_t sh[1025];
  const uint32_t T = blockDim.x, t = threadIdx.x;
  const size_t cnt = A.n, per = (cnt + T - 1) / T, lo = (size_t)t * per < cnt ? (size_t)t * per : cnt, hi = lo + per < cnt ? lo + per : cnt;
  uint64_t sum = 0;
  for (size_t k = lo; k < hi; k++) sum += A.out_off[k];
  sh[t] = sum;
  __syncthreads();
  if (t == 0) { uint64_t acc = 0; for (uint32_t k = 0; k < T; k++) { const uint64_t x = sh[k]; sh[k] = acc; acc += x; } sh[T] = acc; }
  __syncthreads();
  uint64_t acc = sh[t];
  for (size_t k = lo; k < hi; k++) { const uint32_t x = A.out_off[k]; A.out_off[k] = (uint32_t)acc; acc += x; }
  if (t == 0) A.out_off[cnt] = (uint32_t)sh[T];
}

__global__ __launch_bounds__(64) void utf8_lossy_write_kernel(Utf8LossyArgs A) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t off0 = A.off[0];
  for (uint32_t i = blockIdx.x; i < A.n; i += gridDim.x) {
    const uint32_t at = A.out_off[i], end = A.out_off[i + 1];
    if (end > A.cap) continue;          // the caller's blob is too small: the need is reported, nothing is cut short
    bool changed;
    (void)u8l_wave<true>(A.blob + (A.off[i] - off0), (uint32_t)(A.off[i + 1] - A.off[i]), A.out + at, lane, changed);
  }
}

#endif  // device part

}  // namespace zke
