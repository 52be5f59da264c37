// capture_lossy.hip.h — the gather launch of zke_extract_captures_encoded: capture_gather_kernel's verdict fold and tables
// (capture.hip.h) with the two host steps that stood between an extraction and its encoding moved behind them —
//   * String::from_utf8_lossy (helpers/src/regex.rs:35; utf8_lossy.hip.h): the strings of cap_blob are the REPAIRED strings, the
//     tables the reference's CompiledRegex.captures holds.  A column capture_kernel flagged ZKE_CAPF_NOT_UTF8 is measured and written
//     by u8l_wave; a valid one is as long as its span and is copied.  spans and flags stay what the extraction reports.
//   * the encode plan (encode_plan.hip.h's formula, one thread per e-mail): EncodeJob[n] for encode_outputs_placed_kernel, kind 1
//     throughout, the external inputs from the caller's ext_off (which rides in the input image), the matches the e-mail's strings
//     of cap_str_off, the places an exclusive scan of the lengths.
// The device knows the verdict when it plans, so — unlike the host plan, where every e-mail has a place whatever becomes of it — an
// e-mail whose record is not ZKE_OK gets length 0 and NO place: its off is the running offset and its neighbours' places close up.
// An e-mail that has a length but no room (its place would end beyond bytes_cap, or its strings beyond blob_cap) keeps its place in
// the scan — the needs stay exact — and is marked ENC_JOB_NO_ROOM: nothing of it is written, its info says len 0 and a zero digest.
// An encoding of ENC_MAX_LEN bytes or more is marked the same way and counts 0; the entry refuses, before staging, every batch in
// which one could come about (its external inputs are known there), so the mark is a guard, not a path.
// ONE workgroup of 1024 threads like capture_gather_kernel: e-mails by threads (fold, lengths, plan), columns by waves (measure,
// write), the block scans in between.  hdr: [0] strings, [1] blob bytes needed, [2] encoding bytes needed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capture.hip.h"
#include "encode.hip.h"
#include "utf8_lossy.hip.h"

namespace zke {

struct CapLossyArgs {
  CapGatherArgs g;                  // plain == 0; tmp: [n * P + n * G] as there
  const uint8_t* flags;             // [n * G] as capture_kernel left them
  const uint32_t* ext_off;          // [n + 1], or nullptr: no external inputs anywhere
  const uint32_t* ext_str_off;      // (unread without ext_off)
  EncodeJob* jobs;                  // [n]
  uint64_t bytes_cap;               // capacity of the encodings' blob
};

// abi.encode's string[] of the strings [lo, hi) of str_off, as enc_add_array counts it
__device__ __forceinline__ uint64_t cap_enc_array(const uint32_t* str_off, uint32_t lo, uint32_t hi) {
  uint64_t size = 32 + 64 * (uint64_t)(hi - lo);
  for (uint32_t s = lo; s < hi; s++) size += ((uint64_t)(str_off[s + 1] - str_off[s]) + 31) & ~(uint64_t)31;
  return size;
}

__global__ __launch_bounds__(1024) void capture_gather_lossy_kernel(CapLossyArgs L) {
  __shared__ uint64_t sh[1025];
  const CapGatherArgs& A = L.g;
  const uint32_t T = blockDim.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, waves = T >> 6;
  uint32_t* nstr = A.tmp;                              // [n * P]
  uint32_t* nbytes = A.tmp + (size_t)A.n * A.P;        // [n * G]
  const size_t NP = (size_t)A.n * A.P, NG = (size_t)A.n * A.G;
  auto hay_of = [&](uint32_t i, uint32_t p) -> const uint8_t* {
    const uint8_t* hay; uint32_t hlen;
    DfaArgs D = A.d; D.is_body = p >= A.n_header_parts ? 1u : 0u;
    dfa_haystack(D, i, A.d.b.meta + i, hay, hlen);
    (void)hlen;
    return hay;
  };
  auto part_of = [&](uint32_t c) { uint32_t p = 0; while (p + 1 < A.P && c >= A.gbase[p + 1]) p++; return p; };
  // the verdicts and the raw lengths, as capture_gather_kernel
  for (uint32_t i = t; i < A.n; i += T) {
    const bool ok = cap_fold_email(A.results + i, A.parts + (size_t)i * A.P, A.codes + (size_t)i * A.P, A.P, A.n_header_parts);
    for (uint32_t p = 0; p < A.P; p++) {
      const size_t col = (size_t)i * A.G + A.gbase[p];
      cap_part_lengths(ok, A.gbase[p + 1] - A.gbase[p], nstr + (size_t)i * A.P + p, nbytes + col, A.spans + 2 * col);
    }
  }
  __syncthreads();
  // the repaired lengths of the strings that are not UTF-8 (a part that yields no string has lost its spans above)
  for (size_t col = wave; col < NG; col += waves) {
    const uint32_t s = A.spans[2 * col], e = A.spans[2 * col + 1];
    if (s == CAP_NONE || !(L.flags[col] & CAPF_NOT_UTF8)) continue;
    const uint32_t i = (uint32_t)(col / A.G), p = part_of((uint32_t)(col % A.G));
    bool changed;
    const uint32_t len = u8l_wave<false>(hay_of(i, p) + s, e - s, nullptr, lane, changed);
    if (lane == 0) nbytes[col] = len;
  }
  __syncthreads();
  const uint64_t strings = cap_block_scan(nstr, NP, sh);
  for (size_t k = t; k < NP; k += T) A.cap_off[k] = nstr[k];
  if (t == 0) A.cap_off[NP] = (uint32_t)strings;
  const uint64_t bytes = cap_block_scan(nbytes, NG, sh);
  if (t == 0) { A.hdr[0] = strings; A.hdr[1] = bytes; }
  __syncthreads();                                     // cap_off is read below by other threads than wrote it
  // strings in column order, a wave per column: string index = cap_off[i * P + p] + (c - gbase[p])
  for (size_t col = wave; col < NG; col += waves) {
    const uint32_t i = (uint32_t)(col / A.G), c = (uint32_t)(col % A.G), p = part_of(c);
    const size_t ip = (size_t)i * A.P + p;
    const uint32_t first = A.cap_off[ip], cnt = A.cap_off[ip + 1] - first;
    if (!cnt) continue;
    const uint32_t sidx = first + (c - A.gbase[p]), at = nbytes[col];
    const uint32_t len = (uint32_t)((col + 1 < NG ? (uint64_t)nbytes[col + 1] : bytes) - at);
    if (lane == 0) {
      A.cap_str_off[sidx] = at;
      if (sidx + 1 == strings) A.cap_str_off[strings] = (uint32_t)bytes;
    }
    if ((uint64_t)at + len > A.blob_cap) continue;     // the blob is too small: sizes are reported, nothing is cut short silently
    const uint32_t s = A.spans[2 * col], e = A.spans[2 * col + 1];
    if (s == CAP_NONE || e == s) continue;
    const uint8_t* src = hay_of(i, p) + s;
    if (L.flags[col] & CAPF_NOT_UTF8) {
      bool changed;
      (void)u8l_wave<true>(src, e - s, A.cap_blob + at, lane, changed);
    } else {
      for (uint32_t k = lane; k < len; k += 64) A.cap_blob[at + k] = src[k];
    }
  }
  if (t == 0 && strings == 0) A.cap_str_off[0] = 0;
  __syncthreads();                                     // both offset tables are complete
  // the plan: a thread per e-mail; its length into lenv (the strings-per-part counts are no longer needed: n <= n * P words)
  uint32_t* lenv = A.tmp;
  for (uint32_t i = t; i < A.n; i += T) {
    EncodeJob J{};
    J.kind = ENC_KIND_WITH_REGEX;
    if (L.ext_off) { J.ext_lo = L.ext_off[i]; J.ext_hi = L.ext_off[i + 1]; }
    J.match_lo = A.cap_off[(size_t)i * A.P]; J.match_hi = A.cap_off[(size_t)(i + 1) * A.P];
    uint64_t size = 0;
    if (A.results[i].status == ZKE_OK) {
      size = 32 + 96 + 64 + cap_enc_array(L.ext_str_off, J.ext_lo, J.ext_hi) + cap_enc_array(A.cap_str_off, J.match_lo, J.match_hi);
      if (size >= ENC_MAX_LEN) { size = 0; J.reserved = ENC_JOB_NO_ROOM; }
      else if (J.match_hi > J.match_lo && A.cap_str_off[J.match_hi] > A.blob_cap) J.reserved = ENC_JOB_NO_ROOM;      // its strings were not written
    }
    lenv[i] = (uint32_t)size;
    L.jobs[i] = J;
  }
  __syncthreads();
  // the places: an exclusive scan of the lengths in 64 bits, straight into the jobs
  {
    const size_t cnt = A.n, per = (cnt + T - 1) / T, lo = (size_t)t * per < cnt ? (size_t)t * per : cnt, hi = lo + per < cnt ? lo + per : cnt;
    uint64_t sum = 0;
    for (size_t k = lo; k < hi; k++) sum += lenv[k];
    sh[t] = sum;
    __syncthreads();
    if (t == 0) { uint64_t acc = 0; for (uint32_t k = 0; k < T; k++) { const uint64_t x = sh[k]; sh[k] = acc; acc += x; } sh[T] = acc; }
    __syncthreads();
    uint64_t acc = sh[t];
    for (size_t k = lo; k < hi; k++) {
      const uint32_t len = lenv[k];
      L.jobs[k].enc_off = acc;
      if (len && acc + len > L.bytes_cap) L.jobs[k].reserved = ENC_JOB_NO_ROOM;
      acc += len;
    }
    if (t == 0) A.hdr[2] = sh[T];
  }
}

}  // namespace zke
