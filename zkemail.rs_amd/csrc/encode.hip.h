// encode.hip.h — VerificationOutput::from_parts(email, matches).abi_encode() (core/src/io.rs:28-44) for whole batches, one e-mail
// per wavefront like the front end and body_extract_kernel: the bytes a zkVM front end commits as public values, written where the
// host's plan says (encode_plan.hip.h) from the two witness hashes of the e-mail's record and two string tables in the project's CSR
// shape — the external inputs, flattened [name1, value1, ...] as circuits.rs:18-27 does, and the matches, which is the regex capture
// table the batch already carries (circuits.rs:58-62).  Byte for byte what zke_abi_encode writes for the same hashes and strings.
// Every pointer of EncodeArgs is device memory and nothing here knows which entry filled it.
//
// Mapping.  Head words (32-byte big-endian integers whose low 8 bytes alone can be non-zero: an encoding is shorter than 2^32) are
// single lanes' work.  A string array goes in passes of 64 strings, one per lane: the lane reads its string's two offsets, the wave
// scans the padded lengths (counted in 16-byte chunks) — a string's tail offset is the scan's exclusive value plus `run`, the carry
// of the passes in front — and each lane writes its string's offset word and length word.  The bytes of the pass's strings are then
// ONE flat list of 16-byte chunks dealt to the lanes 64 at a time (a lane finds its chunk's string by a binary search over the scan,
// six cross-lane reads), so ten strings of 20 bytes keep twenty lanes busy once, not two lanes ten times, and a string longer than
// 64 x 16 bytes simply spans several rounds.
//
// Loads.  Destinations are 16-byte aligned (places and everything inside them are multiples of 32, the blob is 64-byte aligned);
// sources are not: a capture string starts at any byte of its blob.  A chunk is therefore read as the ALIGNED 16-byte block that
// holds its first byte and, only when the chunk's valid bytes reach into it, the next aligned block; the two are shifted together
// by the source's residue (a word select and v_alignbyte_b32).  An aligned 16-byte block that holds one byte of a string lies in
// that byte's page, so no load touches memory the string does not share a page with, whatever the blob's alignment and without any
// slack behind it; the bytes picked up beside the string are masked off.  Narrow loads at the edges would cost up to 15 byte loads
// per string end, and almost every string here IS an edge.
// The zero padding behind a string is written here (the masked tail of its last chunk, and a whole zero chunk where the padded
// length asks for one): the blob is a slot's buffer, reused across batches and never cleared.
//
// An e-mail whose record is not ZKE_OK writes nothing into the blob: len 0, a zero digest, an inactive hash job.  The SHA-256 of the
// encodings is the engine's ordinary hash launch over the ShaJob list written here (dst: the info's digest field).
// No LDS, no scratch: every loop-carried value is a wave-uniform scalar or one word per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zkemail_amd.h"
#include "encode_plan.hip.h"
#include "sha256.hip.h"

namespace zke {

struct EncodeArgs {
  uint32_t n;
  const zke_result* records;          // [n] status, from_domain_hash, public_key_hash
  const EncodeJob* jobs;              // [n]
  const uint32_t* ext_str_off; const uint8_t* ext_blob;          // external inputs (unread when no job names a string)
  const uint32_t* match_str_off; const uint8_t* match_blob;      // matches (likewise)
  zke_encoded_info* infos;            // [n]
  uint8_t* bytes;                     // 16-byte aligned; e-mail i's place is bytes[jobs[i].enc_off ..)
  ShaJob* sha;                        // [n] the digest launch's jobs
};

// EncodeJob.reserved of a job the device planned (capture_lossy.hip.h): the e-mail has no room — its place would end beyond the
// blob, or its strings were not written — and encode_outputs_placed_kernel treats it like an e-mail that is not ZKE_OK
constexpr uint32_t ENC_JOB_NO_ROOM = 1;

typedef uint32_t enc_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void enc_store16(uint8_t* dst, enc_u4 v) { *reinterpret_cast<enc_u4*>(dst) = v; }
// a head word: v as a 32-byte big-endian integer
__device__ __forceinline__ void enc_word(uint8_t* dst, uint64_t v) {
  enc_store16(dst, enc_u4{0, 0, 0, 0});
  enc_store16(dst + 16, enc_u4{0, 0, __builtin_bswap32((uint32_t)(v >> 32)), __builtin_bswap32((uint32_t)v)});
}
// src[0, k) (1 <= k <= 16) followed by 16 - k zero bytes, from aligned loads (the file comment says why they are legal)
__device__ __forceinline__ enc_u4 enc_load_chunk(const uint8_t* src, uint32_t k) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src);
  const uint32_t sh = (uint32_t)(a & 15);
  const enc_u4* ab = reinterpret_cast<const enc_u4*>(a - sh);
  const enc_u4 lo = ab[0];
  enc_u4 hi{0, 0, 0, 0};
  if (sh + k > 16) hi = ab[1];
  uint32_t w0 = lo.x, w1 = lo.y, w2 = lo.z, w3 = lo.w, w4 = hi.x, w5 = hi.y, w6 = hi.z, w7 = hi.w;
  if (sh & 8) { w0 = w2; w1 = w3; w2 = w4; w3 = w5; w4 = w6; w5 = w7; }
  if (sh & 4) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; }
  const uint32_t bs = sh & 3;
  enc_u4 o{__builtin_amdgcn_alignbyte(w1, w0, bs), __builtin_amdgcn_alignbyte(w2, w1, bs), __builtin_amdgcn_alignbyte(w3, w2, bs),
           __builtin_amdgcn_alignbyte(w4, w3, bs)};
  auto keep = [k](uint32_t first) { return k >= first + 4 ? 0xFFFFFFFFu : k > first ? (1u << (8 * (k - first))) - 1u : 0u; };
  o.x &= keep(0); o.y &= keep(4); o.z &= keep(8); o.w &= keep(12);
  return o;
}

// inclusive scan over the wave
__device__ __forceinline__ uint32_t enc_scan(uint32_t x, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, d);
    if (lane >= d) x += y;
  }
  return x;
}

// abi.encode's string[] of the strings [lo, hi) at dst; returns its size.  Called by the whole wave, with wave-uniform arguments.
__device__ __forceinline__ uint32_t enc_string_array(uint8_t* __restrict__ dst, const uint32_t* __restrict__ str_off,
                                                     const uint8_t* __restrict__ blob, uint32_t lo, uint32_t hi, uint32_t lane) {
  const uint32_t cnt = hi - lo;
  if (lane == 0) enc_word(dst, cnt);
  uint8_t* offs = dst + 32;                 // the offsets, and what a string's offset is relative to
  uint32_t run = 32 * cnt;                  // where the next pass's first tail starts
  for (uint32_t base = 0; base < cnt; base += 64) {
    const uint32_t idx = base + lane;
    const bool active = idx < cnt;
    const uint32_t s0 = active ? str_off[lo + idx] : 0u, s1 = active ? str_off[lo + idx + 1] : 0u;
    const uint32_t len = s1 - s0;
    const uint32_t nc = active ? ((len + 31) >> 5) << 1 : 0u;       // 16-byte chunks of the padded string
    const uint32_t incl = enc_scan(nc, lane), excl = incl - nc;
    const uint32_t tail = run + 32 * lane + 16 * excl;               // (the active lanes are a prefix: `lane` tails lie in front)
    if (active) {
      enc_word(offs + 32 * (size_t)idx, tail);
      enc_word(offs + tail, len);
    }
    const uint32_t chunks = (uint32_t)__shfl((int)incl, 63);
    for (uint32_t fb = 0; fb < chunks; fb += 64) {
      const uint32_t f = fb + lane;
      uint32_t j = 0;                         // the first lane whose inclusive count is beyond f: the chunk's string
#pragma unroll
      for (uint32_t s = 32; s >= 1; s >>= 1) {
        const uint32_t v = (uint32_t)__shfl((int)incl, (int)(j + s - 1));
        if (v <= f) j += s;
      }
      j &= 63;
      const uint32_t je = (uint32_t)__shfl((int)excl, (int)j), jt = (uint32_t)__shfl((int)tail, (int)j);
      const uint32_t jl = (uint32_t)__shfl((int)len, (int)j), js = (uint32_t)__shfl((int)s0, (int)j);
      if (f < chunks) {
        const uint32_t off = (f - je) * 16;
        const uint32_t k = jl > off ? (jl - off < 16 ? jl - off : 16u) : 0u;
        enc_u4 v{0, 0, 0, 0};
        if (k) v = enc_load_chunk(blob + js + off, k);
        enc_store16(offs + jt + 32 + off, v);
      }
    }
    run += 32 * (cnt - base < 64 ? cnt - base : 64u) + 16 * chunks;
  }
  return 32 + run;
}

// PLACED: the jobs are a device plan's (capture_lossy.hip.h), which marks the e-mails that have no room
template <bool PLACED = false>
__device__ __forceinline__ void encode_email(const EncodeArgs& A, const uint32_t i) {
  const uint32_t lane = threadIdx.x & 63;
  const EncodeJob J = A.jobs[i];
  const zke_result* R = A.records + i;
  const bool ok = R->status == ZKE_OK && !(PLACED && J.reserved == ENC_JOB_NO_ROOM);
  uint8_t* out = A.bytes + J.enc_off;
  uint32_t len = 0;
  if (ok) {
    const bool with_regex = J.kind == ENC_KIND_WITH_REGEX;
    const uint32_t tuple = with_regex ? 96u : 32u;                   // where the SolEmailOutput tuple starts
    if (lane == 0) enc_word(out, 0x20);
    if (lane == 1 && with_regex) enc_word(out + 32, 0x40);
    if (lane == 2) enc_word(out + tuple + 64, 0x60);
    if (lane >= 4 && lane < 8) {             // from_domain_hash and public_key_hash lie side by side in the record: 4 x 16 bytes
      const uint32_t* h = reinterpret_cast<const uint32_t*>(R->from_domain_hash) + 4 * (lane - 4);
      enc_store16(out + tuple + 16 * (lane - 4), enc_u4{h[0], h[1], h[2], h[3]});
    }
    const uint32_t ext = enc_string_array(out + tuple + 96, A.ext_str_off, A.ext_blob, J.ext_lo, J.ext_hi, lane);
    len = tuple + 96 + ext;
    if (with_regex) {
      if (lane == 0) enc_word(out + 64, 0x40 + 96 + (uint64_t)ext);
      len += enc_string_array(out + len, A.match_str_off, A.match_blob, J.match_lo, J.match_hi, lane);
    }
  }
  // the info (off, len, kind; the digest is the hash launch's, zero when there is nothing to hash) and the hash job
  if (lane < 4) {
    const uint32_t v = lane == 0 ? (uint32_t)J.enc_off : lane == 1 ? (uint32_t)(J.enc_off >> 32) : lane == 2 ? len : J.kind;
    reinterpret_cast<uint32_t*>(A.infos + i)[lane] = v;
  } else if (lane < 12 && !ok) {
    reinterpret_cast<uint32_t*>(A.infos + i)[lane] = 0;
  }
  if (lane >= 16 && lane < 22) {
    const uint64_t src = ok ? reinterpret_cast<uint64_t>(out) : 0, dst = ok ? reinterpret_cast<uint64_t>(A.infos[i].digest) : 0;
    const uint32_t w = lane - 16;
    const uint32_t v = w == 0 ? (uint32_t)src : w == 1 ? (uint32_t)(src >> 32) : w == 2 ? (uint32_t)dst : w == 3 ? (uint32_t)(dst >> 32) : w == 4 ? len : 0u;
    reinterpret_cast<uint32_t*>(A.sha + i)[w] = v;
  }
}

__global__ __launch_bounds__(64) void encode_outputs_kernel(EncodeArgs A) {
  const uint32_t email = blockIdx.x;
  if (email >= A.n) return;
  encode_email(A, email);
}

// the same over a device plan: an e-mail marked ENC_JOB_NO_ROOM writes nothing — len 0, a zero digest, an inactive hash job
__global__ __launch_bounds__(64) void encode_outputs_placed_kernel(EncodeArgs A) {
  const uint32_t email = blockIdx.x;
  if (email >= A.n) return;
  encode_email<true>(A, email);
}

}  // namespace zke
