// bytes.hip.h — the 64-byte-wide scanner every one-item-per-wavefront parser here is built from (the e-mail front end
// parse.hip.h, the signature scan sigscan.hip.h, the key records keyrec.hip.h): byte strings with an LDS window and one
// excision, find first / find last by ballot, short literals as constant words, the LDS staging of an item's head, and the
// output stream the header canonicalisation writes the preimage through.  Control flow is wave-uniform throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lanes.hip.h"
#include "sha256.hip.h"      // uint4_unaligned

namespace zke {

constexpr uint32_t OOB = 0x100;       // "no byte here"
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t WNONE = 0x80000000u;   // "no window loaded" (e-mails are < 2^31 bytes)

// ------------------------------------------------------------------ byte strings and windows
struct Str {                  // logical string over global memory with one optional excision
  const uint8_t* base;
  uint32_t len;               // logical length
  uint32_t cut, skip;         // logical index >= cut reads base[index + skip]
  const uint8_t* lds;         // LDS copy of base[0 .. lds_len) (the staged head of the e-mail), or nullptr
  uint32_t lds_len;
};
__device__ __forceinline__ Str mkstr(const uint8_t* b, uint32_t len) { return Str{b, len, NONE, 0, nullptr, 0}; }
// s[a, b) as a string of its own (keeps the LDS window)
__device__ __forceinline__ Str substr(const Str& s, uint32_t a, uint32_t b) {
  Str r{s.base + a, b - a, NONE, 0, nullptr, 0};
  if (a < s.lds_len) { r.lds = s.lds + a; r.lds_len = s.lds_len - a; }
  return r;
}
__device__ __forceinline__ uint32_t ldb(const Str& s, uint32_t l) {
  if (l >= s.len) return OOB;
  const uint32_t phys = l + (l >= s.cut ? s.skip : 0u);
  const uint8_t* p = phys < s.lds_len ? s.lds + phys : s.base + phys;     // one flat load either way
  return (uint32_t)*p;
}
struct Win { uint32_t wpos; uint32_t c; };   // c = byte at logical wpos + lane (OOB beyond the end)

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ void wload(const Str& s, Win& w, uint32_t pos) { w.wpos = pos; w.c = ldb(s, pos + lane_id()); }
__device__ __forceinline__ uint32_t at(const Str& s, Win& w, uint32_t pos) {   // uniform pos -> uniform byte
  if (pos - w.wpos >= 64u) wload(s, w, pos);
  return __builtin_amdgcn_readlane(w.c, pos - w.wpos);
}
// A value every lane holds alike (loaded from LDS or memory at a wave-uniform address), as a scalar: branches on it are
// then scalar branches, not exec-mask regions — the parser's control flow is wave-uniform, but the compiler can only see
// that where the values come out of v_readfirstlane / v_readlane.
__device__ __forceinline__ uint32_t uni(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {     // set bits of m in the lanes below this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ uint64_t bits_from(uint32_t rel) { return rel >= 64 ? 0ull : (~0ull << rel); }
__device__ __forceinline__ uint64_t bits_below(uint32_t rel) { return rel >= 64 ? ~0ull : ((1ull << rel) - 1); }

// dst[0, n) = src[0, n) with dst in LDS, 16-byte aligned: 16-byte lane-contiguous loads, a byte tail, and the wave sees the
// copy when this returns.  Every later scan of the staged bytes then costs LDS latency instead of a dependent L2 round trip.
__device__ __forceinline__ void stage_lds(uint8_t* dst, const uint8_t* src, uint32_t n) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t full = n & ~15u;
  for (uint32_t base = 0; base < full; base += 64 * 16) {
    const uint32_t o = base + lane * 16;
    if (o < full) *(uint4*)(dst + o) = *(const uint4_unaligned*)(src + o);
  }
  { const uint32_t o = full + lane; if (o < n) dst[o] = src[o]; }        // n - full < 16
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// first l in [pos, end) with pred(byte), else end
template <class P>
__device__ __forceinline__ uint32_t wfind(const Str& s, Win& w, uint32_t pos, uint32_t end, P pred) {
  while (pos < end) {
    if (pos - w.wpos >= 64u) wload(s, w, pos);
    const uint32_t rel = pos - w.wpos;
    uint64_t m = __ballot(pred(w.c) && (w.wpos + lane_id()) < end) & bits_from(rel);
    if (m) return w.wpos + (uint32_t)__builtin_ctzll(m);
    pos = w.wpos + 64;
  }
  return end;
}
// last l in [start, end) with pred(byte), else NONE
template <class P>
__device__ __forceinline__ uint32_t wrfind(const Str& s, Win& w, uint32_t start, uint32_t end, P pred) {
  uint32_t pos = end;
  while (pos > start) {
    const uint32_t ws = (pos - start > 64u) ? pos - 64u : start;
    if (!(ws >= w.wpos && pos <= w.wpos + 64u)) wload(s, w, ws);
    const uint32_t l = w.wpos + lane_id();
    uint64_t m = __ballot(pred(w.c) && l >= ws && l < pos);
    if (m) return w.wpos + 63u - (uint32_t)__builtin_clzll(m);
    pos = ws;
  }
  return NONE;
}

__device__ __forceinline__ bool is_fws(uint32_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
__device__ __forceinline__ bool is_wsp(uint32_t c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ bool is_valchar(uint32_t c) { return (c >= 0x21 && c <= 0x3a) || (c >= 0x3c && c <= 0x7e); }
__device__ __forceinline__ bool is_alpha(uint32_t c) { return ((c | 0x20) >= 'a' && (c | 0x20) <= 'z') && c < 0x80; }
__device__ __forceinline__ bool is_alnumpunc(uint32_t c) { return is_alpha(c) || (c >= '0' && c <= '9') || c == '_'; }
__device__ __forceinline__ uint32_t lower(uint32_t c) { return (c >= 'A' && c <= 'Z') ? c + 32 : c; }

// case-insensitive equality of s[a, a+n) with a byte string in LDS / constant / global memory
__device__ __forceinline__ bool span_ieq(const Str& s, uint32_t a, uint32_t n, const uint8_t* name, uint32_t nlen) {
  if (n != nlen) return false;
  for (uint32_t o = 0; o < n; o += 64) {
    const uint32_t l = o + lane_id();
    bool bad = false;
    if (l < n) bad = lower(ldb(s, a + l)) != lower(name[l]);
    if (__ballot(bad)) return false;
  }
  return true;
}
// Does v[p, p+n) equal v[a, a+n)?
__device__ __forceinline__ bool same_bytes(const Str& v, uint32_t p, uint32_t a, uint32_t n) {
  for (uint32_t o = 0; o < n; o += 64) {
    const uint32_t l = o + lane_id();
    bool bad = l < n && ldb(v, p + l) != ldb(v, a + l);
    if (__ballot(bad)) return false;
  }
  return true;
}

// Short literals (<= 16 bytes) as four constant words: byte `lane` of one comes out of two v_perm_b32 on constants —
// no per-lane load from constant memory (a dependent L2 round trip per comparison) and no hoisted per-lane address of
// every literal (two registers each, live across the whole signature loop: they were what the front end spilled).
struct Lit { uint32_t w0, w1, w2, w3, n; };
template <size_t N>
constexpr Lit LIT(const char (&s)[N]) {
  static_assert(N >= 1 && N - 1 <= 16, "literal too long");
  uint32_t w[4] = {0, 0, 0, 0};
  for (size_t i = 0; i + 1 < N; i++) w[i / 4] |= (uint32_t)(uint8_t)s[i] << (8 * (i % 4));
  return Lit{w[0], w[1], w[2], w[3], (uint32_t)(N - 1)};
}
__device__ __forceinline__ uint32_t lit_at(const Lit& t, uint32_t lane) {      // byte `lane` (< 16) of the literal
  const uint32_t sel = (lane & 7u) | 0x0c0c0c00u;
  const uint32_t lo = __builtin_amdgcn_perm(t.w1, t.w0, sel);
  if (t.n <= 8) return lo;
  const uint32_t hi = __builtin_amdgcn_perm(t.w3, t.w2, sel);
  return (lane & 8u) ? hi : lo;
}
// case-insensitive equality of s[a, a+n) with a lower-case literal
__device__ __forceinline__ bool span_ieq(const Str& s, uint32_t a, uint32_t n, const Lit& t) {
  if (n != t.n) return false;
  const uint32_t l = (uint32_t)lane_id();
  const bool bad = l < n && lower(ldb(s, a + l)) != lit_at(t, l);
  return __ballot(bad) == 0;
}

// ------------------------------------------------------------------ output stream (preimage)
struct Out { uint8_t* p; uint32_t o, cap; bool overflow; };
__device__ __forceinline__ void emit_lit(Out& out, const Lit& t) {
  if (out.o + t.n > out.cap) { out.overflow = true; return; }
  if ((uint32_t)lane_id() < t.n) out.p[out.o + lane_id()] = (uint8_t)lit_at(t, (uint32_t)lane_id());
  out.o += t.n;
}
template <class F>   // copy s[a,b) through a byte map
__device__ __forceinline__ void emit_map(Out& out, const Str& s, uint32_t a, uint32_t b, F f) {
  if (b <= a) return;
  if (out.o + (b - a) > out.cap) { out.overflow = true; return; }
  for (uint32_t base = a; base < b; base += 64) {            // uniform trip count: the loop control stays on the scalar unit
    const uint32_t l = base + (uint32_t)lane_id();
    if (l < b) out.p[out.o + (l - a)] = (uint8_t)f(ldb(s, l));
  }
  out.o += b - a;
}

// cfdkim canonicalize_header_relaxed value part: unfold (drop CRLF), WSP runs -> one SP, trim both ends.
// One forward pass, one load per lane and 64-byte chunk (issued a chunk ahead; the neighbours come over DPP):
// a WSP run becomes the single SP written IN FRONT OF the next kept non-WSP byte, so leading runs (nothing
// emitted yet) and trailing runs (no such byte) vanish without a backward scan for the last kept byte.
__device__ __forceinline__ uint64_t uni64(uint64_t x) {
  return ((uint64_t)uni((uint32_t)(x >> 32)) << 32) | (uint64_t)uni((uint32_t)x);      // (the builtin returns int: widen as unsigned)
}
__device__ __forceinline__ void emit_relaxed_value(Out& out, const Str& v) {
  const uint32_t L = v.len;
  if (L == 0) return;
  const int lane = lane_id();
  // (every loop-carried value below is wave-uniform; said so with v_readfirstlane once per step, or the compiler takes the
  // loop for a divergent one — counters in vector registers, an exec-mask ledger around every branch)
  uint64_t cin = 0;            // a kept WSP byte lies behind the last kept non-WSP byte in front of this chunk
  uint32_t started = 0;        // a non-WSP byte has been emitted
  uint32_t prev_last = OOB;    // raw byte in front of this chunk
  uint32_t o = uni(out.o);
  const uint32_t cap = uni(out.cap);
  uint32_t cur = ldb(v, (uint32_t)lane);
  for (uint32_t base = 0; base < L; base += 64) {
    const uint32_t nxt = ldb(v, base + 64 + lane);                 // next chunk, in flight during this one
    const uint32_t l = base + lane;
    uint32_t cp = lane_down(cur); if (lane == 0) cp = prev_last;
    const uint32_t nfirst = __builtin_amdgcn_readfirstlane(nxt);     // outside the lane test: all lanes active here
    uint32_t cn = lane_up(cur); if (lane == 63) cn = nfirst;
    const bool crlf = (cur == '\r' && cn == '\n') || (cur == '\n' && cp == '\r');
    const bool kept = l < L && !crlf;
    const bool wsp = is_wsp(cur);
    const bool nw = kept && !wsp;
    const uint64_t W = __ballot(kept && wsp), N = __ballot(nw);
    // "a kept WSP lies between byte i and the last kept non-WSP byte below it" is a carry chain over the chunk — a WSP byte
    // generates, a dropped byte (CRLF, beyond the end) propagates, a non-WSP byte kills — solved for all 64 bytes by ONE
    // 64-bit addition on the scalar unit (a = generate | propagate, b = generate: the carry INTO bit i is sum ^ a ^ b).
    const uint64_t a = ~N, b = W;
    const uint64_t sum = a + b + cin;
    const uint64_t C = sum ^ a ^ b;
    uint64_t S = N & C;                                            // non-WSP bytes that get the run's single SP in front
    S &= started ? ~0ull : ~(N & (0 - N));                         // ... except the first one of the value: leading WSP vanishes
    S = uni64(S);
    cin = uni64(((a & b) | ((a | b) & ~sum)) >> 63);               // the carry out of bit 63
    const uint32_t cnt = uni((uint32_t)__builtin_popcountll(N) + (uint32_t)__builtin_popcountll(S));
    if (o + cnt > cap) { out.o = o; out.overflow = true; return; }
    if (nw) {
      uint8_t* dst = out.p + o + lanes_below(N) + lanes_below(S);
      if ((S >> lane) & 1) { dst[0] = (uint8_t)' '; dst[1] = (uint8_t)cur; } else dst[0] = (uint8_t)cur;
    }
    o = uni(o + cnt);
    started = uni(started | (N != 0 ? 1u : 0u));
    prev_last = __builtin_amdgcn_readlane(cur, 63);
    cur = nxt;
  }
  out.o = o;
}

// cfdkim canonicalize_header_{relaxed,simple}(key, value); the CRLF is appended by the caller's choice
__device__ __forceinline__ void emit_header(Out& out, const Str& key, const Str& val, bool relaxed, bool crlf) {
  if (relaxed) {
    uint32_t ke = key.len;
    if (ke && is_wsp(uni(ldb(key, ke - 1)))) {            // WSP in front of the ':' (rare): the name ends at its last non-WSP byte
      Win w; w.wpos = WNONE; w.c = 0;
      ke = wrfind(key, w, 0, key.len, [](uint32_t c) { return !is_wsp(c); });
      ke = (ke == NONE) ? 0 : ke + 1;
    }
    if (ke < 64) {                                        // the lower-cased name and its ':' as one store
      if (out.o + ke + 1 > out.cap) { out.overflow = true; return; }
      const uint32_t l = (uint32_t)lane_id();
      if (l <= ke) out.p[out.o + l] = l < ke ? (uint8_t)lower(ldb(key, l)) : (uint8_t)':';
      out.o += ke + 1;
    } else {
      emit_map(out, key, 0, ke, [](uint32_t c) { return lower(c); });
      emit_lit(out, LIT(":"));
    }
    emit_relaxed_value(out, val);
  } else {
    emit_map(out, key, 0, key.len, [](uint32_t c) { return c; });
    emit_lit(out, LIT(": "));
    emit_map(out, val, 0, val.len, [](uint32_t c) { return c; });
  }
  if (crlf) emit_lit(out, LIT("\r\n"));
}

}  // namespace zke
