// keydec.hip.h — what a key and a signature are decoded with, for the verify path (parse.hip.h) and the key records
// (keyrec.hip.h) alike: DER lengths and INTEGERs, the PKCS#1 RSAPublicKey walk (rsa 0.9.6 RsaPublicKey::from_pkcs1_der +
// check_public, RFC 8017 A.1.1), the choice of the RSA routine by the key cache, and base64 STANDARD, strict.
#pragma once
#include "zkemail_amd.h"
#include "rsa.hip.h"
#include "bytes.hip.h"
#include "stage_plan.hip.h"      // ROUTE_*

namespace zke {

// ------------------------------------------------------------------ PKCS#1 RSAPublicKey DER
__device__ __forceinline__ uint32_t der_len(const Str& k, Win& w, uint32_t p, uint32_t avail, uint32_t& out) {
  if (avail < 1) return 0;
  const uint32_t b0 = at(k, w, p);
  if (b0 < 0x80) { out = b0; return 1; }
  const uint32_t nb = b0 & 0x7f;
  if (nb == 0 || nb > 4 || nb + 1 > avail) return 0;
  uint32_t v = 0;
  for (uint32_t i = 0; i < nb; i++) v = (v << 8) | at(k, w, p + 1 + i);
  if (at(k, w, p + 1) == 0) return 0;
  if (nb == 1 && v < 0x80) return 0;
  if (nb == 4 && (v >> 31)) return 0;
  out = v;
  return nb + 1;
}
// INTEGER at p: value span [vp, vp+vl) with one sign octet stripped; returns bytes used or 0
__device__ __forceinline__ uint32_t der_uint(const Str& k, Win& w, uint32_t p, uint32_t avail, uint32_t& vp, uint32_t& vl) {
  if (avail < 2 || at(k, w, p) != 0x02) return 0;
  uint32_t l, c = der_len(k, w, p + 1, avail - 1, l);
  if (!c || l == 0 || (uint64_t)1 + c + l > avail) return 0;
  uint32_t s = p + 1 + c;
  const uint32_t v0 = at(k, w, s);
  if (v0 & 0x80) return 0;
  if (l > 1 && v0 == 0 && !(at(k, w, s + 1) & 0x80)) return 0;
  vp = s; vl = l;
  if (l > 1 && v0 == 0) { vp = s + 1; vl = l - 1; }
  return 1 + c + l;
}
// PKCS#1 RSAPublicKey at k[p0, p0 + len) (RFC 8017 A.1.1): the structure rsa 0.9.6 from_pkcs1_der reads — SEQUENCE { INTEGER n,
// INTEGER e } filling the input —, then the range RsaPublicKey::new applies, in its order: at most 4096 bits, at most 8
// exponent octets, 2 <= e <= 2^33 - 1.  The verify path and the key records map the two failures to codes of their own.
enum : uint32_t { PKCS1_OK = 0, PKCS1_DER, PKCS1_RANGE };
struct Pkcs1 { uint32_t np, nl, bits; uint64_t e; };      // the modulus k[np, np + nl), sign octet stripped; its bit length; the exponent
__device__ __forceinline__ uint32_t pkcs1_walk(const Str& k, Win& w, uint32_t p0, uint32_t len, Pkcs1& out) {
  if (len < 2 || at(k, w, p0) != 0x30) return PKCS1_DER;
  uint32_t sl, c = der_len(k, w, p0 + 1, len - 1, sl);
  if (!c || (uint64_t)1 + c + sl != len) return PKCS1_DER;
  uint32_t p = p0 + 1 + c, avail = sl, np, nl, ep, el;
  uint32_t used = der_uint(k, w, p, avail, np, nl);
  if (!used) return PKCS1_DER;
  p += used; avail -= used;
  used = der_uint(k, w, p, avail, ep, el);
  if (!used || used != avail) return PKCS1_DER;
  const uint32_t n0 = at(k, w, np);
  uint32_t bits = 0;
  if (!(nl == 1 && n0 == 0)) bits = nl * 8 - (uint32_t)(__builtin_clz(n0) - 24);
  if (bits > 4096) return PKCS1_RANGE;
  if (el > 8) return PKCS1_RANGE;
  uint64_t e = 0;
  for (uint32_t i = 0; i < el; i++) e = (e << 8) | at(k, w, ep + i);
  if (e < 2 || e > ((1ull << 33) - 1)) return PKCS1_RANGE;
  out = Pkcs1{np, nl, bits, e};
  return PKCS1_OK;
}
// returns 0 or ZKE_D_KEY_*; fills the RSA job's modulus / exponent
__device__ __forceinline__ uint32_t decode_rsa_key(const Str& k, RsaJob* J, Pkcs1& pk, uint32_t& even) {
  Win w; w.wpos = WNONE; w.c = 0;
  const uint32_t r = pkcs1_walk(k, w, 0, k.len, pk);
  if (r) return r == PKCS1_DER ? ZKE_D_KEY_DER : ZKE_D_KEY_RANGE;
  const uint32_t np = pk.np, nl = pk.nl, bits = pk.bits;
  // modulus, big-endian, right-aligned in the 512-byte field (zero fill in front)
  {
    // (the eight loads of a lane leave together; interleaved with the stores each waited for its own round trip)
    uint8_t mb[8];
#pragma unroll
    for (uint32_t t = 0; t < 8; t++) {
      const uint32_t o = (uint32_t)lane_id() + 64 * t;
      mb[t] = o >= 512 - nl ? (uint8_t)ldb(k, np + (o - (512 - nl))) : (uint8_t)0;
    }
#pragma unroll
    for (uint32_t t = 0; t < 8; t++) J->mod[(uint32_t)lane_id() + 64 * t] = mb[t];
  }
  even = !(at(k, w, np + nl - 1) & 1) && bits != 0;
  if (lane_id() == 0) { J->e = pk.e; J->k = nl; J->bits = bits; }
  return 0;
}
// The same decode in two parts, as the body canonicaliser is (canon_body_compute / canon_body_publish), for the round-0 front end with
// a helper wave (parse.hip.h): the helper runs the first before anything is known about the e-mail and the second behind a barrier,
// when the front-end wave has come through the key site.  Together they compute and store exactly what decode_rsa_key does; that one
// keeps its text (the modulus stored before the last byte is looked at for `even`), and with it the one-wave kernels their instruction streams.
//   compute  returns 0 or ZKE_D_KEY_*; pk, `even`, and byte lane + 64 t of the 512-byte modulus field in mb[t].  Reads the key, writes nothing.
//   store    the RSA job's modulus / exponent
struct RsaModBytes { uint8_t mb[8]; };
__device__ __forceinline__ uint32_t decode_rsa_key_compute(const Str& k, Pkcs1& pk, uint32_t& even, RsaModBytes& m) {
  Win w; w.wpos = WNONE; w.c = 0;
  const uint32_t r = pkcs1_walk(k, w, 0, k.len, pk);
  if (r) return r == PKCS1_DER ? ZKE_D_KEY_DER : ZKE_D_KEY_RANGE;
  const uint32_t np = pk.np, nl = pk.nl;
#pragma unroll
  for (uint32_t t = 0; t < 8; t++) {
    const uint32_t o = (uint32_t)lane_id() + 64 * t;
    m.mb[t] = o >= 512 - nl ? (uint8_t)ldb(k, np + (o - (512 - nl))) : (uint8_t)0;
  }
  even = !(at(k, w, np + nl - 1) & 1) && pk.bits != 0;
  return 0;
}
__device__ __forceinline__ void decode_rsa_key_store(RsaJob* J, const Pkcs1& pk, const RsaModBytes& m) {
#pragma unroll
  for (uint32_t t = 0; t < 8; t++) J->mod[(uint32_t)lane_id() + 64 * t] = m.mb[t];
  if (lane_id() == 0) { J->e = pk.e; J->k = pk.nl; J->bits = pk.bits; }
}

// Which RSA routine takes this key's signatures: RSA_F_QUAD / RSA_F_OCT when the lane-group kernel for its size is part of
// the batch's launch (mask: ROUTE_QUAD / ROUTE_OCT; ROUTE_OCT9: the launch has the eight-lane role for moduli <= 2048 bits, RSA_F_OCT9, in
// place of the four-lane one) and the key's Montgomery constants are in the cache — the modulus [np, np + nl) of
// the DER key compared limb by limb with the entry, so a hit is exact; 0 = the one-signature-per-wave routine (which
// fills the cache for the next batch).
__device__ __forceinline__ uint32_t rsa_route(const Str& k, uint32_t np, uint32_t nl, uint32_t bits, const KeyCacheEntry* cache, uint32_t mask) {
  // (the bits above RSA_F_* say why a key was not routed: zke_debug_out.rsa_route shows them to the tests)
  if (bits < 512 || !(mask & (bits <= 2048 ? ROUTE_QUAD | ROUTE_OCT9 : ROUTE_OCT))) return 0x100;
  const uint32_t lane = (uint32_t)lane_id();
  auto limb = [&](uint32_t L) -> uint32_t {       // little-endian 32-bit limb L of the big-endian modulus
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) { const uint32_t pos = 4 * L + b; if (pos < nl) v |= ldb(k, np + nl - 1 - pos) << (8 * b); }
    return v;
  };
  const uint32_t l0 = limb(lane), l1 = limb(64 + lane);
  const KeyCacheEntry* E = cache + key_cache_slot(__builtin_amdgcn_readfirstlane(l0), __builtin_amdgcn_readlane(l0, 1));
  // All four loads leave before the first answer is looked at: each is an agent-scope load served at the coherence point, a
  // round trip of a microsecond or more, and three of them in a row (state, then bits, then the limbs) were a twentieth of the
  // wave's life.  An entry is written once and immutable from state == 2 on (rsa_kernel.hip.h): limbs served before the
  // publication beside a state served after it can only turn a hit into a miss — the wave routine then takes the signature.
  const uint32_t st = ld_agent(&E->state), eb = ld_agent(&E->bits), m0 = ld_agent(&E->mod[lane]), m1 = ld_agent(&E->mod[64 + lane]);
  if (st != 2u) return 0x200;                                       // not cached (yet)
  if (eb != bits) return 0x400;                                     // the slot belongs to another key
  const bool same = m0 == l0 && m1 == l1;
  return __ballot(!same) == 0 ? (bits > 2048 ? (uint32_t)RSA_F_OCT : (mask & ROUTE_OCT9) ? (uint32_t)RSA_F_OCT9 : (uint32_t)RSA_F_QUAD) : 0x400u;
}

// ------------------------------------------------------------------ base64 STANDARD, strict
__device__ __forceinline__ uint32_t b64v(uint32_t c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return 64;
}
// how many '=' end the string s[0, n) in LDS (n > 0, a multiple of 4): 0, 1 or 2
__device__ __forceinline__ uint32_t b64_pad(const uint8_t* s, uint32_t n) {
  return (uni(s[n - 1]) == '=') ? ((uni(s[n - 2]) == '=') ? 2u : 1u) : 0u;
}
// Quad q of the nq quads of s, as the base64 crate's STANDARD engine decodes them (padding required: pad = b64_pad): the
// 24 bits, how many of the three bytes count (nb), and `bad` — a character outside the alphabet, '=' anywhere but in the
// pad, or non-zero bits behind the last byte.  One lane per quad; where the bytes land is the caller's business.
struct B64Quad { uint32_t v, nb; bool bad; };
__device__ __forceinline__ B64Quad b64_quad(const uint8_t* s, uint32_t nq, uint32_t pad, uint32_t q) {
  const bool last = (q + 1 == nq);
  const uint32_t a = b64v(s[4 * q]), b = b64v(s[4 * q + 1]);
  uint32_t c = b64v(s[4 * q + 2]), d = b64v(s[4 * q + 3]);
  B64Quad r{0, 3, false};
  if (last && pad == 2) { c = 0; d = 0; r.nb = 1; if (b & 15) r.bad = true; }
  else if (last && pad == 1) { d = 0; r.nb = 2; if (c < 64 && (c & 3)) r.bad = true; }
  if (a > 63 || b > 63 || c > 63 || d > 63) r.bad = true;
  r.v = (a << 18) | (b << 12) | (c << 6) | d;
  return r;
}
// b=: s[0, n) (FWS-stripped, LDS) decoded into J->sig (right-aligned).  false = not canonical base64.
__device__ __forceinline__ bool decode_sig(const uint8_t* s, uint32_t n, RsaJob* J, uint32_t& sig_len) {
  sig_len = 0;
  uint32_t pad = 0, total = 0;
  const bool shape_ok = (n % 4) == 0;
  if (shape_ok && n) {
    pad = b64_pad(s, n);
    total = 3 * (n / 4) - pad;
  }
  {   // zero the part of the field the decoded bytes will not cover
    const uint32_t zend = (shape_ok && total <= 512) ? 512 - total : 512;
    for (uint32_t base = 0; base < zend; base += 64) { const uint32_t o = base + (uint32_t)lane_id(); if (o < zend) J->sig[o] = 0; }
  }
  if (!shape_ok) return false;
  if (n == 0) return true;
  bool bad = false;
  for (uint32_t q0 = 0; q0 < n / 4; q0 += 64) {
    const uint32_t q = q0 + lane_id();
    if (q < n / 4) {
      const B64Quad t = b64_quad(s, n / 4, pad, q);
      bad = bad || t.bad;
      if (total <= 512) {
        const uint32_t dst = 512 - total + 3 * q;
        J->sig[dst] = (uint8_t)(t.v >> 16);
        if (t.nb > 1) J->sig[dst + 1] = (uint8_t)(t.v >> 8);
        if (t.nb > 2) J->sig[dst + 2] = (uint8_t)t.v;
      }
    }
  }
  sig_len = total;
  return __ballot(bad) == 0;
}

}  // namespace zke
