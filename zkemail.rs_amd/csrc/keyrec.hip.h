// keyrec.hip.h — DKIM key records: what a resolver returns ("v=DKIM1; k=rsa; p=MIGfMA0G...") into the (key, key_type) pair
// Email.public_key and the verify launches take.  The reference does this on the host, once per candidate, at
// helpers/src/dkim.rs:67-111; here it is one launch over all records of a batch, one record per wavefront.
//
// Mapping.  One record per wave (64 lanes): a record is 0.1 - 0.8 KB, its base64 text 200 - 740 characters, so a wave's 64
// lanes x 4 characters decode it in 1 - 3 steps and every scan (';', white space, tag names) is a ballot over 64 bytes.  A lane
// group per record (8 or 16 lanes) would pack more records into a wave but serialise exactly those steps; the launch is a
// few microseconds beside the three verify launches either way (tools/keyrec_probe.py), so the plain mapping stays.
//
// Phases, all on the record's copy in LDS (the record is read from HBM once, 16 bytes per lane):
//   1. find the tags — ZKE_KEYREC_ARCHIVE: dkim.rs:74-85, split at ';', ASCII trim, "k=" / "p=" prefixes, last wins;
//      ZKE_KEYREC_DNS: RFC 6376 3.6.1 in the tag-list grammar of the signature parser (taglist.hip.h, parse_tag_spec), FWS
//      removed from the k= and p= values in place;
//   2. base64 STANDARD, strict (padding required, trailing bits zero): each lane takes four characters, 192 bytes per step;
//   3. k=rsa: SubjectPublicKeyInfo first, then PKCS#1, then the range RsaPublicKey::new applies — with der_len / der_uint of
//      keydec.hip.h, the one copy decode_rsa_key uses too; k=ed25519: 32 bytes.
//
// "Re-encoding" (dkim.rs:100 to_pkcs1_der).  DER admits exactly one encoding per value and the der crate rejects every other
// one, so the PKCS#1 bytes a validated key re-encodes to ARE the bytes it was decoded from: for a SubjectPublicKeyInfo the
// tail behind the BIT STRING's unused-bits octet, for PKCS#1 the whole input.  The kernel validates, then copies that slice;
// there is no encoder.
//
// Output.  One zke_key_info per record; the key bytes of record i at keys[rec_off[i] ..) — a decoded key is shorter than its
// record, so the records' own offsets give every wave a private place without a counter.  The host compacts them while it copies
// them out (zke_decode_key_records); for zke_select_keys_from_records keyrec_pack_kernel / keyrec_gather_kernel turn them into the
// packed CSR key_blob[key_off[i] .. key_off[i+1]) + key_type[i] the front end reads, in HBM.
#pragma once
#include "bytes.hip.h"
#include "keydec.hip.h"

namespace zke {

constexpr uint32_t KEYREC_DER_MAX = 3072;        // 3/4 of ZKE_KEYREC_MAX_BYTES

struct KeyrecArgs {
  uint32_t m, mode;
  const uint8_t* rec; const uint64_t* rec_off;      // record i = rec[rec_off[i] .. rec_off[i+1])
  zke_key_info* infos;                              // [m]
  uint8_t* keys;                                    // key i at keys[rec_off[i] - rec_off[0] ..)
};

struct KeyrecLds {
  __attribute__((aligned(16))) uint8_t rec[ZKE_KEYREC_MAX_BYTES];
  uint8_t der[KEYREC_DER_MAX];
};

// first l in [pos, end) with pred(s[l]), else end  /  last such l, else NONE.  s is LDS; results are wave-uniform
template <class P>
__device__ __forceinline__ uint32_t kr_find(const uint8_t* s, uint32_t pos, uint32_t end, P pred) {
  for (uint32_t base = pos; base < end; base += 64) {
    const uint32_t l = base + (uint32_t)lane_id();
    const uint64_t m = __ballot(l < end && pred((uint32_t)s[l < end ? l : pos]));
    if (m) return base + (uint32_t)__builtin_ctzll(m);
  }
  return end;
}
template <class P>
__device__ __forceinline__ uint32_t kr_rfind(const uint8_t* s, uint32_t start, uint32_t end, P pred) {
  for (uint32_t hi = end; hi > start;) {
    const uint32_t lo = hi - start > 64u ? hi - 64u : start;
    const uint32_t l = lo + (uint32_t)lane_id();
    const uint64_t m = __ballot(l < hi && pred((uint32_t)s[l < hi ? l : lo]));
    if (m) return lo + 63u - (uint32_t)__builtin_clzll(m);
    hi = lo;
  }
  return NONE;
}
__device__ __forceinline__ uint32_t kr_at(const uint8_t* s, uint32_t l) { return uni((uint32_t)s[l]); }
// remove FWS from s[a, b) in place; returns the new end.  (Every lane of a step reads before any lane writes, and a write goes
// to an index at or below the one it was read from.)
__device__ __forceinline__ uint32_t kr_strip(uint8_t* s, uint32_t a, uint32_t b) {
  uint32_t o = a;
  for (uint32_t base = a; base < b; base += 64) {
    const uint32_t l = base + (uint32_t)lane_id();
    const uint32_t c = l < b ? (uint32_t)s[l] : OOB;
    const bool k = l < b && !is_fws(c);
    const uint64_t m = __ballot(k);
    __builtin_amdgcn_wave_barrier();
    if (k) s[o + lanes_below(m)] = (uint8_t)c;
    __builtin_amdgcn_wave_barrier();
    o += (uint32_t)__builtin_popcountll(m);
  }
  return o;
}
__device__ __forceinline__ bool kr_eq(const uint8_t* s, uint32_t a, uint32_t b, const Lit& t) {
  if (b - a != t.n) return false;
  const uint32_t l = (uint32_t)lane_id();
  return __ballot(l < t.n && (uint32_t)s[a + (l < t.n ? l : 0)] != lit_at(t, l)) == 0;
}
// str::trim's ASCII share: U+0009..U+000D and space
__device__ __forceinline__ bool is_trim_ws(uint32_t c) { return (c >= 9 && c <= 13) || c == ' '; }

// PKCS#1 RSAPublicKey at k[p0, p0 + len): pkcs1_walk (keydec.hip.h), the walk decode_rsa_key takes, under the key records' codes.
// 0, ZKE_D_KEYREC_DER or ZKE_D_KEYREC_RANGE
__device__ __forceinline__ uint32_t kr_pkcs1(const Str& k, Win& w, uint32_t p0, uint32_t len) {
  Pkcs1 pk;
  const uint32_t r = pkcs1_walk(k, w, p0, len, pk);
  return r == PKCS1_OK ? 0u : r == PKCS1_DER ? (uint32_t)ZKE_D_KEYREC_DER : (uint32_t)ZKE_D_KEYREC_RANGE;
}

// SubjectPublicKeyInfo at k[0, len) (rsa 0.9.6 from_public_key_der: spki 0.7 + verify_algorithm_id): the outer SEQUENCE fills the
// input; AlgorithmIdentifier = SEQUENCE { OID rsaEncryption, NULL } — one DER encoding, 15 bytes; BIT STRING with 0 unused bits
// to the end; in it the PKCS#1 key at [off, off + klen).  0, ZKE_D_KEYREC_DER (no SubjectPublicKeyInfo) or ZKE_D_KEYREC_RANGE
__device__ __forceinline__ uint32_t kr_spki(const Str& k, Win& w, uint32_t len, uint32_t& off, uint32_t& klen) {
  if (len < 2 || at(k, w, 0) != 0x30) return ZKE_D_KEYREC_DER;
  uint32_t sl, c = der_len(k, w, 1, len - 1, sl);
  if (!c || (uint64_t)1 + c + sl != len) return ZKE_D_KEYREC_DER;
  uint32_t p = 1 + c, avail = sl;
  if (avail < 15) return ZKE_D_KEYREC_DER;
  {
    constexpr Lit ALG = LIT("\x30\x0d\x06\x09\x2a\x86\x48\x86\xf7\x0d\x01\x01\x01\x05\x00");
    static_assert(ALG.n == 15, "AlgorithmIdentifier of rsaEncryption");
    const uint32_t l = (uint32_t)lane_id();
    if (__ballot(l < 15 && ldb(k, p + l) != lit_at(ALG, l))) return ZKE_D_KEYREC_DER;
  }
  p += 15; avail -= 15;
  if (avail < 2 || at(k, w, p) != 0x03) return ZKE_D_KEYREC_DER;
  uint32_t bl;
  c = der_len(k, w, p + 1, avail - 1, bl);
  if (!c || (uint64_t)1 + c + bl != avail || bl < 1) return ZKE_D_KEYREC_DER;
  if (at(k, w, p + 1 + c) != 0) return ZKE_D_KEYREC_DER;              // unused bits
  off = p + 1 + c + 1; klen = bl - 1;
  return kr_pkcs1(k, w, off, klen);
}

__device__ __forceinline__ void keyrec_record(const KeyrecArgs& A, const uint32_t i, KeyrecLds& L) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint64_t r0 = A.rec_off[i], r1 = A.rec_off[i + 1], rel = r0 - A.rec_off[0];
  auto finish = [&](uint32_t code, uint32_t key_type, uint32_t key_len) {
    const uint32_t v = lane == 0 ? code : lane == 1 ? key_type : lane == 2 ? (uint32_t)rel : key_len;
    if (lane < 4) reinterpret_cast<uint32_t*>(A.infos + i)[lane] = v;
  };
  if (r1 == r0) { finish(ZKE_D_KEYREC_NO_KEY, 0, 0); return; }                       // the fetch failed (generator.rs:33)
  if (r1 - r0 > ZKE_KEYREC_MAX_BYTES) { finish(ZKE_D_KEYREC_TOO_LONG, 0, 0); return; }
  const uint32_t n = (uint32_t)(r1 - r0);
  uint8_t* s = L.rec;
  stage_lds(s, A.rec + r0, n);

  // ---- phase 1: the k= and p= values, s[kt_s, kt_e) and s[pk_s, pk_e)
  uint32_t kt_s = 0, kt_e = 0, pk_s = 0, pk_e = 0;
  if (A.mode == ZKE_KEYREC_ARCHIVE) {
    // k.value.contains("p=") && !k.value.ends_with("p=")                            dkim.rs:69-71
    bool has = false;
    for (uint32_t base = 0; base + 1 < n; base += 64) {
      const uint32_t l = base + lane;
      has = has || (l + 1 < n && s[l] == 'p' && s[l + 1] == '=');
    }
    if (!__ballot(has) || (kr_at(s, n - 2) == 'p' && kr_at(s, n - 1) == '=')) { finish(ZKE_D_KEYREC_NO_KEY, 0, 0); return; }
    // value.split(';').map(str::trim).fold(..)                                       dkim.rs:74-85
    bool edge = false;
    for (uint32_t pos = 0;;) {
      const uint32_t semi = kr_find(s, pos, n, [](uint32_t c) { return c == ';'; });
      const uint32_t a = kr_find(s, pos, semi, [](uint32_t c) { return !is_trim_ws(c); });
      if (a < semi) {
        const uint32_t b = kr_rfind(s, a, semi, [](uint32_t c) { return !is_trim_ws(c); }) + 1;
        const uint32_t c0 = kr_at(s, a);
        edge = edge || c0 >= 0x80 || kr_at(s, b - 1) >= 0x80;
        if (b - a >= 2 && kr_at(s, a + 1) == '=') {
          if (c0 == 'k') { kt_s = a + 2; kt_e = b; }
          if (c0 == 'p') { pk_s = a + 2; pk_e = b; }
        }
      }
      if (semi >= n) break;
      pos = semi + 1;
    }
    if (edge) { finish(ZKE_D_KEYREC_NON_ASCII_EDGE, 0, 0); return; }
  } else {
    if (kr_find(s, 0, n, [](uint32_t c) { return c >= 0x80; }) < n) { finish(ZKE_D_KEYREC_SYNTAX, 0, 0); return; }
    bool have_p = false;
    for (uint32_t pos = 0, idx = 0;; idx++) {
      // tag-spec = [FWS] tag-name [FWS] "=" [FWS] tag-value [FWS]   (taglist.hip.h, parse_tag_spec)
      uint32_t p = kr_find(s, pos, n, [](uint32_t c) { return !is_fws(c); });
      bool ok = p < n && is_alpha(kr_at(s, p));
      uint32_t ns = p, ne = p, rs = 0, re = 0, rend = 0;
      if (ok) {
        ne = kr_find(s, p, n, [](uint32_t c) { return !is_alnumpunc(c); });
        p = kr_find(s, ne, n, [](uint32_t c) { return !is_fws(c); });
        ok = p < n && kr_at(s, p) == '=';
      }
      if (ok) {
        rs = kr_find(s, p + 1, n, [](uint32_t c) { return !is_fws(c); });
        rend = kr_find(s, rs, n, [](uint32_t c) { return !(is_valchar(c) || is_fws(c)); });
        re = kr_rfind(s, rs, rend, [](uint32_t c) { return is_valchar(c); });
        re = re == NONE ? rs : re + 1;
      }
      if (!ok) {
        if (idx == 0) { finish(ZKE_D_KEYREC_SYNTAX, 0, 0); return; }
        break;                                  // what follows the last well-formed tag-spec is not read
      }
      if (ne - ns == 1) {
        const uint32_t c0 = kr_at(s, ns);
        if (c0 == 'v') {
          if (idx != 0 || !kr_eq(s, rs, kr_strip(s, rs, re), LIT("DKIM1"))) { finish(ZKE_D_KEYREC_VERSION, 0, 0); return; }
        } else if (c0 == 'k') {
          kt_s = rs; kt_e = kr_strip(s, rs, re);
        } else if (c0 == 'p') {
          pk_s = rs; pk_e = kr_strip(s, rs, re); have_p = true;
        }
      }
      if (!(rend < n && kr_at(s, rend) == ';')) break;
      pos = rend + 1;
    }
    if (!have_p) { finish(ZKE_D_KEYREC_NO_KEY, 0, 0); return; }
  }
  if (pk_e == pk_s) { finish(ZKE_D_KEYREC_NO_KEY, 0, 0); return; }                    // "No public key found" dkim.rs:92-94 / revoked
  uint32_t key_type = ZKE_KEY_RSA;                                                    // an empty type is "rsa"  dkim.rs:88-90
  if (kt_e != kt_s && !kr_eq(s, kt_s, kt_e, LIT("rsa"))) {
    if (!kr_eq(s, kt_s, kt_e, LIT("ed25519"))) { finish(ZKE_D_KEYREC_TYPE, ZKE_KEY_OTHER, 0); return; }
    key_type = ZKE_KEY_ED25519;
  }

  // ---- phase 2: STANDARD.decode(&public_key)                                       dkim.rs:97, :104
  const uint32_t nc = pk_e - pk_s;
  if (nc % 4) { finish(ZKE_D_KEYREC_B64, key_type, 0); return; }
  const uint8_t* t = s + pk_s;
  const uint32_t pad = b64_pad(t, nc);
  const uint32_t total = 3 * (nc / 4) - pad;                                          // <= 3069 < KEYREC_DER_MAX
  {
    bool bad = false;
    for (uint32_t q0 = 0; q0 < nc / 4; q0 += 64) {
      const uint32_t q = q0 + lane;
      if (q < nc / 4) {
        const B64Quad d = b64_quad(t, nc / 4, pad, q);
        bad = bad || d.bad;
        L.der[3 * q] = (uint8_t)(d.v >> 16);
        if (d.nb > 1) L.der[3 * q + 1] = (uint8_t)(d.v >> 8);
        if (d.nb > 2) L.der[3 * q + 2] = (uint8_t)d.v;
      }
    }
    if (__ballot(bad)) { finish(ZKE_D_KEYREC_B64, key_type, 0); return; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  // ---- phase 3: the key
  uint32_t off = 0, klen = total;
  if (key_type == ZKE_KEY_ED25519) {
    if (total != 32) { finish(ZKE_D_KEYREC_ED25519_LEN, key_type, 0); return; }       // dkim.rs:105-107
  } else {
    const Str k = mkstr(L.der, total);
    Win w; w.wpos = WNONE; w.c = 0;
    uint32_t r = kr_spki(k, w, total, off, klen);                                     // from_public_key_der ...
    if (r == ZKE_D_KEYREC_DER) { off = 0; klen = total; r = kr_pkcs1(k, w, 0, total); }   // ... .or_else(from_pkcs1_der)
    if (r) { finish(r, key_type, 0); return; }
  }
  uint8_t* dst = A.keys + rel;                     // klen <= 3/4 n: inside this record's own range
  for (uint32_t o = lane; o < klen; o += 64) dst[o] = L.der[off + o];
  finish(0, key_type, klen);
}

__global__ __launch_bounds__(64) void keyrec_kernel(KeyrecArgs A) {
  __shared__ KeyrecLds L[1];
  const uint32_t i = blockIdx.x;
  if (i >= A.m) return;
  keyrec_record(A, i, L[0]);
}

// ---- the decoded keys as the front end's key section (zke_select_keys_from_records): a length pass and a scan by ONE wave — m is
// the number of candidate keys of a batch, 64 per step —, then one wave per key copies its bytes.  A record without a key becomes
// an empty RSA key: the record verify_email gives it is ZKE_KEY_DECODE_FAIL.
struct KeyrecPackArgs {
  uint32_t m;
  const zke_key_info* infos;
  const uint8_t* keys;            // key i at keys[infos[i].key_off ..)
  uint64_t* key_off;              // [m + 1]
  uint8_t* key_type;              // [m]
  uint8_t* key_blob;
};

__global__ __launch_bounds__(64) void keyrec_pack_kernel(KeyrecPackArgs A) {
  const uint32_t lane = (uint32_t)lane_id();
  uint64_t carry = 0;
  for (uint32_t base = 0; base < A.m; base += 64) {
    const uint32_t i = base + lane;
    uint32_t len = 0, kt = ZKE_KEY_RSA;
    if (i < A.m && A.infos[i].code == 0) { len = A.infos[i].key_len; kt = A.infos[i].key_type; }
    uint32_t incl = len;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (i < A.m) { A.key_off[i] = carry + incl - len; A.key_type[i] = (uint8_t)kt; }
    carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  }
  if (lane == 0) A.key_off[A.m] = carry;
}

__global__ __launch_bounds__(64) void keyrec_gather_kernel(KeyrecPackArgs A) {
  const uint32_t i = blockIdx.x, lane = (uint32_t)lane_id();
  if (i >= A.m || A.infos[i].code != 0) return;
  const uint32_t len = A.infos[i].key_len;
  const uint8_t* src = A.keys + A.infos[i].key_off;
  uint8_t* dst = A.key_blob + A.key_off[i];
  for (uint32_t o = lane; o < len; o += 64) dst[o] = src[o];
}

}  // namespace zke
