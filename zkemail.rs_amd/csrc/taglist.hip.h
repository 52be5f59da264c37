// taglist.hip.h — the LDS image of a front-end wave and cfdkim's view of one DKIM-Signature header value: the tag-list
// grammar (RFC 6376 §3.2; one lane per tag-spec, or serially), validate_header, and what the verify path (parse.hip.h) and
// the signature scan (sigscan.hip.h) both ask of a validated signature: does d= name from_domain, which scheme is a=.
#pragma once
#include "zkemail_amd.h"
#include "bytes.hip.h"

namespace zke {

enum : int { TG_V = 0, TG_A, TG_B, TG_BH, TG_D, TG_H, TG_S, TG_I, TG_Q, TG_C, TG_L, TG_X, TG_N };
constexpr uint32_t HDR_LDS_ENTRIES = 64;                // header spans kept in LDS; entries 64..255 overflow to the scratch slot
constexpr uint32_t HDR_OVF_BYTES = (ZKE_MAX_HEADERS - HDR_LDS_ENTRIES) * 16;
constexpr uint32_t PARSE_STAGE_BYTES = 3568;   // header blocks beyond this are read from HBM past the staged part

// ------------------------------------------------------------------ LDS image of one wave
constexpr uint32_t SEG_CAP = 40;       // tag-specs the lane-per-tag parse looks at: ZKE_MAX_TAGS + 1 decide everything
static_assert(SEG_CAP > ZKE_MAX_TAGS && SEG_CAP <= 64, "one lane per tag-spec");
struct ParseLds {
  uint32_t hdr[4 * HDR_LDS_ENTRIES];   // key_start, key_end, val_start, val_end of headers 0..127 (hdr_get / hdr_put)
  uint32_t tag[TG_N][4];               // raw_s, raw_e, val_off, val_len (last occurrence wins, as IndexMap::insert)
  uint8_t tagbuf[ZKE_MAX_TAGBUF];      // FWS-stripped tag values
  uint16_t seg[5][SEG_CAP];            // lane-per-tag parse: position of the k-th ';', and of tag-spec k: raw_s, raw_e, val_off, val_end
  __attribute__((aligned(16))) uint8_t stage[PARSE_STAGE_BYTES];   // head of the e-mail (header block), copied in 16-byte lanes
};
// Stage the head of the e-mail in LDS: every later scan of the header block (split, tag lists, canonicalisation) reads it there.
__device__ __forceinline__ void stage_head(Str& raw, ParseLds& L) {
  const uint32_t want = raw.len < PARSE_STAGE_BYTES ? raw.len : PARSE_STAGE_BYTES;
  stage_lds(L.stage, raw.base, want);
  // The staged pointer goes through an empty asm (two scalar registers, no instruction).  Where L is a static __shared__ object
  // (next_round, verdict.hip.h) the compiler carries it as the constant {offset, src_shared_base}; the host-sanitizer tests build the
  // engine with -O1 -g -fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer, and that build then ends with "Illegal
  // instruction detected: V_CMP_NE_U32_e32 0, $src_shared_base" at ldb's select between the staged head and the e-mail in HBM
  // (find_last in parse_email).  Without the sanitizer flags, and at -O3, the same source compiles.
  const uint8_t* staged = L.stage;
  asm volatile("" : "+s"(staged));
  raw.lds = staged; raw.lds_len = want;
}

// Header span table: 64 entries in LDS (10 KB of LDS per wave would cap a CU at 16 front-end waves; 6.7 KB lets the
// register budget decide: 24), the rest — e-mails with more than 64 header fields — in the e-mail's scratch slot.
// The overflow is written and read back by the same wave: the reads go around L1 (agent-scope atomic loads).
struct HdrSpan { uint32_t ks, ke, vs, ve; };
__device__ __forceinline__ void hdr_put(ParseLds& L, uint32_t* ovf, uint32_t x, uint32_t ks, uint32_t ke, uint32_t vs, uint32_t ve) {
  if (lane_id() != 0) return;
  uint32_t* p = x < HDR_LDS_ENTRIES ? L.hdr + 4 * x : ovf + 4 * (x - HDR_LDS_ENTRIES);
  p[0] = ks; p[1] = ke; p[2] = vs; p[3] = ve;
}
__device__ __forceinline__ HdrSpan hdr_get(const ParseLds& L, const uint32_t* ovf, uint32_t x) {
  if (x < HDR_LDS_ENTRIES) return HdrSpan{uni(L.hdr[4 * x]), uni(L.hdr[4 * x + 1]), uni(L.hdr[4 * x + 2]), uni(L.hdr[4 * x + 3])};
  const uint32_t* p = ovf + 4 * (x - HDR_LDS_ENTRIES);
  auto ld = [](const uint32_t* q) { return uni(__hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); };
  return HdrSpan{ld(p), ld(p + 1), ld(p + 2), ld(p + 3)};
}

// strip FWS from v[rs,re) into tagbuf at *tb; returns false on overflow
__device__ __forceinline__ bool strip_to_lds(ParseLds& L, const Str& v, uint32_t rs, uint32_t re, uint32_t& tb) {
  for (uint32_t base = rs; base < re; base += 64) {
    const uint32_t l = base + lane_id();
    const uint32_t c = l < re ? ldb(v, l) : OOB;
    const bool k = l < re && !is_fws(c);
    const uint64_t m = __ballot(k);
    const uint32_t cnt = (uint32_t)__builtin_popcountll(m);
    if (tb + cnt > ZKE_MAX_TAGBUF) return false;
    if (k) L.tagbuf[tb + (uint32_t)__builtin_popcountll(m & bits_below(lane_id()))] = (uint8_t)c;
    tb += cnt;
  }
  return true;
}
__device__ __forceinline__ uint32_t tagf(const ParseLds& L, int id, int k) { return uni(L.tag[id][k]); }    // k: 0 raw_s, 1 raw_e, 2 val_off, 3 val_len
// a tag's stripped value, first 16 bytes: lane l holds byte l; compared with literals without touching memory again
struct TagVal { uint32_t len, c; };
__device__ __forceinline__ TagVal tagval(const ParseLds& L, int id) {
  TagVal v{tagf(L, id, 3), 0};
  if ((uint32_t)lane_id() < v.len && lane_id() < 16) v.c = L.tagbuf[tagf(L, id, 2) + lane_id()];
  return v;
}
__device__ __forceinline__ bool operator==(const TagVal& v, const Lit& t) {
  if (v.len != t.n) return false;
  const uint32_t l = (uint32_t)lane_id();
  return __ballot(l < t.n && v.c != lit_at(t, l)) == 0;
}
__device__ __forceinline__ bool tagval_eq(const ParseLds& L, int id, const Lit& t) { return tagval(L, id) == t; }

// tag-spec = [FWS] tag-name [FWS] "=" [FWS] tag-value [FWS]   (cfdkim parser::tag_spec)
// returns the position after the spec, or NONE.  err: 0 ok, else ZKE_D_U_*
__device__ __forceinline__ uint32_t parse_tag_spec(ParseLds& L, const Str& v, Win& w, uint32_t pos, uint32_t& present,
                                                   uint32_t& ntags, uint32_t& tb, uint32_t& err) {
  const uint32_t n = v.len;
  uint32_t p = wfind(v, w, pos, n, [](uint32_t c) { return !is_fws(c); });
  if (p >= n || !is_alpha(at(v, w, p))) return NONE;
  const uint32_t ns = p;
  const uint32_t ne = wfind(v, w, p, n, [](uint32_t c) { return !is_alnumpunc(c); });
  p = wfind(v, w, ne, n, [](uint32_t c) { return !is_fws(c); });
  if (p >= n || at(v, w, p) != '=') return NONE;
  const uint32_t rs = wfind(v, w, p + 1, n, [](uint32_t c) { return !is_fws(c); });
  const uint32_t rend = wfind(v, w, rs, n, [](uint32_t c) { return !(is_valchar(c) || is_fws(c)); });
  uint32_t re = wrfind(v, w, rs, rend, [](uint32_t c) { return is_valchar(c); });
  re = (re == NONE) ? rs : re + 1;
  ntags++;
  if (ntags > ZKE_MAX_TAGS) { err = ZKE_D_U_TOO_MANY_TAGS; return rend; }
  // classify the name (case-sensitive, exact)
  int id = -1;
  const uint32_t c0 = at(v, w, ns);
  if (ne - ns == 1) {
    switch (c0) {
      case 'v': id = TG_V; break; case 'a': id = TG_A; break; case 'b': id = TG_B; break; case 'd': id = TG_D; break;
      case 'h': id = TG_H; break; case 's': id = TG_S; break; case 'i': id = TG_I; break; case 'q': id = TG_Q; break;
      case 'c': id = TG_C; break; case 'l': id = TG_L; break; case 'x': id = TG_X; break; default: break;
    }
  } else if (ne - ns == 2 && c0 == 'b' && at(v, w, ns + 1) == 'h') {
    id = TG_BH;
  }
  const uint32_t off = tb;
  if (!strip_to_lds(L, v, rs, re, tb)) { err = ZKE_D_U_SIG_TOO_LONG; return rend; }
  if (id >= 0) {
    if (lane_id() == 0) { L.tag[id][0] = rs; L.tag[id][1] = re; L.tag[id][2] = off; L.tag[id][3] = tb - off; }
    present |= 1u << id;
  }
  return rend;
}

// The tag list, serially: one tag-spec after the other, each scan 64 bytes wide (the later signature rounds inside the
// verdict launch, and whatever the lane-per-tag parse below hands back).  0, ZKE_D_SIG_SYNTAX or ZKE_D_U_*
__device__ __forceinline__ uint32_t taglist_serial(ParseLds& L, const Str& v, uint32_t& present) {
  Win w; w.wpos = WNONE; w.c = 0;
  uint32_t ntags = 0, tb = 0, err = 0;
  present = 0;
  if (wfind(v, w, 0, v.len, [](uint32_t c) { return c >= 0x80 && c != OOB; }) < v.len) return ZKE_D_U_SIG_NON_ASCII;
  uint32_t p = parse_tag_spec(L, v, w, 0, present, ntags, tb, err);
  if (p == NONE) return ZKE_D_SIG_SYNTAX;
  while (!err && p < v.len && at(v, w, p) == ';') {
    const uint32_t q = parse_tag_spec(L, v, w, p + 1, present, ntags, tb, err);
    if (q == NONE) break;
    p = q;
  }
  return err;
}

constexpr uint32_t TL_SERIAL = 0xFFFFFFF0u;      // "take taglist_serial"

// The tag list, one LANE per tag-spec.  A tag value holds no ';' (valchar excludes it), a name and FWS do not either,
// so the tag-specs are exactly the ';'-separated pieces of v — up to the first byte that is neither valchar, FWS nor
// ';': the value it sits in ends there and nothing behind it is parsed (parse_tag_list stops silently), which is the
// parse of v cut off at that byte.  Three steps:
//   1. 64 bytes of v per step: the ';' write their positions into seg[0] by rank; first bad byte; any byte >= 0x80;
//   2. lane k walks the head of piece k ([FWS] name [FWS] "=" [FWS]) and its tail (FWS in front of the ';') byte by
//      byte — a handful of bytes each, all pieces at once; the first piece that is no tag-spec ends the list;
//   3. 64 bytes per step again: a byte looks its piece up by the number of ';' in front of it and is kept when it lies
//      in the piece's value and is not FWS (compaction into tagbuf); the bytes at raw_s / raw_e - 1 note where the
//      stripped value begins and ends.
// A piece whose head or tail needs more than WALK_BUDGET steps (long runs of FWS, long names) hands the whole list to
// taglist_serial, as does a value of 64 KB or more.
constexpr uint32_t WALK_BUDGET = 40;
__device__ __forceinline__ uint32_t taglist_lanes(ParseLds& L, const Str& v, uint32_t& present) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t n = v.len;
  present = 0;
  if (n > 0xFFFFu) return TL_SERIAL;
  // ---- 1
  uint32_t nsemi = 0, neff = n;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t p = base + lane;
    const uint32_t c = ldb(v, p);                       // OOB behind the end
    if (__ballot(p < n && c >= 0x80)) return ZKE_D_U_SIG_NON_ASCII;
    if (base < neff) {
      const bool semi = c == ';';
      const uint64_t bm = __ballot(p < n && !(is_valchar(c) || is_fws(c) || semi));
      const uint32_t lim = bm ? (uint32_t)__builtin_ctzll(bm) : 64u;
      const uint64_t sm = __ballot(semi) & bits_below(lim);
      const uint32_t rank = nsemi + lanes_below(sm);
      if (semi && lane < lim && rank < SEG_CAP) L.seg[0][rank] = (uint16_t)p;
      nsemi += (uint32_t)__builtin_popcountll(sm);
      if (bm) neff = base + lim;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // ---- 2
  const uint32_t nseg = nsemi + 1 < SEG_CAP ? nsemi + 1 : SEG_CAP;
  const bool active = lane < nseg;
  uint32_t s = 0, e = neff;
  if (active) {
    if (lane > 0) s = (uint32_t)L.seg[0][lane - 1] + 1u;
    if (lane < nsemi) e = (uint32_t)L.seg[0][lane];
  }
  uint32_t budget = active ? WALK_BUDGET : 0u;
  uint32_t p = s, c = OOB;
  auto walk = [&](auto pred) {        // p: first position in [p, e) whose byte fails pred; c: that byte (OOB at e)
    for (;;) {
      c = (p < e && budget) ? ldb(v, p) : OOB;
      if (c == OOB || !pred(c)) break;
      p++; budget--;
    }
  };
  bool ok = active;
  walk([](uint32_t x) { return is_fws(x); });
  ok = ok && is_alpha(c);
  const uint32_t ns = p, c0 = c;
  if (ok) { p++; walk([](uint32_t x) { return is_alnumpunc(x); }); }
  const uint32_t nl = p - ns;
  uint32_t c1 = 0;
  if (ok && nl == 2) c1 = ldb(v, ns + 1);
  if (ok) walk([](uint32_t x) { return is_fws(x); });
  ok = ok && c == '=';
  if (ok) { p++; walk([](uint32_t x) { return is_fws(x); }); }
  const uint32_t rs = p;
  uint32_t re = e;
  if (ok) {
    for (;;) {                         // everything in [rs, e) is valchar or FWS: the last valchar is the last non-FWS
      if (!(re > rs && budget)) break;
      if (!is_fws(ldb(v, re - 1))) break;
      re--; budget--;
    }
  }
  if (__ballot(active && budget == 0)) return TL_SERIAL;
  const uint64_t nm = __ballot(active && !ok);
  const uint32_t T = nm ? (uint32_t)__builtin_ctzll(nm) : nseg;
  if (T == 0) return ZKE_D_SIG_SYNTAX;
  const uint32_t Tcap = T < ZKE_MAX_TAGS ? T : ZKE_MAX_TAGS;
  const bool mine = lane < Tcap;
  // the name (case-sensitive, exact); the last tag of a name wins (IndexMap::insert)
  int id = -1;
  if (mine && nl == 1) {
    switch (c0) {
      case 'v': id = TG_V; break; case 'a': id = TG_A; break; case 'b': id = TG_B; break; case 'd': id = TG_D; break;
      case 'h': id = TG_H; break; case 's': id = TG_S; break; case 'i': id = TG_I; break; case 'q': id = TG_Q; break;
      case 'c': id = TG_C; break; case 'l': id = TG_L; break; case 'x': id = TG_X; break; default: break;
    }
  } else if (mine && nl == 2 && c0 == 'b' && c1 == 'h') {
    id = TG_BH;
  }
  bool winner = false;
#pragma unroll
  for (int x = 0; x < TG_N; x++) {
    const uint64_t m = __ballot(id == x);
    if (m) { present |= 1u << x; winner = winner || (id == x && lane == 63u - (uint32_t)__builtin_clzll(m)); }
  }
  if (mine) { L.seg[1][lane] = (uint16_t)rs; L.seg[2][lane] = (uint16_t)(re > rs ? re : rs); L.seg[3][lane] = 0; L.seg[4][lane] = 0; }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // ---- 3
  uint32_t tb = 0, before = 0;         // bytes kept, ';' passed
  for (uint32_t base = 0; base < neff && before < Tcap; base += 64) {
    const uint32_t q = base + lane;
    const uint32_t b = q < neff ? ldb(v, q) : OOB;
    const uint64_t sm = __ballot(b == ';');
    const uint32_t k = before + lanes_below(sm);
    before += (uint32_t)__builtin_popcountll(sm);
    uint32_t vs = 0, ve = 0;
    if (k < Tcap) { vs = L.seg[1][k]; ve = L.seg[2][k]; }
    const bool keep = q >= vs && q < ve && !is_fws(b);
    const uint64_t km = __ballot(keep);
    const uint32_t d = tb + lanes_below(km);
    if (keep && d < ZKE_MAX_TAGBUF) {
      L.tagbuf[d] = (uint8_t)b;
      if (q == vs) L.seg[3][k] = (uint16_t)d;
      if (q + 1 == ve) L.seg[4][k] = (uint16_t)(d + 1);
    }
    tb += (uint32_t)__builtin_popcountll(km);
  }
  if (tb > ZKE_MAX_TAGBUF) return ZKE_D_U_SIG_TOO_LONG;
  if (T > ZKE_MAX_TAGS) return ZKE_D_U_TOO_MANY_TAGS;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (winner) {
    const uint32_t off = L.seg[3][lane], end = L.seg[4][lane];
    L.tag[id][0] = rs; L.tag[id][1] = re > rs ? re : rs; L.tag[id][2] = off; L.tag[id][3] = end - off;
  }
  return 0;
}

// cfdkim validate_header over the header value v.  0 = valid, else ZKE_D_* (ZKE_D_U_SIG_NON_ASCII: a byte >= 0x80 —
// from_utf8_lossy would rewrite it — is reported, never guessed)
// `strict`: ZKE_STRICT_* (zke_options' strictness flags: the readings of cfdkim that could not be verified offline); `now`: the
// time x= is compared with.
template <bool FAST>
__device__ __forceinline__ uint32_t validate_sig(ParseLds& L, const Str& v, uint32_t& present, uint32_t strict, uint64_t now) {
  uint32_t err = FAST ? taglist_lanes(L, v, present) : TL_SERIAL;
  if (err == TL_SERIAL) err = taglist_serial(L, v, present);
  if (err) return err;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint32_t req = (1u << TG_V) | (1u << TG_A) | (1u << TG_B) | (1u << TG_BH) | (1u << TG_D) | (1u << TG_H) | (1u << TG_S);
  if ((present & req) != req) return ZKE_D_MISSING_TAG;
  if (!tagval_eq(L, TG_V, LIT("1"))) return ZKE_D_INCOMPATIBLE_VERSION;
  if (present & (1u << TG_I)) {
    // STRICTNESS SITE i_must_be_subdomain (oracle: validate_header, same name).  Default: user.ends_with(signing_domain), a plain
    // suffix test on the bytes.  ZKE_STRICT_I_SUBDOMAIN: the domain of i= (behind its last '@'; the whole value without one)
    // equals d= or ends with "." d=, ASCII case folded (RFC 6376 §3.5 "same as or a subdomain of").
    const uint32_t il = tagf(L, TG_I, 3), dl = tagf(L, TG_D, 3), io = tagf(L, TG_I, 2), dofs = tagf(L, TG_D, 2);
    const bool sub = (strict & ZKE_STRICT_I_SUBDOMAIN) != 0;
    uint32_t dom_s = 0;                 // where the domain of i= starts (sub only)
    if (sub) {
      for (uint32_t o = 0; o < il; o += 64) {
        const uint32_t l = o + lane_id();
        const uint64_t m = __ballot(l < il && L.tagbuf[io + l] == '@');
        if (m) dom_s = o + 64u - (uint32_t)__builtin_clzll(m);
      }
    }
    if (il - dom_s < dl) return ZKE_D_DOMAIN_MISMATCH;
    bool bad = false;
    for (uint32_t o = 0; o < dl; o += 64) {
      const uint32_t l = o + lane_id();
      if (l < dl) {
        const uint32_t a = L.tagbuf[io + il - dl + l], b = L.tagbuf[dofs + l];
        bad |= sub ? lower(a) != lower(b) : a != b;
      }
    }
    if (__ballot(bad)) return ZKE_D_DOMAIN_MISMATCH;
    if (sub && il - dom_s > dl && uni(L.tagbuf[io + il - dl - 1]) != '.') return ZKE_D_DOMAIN_MISMATCH;
  }
  {   // h= must name "from" (split on ':', lower-cased)
    const uint32_t ho = tagf(L, TG_H, 2), hl = tagf(L, TG_H, 3);
    bool found = false;
    for (uint32_t o = 0; o < hl; o += 64) {
      const uint32_t l = o + lane_id();
      if (l + 4 <= hl) {
        const uint8_t* h = L.tagbuf + ho;
        const bool st = (l == 0) || h[l - 1] == ':';
        const bool en = (l + 4 == hl) || h[l + 4] == ':';
        found |= st && en && lower(h[l]) == 'f' && lower(h[l + 1]) == 'r' && lower(h[l + 2]) == 'o' && lower(h[l + 3]) == 'm';
      }
    }
    if (!__ballot(found)) return ZKE_D_FROM_NOT_SIGNED;
  }
  if ((present & (1u << TG_Q)) && !tagval_eq(L, TG_Q, LIT("dns/txt"))) return ZKE_D_BAD_QUERY_METHOD;
  if ((strict & ZKE_STRICT_EXPIRY_X) && (present & (1u << TG_X))) {
    // STRICTNESS SITE enforce_expiry_x (oracle: validate_header, same name).  Default: x= is ignored — a zkVM guest has no clock.
    // ZKE_STRICT_EXPIRY_X: cloudflare/dkim's rule — x= parsed as i64 (str::parse: optional sign, digits, no overflow; anything
    // else counts as 0), fifteen minutes of drift allowed, expired when now > x + 900.
    const uint8_t* xs = L.tagbuf + tagf(L, TG_X, 2);
    const uint32_t xn = tagf(L, TG_X, 3);
    uint32_t k = 0;
    bool neg = false, okx = xn > 0;
    if (okx) { const uint32_t c = uni(xs[0]); if (c == '+' || c == '-') { neg = c == '-'; k = 1; okx = xn > 1; } }
    uint64_t mag = 0;
    const uint64_t lim = neg ? (1ull << 63) : (1ull << 63) - 1;
    for (; okx && k < xn; k++) {
      const uint32_t c = uni(xs[k]);
      if (c < '0' || c > '9') { okx = false; break; }
      const uint64_t d = c - '0';
      if (mag > (lim - d) / 10) { okx = false; break; }
      mag = mag * 10 + d;
    }
    const int64_t x = okx ? (neg ? (int64_t)(0 - mag) : (int64_t)mag) : 0;
    const int64_t deadline = x > INT64_MAX - 900 ? INT64_MAX : x + 900;
    if ((int64_t)now > deadline) return ZKE_D_SIG_EXPIRED;
  }
  return 0;
}

// usize::from_str (optional '+', decimal digits, no overflow) on a stripped tag value
__device__ __forceinline__ bool parse_usize_tag(const ParseLds& L, int id, uint64_t& out) {
  const uint8_t* s = L.tagbuf + tagf(L, id, 2);
  const uint32_t n = tagf(L, id, 3);
  uint32_t i = 0;
  if (n && uni(s[0]) == '+') i = 1;
  if (i >= n) return false;
  uint64_t v = 0;
  for (; i < n; i++) {
    const uint32_t c = uni(s[i]);
    if (c < '0' || c > '9') return false;
    const uint64_t d = c - '0';
    if (v > (0xFFFFFFFFFFFFFFFFull - d) / 10) return false;
    v = v * 10 + d;
  }
  out = v;
  return true;
}

// ------------------------------------------------------------------ a validated signature against from_domain; its a=
// cfdkim compares d= and from_domain lower-cased as Unicode strings; d= is ASCII whenever a signature gets that far,
// so folding ASCII alone is exact unless from_domain holds U+212A KELVIN SIGN (to_lowercase() = "k", the one
// non-ASCII character with an ASCII lower case): reported (ZKE_D_U_DOMAIN_FOLD), never guessed
__device__ __forceinline__ bool domain_has_kelvin(const Str& dom) {
  bool kelvin = false;
  for (uint32_t base = 0; base + 2 < dom.len; base += 64) {
    const uint32_t o = base + (uint32_t)lane_id();
    kelvin = kelvin || (o + 2 < dom.len && ldb(dom, o) == 0xE2 && ldb(dom, o + 1) == 0x84 && ldb(dom, o + 2) == 0xAA);
  }
  return __ballot(kelvin) != 0;
}
// signing_domain.to_lowercase() == from_domain.to_lowercase(): the length first, then the ASCII fold
__device__ __forceinline__ bool sig_names_domain(const ParseLds& L, const Str& dom) {
  if (tagf(L, TG_D, 3) != dom.len) return false;
  bool bad = false;
  const uint32_t dofs = tagf(L, TG_D, 2);
  for (uint32_t o = 0; o < dom.len; o += 64) {
    const uint32_t l = o + (uint32_t)lane_id();
    if (l < dom.len) bad |= lower(L.tagbuf[dofs + l]) != lower(ldb(dom, l));
  }
  return __ballot(bad) == 0;
}
// a= (parser::parse_hash_algo; RFC 8463: ed25519-sha256 = SHA-256 hashes, Ed25519 signature) as ZKE_SIG_ALGO_*
__device__ __forceinline__ uint32_t sig_algo(const ParseLds& L) {
  const TagVal a = tagval(L, TG_A);
  return a == LIT("rsa-sha256") ? ZKE_SIG_ALGO_RSA_SHA256 : a == LIT("rsa-sha1") ? ZKE_SIG_ALGO_RSA_SHA1
       : a == LIT("ed25519-sha256") ? ZKE_SIG_ALGO_ED25519_SHA256 : ZKE_SIG_ALGO_OTHER;
}

}  // namespace zke
