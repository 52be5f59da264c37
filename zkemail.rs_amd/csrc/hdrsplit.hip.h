// hdrsplit.hip.h — mailparse 0.15.0 parse_mail over the top-level message, as the verify path (parse.hip.h) and the signature
// scan (sigscan.hip.h) run it: the header split into the wave's span table (line-parallel inside the staged head, serial
// beyond it), cfdkim's get_body, the walk over the MIME subparts behind the first Content-Type header (mime.hip.h), and the
// walk over the header fields named DKIM-Signature.
#pragma once
#include "taglist.hip.h"

namespace zke {

// ------------------------------------------------------------------ mailparse header split
// parse_headers / parse_header over `raw`: sink(ix, key_end, vs, ve) for every header field (false = stop: too many).
// Returns the header count or NONE with perr set; hdr_end = where the list stopped (the empty line, or the end).
template <class Sink>
__device__ __forceinline__ uint32_t scan_headers(const Str& raw, uint32_t& perr, uint32_t& hdr_end, Sink sink) {
  Win w; w.wpos = WNONE; w.c = 0;
  const uint32_t len = raw.len;
  uint32_t ix = 0, nh = 0;
  perr = 0;
  for (;;) {
    if (ix >= len) break;
    const uint32_t c0 = at(raw, w, ix);
    if (c0 == '\n') break;
    if (c0 == '\r') {
      if (ix + 1 < len && at(raw, w, ix + 1) == '\n') break;
      perr = ZKE_D_HDR_LONE_CR;
      return NONE;
    }
    if (c0 == ' ') { perr = ZKE_D_HDR_LEADING_SPACE; return NONE; }
    uint32_t key_end, vs, ve, next;
    const uint32_t p = wfind(raw, w, ix, len, [](uint32_t c) { return c == ':' || c == '\n'; });
    if (p >= len) {
      key_end = len; vs = ve = len; next = len;
    } else if (at(raw, w, p) == '\n') {
      key_end = p; vs = ve = p; next = p + 1;
    } else {
      key_end = p;
      vs = wfind(raw, w, p + 1, len, [](uint32_t c) { return c != ' '; });
      // header end: first LF at q >= vs whose successor is not SP / HTAB (or which ends the input)
      uint32_t q = vs;
      for (;;) {
        q = wfind(raw, w, q, len, [](uint32_t c) { return c == '\n'; });
        if (q >= len) break;
        const uint32_t nx = (q + 1 < len) ? at(raw, w, q + 1) : OOB;
        if (nx == ' ' || nx == '\t') { q++; continue; }
        break;
      }
      next = (q < len) ? q + 1 : len;
      const uint32_t lim = (q < len) ? q : len;
      const uint32_t lastv = wrfind(raw, w, vs, lim, [](uint32_t c) { return c != '\r' && c != '\n'; });
      ve = (lastv == NONE) ? vs : lastv + 1;
    }
    if (!sink(ix, key_end, vs, ve)) { perr = ZKE_D_U_TOO_MANY_HEADERS; return NONE; }
    nh++;
    ix = next;
  }
  hdr_end = ix;
  return nh;
}
// Fills L.hdr; returns the header count or NONE with perr set.
__device__ __forceinline__ uint32_t split_headers(ParseLds& L, uint32_t* ovf, const Str& raw, uint32_t& perr, uint32_t& hdr_end) {
  uint32_t nh = 0;
  const uint32_t r = scan_headers(raw, perr, hdr_end, [&](uint32_t ix, uint32_t key_end, uint32_t vs, uint32_t ve) {
    if (nh >= ZKE_MAX_HEADERS) return false;
    hdr_put(L, ovf, nh, ix, key_end, vs, ve);
    nh++;
    return true;
  });
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return r;
}

// The same split for a header block that lies inside the staged head (every ordinary e-mail), LINE-parallel: the serial
// form walked the block header by header with a handful of dependent single-byte LDS reads each (2.5 k of the front end's
// 9 k scalar instructions per e-mail, 22 % of its cycles).
//   pass A, 64 bytes per step: ballots of LF and ':'; every LF lane stores its position under its line number, every
//   lane holding the FIRST ':' of its line stores that; stops at the first empty line (LF followed by LF or CRLF), which
//   ends the header list whatever the state (an empty line never starts with SP / HTAB).
//   pass B, 64 lines per step, one lane per line: W = the line starts with SP / HTAB, C = it holds a ':'.  "Inside a
//   value after line i" is V[i] = C[i] | (W[i] & V[i-1]) — a carry chain, solved for all 64 lines by ONE 64-bit addition
//   (a = W | C, b = C: carry into bit i+1 = V[i]).  Line i continues a header iff W[i] & V[i-1]; every other line starts
//   one (or is an error: SP first, CR not followed by LF).  A header's lane stores key and value start, the lane of its
//   last line (the next line does not continue it) stores the value end.
// Returns false when it does not apply — no empty line inside the staged part, or more than LINE_CAP lines before it —
// and the caller runs split_headers above.
constexpr uint32_t LINE_CAP = ZKE_MAX_TAGBUF / 4;      // two u16 tables in the (still unused) tag buffer
__device__ __forceinline__ bool split_headers_lines(ParseLds& L, uint32_t* ovf, const Str& raw, uint32_t& nh_out, uint32_t& perr,
                                                    uint32_t& hdr_end) {
#ifdef ZKE_NO_LINE_SPLIT
  return false;
#endif
  const uint32_t len = raw.len, staged = raw.lds_len;
  const uint32_t lane = (uint32_t)lane_id();
  uint16_t* lfpos = (uint16_t*)L.tagbuf;               // line g = [g ? lfpos[g-1] + 1 : 0, lfpos[g]]
  uint16_t* colpos = lfpos + LINE_CAP;                 // its first ':' (0xFFFF: none)
  perr = 0;
  auto sb = [&](uint32_t pos) -> uint32_t { return pos < staged ? (uint32_t)L.stage[pos] : OOB; };
  if (len == 0) { nh_out = 0; hdr_end = 0; return true; }
  {
    const uint32_t c0 = uni(sb(0)), c1 = uni(sb(1));
    if (c0 == '\n' || (c0 == '\r' && c1 == '\n')) { nh_out = 0; hdr_end = 0; return true; }     // the list is empty
  }
  // ---- pass A
  uint32_t n_lines = 0, cut = NONE;
  bool colon_seen = false;                             // the line that runs into this chunk already holds a ':'
  if (lane == 0) colpos[0] = 0xFFFF;
  for (uint32_t base = 0; base < staged; base += 64) {
    const uint32_t l = base + lane;
    const uint32_t c = sb(l), n1 = sb(l + 1), n2 = sb(l + 2);
    uint64_t Lm = __ballot(c == '\n'), Cm = __ballot(c == ':');
    const uint64_t Bm = __ballot(c == '\n' && (n1 == '\n' || (n1 == '\r' && n2 == '\n')));
    uint32_t cutbit = 64;
    if (Bm) { cutbit = (uint32_t)__builtin_ctzll(Bm); Lm &= bits_below(cutbit + 1); Cm &= bits_below(cutbit); }
    const uint32_t line = n_lines + lanes_below(Lm);             // the line this byte lies in (its LF closes it)
    if ((Lm >> lane) & 1) {
      if (line < LINE_CAP) lfpos[line] = (uint16_t)l;
      if (line + 1 < LINE_CAP) colpos[line + 1] = 0xFFFF;
    }
    // "no ':' yet in this line" in front of every byte: a carry chain — an LF generates, a ':' kills, everything else passes
    // it on — solved by one 64-bit addition (a = generate | propagate = ~Cm, b = generate = Lm; the carry INTO bit i is sum ^ a ^ b)
    const uint64_t ca = ~Cm, cb = Lm, cin = colon_seen ? 0ull : 1ull;
    const uint64_t sum = ca + cb + cin;
    const uint64_t F = Cm & (sum ^ ca ^ cb);                       // the first ':' of each line
    if (((F >> lane) & 1) && line < LINE_CAP) colpos[line] = (uint16_t)l;
    colon_seen = (((ca & cb) | ((ca | cb) & ~sum)) >> 63) == 0;    // no carry out: a ':' behind the chunk's last LF
    n_lines += (uint32_t)__builtin_popcountll(Lm);
    if (Bm) { cut = base + cutbit; break; }
  }
  if (cut == NONE || n_lines > LINE_CAP) return false;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // ---- pass B
  uint32_t nh = 0;
  uint64_t vcarry = 0;                                 // inside a value after the previous group's last line
  for (uint32_t G = 0; G < n_lines; G += 64) {
    const uint32_t g = G + lane;
    const bool valid = g < n_lines;
    uint32_t s = 0, e = 0, c0 = OOB, c1 = OOB, col = 0xFFFF, nx = OOB;
    if (valid) {
      s = g ? (uint32_t)lfpos[g - 1] + 1u : 0u;
      e = lfpos[g];
      c0 = L.stage[s]; c1 = L.stage[s + 1];            // a line in front of the first empty one holds a byte besides its LF
      col = colpos[g];
      nx = L.stage[e + 1];                             // staged: pass A read it
    }
    const bool W = c0 == ' ' || c0 == '\t', C = col != 0xFFFF;
    const uint64_t VM = __ballot(valid), Wm = __ballot(valid && W), Cm = __ballot(valid && C);
    const uint64_t a = Wm | Cm, b = Cm;
    const uint64_t Vprev = (a + b + vcarry) ^ a ^ b;   // bit i: inside a value after line i - 1
    const uint64_t cont = Wm & Vprev;
    const uint64_t HS = VM & ~cont;                    // lines that start a header
    const bool hs = (HS >> lane) & 1;
    const uint64_t below = bits_below(lane);
    const uint32_t hr = nh + (uint32_t)__builtin_popcountll(HS & below);
    const uint64_t bad = (HS & __ballot(valid && (c0 == ' ' || (c0 == '\r' && c1 != '\n')))) | __ballot(hs && hr >= ZKE_MAX_HEADERS);
    if (bad) {                                         // the first one in line order, as the serial walk meets them
      const uint32_t f = (uint32_t)__builtin_ctzll(bad);
      const uint32_t fc = __builtin_amdgcn_readlane(c0, f);
      // (a header-start line whose first byte is CR is not followed by LF: that would be the empty line)
      perr = fc == ' ' ? ZKE_D_HDR_LEADING_SPACE : fc == '\r' ? ZKE_D_HDR_LONE_CR : ZKE_D_U_TOO_MANY_HEADERS;
      nh_out = NONE;
      return true;
    }
    if (hs) {
      uint32_t ke = e, vs = e;
      if (C) { ke = col; vs = col + 1; while (L.stage[vs] == ' ') vs++; }      // ends at the line's LF at the latest
      uint32_t* p = hr < HDR_LDS_ENTRIES ? L.hdr + 4 * hr : ovf + 4 * (hr - HDR_LDS_ENTRIES);
      p[0] = s; p[1] = ke; p[2] = vs;
      if (!C) p[3] = e;                                // a line without ':' is a key with an empty value
    }
    const bool inval = hs ? C : true;                  // inside a value after this line
    if (valid && inval && !(nx == ' ' || nx == '\t')) {   // the last line of a header with a value: strip trailing CR / LF
      uint32_t q = e;
      while (q > s) { const uint32_t t = L.stage[q - 1]; if (t != '\r' && t != '\n') break; q--; }
      const uint32_t h = nh + (uint32_t)__builtin_popcountll(HS & bits_below(lane + 1)) - 1u;
      uint32_t* p = h < HDR_LDS_ENTRIES ? L.hdr + 4 * h : ovf + 4 * (h - HDR_LDS_ENTRIES);
      p[3] = q;
    }
    nh += (uint32_t)__builtin_popcountll(HS);
    vcarry = ((Cm >> 63) & 1) | (((Wm >> 63) & 1) & ((Vprev >> 63) & 1));
  }
  hdr_end = cut + 1;                                   // the empty line
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  nh_out = nh;
  return true;
}

// cfdkim get_body: everything after the first CRLFCRLF (empty when there is none).
// `from`: a position no CRLFCRLF starts in front of.  After split_headers that is hdr_end - 2: bytes p..p+3 =
// CRLFCRLF make p+2 a line start that begins with CRLF (the LF at p+1 cannot continue a folded line: CR follows),
// and the header split stops at the first such line start, so p + 2 >= hdr_end.
__device__ __forceinline__ uint32_t find_body(const Str& raw, uint32_t from) {
  const uint32_t len = raw.len;
  for (uint32_t base = from; base + 4 <= len; base += 61) {
    const uint32_t c = ldb(raw, base + lane_id());
    const uint64_t r = __ballot(c == '\r'), n = __ballot(c == '\n');
    uint64_t m = r & (n >> 1) & (r >> 2) & (n >> 3) & bits_below(61);
    if (m) return base + (uint32_t)__builtin_ctzll(m) + 4;
  }
  return len;
}

}  // namespace zke
#include "mime.hip.h"      // a subpart's header block goes through scan_headers above
namespace zke {

// ------------------------------------------------------------------ header fields by name
// lane x: where header field x's name starts and how long it is (fields 0..63; later ones are looked up one by one)
struct HdrNames { uint32_t ks, nl; };
__device__ __forceinline__ HdrNames hdr_names(const ParseLds& L, uint32_t nh) {
  HdrNames hn{0, NONE};
  const uint32_t lane = (uint32_t)lane_id();
  if (lane < nh && lane < HDR_LDS_ENTRIES) { hn.ks = L.hdr[4 * lane]; hn.nl = L.hdr[4 * lane + 1] - hn.ks; }
  return hn;
}

// Still parse_mail: the MIME subparts of the top-level message (mime.hip.h).  Its first Content-Type header decides — fields
// 0..63 tested by name length first, all at once, the later ones one by one.  Returns mime_walk's status (0: nothing wrong,
// or no Content-Type at all) with its `detail`.  The walk's stack is the tag buffer: not in use yet.  `part`: mime.hip.h, MimeNoParts
// (a message without a Content-Type header never reaches the walk: no call at all, it is a leaf).
template <class Parts = MimeNoParts>
__device__ __forceinline__ uint32_t mime_subparts(ParseLds& L, const uint32_t* hdr_ovf, const Str& raw, const HdrNames& hn, uint32_t nh,
                                                  uint32_t hdr_end, uint32_t& detail, Parts part = Parts()) {
  bool has_ct = false;
  uint32_t cvs = 0, cve = 0;
  for (uint64_t m = __ballot(hn.nl == 12u); m; m &= m - 1) {
    const uint32_t x = (uint32_t)__builtin_ctzll(m);
    if (span_ieq(raw, __builtin_amdgcn_readlane(hn.ks, x), 12, LIT("content-type"))) { const HdrSpan hs = hdr_get(L, hdr_ovf, x); has_ct = true; cvs = hs.vs; cve = hs.ve; break; }
  }
  for (uint32_t x = HDR_LDS_ENTRIES; !has_ct && x < nh; x++) {
    const HdrSpan hs = hdr_get(L, hdr_ovf, x);
    if (span_ieq(raw, hs.ks, hs.ke - hs.ks, LIT("content-type"))) { has_ct = true; cvs = hs.vs; cve = hs.ve; }
  }
  if (!has_ct) return 0;
  uint32_t ixb = hdr_end;                      // behind the empty line that ended the header list
  if (ixb < raw.len) ixb += (uni(ldb(raw, ixb)) == '\r') ? 2u : 1u;
  return mime_walk((uint32_t*)L.tagbuf, raw, ixb, true, cvs, cve, detail, part);
}

// The first header field at or after hx that is named DKIM-Signature, its spans in hs; NONE when there is none.  Only a
// 14-byte name can be one: fields 0..63 are passed over by name length without a look at their bytes.
__device__ __forceinline__ uint32_t next_sig_header(const ParseLds& L, const uint32_t* hdr_ovf, const Str& raw, const HdrNames& hn, uint32_t nh,
                                                    uint32_t hx, HdrSpan& hs) {
  const uint64_t sig_len_mask = __ballot(hn.nl == 14u);
  for (; hx < nh; hx++) {
    if (hx < 64 && !((sig_len_mask >> hx) & 1)) continue;
    hs = hdr_get(L, hdr_ovf, hx);
    if (span_ieq(raw, hs.ks, hs.ke - hs.ks, LIT("dkim-signature"))) return hx;
  }
  return NONE;
}

}  // namespace zke
