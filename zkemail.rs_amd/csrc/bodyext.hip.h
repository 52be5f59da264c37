// bodyext.hip.h — extract_email_body (core/src/email.rs:7-23) for whole batches, one e-mail per wavefront like the front end:
// parse_mail, the choice among the message's DIRECT subparts (the first whose mimetype is text/html, else the first, else the
// message itself), that part's body_bytes, and its Content-Transfer-Encoding undone (get_body_raw: base64, quoted-printable,
// anything else as it is).  include/zkemail_amd.h states the rules; tests/body_model.py states them again with string operations.
//
// Step 1, parse: the header split and the MIME walk are the front end's own copies (hdrsplit.hip.h, mime.hip.h); the walk
// reports every part it accepts through its `part` argument, which the verify launches leave empty.  Verdicts and details are
// therefore the verify path's, byte for byte.
// Step 2, selection: mimetypes and the transfer encoding are decided by ballots over 64-byte windows (wfind, span_ieq, mime_trim).
// Step 3, the decode stream: FIXED-WIDTH steps of 64 bytes (one byte per lane) with carries, not line by line — lines of a
// quoted-printable body are 76 bytes by convention but nothing bounds them, a base64 body has no lines the decoder cares about,
// and a step that does not depend on where the lines end costs the same for every input.  The part's bytes are staged through LDS
// 1 KB at a time (16-byte loads); each step filters its 64 bytes (white space for base64, rule (a) for quoted-printable) into an
// LDS buffer by ballot and prefix count, and the decoder proper runs over that buffer:
//   base64   whole quads by b64_quad (keydec.hip.h, the one copy), 64 quads per round; the last two to five characters stay behind
//            until the stream ends, because only then is it known which quad is the last one (padding, trailing bits);
//   QP       windows of 62 characters with the next two in sight (an escape is three characters).  Per window, in masks: which '='
//            start an escape (a wave-uniform loop over the ballot of '='; one consumed by an earlier escape starts nothing, none
//            reaches across a line end), which white space trails its line (a carry chain from every LF downwards, solved by one
//            64-bit addition on the bit-reversed masks), soft breaks, the CRLF every normally ended line owes when a byte follows.
//            White space at the end of a window is written out as if it stayed, and `o_trim` remembers where the line's last other
//            character ended: a line end that turns up later moves the output position back there (and one further back over an
//            '=' that was a soft break after all).  So a run of white space of any length crosses any number of steps with two
//            words of state.
// No scratch: every loop-carried value is a wave-uniform scalar or one byte per lane.
//
// Output.  E-mail i's decoded bytes at bytes[rel ..), rel = raw_off[i] - raw_off[0]: its own raw length is room enough for every
// identity and base64 body.  A quoted-printable body whose lines end in lone LF grows by one byte per line (each becomes CRLF) and
// can outgrow the e-mail; what does not fit in the first raw_len bytes goes on at bytes[spill + rel ..), a second private place of
// the same size (decoded QP is at most twice its source).  No counter either way; the host compacts (host_stage.hip.h, body_compact).
#pragma once
#include "hdrsplit.hip.h"
#include "keydec.hip.h"
#include "parse.hip.h"       // ZKE_PARSE_WAVES: compiled for the front end's occupancy

namespace zke {

struct BodyArgs {
  uint32_t n, flags;                // ZKE_BODYF_*
  const uint8_t* raw; const uint64_t* raw_off;
  zke_body_info* infos;             // [n]; body_off = rel, reserved = the e-mail's raw length (the size of its first place): the host's
  uint8_t* bytes;
  uint64_t spill;                   // where the second places start, in `bytes`
  uint32_t* hdr_ovf;                // [n * HDR_OVF_BYTES / 4]: header spans 64..255 of each e-mail
};

constexpr uint32_t BODY_TILE = 1024;          // bytes of the part staged per round
constexpr uint32_t BODY_B64_ROUND = 256;      // characters decoded per round: 64 quads
constexpr uint32_t BODY_B64_BUF = BODY_B64_ROUND + 2 + 64 + 62;   // what can wait in the buffer (< 258) plus one step, rounded up
constexpr uint32_t BODY_QP_RING = 256;        // at most 63 characters wait, a step adds 64
constexpr uint32_t BODY_QP_WIN = 62;
static_assert(BODY_TILE + BODY_B64_BUF <= PARSE_STAGE_BYTES && BODY_TILE + BODY_QP_RING <= PARSE_STAGE_BYTES, "the decode buffers live in the staged head's LDS");

struct BodyPart { uint32_t ps, pe, ixb, fb; };     // raw[ps, pe), where its body starts, its first boundary line (a multipart that opened a frame) or NONE

__device__ __forceinline__ bool is_hex(uint32_t c) { return (c >= '0' && c <= '9') || ((c | 0x20) >= 'a' && (c | 0x20) <= 'f'); }
__device__ __forceinline__ uint32_t hex_val(uint32_t c) { return c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10; }

// parse_content_type(get_value(v)).mimetype == "text/html": the first ';'-token, trimmed, lower-cased.  (A line break inside the token
// unfolds to a space, at its ends it is trimmed either way: the raw bytes decide as the unfolded value would.)
__device__ __forceinline__ bool mime_is_text_html(const Str& v) {
  Win w; w.wpos = WNONE; w.c = 0;
  uint32_t s = 0, e = wfind(v, w, 0, v.len, [](uint32_t c) { return c == ';'; });
  mime_trim(v, w, s, e);
  return e - s == 9 && span_ieq(v, s, 9, LIT("text/html"));
}

__device__ __forceinline__ void body_email(const BodyArgs& A, const uint32_t i, ParseLds& L) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint64_t r0 = A.raw_off[i], r1 = A.raw_off[i + 1], rel = r0 - A.raw_off[0];
  const uint32_t cap = (uint32_t)(r1 - r0);
  auto finish = [&](uint32_t status, uint32_t detail, uint32_t part, uint32_t enc, uint32_t so, uint32_t sl, uint32_t blen) {
    const uint32_t v = lane == 0 ? status : lane == 1 ? detail : lane == 2 ? part : lane == 3 ? enc : lane == 4 ? so : lane == 5 ? sl
                     : lane == 6 ? blen : lane == 7 ? cap : lane == 8 ? (uint32_t)rel : (uint32_t)(rel >> 32);
    if (lane < 10) reinterpret_cast<uint32_t*>(A.infos + i)[lane] = v;
  };
  if (r1 - r0 >= (1ull << 31)) { finish(ZKE_UNSUPPORTED, ZKE_D_U_EMAIL_TOO_LARGE, 0, 0, 0, 0, 0); return; }
  Str raw = mkstr(A.raw + r0, cap);
  stage_head(raw, L);

  // ---- step 1: mailparse::parse_mail — the header list, then the MIME subparts, which report themselves
  uint32_t perr, hdr_end = 0, nh = 0;
  uint32_t* hdr_ovf = A.hdr_ovf + (size_t)i * (HDR_OVF_BYTES / 4);
  if (!split_headers_lines(L, hdr_ovf, raw, nh, perr, hdr_end)) nh = split_headers(L, hdr_ovf, raw, perr, hdr_end);
  if (nh == NONE) { finish(perr == ZKE_D_U_TOO_MANY_HEADERS ? ZKE_UNSUPPORTED : ZKE_PARSE_FAIL, perr, 0, 0, 0, 0, 0); return; }
  const HdrNames hn = hdr_names(L, nh);
  uint32_t ixb0 = hdr_end;                      // behind the empty line that ended the header list (mime_subparts)
  if (ixb0 < raw.len) ixb0 += (uni(ldb(raw, ixb0)) == '\r') ? 2u : 1u;
  // (the candidates as plain words, each assigned by a select: as structs assigned under the two tests they went through scratch)
  uint32_t top_fb = NONE, f_ps = 0, f_pe = 0, f_ixb = 0, f_fb = NONE, h_ps = 0, h_pe = 0, h_ixb = 0, h_fb = NONE;
  uint32_t n_children = 0, html_ix = 0;
  {
    uint32_t md = 0;
    const uint32_t mr = mime_subparts(L, hdr_ovf, raw, hn, nh, hdr_end, md,
        [&](uint32_t level, uint32_t ps, uint32_t pe, uint32_t ixb, bool ct, uint32_t cvs, uint32_t cve, uint32_t fb) {
          if (level == 0) { top_fb = fb; return; }
          if (level != 1) return;               // nested children are no candidates
          n_children++;
          const bool isf = n_children == 1;
          f_ps = isf ? ps : f_ps; f_pe = isf ? pe : f_pe; f_ixb = isf ? ixb : f_ixb; f_fb = isf ? fb : f_fb;
          const bool ish = !html_ix && ct && mime_is_text_html(substr(raw, cvs, cve));
          h_ps = ish ? ps : h_ps; h_pe = ish ? pe : h_pe; h_ixb = ish ? ixb : h_ixb; h_fb = ish ? fb : h_fb;
          html_ix = ish ? n_children : html_ix;
        });
    if (mr) { finish(mr, md, 0, 0, 0, 0, 0); return; }
  }

  // ---- step 2: the part and its body_bytes
  const BodyPart P{html_ix ? h_ps : n_children ? f_ps : 0u, html_ix ? h_pe : n_children ? f_pe : raw.len,
                   html_ix ? h_ixb : n_children ? f_ixb : ixb0, html_ix ? h_fb : n_children ? f_fb : top_fb};
  const uint32_t partno = html_ix ? (html_ix | 0x80000000u) : n_children ? 1u : 0u;
  const uint32_t so = P.ixb < P.pe ? P.ixb : P.pe;
  uint32_t end = P.fb != NONE ? P.fb : P.pe;
  // STRICTNESS SITE part_keeps_eol (tests/body_model.py, same name).  Default: an end that is a boundary line — a subpart's own end, the
  // end of a multipart's preamble — is moved back over the line break in front of that line.  ZKE_BODYF_PART_KEEPS_EOL: left alone.
  if ((P.fb != NONE || partno != 0) && !(A.flags & ZKE_BODYF_PART_KEEPS_EOL)) {
    if (end > so && uni(ldb(raw, end - 1)) == '\n') {
      end--;
      if (end > so && uni(ldb(raw, end - 1)) == '\r') end--;
    }
  }
  const uint32_t sl = end - so;

  // its first Content-Transfer-Encoding header: get_value, lower-cased, compared whole
  uint32_t enc = ZKE_CTE_IDENTITY;
  {
    const Str sub = substr(raw, P.ps, P.pe);
    uint32_t perr2 = 0, he2 = 0, vs = 0, ve = 0;
    bool have = false;
    (void)scan_headers(sub, perr2, he2, [&](uint32_t ix, uint32_t key_end, uint32_t s, uint32_t e) {
      if (!have && key_end - ix == 25 && span_ieq(sub, ix, 16, LIT("content-transfer")) && span_ieq(sub, ix + 16, 9, LIT("-encoding"))) { have = true; vs = s; ve = e; }
      return true;
    });
    if (have) {
      const Str v = substr(sub, vs, ve);
      if (mime_undecidable(v, 0, v.len)) { finish(ZKE_UNSUPPORTED, ZKE_D_U_BODY_CTE, partno, 0, so, sl, 0); return; }
      Win w; w.wpos = WNONE; w.c = 0;
      // a value of several lines unfolds to one with a space in it: neither name.  One line: trim_start, then the whole of it.
      if (wfind(v, w, 0, v.len, [](uint32_t c) { return c == '\n'; }) == v.len) {
        const uint32_t s = wfind(v, w, 0, v.len, [](uint32_t c) { return !rust_ws(c); });
        if (span_ieq(v, s, v.len - s, LIT("base64"))) enc = ZKE_CTE_BASE64;
        else if (span_ieq(v, s, v.len - s, LIT("quoted-printable"))) enc = ZKE_CTE_QP;
      }
    }
  }

  // ---- step 3: the decode stream.  Parsing is over: the staged head is dead, its LDS holds the tile and the decoder's buffer.
  const uint8_t* src = raw.base + so;
  uint8_t* const out0 = A.bytes + rel;
  uint8_t* const out1 = A.bytes + A.spill + rel;
  auto put = [&](uint32_t o, uint32_t v) { *(o < cap ? out0 + o : out1 + (o - cap)) = (uint8_t)v; };
  uint8_t* const tile = L.stage;
  uint8_t* const buf = L.stage + BODY_TILE;
  auto lds_sync = [] { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); };

  if (enc == ZKE_CTE_IDENTITY) {
    for (uint32_t base = 0; base < sl; base += 64) { const uint32_t l = base + lane; if (l < sl) out0[l] = src[l]; }      // sl <= cap
    finish(ZKE_OK, 0, partno, enc, so, sl, sl);
    return;
  }

  if (enc == ZKE_CTE_BASE64) {
    uint32_t t = 0, Q = 0;                       // characters waiting in buf, quads decoded
    bool badc = false;
    auto quads = [&](uint32_t from, uint32_t nq) {      // buf[from ..): nq <= 64 quads, none of them the last
      if (lane < nq) {
        const B64Quad d = b64_quad(buf + from, nq + 1, 0, lane);
        badc = badc || d.bad;
        uint8_t* dst = out0 + 3 * (size_t)(Q + lane);    // 3/4 of the part: inside the first place
        dst[0] = (uint8_t)(d.v >> 16); dst[1] = (uint8_t)(d.v >> 8); dst[2] = (uint8_t)d.v;
      }
      Q += nq;
    };
    for (uint32_t tb = 0; tb < sl; tb += BODY_TILE) {
      const uint32_t tn = sl - tb < BODY_TILE ? sl - tb : BODY_TILE;
      stage_lds(tile, src + tb, tn);
      for (uint32_t s = 0; s < tn; s += 64) {
        const uint32_t l = s + lane;
        const uint32_t c = l < tn ? (uint32_t)tile[l] : OOB;
        // u8::is_ascii_whitespace: HT LF FF CR SP — not VT
        const bool keep = l < tn && !(c == ' ' || c == '\t' || c == '\n' || c == '\f' || c == '\r');
        const uint64_t m = __ballot(keep);
        if (keep) buf[t + lanes_below(m)] = (uint8_t)c;
        t += (uint32_t)__builtin_popcountll(m);
        lds_sync();
        if (t >= BODY_B64_ROUND + 2) {           // two characters at least stay: whether they are padding shows at the end
          quads(0, 64);
          const uint32_t rem = t - BODY_B64_ROUND;       // <= 65
          const uint32_t v0 = lane < rem ? (uint32_t)buf[BODY_B64_ROUND + lane] : 0u, v1 = 64 + lane < rem ? (uint32_t)buf[BODY_B64_ROUND + 64 + lane] : 0u;
          lds_sync();
          if (lane < rem) buf[lane] = (uint8_t)v0;
          if (64 + lane < rem) buf[64 + lane] = (uint8_t)v1;
          lds_sync();
          t = rem;
        }
      }
    }
    // the end: t < 258 characters
    uint32_t from = 0;
    for (uint32_t left = t >= 2 ? (t - 2) / 4 : 0; left;) { const uint32_t nq = left < 64 ? left : 64; quads(from, nq); from += 4 * nq; left -= nq; }
    const uint32_t r = t - from;                 // 0 (nothing at all), 1 (one character in all), or 2..5
    const uint32_t pad = (r >= 1 && uni(buf[t - 1]) == '=') ? ((r >= 2 && uni(buf[t - 2]) == '=') ? 2u : 1u) : 0u;
    if (lane < r - pad) badc = badc || b64v(buf[from + lane]) > 63;
    uint32_t detail = 0, total = 3 * Q;
    if (__ballot(badc)) detail = ZKE_D_BODY_B64_CHAR;
    else if (r % 4) detail = ZKE_D_BODY_B64_LENGTH;
    else if (r == 4) {
      const B64Quad d = b64_quad(buf + from, 1, pad, 0);      // every lane the same quad
      if (d.bad) detail = ZKE_D_BODY_B64_TRAILING_BITS;
      else {
        if (lane < d.nb) out0[3 * (size_t)Q + lane] = (uint8_t)(d.v >> (16 - 8 * lane));
        total += d.nb;
      }
    }
    if (detail) finish(ZKE_BODY_DECODE_FAIL, detail, partno, enc, so, sl, 0);
    else finish(ZKE_OK, 0, partno, enc, so, sl, total);
    return;
  }

  // quoted_printable::decode(.., Robust)
  uint32_t h = 0, t = 0;                         // ring: head, characters waiting
  uint32_t o = 0, o_trim = 0;                    // output position; where the current line's last character that is no white space ended
  bool la_eq = false;                            // ... and that character is an '=' that started an escape (written out as it is so far)
  uint32_t skip_in = 0;                          // characters at the head an escape of the previous window consumed
  bool sup_in = false;                           // ... and decoded: they are not written
  for (uint32_t tb = 0; tb < sl; tb += BODY_TILE) {
    const uint32_t tn = sl - tb < BODY_TILE ? sl - tb : BODY_TILE;
    stage_lds(tile, src + tb, tn);
    for (uint32_t s = 0; s < tn; s += 64) {
      {
        const uint32_t l = s + lane;
        const uint32_t c = l < tn ? (uint32_t)tile[l] : OOB;
        const bool keep = l < tn && (c == '\t' || c == '\r' || c == '\n' || (c >= 0x20 && c <= 0x7e));      // rule (a)
        const uint64_t m = __ballot(keep);
        if (keep) buf[(h + t + lanes_below(m)) & (BODY_QP_RING - 1)] = (uint8_t)c;
        t += (uint32_t)__builtin_popcountll(m);
        lds_sync();
      }
      const bool fin = tb + s + 64 >= sl;        // nothing follows what the ring holds
      while (t >= 64 || (fin && t)) {
        const uint32_t Pn = fin ? (t < BODY_QP_WIN ? t : BODY_QP_WIN) : BODY_QP_WIN;       // not final: two characters behind the window at least
        const bool in = lane < Pn;
        const uint32_t c0 = lane < t ? (uint32_t)buf[(h + lane) & (BODY_QP_RING - 1)] : OOB;
        const uint32_t c1 = lane + 1 < t ? (uint32_t)buf[(h + lane + 1) & (BODY_QP_RING - 1)] : OOB;
        const uint32_t c2 = lane + 2 < t ? (uint32_t)buf[(h + lane + 2) & (BODY_QP_RING - 1)] : OOB;
        const uint64_t WIN = bits_below(Pn);
        const uint64_t NL = __ballot(in && c0 == '\n'), T = __ballot(in && (c0 == ' ' || c0 == '\t' || c0 == '\r')), E = __ballot(in && c0 == '=');
        const uint64_t N1 = __ballot(c1 == '\n' || c1 == OOB), N2 = __ballot(c2 == '\n' || c2 == OOB), HX = __ballot(is_hex(c1) && is_hex(c2));
        // (i) which '=' start an escape: in order, each consuming the (at most two) characters of its line behind it
        uint64_t ACT = 0;
        uint32_t cu = skip_in;
        bool lastdec = sup_in;
        for (uint64_t m = E; m; m &= m - 1) {
          const uint32_t p = (uint32_t)__builtin_ctzll(m);
          if (p < cu) continue;
          ACT |= 1ull << p;
          cu = p + (((N1 >> p) & 1) ? 1u : ((N2 >> p) & 1) ? 2u : 3u);
          lastdec = (HX >> p) & 1;
        }
        const uint64_t D = ACT & HX;                                        // rule (f): one byte for three
        const uint64_t SUP = (((D << 1) | (D << 2)) | (sup_in ? bits_below(skip_in) : 0ull)) & WIN;
        // (ii) white space that trails its line: every run that reaches an LF, found from the LF downwards
        uint64_t TR;
        {
          const uint64_t rT = __builtin_bitreverse64(T), rN = __builtin_bitreverse64(NL), x = rT | rN;
          TR = __builtin_bitreverse64(((x + rN) ^ x) & rT);
        }
        const bool joins = ((TR | NL) & 1) != 0;                            // the line that ends first ends with what the earlier windows left open
        if (joins) o = o_trim - (la_eq ? 1u : 0u);
        // (iii) soft breaks: an escape's '=' as the last character of its trimmed line; its LF owes nothing
        const uint64_t SOFT = ACT & ((TR | NL) >> 1);
        uint64_t NLS;
        { const uint64_t y = TR | SOFT; NLS = ((y + SOFT) ^ y) & NL; }
        if (joins && la_eq) NLS |= NL & (0 - NL);
        const uint64_t lastnl = (fin && Pn == t) ? (1ull << (Pn - 1)) : 0ull;       // the stream's last byte: no line follows it
        const uint64_t M2 = NL & ~NLS & ~lastnl;                            // rule (h): CRLF
        const uint64_t M1 = WIN & ~NL & ~TR & ~SUP & ~SOFT;
        const uint32_t off = o + lanes_below(M1) + 2 * lanes_below(M2);
        if ((M1 >> lane) & 1) put(off, ((D >> lane) & 1) ? (hex_val(c1) << 4 | hex_val(c2)) : c0);
        if ((M2 >> lane) & 1) { put(off, '\r'); put(off + 1, '\n'); }
        // the state behind the window
        auto upto = [&](uint32_t q) { const uint64_t b = bits_below(q + 1); return (uint32_t)__builtin_popcountll(M1 & b) + 2 * (uint32_t)__builtin_popcountll(M2 & b); };
        const uint64_t open_line = NL ? bits_from(64 - (uint32_t)__builtin_clzll(NL)) : ~0ull;
        const uint64_t NW = WIN & ~T & ~NL & open_line;
        if (NW) {
          const uint32_t q = 63 - (uint32_t)__builtin_clzll(NW);
          o_trim = o + upto(q);
          la_eq = ((ACT & ~D) >> q) & 1;
        } else if (NL) {
          o_trim = o + upto(63 - (uint32_t)__builtin_clzll(NL));
          la_eq = false;
        }
        o += (uint32_t)__builtin_popcountll(M1) + 2 * (uint32_t)__builtin_popcountll(M2);
        skip_in = cu > Pn ? cu - Pn : 0;
        sup_in = lastdec;
        h = (h + Pn) & (BODY_QP_RING - 1);
        t -= Pn;
      }
    }
  }
  // the end of the input ends the last line: its trailing white space goes, and a soft break's '='
  o = o_trim - (la_eq ? 1u : 0u);
  finish(ZKE_OK, 0, partno, enc, so, sl, o);
}

__global__ __launch_bounds__(64, ZKE_PARSE_WAVES) void body_extract_kernel(BodyArgs A) {
  __shared__ ParseLds L[1];
  const uint32_t email = blockIdx.x;
  if (email >= A.n) return;
  body_email(A, email, L[0]);
}

}  // namespace zke
