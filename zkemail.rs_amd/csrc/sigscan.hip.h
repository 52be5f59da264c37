// sigscan.hip.h — the DKIM-Signature scan: the first step of the reference's input generation
// (helpers/src/generator.rs:17-30), one e-mail per wavefront like the front end and built from the front end's own helpers
// (hdrsplit.hip.h: the header split, the MIME subpart walk, the DKIM-Signature fields; taglist.hip.h: validate_sig, the
// ASCII-folded d= / from_domain comparison, a=).
//
// Per e-mail: parse_mail, then EVERY header field named DKIM-Signature in file order gets one record — its validate_header
// verdict, whether d= names from_domain, a= classified, the FWS-stripped s= value, the span of the header's value.  No key is
// read, no SHA or RSA job is written; EmailMeta, the result records and the slot's verify workspace are not touched (the
// overflow of the header span table has an area of its own), so a scan and a verification may share a slot back to back.
//
// Output.  status[4 * i ..] = {status, detail, n_signatures, n_candidates}; the first max_sigs records of e-mail i at
// recs[i * max_sigs ..] (the host compacts them into the CSR while it copies them out: no serial pass on the device); the
// selectors in sel_blob, each placed by ONE agent-scope atomic add on *sel_used (the blob's order is unspecified: a string is
// (sel_off, sel_len) and nothing else).  A selector that does not fit is not written, the counter still advances: the host
// reads the size a second call needs from it.
#pragma once
#include "hdrsplit.hip.h"
#include "parse.hip.h"       // ZKE_PARSE_WAVES: the scan is compiled for the front end's occupancy

namespace zke {

struct SigScanArgs {
  uint32_t n, max_sigs;
  const uint8_t* raw; const uint64_t* raw_off;
  const uint8_t* dom; const uint64_t* dom_off;
  uint32_t strict;                  // ZKE_STRICT_*, exactly as validate_sig takes them
  uint64_t now;
  uint32_t* status;                 // [4 n]
  zke_sig_info* recs;               // [n * max_sigs]
  uint8_t* sel_blob; uint32_t sel_cap;
  uint32_t* sel_used;               // zero at launch
  uint32_t* hdr_ovf;                // [n * HDR_OVF_BYTES / 4]: header spans 64..255 of each e-mail
};

__device__ __forceinline__ void sigscan_email(const SigScanArgs& A, const uint32_t i, ParseLds& L) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint64_t r0 = A.raw_off[i], r1 = A.raw_off[i + 1];
  auto finish = [&](uint32_t status, uint32_t detail, uint32_t nsig, uint32_t ncand) {
    const uint32_t v = lane == 0 ? status : lane == 1 ? detail : lane == 2 ? nsig : ncand;
    if (lane < 4) A.status[4 * (size_t)i + lane] = v;
  };
  if (r1 - r0 >= (1ull << 31)) { finish(ZKE_UNSUPPORTED, ZKE_D_U_EMAIL_TOO_LARGE, 0, 0); return; }
  Str raw = mkstr(A.raw + r0, (uint32_t)(r1 - r0));
  stage_head(raw, L);
  const Str dom = mkstr(A.dom + A.dom_off[i], (uint32_t)(A.dom_off[i + 1] - A.dom_off[i]));

  // ---- mailparse::parse_mail: the header list, then the MIME subparts
  uint32_t perr, hdr_end = 0, nh = 0;
  uint32_t* hdr_ovf = A.hdr_ovf + (size_t)i * (HDR_OVF_BYTES / 4);
  if (!split_headers_lines(L, hdr_ovf, raw, nh, perr, hdr_end)) nh = split_headers(L, hdr_ovf, raw, perr, hdr_end);
  if (nh == NONE) { finish(perr == ZKE_D_U_TOO_MANY_HEADERS ? ZKE_UNSUPPORTED : ZKE_PARSE_FAIL, perr, 0, 0); return; }
  const HdrNames hn = hdr_names(L, nh);
  {
    uint32_t md = 0;
    const uint32_t mr = mime_subparts(L, hdr_ovf, raw, hn, nh, hdr_end, md);
    if (mr) { finish(mr, md, 0, 0); return; }
  }
  if (domain_has_kelvin(dom)) { finish(ZKE_UNSUPPORTED, ZKE_D_U_DOMAIN_FOLD, 0, 0); return; }      // the d= comparison below folds ASCII alone

  // ---- every DKIM-Signature header, file order.  (The walk is written out here; through next_sig_header, as parse_email takes it,
  // sigscan_kernel alone measured 2 % longer: profiles/frontend_shared_bench_ab.txt.)
  uint32_t sig_ix = 0, n_cand = 0;
  const uint64_t sig_len_mask = __ballot(hn.nl == 14u);
  for (uint32_t hx = 0; hx < nh; hx++) {
    if (hx < 64 && !((sig_len_mask >> hx) & 1)) continue;
    const HdrSpan hs = hdr_get(L, hdr_ovf, hx);
    if (!span_ieq(raw, hs.ks, hs.ke - hs.ks, LIT("dkim-signature"))) continue;
    const uint32_t this_ix = sig_ix++;
    const Str v = substr(raw, hs.vs, hs.ve);
    uint32_t present;
    uint32_t code = validate_sig<true>(L, v, present, A.strict, A.now);
    uint32_t algo = 0, sel_off = 0, sel_len = 0;
    if (code == 0) {
      if (sig_names_domain(L, dom)) n_cand++; else code = ZKE_D_NEUTRAL;
      algo = sig_algo(L);
      if (this_ix < A.max_sigs) {
        sel_len = tagf(L, TG_S, 3);                       // <= ZKE_MAX_TAGBUF
        if (sel_len) {
          uint32_t at = 0;
          if (lane == 0) at = atomicAdd(A.sel_used, sel_len);
          sel_off = uni(at);
          if (sel_off <= A.sel_cap && sel_len <= A.sel_cap - sel_off) {
            const uint8_t* s = L.tagbuf + tagf(L, TG_S, 2);
            for (uint32_t o = lane; o < sel_len; o += 64) A.sel_blob[sel_off + o] = s[o];
          }
        }
      }
    }
    if (this_ix < A.max_sigs) {
      const uint32_t w = lane == 0 ? hx : lane == 1 ? code : lane == 2 ? algo : lane == 3 ? sel_off : lane == 4 ? sel_len
                       : lane == 5 ? hs.vs : lane == 6 ? hs.ve : 0u;
      if (lane < 8) reinterpret_cast<uint32_t*>(A.recs + (size_t)i * A.max_sigs + this_ix)[lane] = w;
    }
  }
  finish(ZKE_OK, 0, sig_ix, n_cand);
}

__global__ __launch_bounds__(64, ZKE_PARSE_WAVES) void sigscan_kernel(SigScanArgs A) {
  __shared__ ParseLds L[1];
  const uint32_t email = blockIdx.x;
  if (email >= A.n) return;
  sigscan_email(A, email, L[0]);
}

}  // namespace zke
