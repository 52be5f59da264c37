// qpmap.hip.h — the second return value of remove_quoted_printable_soft_breaks (core/src/email.rs:61-86): index_map, the
// position in the body as it was signed of every byte the filter keeps.
//   * qp_index_kernel (zke_qp_clean_batch): the reference function over plain bodies, both return values, one body per wave.
//     The ballot formulation of qp_wave (regex.hip.h) — the 3-byte pattern "=\r\n" as shifted ballots, 1 or 2 dropped bytes
//     carried into the next 64-byte step, the popcount-prefix rank — with the lane's source position stored beside the byte.
//   * capture_origin_kernel (zke_extract_captures_mapped): where the spans an extraction reports in the QP-cleaned canonical
//     body lie in the canonical body itself (the bytes bh= is the hash of).  No map is materialised: a span asks for two
//     entries of it, so the wave walks the body once with the keep-mask ballots and answers the e-mail's queries on the way.
// qp_wave and regex_prep_kernel are not touched: the verify path never needs the map (circuits.rs:37 discards it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capture.hip.h"

namespace zke {

constexpr uint32_t QP_NO_INDEX = ZKE_QP_NO_INDEX;

// The keep mask of the 64-byte step at `base` of an n-byte body: bit l set = byte base + l is kept.  `carry`: how many leading
// bytes of this step belong to a "=\r\n" begun in the previous one (in: this step's, out: the next step's).  c: the lane's byte.
__device__ __forceinline__ uint64_t qp_keep_mask(const uint8_t* src, uint32_t n, uint32_t base, int lane, uint32_t& carry, uint32_t& c) {
  const uint32_t l = base + lane;
  c = l < n ? src[l] : OOB;
  const uint32_t c1 = l + 1 < n ? src[l + 1] : OOB, c2 = l + 2 < n ? src[l + 2] : OOB;
  const uint64_t D = __ballot(c == '=' && c1 == '\r' && c2 == '\n');
  uint64_t drop = D | (D << 1) | (D << 2);
  if (carry == 2) drop |= 3; else if (carry == 1) drop |= 1;
  carry = (D >> 63) ? 2u : ((D >> 62) & 1 ? 1u : 0u);
  return __ballot(l < n && !((drop >> lane) & 1));
}

// ---- zke_qp_clean_batch ------------------------------------------------------------------------------------------------
// Body i = blob[off[i] - off[0] .. off[i + 1] - off[0]); cleaned and index_map are laid out by the same rebased offsets.  Any of
// the three outputs may be null.  The host bounds the grid; each wave loops over its bodies.
struct QpIndexArgs { uint32_t n; const uint8_t* blob; const uint64_t* off; uint8_t* cleaned; uint32_t* index_map; uint32_t* clean_len; };

__global__ __launch_bounds__(64) void qp_index_kernel(QpIndexArgs A) {
  const int lane = lane_id();
  const uint64_t off0 = A.off[0];
  for (uint32_t i = blockIdx.x; i < A.n; i += gridDim.x) {
    const uint64_t at = A.off[i] - off0;
    const uint32_t n = (uint32_t)(A.off[i + 1] - A.off[i]);
    const uint8_t* src = A.blob + at;
    uint8_t* dst = A.cleaned ? A.cleaned + at : nullptr;
    uint32_t* im = A.index_map ? A.index_map + at : nullptr;
    uint32_t o = 0, carry = 0;
    for (uint32_t base = 0; base < n; base += 64) {
      uint32_t c;
      const uint64_t Km = qp_keep_mask(src, n, base, lane, carry, c);
      if ((Km >> lane) & 1) {
        const uint32_t to = o + (uint32_t)__builtin_popcountll(Km & bits_below(lane));
        if (dst) dst[to] = (uint8_t)c;
        if (im) im[to] = base + lane;
      }
      o += (uint32_t)__builtin_popcountll(Km);
    }
    for (uint32_t l = o + lane; l < n; l += 64) {      // email.rs:79-84: both padded back to the original length
      if (dst) dst[l] = 0;
      if (im) im[l] = QP_NO_INDEX;
    }
    if (lane == 0 && A.clean_len) A.clean_len[i] = o;
  }
}

// ---- zke_extract_captures_mapped ---------------------------------------------------------------------------------------
// position of the r-th set bit of m (r < popcount(m))
__device__ __forceinline__ uint32_t qp_select(uint64_t m, uint32_t r) {
  uint32_t w = (uint32_t)m, pos = 0;
  uint32_t cnt = (uint32_t)__builtin_popcount(w);
  if (r >= cnt) { r -= cnt; pos = 32; w = (uint32_t)(m >> 32); }
#pragma unroll
  for (uint32_t h = 16; h; h >>= 1) {
    cnt = (uint32_t)__builtin_popcount(w & ((1u << h) - 1));
    if (r >= cnt) { r -= cnt; pos += h; w >>= h; }
  }
  return pos;
}

constexpr uint32_t ORG_MAX_QUERIES = 2 * CAP_MAX_PARTS * ZKE_CAP_MAX_GROUPS;       // two map entries per body-part group
constexpr uint32_t ORG_SLOTS = ORG_MAX_QUERIES / 64;                               // queries per lane

struct CapOriginArgs {
  uint32_t n, G, gb0;             // gb0: the first body-part column among the e-mail's G (= the header parts' groups)
  DfaArgs d;                      // b (the canonicalize pass's view), scratch_v: as the DFA launches had them
  const zke_result* results;
  const uint32_t* spans;          // [n * G * 2] as capture_gather_kernel left them
  uint32_t* org_spans;            // [n * G * 2]
  uint8_t* org_flags;             // [n * G]
};

// One wave per e-mail, behind the gather launch (capture_origin_kernel here; capture_origin_mixed_kernel, capture_mixed.hip.h, with
// the e-mail's own column range).  Header columns and e-mails without strings keep their pair, flags 0.  For
// the body columns of an e-mail whose record is ZKE_OK, with im = the index map of the e-mail's regex haystack (the canonical
// body regex_prep_kernel feeds to qp_wave, n bytes) and {s, e} the span:
//     start = s < n ? im[s] : NO_INDEX;   end = e == s ? start : (im[e - 1] == NO_INDEX ? NO_INDEX : im[e - 1] + 1)
// Query k of the e-mail (k = 2 * body column + {0: s, 1: e - 1}) belongs to lane k & 63, slot k >> 6: a column's two queries sit
// in neighbouring lanes of one slot.
// The origins of one e-mail by one wave: its G columns start at column `row`, the body parts' at row + gb0; ok: its record is ZKE_OK.
__device__ __forceinline__ void cap_origin_email(const DfaArgs& d, uint32_t i, size_t row, uint32_t G, uint32_t gb0, bool ok, const uint32_t* spans,
                                                 uint32_t* org_spans, uint8_t* org_flags, int lane) {
  const uint32_t ident_to = ok ? gb0 : G;          // columns [0, ident_to): origin = span
  for (uint32_t c = lane; c < ident_to; c += 64) {
    org_spans[2 * (row + c)] = spans[2 * (row + c)];
    org_spans[2 * (row + c) + 1] = spans[2 * (row + c) + 1];
    org_flags[row + c] = 0;
  }
  if (!ok) return;
  const uint32_t Gb = G - gb0;
  const uint32_t slots = (2 * Gb + 63) / 64;
  // the haystack before the QP filter: the src / n choice of regex_prep_kernel, read from what that pass left in its EmailMeta
  const BatchDev& B = d.b;
  const EmailMeta* M = B.meta + i;
  const uint64_t r0 = B.raw_off[i];
  const uint32_t raw_len = (uint32_t)(B.raw_off[i + 1] - r0);
  const uint32_t n = M->hashed_len;
  const uint8_t* src = M->body_src_is_raw ? B.raw + r0 + M->body_off
                     : (M->reuse ? region_b(d.scratch_v, d.scratch_v_off, i, raw_len) : region_b(B.scratch, B.scratch_off, i, raw_len));
  uint32_t q[ORG_SLOTS], res[ORG_SLOTS];
#pragma unroll
  for (uint32_t j = 0; j < ORG_SLOTS; j++) {
    q[j] = QP_NO_INDEX; res[j] = QP_NO_INDEX;
    const uint32_t k = j * 64 + lane, c = k >> 1;
    if (j < slots && c < Gb) {
      const uint32_t s = spans[2 * (row + gb0 + c)], e = spans[2 * (row + gb0 + c) + 1];
      if (!(k & 1)) q[j] = s;
      else if (e > s && e != CAP_NONE) q[j] = e - 1;
    }
  }
  uint32_t o = 0, carry = 0;
  for (uint32_t base = 0; base < n; base += 64) {
    uint32_t c;
    const uint64_t Km = qp_keep_mask(src, n, base, lane, carry, c);
    const uint32_t cnt = (uint32_t)__builtin_popcountll(Km);
#pragma unroll
    for (uint32_t j = 0; j < ORG_SLOTS; j++)
      if (j < slots && q[j] - o < cnt) res[j] = base + qp_select(Km, q[j] - o);      // (o <= q < o + cnt; an unasked slot holds NO_INDEX)
    o += cnt;
  }
  // queries at or beyond the final o kept NO_INDEX.  Even lanes hold a column's start, their odd neighbours its last byte.
#pragma unroll
  for (uint32_t j = 0; j < ORG_SLOTS; j++) {
    if (j >= slots) break;
    const uint32_t k = j * 64 + lane, c = k >> 1;
    const uint32_t last = (uint32_t)__shfl_xor((int)res[j], 1);                       // even lanes: im[e - 1]
    if (!(k & 1) && c < Gb) {
      const size_t col = row + gb0 + c;
      const uint32_t s = spans[2 * col], e = spans[2 * col + 1];
      uint32_t start = res[j], end = e == s ? start : (last == QP_NO_INDEX ? QP_NO_INDEX : last + 1);
      uint8_t flag = 0;
      if (s == CAP_NONE && e == CAP_NONE) { start = s; end = e; }                     // no string: the pair stands
      else if (start == QP_NO_INDEX || end == QP_NO_INDEX) flag = ZKE_ORGF_PADDING;
      else if (end - start != e - s) flag = ZKE_ORGF_SPLIT;
      org_spans[2 * col] = start; org_spans[2 * col + 1] = end;
      org_flags[col] = flag;
    }
  }
}

__global__ __launch_bounds__(64) void capture_origin_kernel(CapOriginArgs A) {
  const int lane = lane_id();
  const uint32_t i = blockIdx.x;
  if (i >= A.n) return;
  cap_origin_email(A.d, i, (size_t)i * A.G, A.G, A.gb0, A.results[i].status == ZKE_OK, A.spans, A.org_spans, A.org_flags, lane);
}

}  // namespace zke
