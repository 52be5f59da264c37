// capture_mixed.hip.h — capture extraction behind the regex stage of a batch whose e-mails carry DIFFERENT regex configs
// (zke_extract_captures_mixed): what capture.hip.h / qpmap.hip.h do for one part list per batch, over ragged jobs and columns.
// E-mail i's part p is job job_off[i] + p, requested group k of it column col_off[i] + gbase[p] + k (mixed_plan.hip.h); the parts'
// programs and groups come from a config-major CapPartDev table in the staged image (at most 64 x 16 entries: it does not fit kernel
// arguments), found through the e-mail's config {first part, header parts, G, first body column}.  The walk, the fold, the scans,
// the gather and the origin queries are capture.hip.h's and qpmap.hip.h's device routines; only the index arithmetic lives here.
// A job is mapped to its e-mail by a binary search of job_off, a column by one of col_off: the operands of the first are
// wave-uniform (one wave per job), the second runs once per column in the gather's last pass.
#pragma once
#include "capture.hip.h"
#include "qpmap.hip.h"
#include "mixed_plan.hip.h"

namespace zke {

static_assert(CAPMIX_MAX_PARTS == CAP_MAX_PARTS && CAPMIX_MAX_PARTS == ZKE_CAP_MAX_PARTS && CAPMIX_MAX_GROUPS == ZKE_CAP_MAX_GROUPS &&
              CAPMIX_MAX_COLUMNS * ZKE_CAP_MAX_SPAN == (1ull << 32), "mixed_plan.hip.h restates the capture limits");

// The tables of a mixed extraction in the slot's staged image.
struct CapMixedTables {
  const uint32_t* job_off;      // [n + 1]
  const uint32_t* col_off;      // [n + 1]
  const uint32_t* cap_cfg;      // [n] config index or MIXED_NONE
  const CapMixedCfg* cfgs;      // [n_configs]
  const CapPartDev* part;       // config-major part table (gbase: the part's first column among its config's G)
};
// The e-mail that owns entry `x` of a ragged range: the first i with off[i + 1] > x (x < off[n]; e-mails without entries are never found).
__device__ __forceinline__ uint32_t capmix_owner(const uint32_t* off, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid + 1] > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

struct CapMixedArgs {
  uint32_t n, J;
  DfaArgs d;                    // b, scratch_v, clean ... as the mixed DFA launches had them
  CapMixedTables t;
  const PartRes* parts;         // [J]
  uint32_t* spans;              // [Gt * 2]
  uint8_t* flags;               // [Gt]
  uint32_t* codes;              // [J]
  uint64_t* work;               // [waves * CAP_WORK_WORDS]
};

// One wave per job; the host bounds the grid (CAP_WORK_WAVES when ANY part of ANY config keeps its rows in the workspace) and each
// wave loops.  blockDim = 64.  Everything that selects the item's e-mail, config and part is wave-uniform.
__global__ __launch_bounds__(64) void capture_mixed_kernel(CapMixedArgs A) {
  __shared__ uint64_t lds_rows[CAP_ROWS * CAP_LDS_WORDS];
  const int lane = threadIdx.x;
  for (uint32_t item = blockIdx.x; item < A.J; item += gridDim.x) {
    const uint32_t i = capmix_owner(A.t.job_off, A.n, item), p = item - A.t.job_off[i];
    const CapMixedCfg cf = A.t.cfgs[A.t.cap_cfg[i]];
    const CapPartDev& part = A.t.part[cf.part0 + p];
    cap_item(part, A.parts[item],
             [&](const uint8_t*& hay, uint32_t& hlen) { DfaArgs D = A.d; D.is_body = p >= cf.nh ? 1u : 0u; dfa_haystack(D, i, A.d.b.meta + i, hay, hlen); },
             lds_rows, A.work, A.spans, A.flags, (size_t)A.t.col_off[i], A.codes, item, lane);
  }
}

// The tables in the form zke_verify_emails_mixed takes (cap_off [J + 1], cap_str_off, cap_blob) and the capture verdict folded into
// the records: per e-mail over its own P_i parts with its own n_header_parts.  capture_gather_kernel's shape — ONE workgroup of 1024
// threads: lengths -> exclusive scan -> gather — and its routines.  E-mails without a config own no job and no column and are skipped.
struct CapGatherMixedArgs {
  uint32_t n, J, Gt;
  DfaArgs d;
  CapMixedTables t;
  const PartRes* parts; const uint32_t* codes; uint32_t* spans;
  zke_result* results;
  uint32_t* cap_off;            // [J + 1]
  uint32_t* cap_str_off;        // [Gt + 1]
  uint8_t* cap_blob; uint64_t blob_cap;
  uint64_t* hdr;
  uint32_t* tmp;                // [J + Gt] scratch: strings per job, bytes per column
};
__global__ __launch_bounds__(1024) void capture_gather_mixed_kernel(CapGatherMixedArgs A) {
  __shared__ uint64_t sh[1025];
  const uint32_t T = blockDim.x, t = threadIdx.x;
  uint32_t* nstr = A.tmp;                              // [J]
  uint32_t* nbytes = A.tmp + A.J;                      // [Gt]
  for (uint32_t i = t; i < A.n; i += T) {
    const uint32_t c = A.t.cap_cfg[i];
    if (c == MIXED_NONE) continue;
    const CapMixedCfg cf = A.t.cfgs[c];
    const uint32_t j0 = A.t.job_off[i], P = A.t.job_off[i + 1] - j0;
    const bool ok = cap_fold_email(A.results + i, A.parts + j0, A.codes + j0, P, cf.nh);
    for (uint32_t p = 0; p < P; p++) {
      const CapPartDev& pd = A.t.part[cf.part0 + p];
      const size_t col = (size_t)A.t.col_off[i] + pd.gbase;
      cap_part_lengths(ok, pd.n_groups, nstr + j0 + p, nbytes + col, A.spans + 2 * col);
    }
  }
  __syncthreads();
  const uint64_t strings = cap_block_scan(nstr, A.J, sh);
  for (size_t k = t; k < A.J; k += T) A.cap_off[k] = nstr[k];
  if (t == 0) A.cap_off[A.J] = (uint32_t)strings;
  const uint64_t bytes = cap_block_scan(nbytes, A.Gt, sh);
  if (t == 0) { A.hdr[0] = strings; A.hdr[1] = bytes; }
  // strings in column order: the column's e-mail by col_off, its part through the config's gbase, string index = cap_off[job] + (c - gbase[p])
  for (uint32_t col = t; col < A.Gt; col += T) {
    const uint32_t i = capmix_owner(A.t.col_off, A.n, col), c = col - A.t.col_off[i];
    const CapMixedCfg cf = A.t.cfgs[A.t.cap_cfg[i]];
    const uint32_t j0 = A.t.job_off[i], P = A.t.job_off[i + 1] - j0;
    uint32_t p = 0;
    while (p + 1 < P && c >= A.t.part[cf.part0 + p + 1].gbase) p++;
    const uint32_t first = A.cap_off[j0 + p], cnt = A.cap_off[j0 + p + 1] - first;
    if (!cnt) continue;
    cap_put_string(first + (c - A.t.part[cf.part0 + p].gbase), nbytes[col], A.spans[2 * (size_t)col], A.spans[2 * (size_t)col + 1], strings, bytes,
                   A.cap_str_off, A.cap_blob, A.blob_cap, [&]() -> const uint8_t* {
                     const uint8_t* hay; uint32_t hlen;
                     DfaArgs D = A.d; D.is_body = p >= cf.nh ? 1u : 0u;
                     dfa_haystack(D, i, A.d.b.meta + i, hay, hlen);
                     return hay;
                   });
  }
  if (t == 0 && strings == 0) A.cap_str_off[0] = 0;
}

// A mapped extraction's origins (capture_origin_kernel's queries, qpmap.hip.h): one wave per e-mail over the e-mail's own column
// range with its config's first body column.  E-mails without a config return at once; a config none of whose body parts asks for
// a group has nothing to ask the index map (its origins are its spans).
struct CapOriginMixedArgs {
  uint32_t n;
  DfaArgs d;
  CapMixedTables t;
  const zke_result* results;
  const uint32_t* spans;        // [Gt * 2] as capture_gather_mixed_kernel left them
  uint32_t* org_spans;          // [Gt * 2]
  uint8_t* org_flags;           // [Gt]
};
__global__ __launch_bounds__(64) void capture_origin_mixed_kernel(CapOriginMixedArgs A) {
  const int lane = lane_id();
  const uint32_t i = blockIdx.x;
  if (i >= A.n) return;
  const uint32_t c = A.t.cap_cfg[i];
  if (c == MIXED_NONE) return;
  const CapMixedCfg cf = A.t.cfgs[c];
  const bool ok = A.results[i].status == ZKE_OK && cf.G > cf.gb0;
  cap_origin_email(A.d, i, A.t.col_off[i], cf.G, cf.gb0, ok, A.spans, A.org_spans, A.org_flags, lane);
}

}  // namespace zke
