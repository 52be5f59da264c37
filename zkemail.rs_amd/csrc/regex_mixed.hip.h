// regex_mixed.hip.h — the regex stage of a batch whose e-mails carry DIFFERENT regex configs (zke_verify_emails_mixed;
// core/src/circuits.rs:31-68 takes one EmailWithRegex at a time, each with its own RegexInfo).  regex.hip.h's launches give
// blockIdx.y a part of the batch's one list and make lane or wave i of the grid e-mail i; here a block is told which e-mails and
// which automaton it owns by the host plan's segment table (mixed_plan.hip.h): one segment per (config, part), the config's
// e-mails a range of the permutation `perm`.  ONE lane-mapped and ONE wave-mapped launch per batch, whatever the number of
// configs and parts; the walk itself is regex.hip.h's (dfa_stage, dfa_part, dfa_chunk_map), the verdict its fold.
#pragma once
#include "regex.hip.h"
#include "mixed_plan.hip.h"

namespace zke {

struct DfaMixedArgs {
  DfaArgs common;               // b, the haystacks, the capture tables (indexed by job), out [J]; re / part / is_body / ... come from the segment
  const MixedSeg* segs;         // this launch's segments, block ranges ascending
  uint32_t n_segs;
  const uint32_t* perm;
  const uint32_t* job_off;      // [n + 1]
};

// The segment that owns block `block`: the first whose block_end lies beyond it (segments without e-mails have no blocks and are
// never found); nullptr past the last segment.  Wave-uniform: every operand is.
__device__ __forceinline__ const MixedSeg* mixed_find_seg(const MixedSeg* segs, uint32_t n_segs, uint32_t block) {
  uint32_t lo = 0, hi = n_segs;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (segs[mid].block_end > block) hi = mid; else lo = mid + 1;
  }
  return lo < n_segs ? segs + lo : nullptr;
}
// The segment's automaton as the DfaArgs dfa_stage / dfa_part read.
__device__ __forceinline__ DfaArgs mixed_seg_args(const DfaMixedArgs& MA, const MixedSeg* S) {
  DfaArgs A = MA.common;
  A.re = reinterpret_cast<const RegexDev*>(S->re);
  A.is_body = S->is_body; A.lds_tables = S->lds_tables; A.idle = S->idle; A.decode_detail = S->decode_detail;
  return A;
}
// (e-mail, part) -> PartRes, as dfa_kernel / dfa_wave_kernel compute it without `finalize`.  dfa_part looks the captures up at
// cap_off[i * P + part]: with P = 0 and part = the job index that is cap_off[job].
__device__ __forceinline__ PartRes mixed_part(DfaArgs A, const DfaLds& F, const DfaLds& Rv, bool valid, uint32_t i, uint32_t job, bool wave, int lane) {
  const EmailMeta* M = A.b.meta + i;
  PartRes pr{PART_SKIPPED, 0, 0, 0};
  if (M->state != ST_CAND) return pr;
  if (!valid) { pr.code = PART_DECODE_FAIL; pr.count = A.decode_detail; return pr; }
  A.P = 0; A.part = job;
  const uint8_t* hay; uint32_t hlen;
  dfa_haystack(A, i, M, hay, hlen);
  return dfa_part(A, F, Rv, i, hay, hlen, wave ? dfa_chunk_map(F, hay, hlen, A.idle, lane) : DfaAccel{0, 0, 0, false});
}

// blockDim = 256; one e-mail per lane.  Dynamic LDS: as dfa_kernel, sized for the launch's largest segment.
__global__ __launch_bounds__(256) void dfa_mixed_kernel(DfaMixedArgs MA) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dlds[];
  const MixedSeg* S = mixed_find_seg(MA.segs, MA.n_segs, blockIdx.x);
  if (!S) return;                                  // (the whole block: nobody is left alone at dfa_stage's barrier)
  const DfaArgs A = mixed_seg_args(MA, S);
  DfaLds F{}, Rv{};
  const bool valid = dfa_stage(A, dlds, F, Rv);
  const uint32_t k = (blockIdx.x - S->block0) * MIXED_LANE_BLOCK + threadIdx.x;
  if (k >= S->count) return;
  const uint32_t i = MA.perm[S->first + k];
  const uint32_t job = MA.job_off[i] + S->part;
  A.out[job] = mixed_part(A, F, Rv, valid, i, job, false, 0);
}

// One e-mail per WAVE (blockDim = 256: four e-mails share the staged tables), with dfa_wave_kernel's clean-chunk pre-pass.
__global__ __launch_bounds__(256) void dfa_mixed_wave_kernel(DfaMixedArgs MA) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dlds[];
  const MixedSeg* S = mixed_find_seg(MA.segs, MA.n_segs, blockIdx.x);
  if (!S) return;
  const DfaArgs A = mixed_seg_args(MA, S);
  DfaLds F{}, Rv{};
  const bool valid = dfa_stage(A, dlds, F, Rv);
  const uint32_t k = (blockIdx.x - S->block0) * MIXED_WAVE_BLOCK + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= S->count) return;
  const uint32_t i = MA.perm[S->first + k];
  const uint32_t job = MA.job_off[i] + S->part;
  const PartRes pr = mixed_part(A, F, Rv, valid, i, job, true, lane);
  if (lane == 0) A.out[job] = pr;
}

// The verdict: one thread per e-mail folds its own P_i parts with its own config's n_header_parts (regex_fold_begin /
// regex_fold_part: header parts, then body parts, stop at the first failing one).  An e-mail without a config keeps the record
// verify_email left: it is neither read nor written.
struct RegexFoldMixedArgs { BatchDev b; const PartRes* parts; const uint32_t* job_off; const uint32_t* email_cfg; };
__global__ void regex_fold_mixed_kernel(RegexFoldMixedArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.b.n) return;
  const uint32_t cfg = A.email_cfg[i];
  if (cfg == MIXED_CFG_NONE) return;
  zke_result* R = A.b.results + i;
  RegexFold fold = regex_fold_begin(R, A.b.meta + i);
  const uint32_t j0 = A.job_off[i], P = A.job_off[i + 1] - j0, nh = cfg & MIXED_CFG_NH_MASK;
  for (uint32_t p = 0; p < P; p++) regex_fold_part(fold, R, p, nh, A.parts[(size_t)j0 + p]);
}

// The preparation (regex_prep_email), one e-mail per wave: e-mails without a config are left out — the mode-1 parse never runs for
// them, so nothing of it can reach their records —, and the cleaned body is produced for the e-mails whose own config has body parts.
struct PrepMixedArgs { PrepArgs prep; const uint32_t* email_cfg; };
__global__ __launch_bounds__(64, ZKE_PARSE_WAVES) void regex_prep_mixed_kernel(PrepMixedArgs A) {
  __shared__ ParseLds L;
  const uint32_t i = blockIdx.x;
  if (i >= A.prep.parse.b.n) return;
  const uint32_t cfg = A.email_cfg[i];
  if (cfg == MIXED_CFG_NONE) return;
  regex_prep_email(A.prep, i, L, (A.prep.want_clean || (cfg & MIXED_CFG_HAS_BODY)) ? 1u : 0u);
}

}  // namespace zke
