// verdict.hip.h — the last launch of a signature round: the Ed25519 stage and the verdict of every e-mail.
//
// One wave per 16 e-mails.  First, four lanes per e-mail (ed25519.hip.h), what ed25519_email_kernel did as a launch of its
// own: the curve-point check of every 32-byte Ed25519 key (round 0; DkimPublicKey::try_from_bytes, core/src/email.rs:28-29)
// and the Ed25519 verification of a=ed25519-sha256 candidates over the SHA-256 header hash — waves without an Ed25519 e-mail
// skip it after one byte load per lane.  Then a lane per e-mail writes the verdict (verdict_lane, canon.hip.h): base64(body hash)
// against bh=, the digest bytes the RSA role left in EmailMeta against the header hash (rsa 0.9.6 pkcs1v15 verify),
// status / detail, the pending counter of the next signature round.  One launch instead of two: with many batches in
// flight every launch of a batch costs the chip's command processor several microseconds whatever it does.
#pragma once
#include "ed25519.hip.h"
#include "rsa_kernel.hip.h"

namespace zke {

struct EdVerdictArgs {
  FinArgs fin; uint32_t skip_ed;
  uint32_t* wave_count;      // the hash / modexp stage's job list is consumed: reset for the next batch
  KeyCacheEntry* cache;      // later signature rounds: per-key Montgomery constants
  uint8_t* em_out;           // parity intermediates (nullptr in production)
  uint32_t strict;           // ZKE_STRICT_* and the x= clock, for the front end of later signature rounds
  uint64_t now;
  uint32_t* wave_feedback;   // pinned host word of the slot: how long the wave-routine job list of this batch was (sizes the next
                             // batch's walkers: stage_plan.hip.h, plan_stage); nullptr: nobody listens
};

// SHA-256 / SHA-1 of one message by ONE LANE (later signature rounds only: two messages per e-mail, a rare path; the
// batched kernels of sha256.hip.h are the hot one).  FIPS 180-4; the digest goes to j.dst as the batch kernels write it.
__device__ __forceinline__ void sha_lane(const ShaJob& j) {
  if (!j.dst) return;
  const uint8_t* src = (const uint8_t*)j.src;
  const uint32_t len = j.len, nblk = (len + 9 + 63) >> 6;
  uint32_t st[8];
  sha_init_state(st, j.pad != 0);
  typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
  for (uint32_t b = 0; b < nblk; b++) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const uint32_t o = 64 * b + 4 * k;
      uint32_t v;
      if (o + 4 <= len) v = __builtin_bswap32(*(const u32_unaligned*)(src + o));
      else {
        v = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const uint32_t q = o + t;
          const uint32_t c = q < len ? (uint32_t)src[q] : (q == len ? 0x80u : 0u);
          v |= c << (24 - 8 * t);
        }
      }
      w[k] = v;
    }
    if (b == nblk - 1) { const uint64_t bits = (uint64_t)len * 8; w[14] = (uint32_t)(bits >> 32); w[15] = (uint32_t)bits; }
    if (j.pad) sha1_compress(st, w); else sha256_compress(st, w);
  }
  sha_store_digest((uint32_t*)j.dst, st, j.pad != 0);
}

// what one lane stored, the other lanes of this wave read back: past this CU's L1 (rare paths only: an agent-scope
// fence is an L2 write-back / invalidate on this chip)
__device__ __forceinline__ void wave_publish() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// The front end, the two hashes and the RSA operation of signature round `round` for the e-mails base + (bits of pend),
// by the whole wave, one e-mail after the other.  A real call: inlined, its loop-invariant addresses would be kept (and
// spilled) across the Ed25519 stage of the caller's loop.
__device__ __noinline__ void next_round(const EdVerdictArgs& A, uint32_t round, uint64_t pend_mask, uint32_t base) {
  __shared__ ParseLds L;
  const BatchDev& B = A.fin.b;
  const int lane = threadIdx.x & 63;
  for (uint64_t pend = pend_mask; pend; pend &= pend - 1) {
    const uint32_t e = base + (uint32_t)__builtin_ctzll(pend);
    const EmailMeta* M = B.meta + e;
    wave_publish();                                   // the verdict lane's EmailMeta / record stores
    ParseArgs pa{B, round, 0, 0, A.strict, A.now, nullptr, 0, nullptr, nullptr};
    parse_email<false>(pa, e, L);
    wave_publish();                                   // the front end's jobs, preimage and canonical body
    if (M->state != ST_CAND) continue;
    if (lane < 2) sha_lane(B.sha[(size_t)lane * B.n_pad + e]);      // kind 0: body, kind 1: header preimage
    wave_publish();
    if (!(M->flags & ZKE_F_ED25519))
      rsa_wave_any(B.rsa, e, nullptr, 0, nullptr, A.em_out, A.cache, B.meta, A.fin.debug_skip_rsa);     // em_ok / em_tail -> EmailMeta
  }
}

// The verdict of one e-mail (M, R, ext: verdict_load) in signature round `round`, by one lane (the 16 verdict lanes of a wave at once): every load first
// (verdict_load), every decision from registers.  `mine`: the Ed25519 stage's result for this e-mail (3: it had no work in this
// round).  Called once per round, so what a later round's front end, hashes and RSA role have rewritten is read again.  A real
// call, as next_round is: inlined, its seventy words in flight compete with what the Ed25519 stage keeps in registers across the
// kernel's loop, and the compiler spills each load behind a wait of its own — one round trip after the other again.
__device__ __noinline__ bool verdict_round(const EdVerdictArgs& A, uint32_t round, EmailMeta* M, zke_result* R, const uint8_t* ext, uint32_t mine) {
  VerdictIn V;
  verdict_load(M, R, ext, V);
  const bool ed_bad = (mine == 0) || (mine == 3 && V.m[ZKE_MW(ed_key_bad)] != 0);      // decided in round 0
  return verdict_lane(A.fin, round, M, R, V, verdict_rsa_ok(V), mine == 2, ed_bad);
}

#ifndef ZKE_VERDICT_WAVES
#define ZKE_VERDICT_WAVES 2      // waves per SIMD the verdict launch is compiled for: at 1 it takes 364 registers (256 + 108 AGPRs), which
                                 // keeps the waves of other launches off its SIMD — RSA batches 26.8 M e-mails/s instead of 27.8 M,
                                 // Ed25519 batches 9.7 M instead of 9.0 M (3 / 4 waves: 7.0 / 6.4 M); round 2, and again in round 3: 168 / 128 registers with 1.5 / 1.9 KB of scratch change nothing for RSA batches
#endif
constexpr uint32_t VERDICT_EMAILS_PER_WAVE = 16;      // a DPP quad per e-mail in the Ed25519 stage

// The rounds of one wave from signature round `round` on, for the e-mails base + (bits of active).  The loop body is the round:
// Ed25519 stage (a quad per e-mail), verdict (a lane per e-mail), and for the e-mails still pending the next round's front end,
// hashes and RSA by the whole wave, one e-mail after the other.
__device__ __forceinline__ void verdict_rounds(const EdVerdictArgs& A, uint32_t round, uint64_t active, uint32_t base) {
  const BatchDev& B = A.fin.b;
  const int lane = threadIdx.x & 63;
  for (;;) {
    // ---- Ed25519 stage, four lanes per e-mail (quad j = e-mail base + j): the curve-point check of every 32-byte key in
    // round 0 (DkimPublicKey::try_from_bytes, core/src/email.rs:28-29), the verification of a=ed25519-sha256 candidates
    // over the SHA-256 header hash
    uint32_t ed_res = 3;                                // 3 = no Ed25519 work for this e-mail in this round
    {
      const uint32_t j = (uint32_t)lane >> 2, i = base + j;
      // the four words a quad decides its work by, requested together (behind one another's conditions they were four round trips)
      uint32_t q_type = 0, q_key_ok = 0, q_state = 0, q_flags = 0;
      const bool qact = (active >> j) & 1;
      if (qact) {
        const EmailMeta* M = B.meta + i;
        q_type = B.key_type[i]; q_key_ok = M->key_ok; q_state = M->state; q_flags = M->flags;
      }
      bool work = false, have_sig = false;
      // (quads without work run along on bytes that are always there: the start of the result records)
      const uint8_t* key = reinterpret_cast<const uint8_t*>(B.results);
      const uint8_t* msg = key;
      const uint8_t* sig = key;
      if (qact && !A.skip_ed && q_type == ZKE_KEY_ED25519 && q_key_ok == 2) {
        const bool cand = q_state == ST_CAND && (q_flags & ZKE_F_ED25519);
        if (round == 0 || cand) {                     // the key itself is checked in round 0
          const RsaJob* J = B.rsa + i;
          work = true;
          have_sig = cand && J->sig_len == 64;        // a b= of any other length cannot be an Ed25519 signature
          key = B.key + B.key_off[i]; msg = B.results[i].header_hash; sig = J->sig + (512 - 64);
        }
      }
      if (__ballot(work)) {
        const uint32_t r = ed25519_verify_quad(key, msg, 32, sig, have_sig);
        if (work) {
          ed_res = r;
          if ((lane & 3) == 0) {
            EmailMeta* M = B.meta + i;
            if (r == 0) M->ed_key_bad = 1;
            M->ed_ok = (r == 2) ? 1u : 0u;
          }
        }
      }
    }
    // ---- verdicts, lane per e-mail (lanes 0..15); e-mail j's Ed25519 result sits in lanes 4j..4j+3
    const uint32_t mine = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(16u * ((uint32_t)lane & 15u)), (int)ed_res);
    bool again = false;
    if (lane < (int)VERDICT_EMAILS_PER_WAVE && ((active >> lane) & 1)) {
      const uint32_t i = base + (uint32_t)lane;
      again = verdict_round(A, round, B.meta + i, B.results + i, B.ext_null ? B.ext_null + i : nullptr, mine);
    }
    active = __ballot(again);
    if (!active) return;
    // ---- the next signature round of the e-mails still undecided (verdict_lane has checked that one is allowed)
    round++;
    next_round(A, round, active, base);
    wave_publish();
  }
}

#if ZKE_VERDICT_ONE_TRIP
// The one call of the launch, made by the waves that RSA batches do not have: one with Ed25519 work (from_next = false: the whole of
// round `round`, every load again) or with e-mails left pending (from_next = true).  A: the kernel's argument where the dispatch
// packet put it (verdict_args_in_place), not a copy: a by-value kernel argument whose address leaves the kernel is copied to
// scratch at kernel entry, by every wave, and the callee is compiled for the kernel's whole register budget either way.
__device__ __noinline__ void verdict_rounds_call(const EdVerdictArgs& A, uint32_t round, uint64_t active, uint32_t base, bool from_next) {
  if (from_next) {
    round++;
    next_round(A, round, active, base);
    wave_publish();
  }
  verdict_rounds(A, round, active, base);
}
// ed_verdict_kernel's one argument in the kernel-argument segment: explicit arguments start at offset 0 of it
__device__ __forceinline__ const EdVerdictArgs& verdict_args_in_place() {
  return *(const EdVerdictArgs*)__builtin_amdgcn_kernarg_segment_ptr();
}
#endif

// One wave: the Ed25519 stage and the verdicts of 16 e-mails, then — for the rare e-mail whose candidate signature failed
// while another same-domain signature is untried — the next signature round of those e-mails right here: cfdkim's
// verify_email_with_key tries the candidates one after the other until one passes (behind core/src/email.rs:31-33).
// Round 0 of every e-mail runs in the batch's three launches; giving the later rounds launches of their own would charge
// every batch for them, here they cost a ballot per wave (verdict_rounds).
//
// ZKE_VERDICT_ONE_TRIP: a wave of an RSA batch has no Ed25519 work and, almost always, no e-mail left pending.  What it does is
// one trip to memory and back: every load its 16 verdicts need — the key type, EmailMeta, the two hashes and the ext flag, by the
// e-mail's verdict lane (verdict_load) — is requested at kernel entry before anything waits; workgroup 0's resets are issued behind
// them.  The words a quad would decide its Ed25519 work by (key type, key_ok, state, flags) are among them, so the verdict lanes say
// whether the wave has any: no second round of loads that waits for the first.
// It has none: the verdicts are decided right here from what is in registers, without a call and without scratch (`mine` = 3: the
// stage wrote nothing, so the copy of EmailMeta is current; ed_key_bad in it is round 0's).  It has some: the wave leaves for
// verdict_rounds_call, which runs the stage and then loads EmailMeta AGAIN for its verdicts — the stage writes ed_key_bad and ed_ok,
// and nothing of the copy fetched at entry is used behind it, those two fields included.  Later signature rounds load again, as ever.
__global__ __launch_bounds__(64, ZKE_VERDICT_WAVES) void ed_verdict_kernel(EdVerdictArgs A) {
  const BatchDev& B = A.fin.b;
  const int lane = threadIdx.x & 63;
  const uint32_t base = blockIdx.x * VERDICT_EMAILS_PER_WAVE;
  const bool lead = blockIdx.x == 0 && lane == 0 && A.wave_count;
#if ZKE_VERDICT_ONE_TRIP
  // ---- every load of the wave, requested before anything waits: the job-list length (workgroup 0), key type and verdict inputs
  const uint32_t round = A.fin.round;
  uint32_t n_wave_jobs = 0;
  if (lead) n_wave_jobs = *A.wave_count;
  const bool vlane = lane < (int)VERDICT_EMAILS_PER_WAVE && base + (uint32_t)lane < B.n;      // verdict lane of e-mail base + lane
  const uint32_t vi = base + (uint32_t)lane;
  uint32_t key_type = 0;
  VerdictIn V;
  if (vlane) {
    key_type = B.key_type[vi];
    verdict_load(B.meta + vi, B.results + vi, B.ext_null ? B.ext_null + vi : nullptr, V);
  }
  if (lead) {
    if (A.wave_feedback) __hip_atomic_store(A.wave_feedback, n_wave_jobs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    *A.wave_count = 0;
  }
#else
  if (lead) {
    if (A.wave_feedback) __hip_atomic_store(A.wave_feedback, *A.wave_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    *A.wave_count = 0;
  }
#endif
  if (blockIdx.x == 0 && B.order)              // the hash stage has consumed the length buckets: counters back to zero for the slot's next batch
    for (uint32_t k = 0; k < 2; k++)
      for (uint32_t c = (uint32_t)lane; c < SHA_CLASSES; c += 64) B.order[sha_order_cnt(k) + c] = 0;
  uint64_t active = 0;                                  // verdict lanes (= e-mails base + lane) this wave still works on
  for (uint32_t j = 0; j < VERDICT_EMAILS_PER_WAVE; j++) if (base + j < B.n) active |= 1ull << j;
#if ZKE_VERDICT_ONE_TRIP
  // (the condition of the Ed25519 stage in verdict_rounds, taken by the e-mail's verdict lane from the words it has: whether ANY
  // quad of the wave would have work is all that is asked here; the key itself is checked in round 0)
  const bool work = vlane && !A.skip_ed && key_type == ZKE_KEY_ED25519 && V.m[ZKE_MW(key_ok)] == 2 &&
                    (round == 0 || (V.m[ZKE_MW(state)] == ST_CAND && (V.m[ZKE_MW(flags)] & ZKE_F_ED25519)));
  bool from_next = false;
  if (!__ballot(work)) {
    bool again = false;
    if (vlane) again = verdict_lane(A.fin, round, B.meta + vi, B.results + vi, V, verdict_rsa_ok(V), false, V.m[ZKE_MW(ed_key_bad)] != 0);
    active = __ballot(again);
    if (!active) return;
    from_next = true;
  }
  verdict_rounds_call(verdict_args_in_place(), round, active, base, from_next);
#else
  verdict_rounds(A, A.fin.round, active, base);
#endif
}

}  // namespace zke
