// rsa_quad.hip.h — RSA verification with FOUR LANES PER SIGNATURE (16 signatures per wavefront) for moduli of up
// to 2048 bits and e = 65537: the same rsa 0.9.6 / num-bigint-dig operation as rsa.hip.h (call site
// core/src/email.rs:31-33; RFC 8017 §8.2.2, §9.2), at about a third of the VALU instructions per signature of the
// one-signature-per-wave routine (DESIGN.md §5 has the measured counts).
//
// Why.  The path is VALU-issue bound and the one-limb-per-lane kernel spends 9 instructions per
// limb and CIOS step: two multiplies, and seven to read the multiplier digit, form the quotient digit, shift the
// accumulator one lane down and keep its carries.  Here a number is G * QL limbs of QBITS bits (QL = 18, QBITS = 29:
// 72 limbs for G = 4), QL consecutive limbs per lane, four lanes (one DPP quad) per signature:
//   * operand limbs are <= 2^QBITS, so a product is <= 2^58, and a register holds 2 QL = 36 of them in its life as a
//     column (QL as a high column of one block, QL as a low column of the next; half of them a * b, half m * n), plus at most
//     two carries < 2^35 (one when it is the first high column, one when the column below it is reduced) and one received
//     limb < 2^QBITS at the hand-over: 36 * 2^58 + 2^36 + 2^29 < 2^63.2, so every column is a plain 64-bit accumulator: ONE
//     v_mad_u64_u32 per limb product, no carry instructions.  (QL = 18 is what lets 29 bits fit: 2 QL * 2^(2 QBITS) must stay
//     below 2^64; 30-bit limbs would overflow a column after 16 products);
//   * the accumulator is a window of 2 QL columns per lane addressed at compile time (column k + r for limb k at
//     step r of a block of QL steps), so nothing is shifted inside a block; the per-step cross-lane work is two
//     quad broadcasts (multiplier digit, quotient digit) for 2 QL = 36 multiplies;
//   * every QL steps the reduced low half of a lane's window (zero in lane 0) moves one lane down and the high half
//     becomes the low half: QL quad rotations + QL additions per 2 QL^2 = 648 multiplies; the masks to QBITS bits (quotient
//     digit, finished column) ride on DPP moves for four lanes (v_and_b32_dpp);
//   * R = 2^(QBITS QL G) = 2^2088 > 2^40 n >= 4n, so values stay in [0, 2n) without any conditional subtraction; carries
//     are normalised once per product (limbs <= 2^QBITS), exactly only for the final result.
// A Montgomery product is 2 (QL G)^2 = 10 368 multiplies for 16 signatures; a block of QL steps compiles to 792 VALU
// instructions, 648 of them multiplies — 44 per step for 16 signatures instead of 9 per step for one (profiles/rsa_trim_static.txt).
// Moduli of 2049..4096 bits run the same code with eight lanes per signature (144 limbs, R = 2^4176, eight blocks of QL steps, 936 each).
//
// R^2 mod n for this radix (2^(2 * 2088) mod n; 2^(2 * 4176) mod n for eight lanes) comes from the key cache.  The front end
// looks a decoded key up there (by modulus: exact) and routes the e-mail's signatures here (RSA_F_QUAD / RSA_F_OCT) when the
// entry exists and e = 65537; a key seen for the first time — and other exponents, keys whose cache slot belongs to
// another key — goes to the one-signature-per-wave routine, which fills the entry (two more 32-bit-radix Montgomery
// products turn 2^(2 * 2048) mod n into 2^(2 * 2088) mod n).  Signatures rsa 0.9.6 rejects before the arithmetic are rejected
// here too.  The algorithm and its register bounds are modelled with Python integers in tests/test_rsa_group_model29.py, the
// deferred masks and the limb classes of the EMSA check in tests/test_rsa_group_trim_model.py.
#pragma once
#include "rsa_kernel.hip.h"

namespace zke {

// QL = 18 limbs per lane, QBITS = 29 bits per limb, QMASK: rsa.hip.h (KeyCacheEntry holds R^2 mod n in this layout)
static_assert(2 * QL < (1 << (64 - 2 * QBITS)), "2 QL products of <= 2^(2 QBITS) and their carries (< one product more) must fit a 64-bit column");
static_assert(4 * QL * QBITS >= 2048 + 2 && 8 * QL * QBITS >= 4096 + 2, "R > 4n for four lanes (<= 2048 bits) and eight (<= 4096)");
// The routines below take the limbs per lane as a parameter L: <4, QL> and <8, QL> are the two above, <8, QL9> is the same 72 limbs
// as <4, QL> on eight lanes — same radix R = 2^2088, same cached constant (KeyCacheEntry::rrq, limb t in lane t / L), so a key
// cached for one is cached for the other.  A step then has 2 * 9 multiplies instead of 36: a block of nine steps is 315 VALU
// instructions and a product eight of them, against four blocks of 921 (profiles/oct9_static.txt) — the launch's RSA chain alone
// measures 82 us instead of 130 — for 1.4 times the instructions per signature: the routine for an engine that cannot keep the
// chip's issue slots busy anyway.  A column lives through 2 L = 18 products: more room in its 64 bits, not less.
constexpr int QL9 = QL / 2;
static_assert(8 * QL9 == 4 * QL, "eight lanes of QL9 limbs hold the number four lanes of QL limbs hold: one radix, one cached constant");
template <int L> struct QBigL { uint32_t v[L]; };             // lane p of the group: limbs L p .. L p + L - 1

// Lane groups of G = 4 (one DPP quad: 72 limbs, moduli <= 2048 bits) or G = 8 (half a DPP row: 144 limbs, <= 4096 bits).
// (bound_ctrl on the full-mask moves: lanes without a source read 0 and the destination needs no initial value)
template <int G> __device__ __forceinline__ uint32_t g_bcast0(uint32_t x) {        // lane 0 of the group to all of it
  uint32_t q = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x00 /*quad_perm:[0,0,0,0]*/, 0xf, 0xf, true);
  if (G == 8) q = (uint32_t)__builtin_amdgcn_update_dpp((int)q, (int)q, 0x114 /*row_shr:4*/, 0xf, 0xA /*lanes 4-7, 12-15*/, false);
  return q;
}
template <int G> __device__ __forceinline__ uint32_t g_rotdown(uint32_t x, int p) {   // lane p <- lane p+1, lane G-1 <- lane 0
  if (G == 4) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x39 /*quad_perm:[1,2,3,0]*/, 0xf, 0xf, true);
  const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x101 /*row_shl:1*/, 0xf, 0xf, true);
  const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x117 /*row_shr:7*/, 0xf, 0xf, true);
  return p == 7 ? b : a;
}
// Eight lanes, where a rotation costs two moves and a select: what the top lane would receive is never used (the multiplier copy:
// a digit block that wraps round reaches lane 0 after G rotations, and G - 1 are consumed) or is zero by construction (the
// hand-over: lane 0's finished columns are multiples of 2^QBITS), so ONE move does — row_shl:1; lanes 7 and 15 read the next
// group's lane 0 or nothing, and the hand-over masks them with a per-lane mask that is zero there.
__device__ __forceinline__ uint32_t g8_shiftdown(uint32_t x) {                        // lane p <- lane p+1 for p < 7; lane 7: unspecified
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x101 /*row_shl:1*/, 0xf, 0xf, true);
}
// ... and a broadcast whose mask rides on the first of its two moves (the quad_perm one has a full mask and no old value)
__device__ __forceinline__ uint32_t g8_bcast0_masked(uint32_t x, uint32_t qm) {
  const uint32_t q = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x00 /*quad_perm:[0,0,0,0]*/, 0xf, 0xf, true) & qm;
  return (uint32_t)__builtin_amdgcn_update_dpp((int)q, (int)q, 0x114 /*row_shr:4*/, 0xf, 0xA /*lanes 4-7, 12-15*/, false);
}
template <int G> __device__ __forceinline__ uint32_t g_fromprev(uint32_t x) {      // lane p <- lane p-1 (lane 0: callers mask it)
  if (G == 4) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x90 /*quad_perm:[0,0,1,2]*/, 0xf, 0xf, true);
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111 /*row_shr:1*/, 0xf, 0xf, true);
}

// QMASK in a VGPR the compiler cannot turn back into a literal: an `and` whose other operand comes out of a full-mask DPP move
// then folds into that move (v_and_b32_dpp; DPP encodings take no literal operand).
__device__ __forceinline__ uint32_t qmask_vgpr() {
  uint32_t qm = QMASK;
  asm("" : "+v"(qm));
  return qm;
}

// W = (a * b + sum_i m_i * n * 2^(QBITS i)) / 2^(QBITS QL G) as QL lazy 64-bit columns per lane (column j of lane p: limb QL p + j).
// A register holds at most 2 QL = 36 products (<= 2^58 each) in its life as a high and then a low column: no overflow.
//   * The quotient digit is masked BEHIND its broadcast: the 32-bit product travels, every lane keeps QBITS bits of it.
//   * A finished column r is not masked in the step.  After the step it is read twice more: `>> QBITS` for the carry (the whole
//     column, as before) and, at the hand-over, its low 32 bits by the lane below — which masks what it receives to QBITS bits.
//     Both are the values a masked column would give; the register is overwritten right after (W[j] = W[QL + j] + recv).  So the
//     column bound is untouched: still at most 2 QL products, two carries and one received limb <= 2^QBITS - 1 per register.
//   With the mask in a VGPR both `and`s fold into their DPP moves for four lanes (v_and_b32_dpp): 792 VALU per block instead of 828.
// (The four blocks written out, each reading its digit from lane blk of b with one quad_perm move and no rotating copy B, are 786
// per block and as fast alone, but 25 KB of code: in flight they give back the gain — profiles/rsa_trim_bench_ab.txt.)
template <int G, int L>
__device__ __forceinline__ void qmont_columns(uint64_t (&W)[2 * L], const QBigL<L>& a, const QBigL<L>& b, const QBigL<L>& n, uint32_t ninv, int p) {
#pragma unroll
  for (int j = 0; j < 2 * L; j++) W[j] = 0;
  const uint32_t qm = qmask_vgpr();
  constexpr bool LEAN = G == 8 && L == QL9;          // the one-move rotations and the masked broadcast above; <8, QL> keeps its code
  uint32_t qm_recv = p == G - 1 ? 0u : QMASK;        // LEAN: the top lane receives nothing
  asm("" : "+v"(qm_recv));
  QBigL<L> B = b;
#pragma unroll 1
  for (int blk = 0; blk < G; blk++) {
    // QL steps: multiplier digits QL blk + r, held by lane 0 of the group after blk rotations of B
#pragma unroll
    for (int r = 0; r < L; r++) {
      const uint32_t bd = g_bcast0<G>(B.v[r]);
#pragma unroll
      for (int k = 0; k < L; k++)           // column r + QL - 1 is touched here for the first time in this block (r > 0)
        W[k + r] = (uint64_t)a.v[k] * bd + ((k == L - 1 && r > 0) ? 0ull : W[k + r]);
      const uint32_t m = LEAN ? g8_bcast0_masked((uint32_t)W[r] * ninv, qm)
                              : g_bcast0<G>((uint32_t)W[r] * ninv) & qm;    // lane 0's column r is the lowest live limb
#pragma unroll
      for (int k = 0; k < L; k++) W[k + r] = (uint64_t)n.v[k] * m + W[k + r];
      W[r + 1] += W[r] >> QBITS;           // lane 0: the column is now a multiple of 2^QBITS; other lanes: a partial carry (< 2^35)
    }
    // the window moves up QL limbs: finished low columns go one lane down (lane 0's are zero mod 2^QBITS and reach the top lane)
#pragma unroll
    for (int j = 0; j < L; j++) {
      const uint32_t recv = LEAN ? g8_shiftdown((uint32_t)W[j]) & qm_recv : g_rotdown<G>((uint32_t)W[j], p) & qm;
      W[j] = W[L + j] + recv;
    }
#pragma unroll
    for (int r = 0; r < L; r++) B.v[r] = LEAN ? g8_shiftdown(B.v[r]) : g_rotdown<G>(B.v[r], p);
  }
}

// columns -> limbs.  CROSS cross-lane passes: 1 leaves limbs <= 2^QBITS (good enough as an operand), G - 1 is exact.
template <int G, int L, int CROSS>
__device__ __forceinline__ void qnorm(QBigL<L>& out, const uint64_t (&W)[2 * L], int p) {
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < L; j++) {
    const uint64_t t = W[j] + c;
    out.v[j] = (uint32_t)t & QMASK;
    c = t >> QBITS;                                             // t < 2^64: c < 2^35
  }
  uint32_t clo = (uint32_t)c, chi = (uint32_t)(c >> 32);       // < 2^35 out of the local pass
#pragma unroll
  for (int pass = 0; pass < CROSS; pass++) {
    uint32_t ilo = g_fromprev<G>(clo), ihi = g_fromprev<G>(chi);
    if (p == 0) { ilo = 0; ihi = 0; }
    const uint64_t t0 = (uint64_t)out.v[0] + (((uint64_t)ihi << 32) | ilo);
    out.v[0] = (uint32_t)t0 & QMASK;
    uint32_t c32 = (uint32_t)(t0 >> QBITS);                    // t0 < 2^29 + 2^35: c32 < 2^7 (first pass), then 0 or 1
#pragma unroll
    for (int j = 1; j < L; j++) {
      const uint32_t t = out.v[j] + c32;
      out.v[j] = t & QMASK;
      c32 = t >> QBITS;
    }
    clo = c32; chi = 0;                                         // 0 or 1 from here on
  }
  uint32_t last = g_fromprev<G>(clo);
  if (p == 0) last = 0;
  out.v[0] += last;                                             // value-preserving; zero after G - 1 passes
}

// bits [QBITS t, QBITS t + QBITS) of a big-endian 512-byte field (RsaJob.mod / .sig)
__device__ __forceinline__ uint32_t qlimb_of(const uint8_t* field, uint32_t t) {
  typedef uint64_t __attribute__((aligned(1))) u64_unaligned;
  const uint32_t bit = (uint32_t)QBITS * t, o = bit >> 3;              // little-endian byte o = field[511 - o]
  if (o >= 512) return 0;                                              // beyond 4096 bits
  const uint32_t oo = o > 504 ? 504u : o;                              // the top limbs: read the field's first 8 bytes and shift
  const uint64_t v = __builtin_bswap64(*(const u64_unaligned*)(field + 504 - oo)) >> (8 * (o - oo));
  return (uint32_t)(v >> (bit & 7)) & QMASK;                           // 7 + QBITS <= 64 - 8 * (o - oo) bits of v, or zeros above the field
}

// One wave: NG = 64 / G signatures.  job0 = the wave's first job.  Llimb: NG x (G * QL + 4) dwords of LDS private to the wave.
//   meta != nullptr: em_ok / em_tail of each signature go to EmailMeta for verdict_kernel (the batch pipeline);
//   hash_base != nullptr: the digest is at hand, ok_out[job] = full verification.
template <int G, int L = QL>
__device__ __forceinline__ void rsa_group_wave(const RsaJob* __restrict__ jobs, uint32_t n, uint32_t job0, uint32_t* Llimb_raw,
                                               const uint8_t* __restrict__ hash_base, size_t hash_stride,
                                               uint32_t* __restrict__ ok_out, uint8_t* __restrict__ em_out,
                                               const KeyCacheEntry* cache, EmailMeta* meta) {
  constexpr int NG = 64 / G, LIMBS = G * L;
  constexpr uint32_t MY_FLAG = G == 4 ? RSA_F_QUAD : L == QL ? RSA_F_OCT : RSA_F_OCT9;
  constexpr uint32_t EM_BYTES = LIMBS == 4 * QL ? 256u : 512u;          // the EM field the limbs cover: RSA-2048 / RSA-4096
  uint32_t (*Llimb)[LIMBS + 4] = reinterpret_cast<uint32_t (*)[LIMBS + 4]>(Llimb_raw);
#ifndef ZKE_QUAD_PRIO
#define ZKE_QUAD_PRIO 3
#endif
  const int lane = threadIdx.x & 63, p = lane & (G - 1), grp = lane / G;
  const uint32_t job = job0 + grp;
  const RsaJob* J = jobs + (job < n ? job : 0);
  uint32_t flags = 0;
  if (job < n) flags = J->flags;
  const bool act = (flags & MY_FLAG) != 0;
  if (__ballot(act) == 0) return;
  // NG signatures share one long dependency chain (~65 k instructions for G = 4): served round-robin with the short waves
  // of other batches it would stretch several times over and hold its whole batch back; the others have parallel slack.
  __builtin_amdgcn_s_setprio(ZKE_QUAD_PRIO);

  // (the signature and the cached constant are operands of one product each: they are read where they are used — s twice — and
  // hold no registers through the seventeen products between: 36 loads per lane, once per signature)
  const KeyCacheEntry* E = cache;
  QBigL<L> nn, acc;
#pragma unroll
  for (int j = 0; j < L; j++) { nn.v[j] = 0; acc.v[j] = 0; }
  uint32_t ninv = 0, kbytes = 0;
  if (act) {
    // the front end found this modulus in the cache (all limbs compared) before it set MY_FLAG; entries are immutable
    const uint32_t n0 = __builtin_bswap32(*(const uint32_t*)(J->mod + 508)), n1 = __builtin_bswap32(*(const uint32_t*)(J->mod + 504));
    E = cache + key_cache_slot(n0, n1);
#pragma unroll
    for (int j = 0; j < L; j++) {
      nn.v[j] = qlimb_of(J->mod, L * p + j);
      acc.v[j] = qlimb_of(J->sig, L * p + j);
    }
    ninv = ld_agent(&E->ninv) & QMASK;
    kbytes = J->k;
  }
  bool take = act;                            // the signature takes part in the arithmetic
  {
    // rsa 0.9.6 rejects a signature whose length is not the modulus length, or with s >= n, before any arithmetic:
    // such a job runs with s = 0, whose EM = 0 has no EMSA shape (em_ok = 0, an all-zero EM block, as the wave path leaves).
    // s >= n: per lane the sign of the highest differing limb; the highest lane of the group that differs decides.
    int c = 0;
#pragma unroll
    for (int j = L - 1; j >= 0; j--) c = c != 0 ? c : (int)(acc.v[j] > nn.v[j]) - (int)(acc.v[j] < nn.v[j]);
    const uint64_t gmask0 = (G == 4 ? 0xFull : 0xFFull);
    const uint64_t gtg = (__ballot(c > 0) >> (G * grp)) & gmask0, ltg = (__ballot(c < 0) >> (G * grp)) & gmask0;
    const bool reject = act && (J->sig_len != kbytes || gtg >= ltg);
    if (reject) {
      take = false;
#pragma unroll
      for (int j = 0; j < L; j++) acc.v[j] = 0;
    }
  }

  // s^65537 in 18 products: s R (into the Montgomery domain), sixteen squarings -> s^65536 R, and the last product takes
  // the PLAIN s: (s^65536 R) s / R = s^65537 — out of the domain without a nineteenth product by one.  That value is
  // < n + n^2 / R (a < 2n, s < n, R > 2^40 n): one conditional subtraction makes it exact.
  uint64_t W[2 * L];
#pragma unroll 1
  for (int step = 0; step < 17; step++) {
    QBigL<L> b = acc;
    if (step == 0) {
#pragma unroll
      for (int j = 0; j < L; j++) b.v[j] = act ? ld_agent(&E->rrq[L * p + j]) : 0u;
    }
    qmont_columns<G, L>(W, acc, b, nn, ninv, p);
    qnorm<G, L, 1>(acc, W, p);
  }
  {
    QBigL<L> s;
#pragma unroll
    for (int j = 0; j < L; j++) s.v[j] = take ? qlimb_of(J->sig, L * p + j) : 0u;
    qmont_columns<G, L>(W, acc, s, nn, ninv, p);
  }
  qnorm<G, L, G - 1>(acc, W, p);                 // exact limbs
  {
    // acc >= n?  Per lane the sign of the highest differing limb; the highest differing lane of the group decides, and the
    // lanes below a lane decide the borrow it starts with.
    int c = 0;
#pragma unroll
    for (int j = L - 1; j >= 0; j--) c = c != 0 ? c : (int)(acc.v[j] > nn.v[j]) - (int)(acc.v[j] < nn.v[j]);
    const uint32_t gm = (G == 4 ? 0xFu : 0xFFu);
    const uint32_t gtg = (uint32_t)(__ballot(c > 0) >> (G * grp)) & gm, ltg = (uint32_t)(__ballot(c < 0) >> (G * grp)) & gm;
    if (gtg >= ltg) {                         // EM + n -> EM (never for a signature that verifies: EM < n / 2^15 there)
      const uint32_t low = (1u << p) - 1u;
      uint32_t borrow = (ltg & low) > (gtg & low) ? 1u : 0u;
#pragma unroll
      for (int j = 0; j < L; j++) {
        const uint32_t t = acc.v[j] - nn.v[j] - borrow;
        acc.v[j] = t & QMASK;
        borrow = t >> 31;
      }
    }
  }

  // EMSA-PKCS1-v1_5 (rsa 0.9.6 pkcs1v15_sign_unpad), limb compares and a byte walk through LDS: the structure in front of the digest is
  // checked here; the digest bytes are compared now (hash_base) or handed to verdict_kernel (meta)
#pragma unroll
  for (int j = 0; j < L; j++) Llimb[grp][L * p + j] = acc.v[j];
  if (p < 4) Llimb[grp][LIMBS + p] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const bool sha1 = (flags & RSA_F_SHA1) != 0;
  const uint32_t hl = sha1 ? 20u : 32u;
  bool bad = false, tail_bad = false;
  if (act) {
    const uint32_t* hw = hash_base ? (const uint32_t*)(hash_base + (size_t)job * hash_stride) : nullptr;
    uint8_t* tail = meta ? reinterpret_cast<uint8_t*>(meta[job].em_tail) : nullptr;
    // Almost all of EM's bytes are the FF run (little-endian bytes [tLen + 1, k - 2)) or the zeros at and above k, whose
    // value depends on nothing but their position: a limb that lies wholly inside the run must be all ones, one wholly at or
    // above bit 8k must be zero — QL compares per lane on the registers — and the byte walk visits only the bytes of the other
    // limbs: the digest, DigestInfo, the 00 separator and the limb that straddles that edge at the bottom, and the limbs
    // around 01 and the top 00.  emsa_byte stays the judge of every byte walked, the single statement of the padding.
    // (k < tLen + 11 makes the ranges meaningless: that verdict is refused below whatever they give, and the walk stays
    // inside the EM_BYTES the limbs cover.)  tests/test_rsa_group_trim_model.py has the classifier for every k.
    const uint32_t tlen = sha1 ? 35u : 51u;
    const uint32_t ff_lo = (8 * (tlen + 1) + QBITS - 1) / QBITS, ff_hi = (8 * (kbytes - 2)) / QBITS;
    const uint32_t z_lo = (8 * kbytes + QBITS - 1) / QBITS;
#pragma unroll
    for (int j = 0; j < L; j++) {
      const uint32_t t = L * (uint32_t)p + j;
      if (t >= ff_lo && t < ff_hi) bad = bad || acc.v[j] != QMASK;
      else if (t >= z_lo) bad = bad || acc.v[j] != 0;
    }
    const uint32_t walk_lo = (QBITS * ff_lo + 7) / 8, walk_hi = (QBITS * ff_hi) / 8;
    const uint32_t walk_top = (QBITS * z_lo + 7) / 8, walk_end = walk_top < EM_BYTES ? walk_top : EM_BYTES;
    // the bottom stretch and the top one; parity / debug, where every byte is written out, keeps the full walk instead
#pragma unroll 1
    for (int part = 0; part < (em_out ? 1 : 2); part++) {
      const uint32_t from = part == 1 ? walk_hi : 0u, to = em_out ? EM_BYTES : part == 0 ? walk_lo : walk_end;
      for (uint32_t i = from + (uint32_t)p; i < to; i += G) {        // little-endian byte index, the group's lanes side by side
        const uint32_t t = (8 * i) / QBITS, sh = 8 * i - QBITS * t;   // t + 1 <= LIMBS - 1; the + 4 words stay as zeroed padding
        const uint64_t two = (uint64_t)Llimb[grp][t] | ((uint64_t)Llimb[grp][t + 1] << QBITS);
        const uint32_t got = (uint32_t)(two >> sh) & 0xff;
        if (i < hl) {
          if (tail) tail[i] = (uint8_t)got;                        // little-endian limb image: byte i of EM counted from its end
          if (hw) tail_bad = tail_bad || got != emsa_byte(i, kbytes, hw, sha1);
        } else {
          bad = bad || got != emsa_byte(i, kbytes, nullptr, sha1);
        }
        if (em_out) em_out[(size_t)job * 512 + 511 - i] = (uint8_t)got;
      }
    }
    if (em_out && EM_BYTES == 256) {
#pragma unroll
      for (int z = 0; z < 64 / G; z++) *(uint32_t*)(em_out + (size_t)job * 512 + (256 / G) * p + 4 * z) = 0;     // upper half of the slot
    }
  }
  const uint64_t badm = __ballot(bad), tbadm = __ballot(tail_bad);
  const uint64_t gmask = (G == 4 ? 0xFull : 0xFFull);
  const bool shape_ok = act && ((badm >> (G * grp)) & gmask) == 0 && kbytes >= (sha1 ? 46u : 62u);      // k >= tLen + 11
  if (act && p == 0) {
    if (ok_out) ok_out[job] = (hash_base && shape_ok && ((tbadm >> (G * grp)) & gmask) == 0) ? 1u : 0u;
    if (meta) meta[job].em_ok = shape_ok ? 1u : 0u;
  }
}

template <int G, int L = QL>
__global__ __launch_bounds__(64) void rsa_group_kernel(const RsaJob* __restrict__ jobs, uint32_t n,
                                                       const uint8_t* __restrict__ hash_base, size_t hash_stride,
                                                       uint32_t* __restrict__ ok_out, uint8_t* __restrict__ em_out,
                                                       const KeyCacheEntry* cache, EmailMeta* meta) {
  constexpr int NG = 64 / G, LIMBS = G * L;
  __shared__ uint32_t Llimb[NG * (LIMBS + 4)];
  rsa_group_wave<G, L>(jobs, n, blockIdx.x * NG, Llimb, hash_base, hash_stride, ok_out, em_out, cache, meta);
}

// (not launched by the engine, which runs the routine inside hash_modexp_kernel: instantiated only for the compiler's resource
// remarks — build.py's verbose build defines ZKE_LIST_GROUP_KERNELS — to show the routine's own register footprint)
#ifdef ZKE_LIST_GROUP_KERNELS
template __global__ void rsa_group_kernel<4>(const RsaJob*, uint32_t, const uint8_t*, size_t, uint32_t*, uint8_t*, const KeyCacheEntry*, EmailMeta*);
template __global__ void rsa_group_kernel<8>(const RsaJob*, uint32_t, const uint8_t*, size_t, uint32_t*, uint8_t*, const KeyCacheEntry*, EmailMeta*);
template __global__ void rsa_group_kernel<8, QL9>(const RsaJob*, uint32_t, const uint8_t*, size_t, uint32_t*, uint8_t*, const KeyCacheEntry*, EmailMeta*);
#endif

}  // namespace zke
