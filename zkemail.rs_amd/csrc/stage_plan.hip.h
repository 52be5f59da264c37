// stage_plan.hip.h — which routines the hash / modexp stage of a batch runs, and with how many workgroups each.
//
// The stage (fused.hip.h) has one SHA-256 role and up to four RSA roles, and each has variants that pay off in different
// regimes.  The choice is a policy on plain integers: what is fixed when the engine is created or grown (StageEnv) and the
// size of the batch go in, a StagePlan comes out.  run_device_pipeline computes it once per batch; the front end routes
// signatures by its route_mask and the launch takes its workgroup counts from it, so the two cannot disagree.  Plain C++:
// no HIP runtime, no engine — tests/cpp/host_fuzz.cpp walks it over a grid on the CPU (tests/golden/stage_plan.txt).
//
// One bound decides between "shorter dependency chain" and "fewer instructions and less LDS": how many batches the engine can
// have on the chip at once.  Streams beyond HIP's queue pool share a hardware queue, and a queue runs its kernels one after the
// other, so that is min(slots that exist now, hardware queues) — zke_engine_reserve only appends, and an engine created with one
// slot and grown to 22 counts 22.  With at most CHAIN_BOUND_IN_FLIGHT batches a batch's time is its dependency chain (DESIGN.md §5
// has the sweep over the queue count); with more the chip is issue- and LDS-bound.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#ifdef __HIP__
#define ZKE_PLAN_FN __host__ __device__ inline
#else
#define ZKE_PLAN_FN inline
#endif

namespace zke {

// ---- route bits: which lane-group RSA roles a batch's launch has.  The front end routes a cached key's signatures by them
// (keydec.hip.h, rsa_route) and the launch gets the matching workgroups.
constexpr uint32_t ROUTE_QUAD = 1u;        // four lanes per signature, moduli <= 2048 bits (rsa_group_wave<4>, RSA_F_QUAD)
constexpr uint32_t ROUTE_OCT = 2u;         // eight lanes, moduli of 2049..4096 bits (rsa_group_wave<8>, RSA_F_OCT)
constexpr uint32_t ROUTE_OCT9 = 4u;        // eight lanes of nine limbs, moduli <= 2048 bits (rsa_group_wave<8, 9>, RSA_F_OCT9): in place of
                                           // ROUTE_QUAD, never beside it.  Its chain per product is a third shorter (2 520 instead of 3 684
                                           // instructions, profiles/oct9_static.txt) and it issues 1.4 times the instructions per signature

// ---- the SHA-256 routines (sha256.hip.h) and the layout of the stage's SHA-256 groups
enum class ShaRoutine : uint32_t {
  TWIN,       // sha256_twin_group: the ring with two lanes per message in the rounds wave, 32 messages per group
  RING,       // sha256_ring_group: two waves per 64 messages, two K+W buffers take the hand-over off the rounds wave's chain (45 KB of LDS per group)
  PAIR,       // sha256_pair_group: two waves per 64 messages, one K+W buffer (28 KB)
  BATCH,      // sha256_batch_kernel: one wave per 64 messages, arrival order; least LDS work per byte, for a chip full of hashes
};
constexpr uint32_t SHA_TWIN_WIDTH = 32;    // messages per group of the twin; every other two-wave group takes 64
ZKE_PLAN_FN uint32_t sha_routine_width(ShaRoutine r) {      // messages per workgroup
  return r == ShaRoutine::BATCH ? 256u : r == ShaRoutine::TWIN ? SHA_TWIN_WIDTH : 64u;
}

// The SHA-256 groups of a launch with a kind layout (kind-major job list, n_pad jobs per kind, n_pad a multiple of 64): kind k takes
// n_pad / width(k) consecutive workgroups, width 32 for the kinds of twin_kinds and 64 otherwise.  The host sizes g_sha by
// sha_stage_groups and the kernel finds its kind by sha_stage_kind: the one place that knows the layout.
constexpr uint32_t SHA_KINDS = 4;          // bodies, header preimages, domains, keys
ZKE_PLAN_FN uint32_t sha_kind_groups(uint32_t n_pad, uint32_t twin_kinds, uint32_t kind) {
  return n_pad / ((twin_kinds >> kind & 1u) ? SHA_TWIN_WIDTH : 64u);
}
ZKE_PLAN_FN uint32_t sha_stage_groups(uint32_t n_pad, uint32_t twin_kinds) {
  uint32_t g = 0;
  for (uint32_t k = 0; k < SHA_KINDS; k++) g += sha_kind_groups(n_pad, twin_kinds, k);
  return g;
}
// workgroup b < g_sha -> its kind; b becomes the group within the kind
ZKE_PLAN_FN uint32_t sha_stage_kind(uint32_t n_pad, uint32_t twin_kinds, uint32_t& b) {
  uint32_t kind = 0;
  for (; kind + 1 < SHA_KINDS; kind++) {
    const uint32_t g = sha_kind_groups(n_pad, twin_kinds, kind);
    if (b < g) break;
    b -= g;
  }
  return kind;
}

// ---- what the choice depends on besides the batch
struct StageEnv {
  uint32_t slots = 0;              // slots that exist now (zke_engine_create, zke_engine_reserve)
  uint32_t hw_queues = 4;          // GPU_MAX_HW_QUEUES as read once, at creation (unset or unreadable: HIP's default of 4)
  // forced choices, from the environment (for the tests of each routine and A/B runs of one build): -1 by the rules below, 0 never, 1 always
  int rsa_oct9 = -1;               // ZKE_RSA_OCT9: ROUTE_OCT9 instead of ROUTE_QUAD
  int sha_ring = -1;               // ZKE_SHA_RING: the ring instead of the pair
  int sha_twin = -1;               // ZKE_SHA_TWIN: the twin wherever the ring is taken
  int front_helper = -1;           // ZKE_FRONT_HELPER: the two-wave front end (a helper wave per e-mail canonicalises the body)
  uint32_t twin_kinds = 3;         // ZKE_SHA_TWIN_KINDS: which kinds of the stage the twin takes (bit 0 bodies, bit 1 header preimages; domains
                                   // and keys are one block each and keep 64-wide groups: 32 more workgroups per batch would keep the RSA
                                   // roles waiting for room)
  uint32_t rsa_quad_min = 256;     // the lane groups for moduli <= 2048 bits join batches of at least this many e-mails.  Low since the modexp
                                   // runs beside SHA-256: its longer chain no longer sits behind the hashes of a small batch; a handful of
                                   // e-mails is still answered sooner by one signature per wave.  (ZKE_RSA_QUAD_MIN under ZKE_DEV_KNOBS)
  uint32_t rsa_oct_min = 128;      // ... eight lanes, moduli above 2048 bits (ZKE_RSA_OCT_MIN under ZKE_DEV_KNOBS)
  uint32_t sha_mapping = 0;        // zke_options.sha_mapping: 0 by launch size, 1 always one wave per 64 messages, 2 always two
  uint32_t rsa_lane_groups = 0;    // zke_options.rsa_lane_groups: 0 by batch size, 1 never, 2 always
  bool key_cache = false;          // the engine has a key cache (the lane groups need a key's Montgomery constants from it)
};

// The environment's part of a StageEnv.  ZKE_RSA_OCT9, ZKE_SHA_RING, ZKE_SHA_TWIN and ZKE_SHA_TWIN_KINDS are read by the shipped library, not
// only under ZKE_DEV_KNOBS: the tests of the routines and A/B runs of one build need them there (INTEGRATION.md §5 lists them).
inline void stage_env_from_environment(StageEnv& v) {
  auto forced = [](const char* name, int& f) { if (const char* s = getenv(name)) f = atoi(s) != 0 ? 1 : 0; };
  // What HIP's queue pool is sized by was read (or is about to be read) by the runtime from the same variable.
  const char* q = getenv("GPU_MAX_HW_QUEUES");
  const int hwq = q ? atoi(q) : 0;
  v.hw_queues = hwq > 0 ? (uint32_t)hwq : 4u;
  forced("ZKE_RSA_OCT9", v.rsa_oct9);
  forced("ZKE_SHA_RING", v.sha_ring);
  forced("ZKE_SHA_TWIN", v.sha_twin);
  forced("ZKE_FRONT_HELPER", v.front_helper);
  if (const char* tk = getenv("ZKE_SHA_TWIN_KINDS")) v.twin_kinds = (uint32_t)atoi(tk) & 3u;
#ifdef ZKE_DEV_KNOBS
  if (const char* rm = getenv("ZKE_RSA_QUAD_MIN")) v.rsa_quad_min = (uint32_t)atoi(rm);
  if (const char* ro = getenv("ZKE_RSA_OCT_MIN")) v.rsa_oct_min = (uint32_t)atoi(ro);
#endif
}

// ---- the rules
inline uint32_t plan_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
inline uint32_t plan_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

constexpr uint32_t CHAIN_BOUND_IN_FLIGHT = 4;
inline bool chain_bound(const StageEnv& v) { return plan_min(v.slots, v.hw_queues) <= CHAIN_BOUND_IN_FLIGHT; }

// Two waves per 64 messages or one, for a hash launch of `groups` groups of 64 messages.  Few messages: the launch is as long as one wave's
// chain of compressions, so the chain is split over two waves.  Many: the chip is full and the one-wave kernel does less LDS work per byte.
constexpr uint32_t SHA_PAIR_MAX_GROUPS = 512;      // 32 768 messages: every BASELINE-sized batch
inline bool sha_takes_pairs(const StageEnv& v, uint32_t groups) { return v.sha_mapping ? v.sha_mapping == 2 : groups <= SHA_PAIR_MAX_GROUPS; }
// Which two-wave routine: the ring where a batch's time is its chain, for 17 KB more LDS per group; the twin is a refinement of the ring (the
// same roles, buffers and LDS, a shorter rounds chain) and on by default.
inline bool sha_takes_ring(const StageEnv& v) { return v.sha_ring >= 0 ? v.sha_ring == 1 : chain_bound(v); }
inline bool sha_takes_twin(const StageEnv& v) { return sha_takes_ring(v) && v.sha_twin != 0; }

// The round-0 front end with a helper wave per e-mail (parse.hip.h, parse_kernel<true>) or with one wave.  The helper shortens the front end's
// chain by the body canonicaliser's length and doubles the launch's waves (+ 3.5 KB of LDS per e-mail).  That pays where a batch's time is its
// chain and the launch leaves the chip room; where 23 hardware queues keep the chip's issue slots busy, or the batch alone fills the chip, the
// extra residents cost more than the chain gains.  The bound on the batch is the chip's SIMD count (256 CUs x 4): the front end is compiled for
// five waves per SIMD (96 registers), so up to one e-mail per SIMD the two-wave launch holds two of those five and leaves the other three, and
// the registers beside them, to the hash / modexp and verdict waves of the other batches in flight, as the one-wave launch of twice the batch
// would.  At 2 048 e-mails it holds four of five; at 4 096 its 8 192 waves exceed the 5 120 the chip holds of this kernel and the launch runs in
// two passes, the chain twice.  Measured (profiles/frontend_helper_bench_ab.txt, section 3: the helper for every batch): batches of 1 024 gain
// 6.8 % with four queues and lose 17 % with 23; with four queues batches of 4 096 and 8 192 lose 17 and 7 %, and the two workloads of 2 048 go
// one each way (+ 3 %, - 4 %).
constexpr uint32_t FRONT_HELPER_MAX_BATCH = 1024;      // = SIMDs of the chip
inline bool front_takes_helper(const StageEnv& v, uint32_t n) {
  return v.front_helper >= 0 ? v.front_helper == 1 : chain_bound(v) && n <= FRONT_HELPER_MAX_BATCH;
}

// Which lane-group RSA roles take part in a batch of n e-mails; any_big = the caller's hint that the batch's keys average more than an
// RSA-2048 key.  Eight lanes of nine limbs is the choice when the engine cannot fill the chip's issue slots.  Only the choice by batch size is
// made this way: rsa_lane_groups = 2 asks for the routines by name and keeps four lanes unless the environment says otherwise.
inline uint32_t rsa_route_mask(const StageEnv& v, uint32_t n, bool any_big) {
  if (!v.key_cache || v.rsa_lane_groups == 1) return 0;
  const bool always = v.rsa_lane_groups == 2;
  const bool oct9 = v.rsa_oct9 >= 0 ? v.rsa_oct9 == 1 : !always && chain_bound(v);
  uint32_t m = 0;
  if (always || n >= v.rsa_quad_min) m |= oct9 ? ROUTE_OCT9 : ROUTE_QUAD;
  if (any_big && (always || n >= v.rsa_oct_min)) m |= ROUTE_OCT;
  return m;
}

// A SHA-256 launch of its own over n messages (zke_sha256_batch; the stage's hashes beyond SHA_PAIR_MAX_GROUPS).  grid == 0: nothing to launch.
struct ShaPlan { ShaRoutine routine; uint32_t grid; };
inline ShaPlan plan_sha(const StageEnv& v, uint32_t n) {
  const ShaRoutine r = !sha_takes_pairs(v, (n + 63) / 64) ? ShaRoutine::BATCH
                       : sha_takes_twin(v)               ? ShaRoutine::TWIN
                       : sha_takes_ring(v)               ? ShaRoutine::RING
                                                         : ShaRoutine::PAIR;
  const uint32_t w = sha_routine_width(r);
  return ShaPlan{r, (n + w - 1) / w};
}

// The one-signature-per-wave role walks the front end's job list: the e-mails whose key is not cached yet (or that the lane groups do not
// take).  Once a stream of batches has its keys cached the list is empty, and every workgroup of the role still has to be given LDS and
// registers on a full chip just to look and leave (57 % of the launch's waves did nothing else).  So the role is sized by what the slot's
// PREVIOUS batch needed — its verdict launch leaves the list's length in a pinned word, no synchronisation, one batch stale —: 8 workgroups
// when that was empty, up to 128 (256 waves: a batch of 1 024 uncached keys takes four rounds of them) when every key was new or nothing
// is known yet (0xFFFFFFFF).  The walkers loop, so a wrong guess costs time, never work.
#ifndef ZKE_WAVE_ROLE_MAX_GROUPS
#define ZKE_WAVE_ROLE_MAX_GROUPS 128
#endif
#ifndef ZKE_WAVE_ROLE_MIN_GROUPS
#define ZKE_WAVE_ROLE_MIN_GROUPS 8
#endif

// The stage of a batch of n e-mails with n_sha SHA-256 jobs (4 * n_pad, kind-major).  Up to SHA_PAIR_MAX_GROUPS groups it is ONE launch; beyond
// that the chip is full of SHA-256 waves anyway: `front` runs first (arrival order), then the RSA roles as a launch without SHA-256 groups.
struct StagePlan {
  uint32_t route_mask;             // ROUTE_*: to the front end as well
  bool front_helper;               // the front end's kernel: parse_kernel<true> (two waves per e-mail) or parse_kernel<false>
  ShaPlan front;                   // SHA-256 as a launch of its own in front; grid == 0: none, the stage's own groups hash
  ShaRoutine routine;              // of the stage's kernel: what its SHA-256 groups run and the LDS it carries (no groups: the pair's)
  uint32_t twin_kinds;             // StageArgs::twin_kinds; launches without a kind layout (`order`) keep 64-wide groups
  uint32_t g_sha, g_wave, g_quad, g_oct, g_oct9;      // workgroups per role (StageArgs)
  uint32_t grid() const { return g_sha + g_wave + g_quad + g_oct + g_oct9; }
};
inline StagePlan plan_stage(const StageEnv& v, uint32_t n, uint32_t n_sha, bool any_big, bool have_order, uint32_t last_wave_jobs) {
  StagePlan p{};
  p.route_mask = rsa_route_mask(v, n, any_big);
  p.front_helper = front_takes_helper(v, n);
  const uint32_t want = last_wave_jobs == 0xFFFFFFFFu ? ZKE_WAVE_ROLE_MAX_GROUPS
                                                      : plan_max(ZKE_WAVE_ROLE_MIN_GROUPS, (plan_min(last_wave_jobs, n) + 1) / 2);
  p.g_wave = plan_min((n + 1) / 2, plan_min(want, ZKE_WAVE_ROLE_MAX_GROUPS));
  p.g_quad = (p.route_mask & ROUTE_QUAD) ? (n + 31) / 32 : 0;
  p.g_oct = (p.route_mask & ROUTE_OCT) ? (n + 15) / 16 : 0;
  p.g_oct9 = (p.route_mask & ROUTE_OCT9) ? (n + 15) / 16 : 0;
  p.routine = ShaRoutine::PAIR;
  const uint32_t groups = (n_sha + 63) / 64;
  if (!sha_takes_pairs(v, groups)) { p.front = plan_sha(v, n_sha); return p; }
  // Launches with the RSA-4096 role take the twin like the others: keeping them on the ring was tried and measured slower
  // (profiles/sha_twin_bench_ab.txt, section 4).
  if (have_order && sha_takes_twin(v)) p.twin_kinds = v.twin_kinds;
  p.g_sha = p.twin_kinds ? sha_stage_groups(n_sha / 4, p.twin_kinds) : groups;
  if (p.g_sha) p.routine = p.twin_kinds ? ShaRoutine::TWIN : sha_takes_ring(v) ? ShaRoutine::RING : ShaRoutine::PAIR;
  return p;
}

}  // namespace zke
