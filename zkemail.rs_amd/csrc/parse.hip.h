// parse.hip.h — device-side restatement of the e-mail front end of verify_dkim.  One e-mail per wavefront parses; in round 0
// (parse_kernel<true>, blockDim = 128) a second wave per e-mail, the helper, decodes the key and canonicalises the body meanwhile.
//
// Replaces, on the verify path (call sites core/src/email.rs:26-33, core/src/circuits.rs:34-35):
//   * mailparse 0.15.0 parse_headers / parse_header (header list) and parse_mail_recursive's walk over the MIME
//     subparts (mime.hip.h: its only effect on this path is the parse error of a malformed subpart header block);
//   * cfdkim validate_header, the tag-list grammar (RFC 6376 §3.2), d= / i= / h= / q= / v= checks,
//     c= / a= / l= parsing, header selection (§5.4.2, bottom-up) and header canonicalisation
//     (§3.4.1 / §3.4.2) producing the header-hash preimage (§3.7);
//   * rsa 0.9.6 RsaPublicKey::from_pkcs1_der + check_public (RFC 8017 A.1.1);
//   * base64 STANDARD decode of b=.
//
// Execution model.  Control flow is wave-uniform (one e-mail, one parser state); the 64 lanes
// are used as a 64-byte-wide scanner: each primitive looks at 64 consecutive bytes at once and
// turns per-byte predicates into 64-bit ballot masks (find first / find last / stream
// compaction by popcount prefix).  The head of the e-mail (3.5 KB: the header block of ordinary mail) is staged
// in LDS with 16-byte lane-contiguous loads; the per-e-mail tables (header spans, tag records, the FWS-stripped
// tag values) live in LDS too.  In round 0 the kernel also does the batch's bookkeeping (batch_prologue), and the body is
// canonicalised in the same launch (canon.hip.h): by the e-mail's helper wave, beside the header-hash preimage, in round 0 ("the
// helper wave of the round-0 front end" below); by the parsing wave itself, after the parse, everywhere else (later signature
// rounds, mode 1) and on round 0's fallback paths — one launch for the whole front end.
//
// This file is the kernel: the batch's records, the phases only the verify path has (c= / l=, the b= removal) and
// parse_email, the list of reference calls with the header-hash preimage written out.  What the signature scan and the key
// records use as well lives in bytes.hip.h (scanner), taglist.hip.h (LDS image, tag list, validate_header), hdrsplit.hip.h
// (header split, MIME subparts, DKIM-Signature fields) and keydec.hip.h (DER, key routing, base64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zkemail_amd.h"
#include "rsa.hip.h"
#include "sha256.hip.h"
#include "bytes.hip.h"
#include "taglist.hip.h"
#include "hdrsplit.hip.h"
#include "keydec.hip.h"

namespace zke {

// Per-e-mail state shared by the kernels of one batch.
struct EmailMeta {
  uint32_t state;             // ST_*
  uint32_t status, detail;    // decided status when state == ST_FINAL
  uint32_t unsupported;       // last ZKE_D_U_* seen on a signature (0 = none)
  uint32_t last_touched_sig;  // oracle's sig_index when nothing passes
  uint32_t cand_total;        // same-domain signatures that reach the hash stage
  uint32_t cand_sig_index;    // signature index (file order) of this round's candidate
  uint32_t cand_hdr;          // header index of this round's candidate
  uint32_t cand_err;          // failure recorded for this round's candidate (finalize)
  uint32_t post_err;          // last non-candidate error located after this round's candidate
  uint32_t pre_err;           // last non-candidate error overall (used when there is no candidate)
  uint32_t flags;             // ZKE_F_*
  uint32_t len_tag_lo, len_tag_hi;
  uint32_t preimage_len;
  uint32_t body_off, body_len;
  uint32_t canon_full_len;    // canonical body length before l=
  uint32_t hashed_len;        // after l=
  uint32_t body_src_is_raw;   // simple canonicalisation hashes the raw bytes in place
  uint32_t n_headers, n_sigs;
  uint32_t first_sig_hdr;     // header index of the first DKIM-Signature (canonicalize_signed_email)
  uint32_t sig_b64_ok;
  uint32_t bh_len;
  uint8_t  bh[48];            // FWS-stripped bh= (first 48 chars)
  uint32_t key_ok;            // 1 = RSA key decoded, 2 = 32-byte Ed25519 key (its point check runs in ed25519_email_kernel)
  uint32_t even_modulus;
  uint32_t reuse;             // mode 1: the first DKIM-Signature is the verified one; scratch of the verify pass is reused
  uint32_t ed_key_bad;        // Ed25519 key is not a curve point (VerifyingKey::from_bytes fails): verdict = KEY_DECODE_FAIL
  uint32_t ed_ok;             // Ed25519 signature of this round's candidate verifies
  uint32_t rsa_route;         // RSA_F_QUAD / RSA_F_OCT: the key's Montgomery constants are cached and a lane-group kernel takes the modexp (round 0)
  uint32_t em_ok;             // the RSA role's result: EM = sig^e mod n has the EMSA-PKCS1-v1_5 shape for this signature's hash ...
  uint32_t em_tail[8];        // ... and EM's trailing digest bytes (little-endian limbs), compared with the header hash by verdict_kernel
};
static_assert(sizeof(EmailMeta) % 8 == 0, "EmailMeta alignment");

enum : uint32_t { ST_FINAL = 0, ST_CAND = 1, ST_PENDING = 2 };

// Batch view handed to the kernels (device pointers).
struct BatchDev {
  uint32_t n;
  const uint8_t* raw; const uint64_t* raw_off;
  const uint8_t* dom; const uint64_t* dom_off;
  const uint8_t* key; const uint64_t* key_off;
  const uint8_t* key_type; const uint8_t* ext_null;
  zke_result* results;
  EmailMeta* meta;
  RsaJob* rsa;
  ShaJob* sha;                // kind-major: sha[kind * n_pad + i], kinds 0 body, 1 header, 2 domain, 3 key
  uint32_t n_pad;
  uint8_t* scratch;           // per e-mail: region A (preimage) then region B (canonical body)
  uint64_t* scratch_off;      // [n+1]; region A = raw_len + PRE_SLACK bytes, region B = raw_len + 16 (written by the round-0 front end)
  uint64_t* clean_off;        // [n+1]; offsets of the QP-cleaned bodies (regex stage), written alongside
  uint32_t* pending;          // e-mails waiting for another signature round (reset by the round-0 front end)
  uint32_t* order;            // length buckets of the body and header-preimage hashes (sha256.hip.h, ShaOrder): 2 x 256 counters (zero at
                              // the start of a batch: the verdict launch of the previous one clears them), then 2 x n_pad keys; or nullptr
  const EmailMeta* meta_verify; // mode 1 only: the verify pass's meta
};
constexpr uint32_t PRE_SLACK = 1024;
constexpr uint32_t SCR_PER_EMAIL = HDR_OVF_BYTES + PRE_SLACK + 64;      // fixed part of an e-mail's scratch slot
constexpr uint32_t CLEAN_PER_EMAIL = 32;

// slot i = [header-span overflow (HDR_OVF_BYTES)] [region A] [region B], at align16(2 * (raw_off[i] - raw_off[0])) + i * SCR_PER_EMAIL;
// scratch_off[i] is the offset of region A
// clean_off[i]   = (raw_off[i] - raw_off[0]) + i * CLEAN_PER_EMAIL
__host__ __device__ inline uint64_t scratch_offset(uint64_t rel, uint32_t i) { return ((2 * rel + 15) & ~15ull) + (uint64_t)i * SCR_PER_EMAIL + HDR_OVF_BYTES; }
__host__ __device__ inline uint64_t clean_offset(uint64_t rel, uint32_t i) { return rel + (uint64_t)i * CLEAN_PER_EMAIL; }

// Round-0 bookkeeping of a batch, done by the front-end kernel itself instead of three tiny launches (an offsets
// kernel and two memsets, each a dispatch that queues behind the other batches in flight): the thread that owns
// e-mail i publishes its two offsets; `lead` threads (t of nt, all in the block that owns e-mail 0) clear the
// SHA jobs of the padding lanes of each kind's last wave, the (n+1)-th offsets and the pending counter.
__device__ __forceinline__ void batch_prologue(const BatchDev& B, uint32_t i, bool owner, bool lead, uint32_t t, uint32_t nt) {
  const uint64_t base = B.raw_off[0];
  if (owner) {
    const uint64_t rel = B.raw_off[i] - base;
    B.scratch_off[i] = scratch_offset(rel, i);
    B.clean_off[i] = clean_offset(rel, i);
  }
  if (lead) {
    for (uint32_t k = 0; k < 4; k++)
      for (uint32_t o = B.n + t; o < B.n_pad; o += nt) { ShaJob z{0, 0, 0, 0}; B.sha[(size_t)k * B.n_pad + o] = z; }
    if (t == 0) {
      const uint64_t rel = B.raw_off[B.n] - base;
      B.scratch_off[B.n] = scratch_offset(rel, B.n);
      B.clean_off[B.n] = clean_offset(rel, B.n);
      *B.pending = 0;
    }
  }
}

// ------------------------------------------------------------------ phases of a candidate signature (verify path only)
// c= (parser::parse_canonicalization): the ZKE_F_*_RELAXED flags; an absent tag is simple/simple.  false = ZKE_D_BAD_CANON
__device__ __forceinline__ bool canon_tag(const ParseLds& L, uint32_t present, uint32_t& flags) {
  flags = 0;
  if (!(present & (1u << TG_C))) return true;
  const TagVal c = tagval(L, TG_C);
  if (c == LIT("relaxed/relaxed")) flags = ZKE_F_HDR_RELAXED | ZKE_F_BODY_RELAXED;
  else if (c == LIT("relaxed/simple") || c == LIT("relaxed")) flags = ZKE_F_HDR_RELAXED;
  else if (c == LIT("simple/simple") || c == LIT("simple")) flags = 0;
  else if (c == LIT("simple/relaxed")) flags = ZKE_F_BODY_RELAXED;
  else return false;
  return true;
}
// l= (compute_body_hash's length parse): its value and ZKE_F_HAS_LENGTH when present.  false = ZKE_D_BAD_LENGTH
__device__ __forceinline__ bool length_tag(const ParseLds& L, uint32_t present, uint32_t& flags, uint64_t& len_tag) {
  if (!(present & (1u << TG_L))) return true;
  if (!parse_usize_tag(L, TG_L, len_tag)) return false;
  flags |= ZKE_F_HAS_LENGTH;
  return true;
}

// ------------------------------------------------------------------ the parse kernel
// mode 0: verify_email_with_key scan (round r picks the r-th same-domain candidate)
// mode 1: canonicalize_signed_email (first DKIM-Signature header, no domain filter; core/src/circuits.rs:34-35)
struct ParseArgs {
  BatchDev b; uint32_t round; uint32_t mode;
  uint32_t debug_stop;              // ZKE_DEV_KNOBS builds only (stage ablation for the profiles): 0 everywhere else
  uint32_t strict;                  // ZKE_STRICT_*: zke_options' strictness flags
  uint64_t now;                     // the time x= is compared with (ZKE_STRICT_EXPIRY_X)
  const KeyCacheEntry* cache;       // per-key Montgomery constants (nullptr: no cache, every signature takes the wave routine)
  uint32_t route_mask;              // ROUTE_* (stage_plan.hip.h): the lane-group RSA roles of this batch's hash / modexp launch (StagePlan::route_mask)
  uint32_t* wave_count;             // job list of the one-signature-per-wave RSA routine: the e-mails not routed to a lane-group kernel
  uint32_t* wave_list;              // (nullptr: no list, the routine looks at every job).  Appended here, consumed by the next launch.
};

#ifdef ZKE_DEV_KNOBS
#define ZKE_DEV_STOP(k) do { if (A.debug_stop == (k)) return; } while (0)
#else
#define ZKE_DEV_STOP(k) do { } while (0)
#endif

// canon.hip.h
constexpr uint32_t CANON_LDS_TRASH = 3504, CANON_LDS_BYTES = 3504 + 64;     // LDS the canonicaliser is lent (canon_body_compute's `lds`)
__device__ __forceinline__ void canon_body_wave(const BatchDev& B, uint32_t i, uint32_t mode, uint32_t flags, uint32_t boff,
                                                uint32_t blen, uint64_t len_tag, uint8_t* lds, bool ignore_l, bool bucket,
                                                uint32_t hdr_len = 0);
struct CanonWhere { const uint8_t* body; uint8_t* regB; };      // the e-mail's body and region B of its scratch slot
__device__ __forceinline__ CanonWhere canon_where(const BatchDev& B, uint32_t i, uint32_t boff);
__device__ __forceinline__ void canon_body_compute(const CanonWhere W, uint32_t flags, uint32_t blen, uint8_t* lds,
                                                   uint32_t& full_out, uint32_t& src_is_raw_out);
__device__ __forceinline__ void canon_body_publish(const BatchDev& B, uint32_t i, const CanonWhere W, uint32_t mode, uint32_t flags, uint64_t len_tag,
                                                   bool ignore_l, bool bucket, uint32_t hdr_len, uint32_t full, uint32_t src_is_raw);

// ------------------------------------------------------------------ the helper wave of the round-0 front end
// parse_kernel<true> gives every e-mail a workgroup of two waves.  Wave 0 is the front end (parse_email<true, 0, true>); wave 1,
// the helper, canonicalises the body (canon_body_compute) while wave 0 selects the headers and writes the header-hash preimage,
// the longest stage of the chain, which needs nothing the canonicaliser produces.  For the body the two meet at exactly two
// workgroup barriers, on every path through the kernel:
//   post  wave 0 has decoded the candidate's b= and knows whether the excised header went to region B (`copied`).  It leaves
//         (flags, body_off, blen, l=) in the mailbox with go = 1, or go = 0 when region B is in use (`copied`) — then it
//         canonicalises by itself at the end, as the one-wave front end does.
//   join  where the one-wave front end calls canon_body_wave.  The helper has left (full, src_is_raw) in the mailbox; wave 0
//         publishes them (canon_body_publish) if what it posted is still the candidate's (flags, l=).  It is not when the posted
//         candidate's preimage overflowed and a later signature took its place: wave 0 then runs compute + publish itself.
// The helper decides nothing: the global memory it writes is the canonical bytes in region B, dead unless a ShaJob points at them,
// and (below) the RsaJob's key fields.  Every record, EmailMeta field, job and bucket key is written by wave 0 where the one-wave
// front end writes it.  A path of wave 0 that ends before a barrier (every finish(...); return, ZKE_DEV_STOP) leaves it to
// parse_kernel, which executes the barriers the mailbox says are missing, with key_go = 0 and go = 0.  Region B has one writer at a
// time: wave 0 writes it (the excised header of a later candidate, the fallback) only behind the join.
//
// ZKE_HELPER_KEYDEC (default 1): a third barrier, in front of the other two, takes the key stage off wave 0's chain as well.  The
// stage needs the key, its type, the key cache and the route mask — nothing of the e-mail —, so the helper, idle until the post,
// runs it at kernel entry while wave 0 splits the headers: decode_rsa_key_compute and rsa_route, both without a store.
//   key   where the key stage stands in the one-wave front end (behind the MIME check).  The helper has left (kr, bits, even,
//         route) in the mailbox; wave 0 leaves key_go = 1 for an RSA key and, behind the barrier, does what it did with the values
//         it computed itself: finish(ZKE_KEY_DECODE_FAIL, kr) or R->rsa_bits, M->key_ok / even_modulus / rsa_route.  The helper
//         then stores the RsaJob's modulus / exponent (decode_rsa_key_store) if key_go && !kr: exactly when the one-wave front end
//         stores them — an e-mail that fails earlier (parse, MIME) never comes through the key site and its job stays as it was.
//         Wave 0's zeroing of J->bits / k / e at entry lies in front of its key barrier, whose release orders it before these stores.
//         An Ed25519 or unknown key type: the helper computes nothing, wave 0 decides as before (key_go = 0).
// Every wave then executes exactly three barriers on every path, in the order key, post, join.  (0: the two-barrier kernel above.)
#ifndef ZKE_HELPER_KEYDEC
#define ZKE_HELPER_KEYDEC 1
#endif
struct HelperBox {                 // the mailbox, in LDS
  uint32_t go;                     // 1: canonicalise with the four values below
  uint32_t flags, body_off, blen;
  uint32_t len_tag_lo, len_tag_hi;
  uint32_t full, src_is_raw;       // the helper's answer (canon_body_compute)
  // wave 0's own: which of its barriers it has executed.  (Here and not in registers: the signature loop's control flow is
  // divergent to the compiler, which would carry them through it in vector registers the front end does not have to spare.)
  uint32_t posted, joined;
  // ZKE_HELPER_KEYDEC (unused, but there, in the two-barrier build: the switch stays out of the layout)
  uint32_t keyed;
  uint32_t key_go;                 // 1: wave 0 came through the key site with an RSA key
  uint32_t kr, bits, even, route;  // the helper's answer: ZKE_D_KEY_* or 0 (decode_rsa_key_compute), Pkcs1::bits, even modulus, rsa_route or 0x800
};

// s_barrier with the workgroup fences __syncthreads() has: LDS traffic in front of it is complete and none behind it moves up
__device__ __forceinline__ void wg_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// File e-mail i's message of `len` bytes (kind 0 body, 1 header preimage) under its length class.  One lane per kind: lanes 0
// and 1 file the body and the header preimage with ONE atomic instruction at the very end of the front end — the positions
// come back after a round trip to the memory side that nothing else waits for.
__device__ __forceinline__ void sha_bucket(uint32_t* order, uint32_t kind, uint32_t n_pad, uint32_t i, uint32_t len) {
  const uint32_t cls = sha_len_class((len + 9 + 63) >> 6);
  order[sha_order_key(kind, n_pad) + i] = (cls << 24) | (atomicAdd(order + sha_order_cnt(kind) + cls, 1u) & 0xFFFFFFu);
}


// The front end of e-mail i by the calling wave (L: the wave's LDS image).  parse_kernel runs it for every e-mail of a
// batch (round 0, and mode 1); the verdict launch runs it again, round by round, for the rare e-mail whose candidate
// signature failed while a later same-domain signature is still untried (verdict.hip.h).
// HELPER (round 0, mode 0, parse_kernel<true> only): the e-mail has a helper wave, H is the mailbox the two share.
template <bool FAST = true, int MODE = 0, bool HELPER = false>
__device__ __forceinline__ void parse_email(const ParseArgs& A, const uint32_t i, ParseLds& L, HelperBox* H = nullptr) {
  static_assert(!HELPER || (FAST && MODE == 0), "the helper wave belongs to the round-0 verify front end");
  const BatchDev& B = A.b;
  const int lane = lane_id();
  EmailMeta* M = B.meta + i;
  zke_result* R = B.results + i;
  RsaJob* J = B.rsa + i;
  const uint32_t round = A.round;
  if (round > 0 && MODE == 0) {
    // later signature rounds: retire this e-mail's jobs of the previous round first, so the SHA / RSA
    // launches of this round only touch e-mails that are still pending
    if (lane < 4) { ShaJob z{0, 0, 0, 0}; B.sha[(size_t)lane * B.n_pad + i] = z; }
    if (lane == 0) J->flags = 0;
    if (M->state != ST_PENDING) return;
  }

  const uint64_t r0 = B.raw_off[i], r1 = B.raw_off[i + 1];
  if (round == 0 && MODE == 0) batch_prologue(B, i, lane == 0, i == 0, (uint32_t)lane, 64);
  Str raw = mkstr(B.raw + r0, (uint32_t)(r1 - r0));
  if (MODE == 0) stage_head(raw, L);
  const Str dom = mkstr(B.dom + B.dom_off[i], (uint32_t)(B.dom_off[i + 1] - B.dom_off[i]));
  const Str key = mkstr(B.key + B.key_off[i], (uint32_t)(B.key_off[i + 1] - B.key_off[i]));
  uint64_t rel0 = r0 - B.raw_off[0];
  // (the three-barrier kernel: the slot's address as a scalar.  As a vector pair — the offsets come from vector loads — it was the
  // value the compiler spilled across the signature loop once the helper's key stage was in the kernel: 8 VGPR spills, 20 B of scratch)
  if constexpr (HELPER && ZKE_HELPER_KEYDEC) rel0 = ((uint64_t)uni((uint32_t)(rel0 >> 32)) << 32) | uni((uint32_t)rel0);
  uint8_t* regA = B.scratch + scratch_offset(rel0, i);
  const uint32_t capA = raw.len + PRE_SLACK;

  auto sha_job = [&](uint32_t kind, const void* src, uint32_t len, void* dst, uint32_t algo = 0) {
    if (lane == 0 && MODE == 0) {
      ShaJob j; j.src = (uint64_t)src; j.dst = (uint64_t)dst; j.len = len; j.pad = algo;
      B.sha[(size_t)kind * B.n_pad + i] = j;
    }
  };
  auto finish = [&](uint32_t status, uint32_t detail) {
    if (lane == 0) { M->state = ST_FINAL; M->status = status; M->detail = detail; }
  };
  const bool bucket = B.order && round == 0 && MODE == 0;        // (later rounds hash by the e-mail's own wave: verdict.hip.h)

  if (MODE == 1) {
    // canonicalize_signed_email runs only for e-mails whose verify_email succeeded (circuits.rs:32-35)
    for (uint32_t o = lane; o < sizeof(EmailMeta) / 4; o += 64) ((uint32_t*)M)[o] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (R->status != ZKE_OK) { finish(R->status, R->detail); return; }
    const EmailMeta* V = B.meta_verify + i;
    // STRICTNESS SITE canon_takes_verified_signature (oracle: verify_one, same name).  Default: canonicalize_signed_email takes
    // the FIRST DKIM-Signature header, whatever its d=.  ZKE_STRICT_CANON_VERIFIED: the signature verify_dkim accepted.
    if (V->first_sig_hdr == V->cand_hdr || (A.strict & ZKE_STRICT_CANON_VERIFIED)) {        // same signature: nothing to recompute
      if (lane == 0) {
        M->state = ST_CAND; M->reuse = 1; M->flags = V->flags; M->preimage_len = V->preimage_len;
        M->body_off = V->body_off; M->body_len = V->body_len; M->canon_full_len = V->canon_full_len;
        // STRICTNESS SITE canon_ignores_l (also canon_body_wave, mode 1): the whole canonical body instead of its first l= bytes
        M->hashed_len = (A.strict & ZKE_STRICT_CANON_IGNORES_L) ? V->canon_full_len : V->hashed_len;
        M->body_src_is_raw = V->body_src_is_raw;
        M->len_tag_lo = V->len_tag_lo; M->len_tag_hi = V->len_tag_hi;
      }
      return;
    }
  } else if (round == 0) {
    // result record and meta start from zero
    for (uint32_t o = lane; o < sizeof(zke_result) / 4; o += 64) ((uint32_t*)R)[o] = 0;
    for (uint32_t o = lane; o < sizeof(EmailMeta) / 4; o += 64) ((uint32_t*)M)[o] = 0;
    for (uint32_t k = 0; k < 4; k++) sha_job(k, nullptr, 0, nullptr);
    if (bucket && lane < 2) B.order[sha_order_key((uint32_t)lane, B.n_pad) + i] = SHA_KEY_NONE;
    if (lane == 0) { J->flags = 0; J->bits = 0; J->k = 0; J->sig_len = 0; J->e = 0; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (lane == 0) R->regex_part = 0xFFFFFFFFu;
    if (r1 - r0 >= (1ull << 31)) { finish(ZKE_UNSUPPORTED, ZKE_D_U_EMAIL_TOO_LARGE); return; }
  }

  if (MODE == 1) stage_head(raw, L);      // (after the early exits above: an e-mail whose canonicalize pass reuses the verify pass never gets here)
  ZKE_DEV_STOP(1);
  // ---- mailparse::parse_mail (core/src/email.rs:26)
  uint32_t perr;
  uint32_t hdr_end = 0;
  uint32_t* hdr_ovf = (uint32_t*)(regA - HDR_OVF_BYTES);       // in front of region A
  uint32_t nh = 0;
  // (the rare later rounds, inlined into the verdict launch, take the serial split: less code there)
  if (!FAST || !split_headers_lines(L, hdr_ovf, raw, nh, perr, hdr_end)) nh = split_headers(L, hdr_ovf, raw, perr, hdr_end);
  if (nh == NONE) {
    finish(perr == ZKE_D_U_TOO_MANY_HEADERS ? ZKE_UNSUPPORTED : ZKE_PARSE_FAIL, perr);
    return;
  }
  ZKE_DEV_STOP(2);
  const uint32_t body_off = find_body(raw, hdr_end >= 2 ? hdr_end - 2 : 0);
  ZKE_DEV_STOP(3);
  if (lane == 0) {
    if (MODE == 0) { R->n_headers = nh; R->body_offset = body_off; }
    M->n_headers = nh; M->body_off = body_off; M->body_len = raw.len - body_off;
  }
  const HdrNames hn = hdr_names(L, nh);
  if (round == 0 && MODE == 0) {
    // ---- still parse_mail: the MIME subparts (mime.hip.h)
    uint32_t md = 0;
    const uint32_t mr = mime_subparts(L, hdr_ovf, raw, hn, nh, hdr_end, md);
    if (mr) { finish(mr, md); return; }
  }

  // ---- DkimPublicKey::try_from_bytes (core/src/email.rs:28-29)
  if (round == 0 && MODE == 0) {
    const uint32_t kt = B.key_type[i];
    if constexpr (HELPER && ZKE_HELPER_KEYDEC) {
      // ---- key: the helper has decoded and routed an RSA key meanwhile (HelperBox); it stores the job's key fields behind this barrier
      if (lane == 0) { H->key_go = kt == ZKE_KEY_RSA ? 1u : 0u; H->keyed = 1; }
      wg_barrier();
    }
    if (kt == ZKE_KEY_ED25519) {
      // raw 32 bytes (helpers/src/dkim.rs:103-108); whether they are a curve point is decided by ed25519_email_kernel
      if (key.len != 32) { finish(ZKE_KEY_DECODE_FAIL, ZKE_D_KEY_DER); return; }
      if (lane == 0) M->key_ok = 2;
    } else {
      if (kt != ZKE_KEY_RSA) { finish(ZKE_KEY_DECODE_FAIL, ZKE_D_KEY_TYPE); return; }
      if constexpr (HELPER && ZKE_HELPER_KEYDEC) {
        const uint32_t kr = uni(H->kr);
        if (kr) { finish(ZKE_KEY_DECODE_FAIL, kr); return; }
        if (lane == 0) { R->rsa_bits = H->bits; M->key_ok = 1; M->even_modulus = H->even; M->rsa_route = H->route; }
      } else {
        Pkcs1 pk{0, 0, 0, 0};
        uint32_t even = 0;
        const uint32_t kr = decode_rsa_key(key, J, pk, even);
        if (kr) { finish(ZKE_KEY_DECODE_FAIL, kr); return; }
        uint32_t route = 0x800;           // no cache, no lane-group kernel in this launch, or an exponent / modulus they do not take
        if (A.cache && A.route_mask && pk.e == 65537 && !even) route = rsa_route(key, pk.np, pk.nl, pk.bits, A.cache, A.route_mask);
        if (lane == 0) { R->rsa_bits = pk.bits; M->key_ok = 1; M->even_modulus = even; M->rsa_route = route; }
      }
    }
    // the two output witnesses (core/src/circuits.rs:16-17)
    sha_job(2, dom.base, dom.len, R->from_domain_hash);
    sha_job(3, key.base, key.len, R->public_key_hash);
    if (domain_has_kelvin(dom)) { finish(ZKE_UNSUPPORTED, ZKE_D_U_DOMAIN_FOLD); return; }      // the d= comparison below folds ASCII alone
  }

  ZKE_DEV_STOP(4);
  // ---- scan the DKIM-Signature headers in file order
  uint32_t sig_ix = 0, cand_count = 0, last_touched = 0, unsupported = 0;
  uint32_t err_all = 0;        // last non-candidate error anywhere
  uint32_t err_after = 0;      // last non-candidate error after this round's candidate
  bool have_cand = false;
  uint32_t first_sig_hdr = NONE;
  uint32_t cand_flags = 0, cand_hdr_len = 0;
  uint64_t cand_len_tag = 0;
  HdrSpan hs;
  for (uint32_t hx = 0; (hx = next_sig_header(L, hdr_ovf, raw, hn, nh, hx, hs)) != NONE; hx++) {
    const uint32_t this_ix = sig_ix++;
    if (first_sig_hdr == NONE) first_sig_hdr = hx;
    if (MODE == 1 && hx != first_sig_hdr) break;
    const Str v = substr(raw, hs.vs, hs.ve);
    auto note_err = [&](uint32_t e) { err_all = e; if (have_cand) err_after = e; last_touched = this_ix; };
    uint32_t present;
    const uint32_t verr = validate_sig<FAST>(L, v, present, A.strict, A.now);
    ZKE_DEV_STOP(5);
    if (verr == ZKE_D_U_SIG_NON_ASCII || verr == ZKE_D_U_TOO_MANY_TAGS || verr == ZKE_D_U_SIG_TOO_LONG) {
      unsupported = verr; last_touched = this_ix;
      if (MODE == 1) { finish(ZKE_UNSUPPORTED, verr); return; }
      continue;
    }
    if (verr) {
      if (MODE == 1) { finish(ZKE_CANON_FAIL, verr); return; }
      note_err(verr);
      continue;
    }
    if (MODE == 0 && !sig_names_domain(L, dom)) continue;
    last_touched = this_ix;
    // c=, a=, l=  (parser::parse_canonicalization, parse_hash_algo, compute_body_hash's length parse)
    uint32_t flags = 0;
    if (!canon_tag(L, present, flags)) {
      if (MODE == 1) { finish(ZKE_CANON_FAIL, ZKE_D_BAD_CANON); return; }
      note_err(ZKE_D_BAD_CANON); continue;
    }
    if (MODE == 0) {
      const uint32_t algo = sig_algo(L);
      if (algo == ZKE_SIG_ALGO_OTHER) { note_err(ZKE_D_BAD_ALGO); continue; }
      const bool ed_alg = algo == ZKE_SIG_ALGO_ED25519_SHA256;
      // a= and the key type must name the same scheme
      if (ed_alg != (B.key_type[i] == ZKE_KEY_ED25519)) { unsupported = ZKE_D_U_ALGO_ED25519; continue; }
      flags |= ed_alg ? ZKE_F_ED25519 : algo == ZKE_SIG_ALGO_RSA_SHA1 ? ZKE_F_SHA1 : 0u;
    }
    uint64_t len_tag = 0;
    if (!length_tag(L, present, flags, len_tag)) {
      if (MODE == 1) { finish(ZKE_CANON_FAIL, ZKE_D_BAD_LENGTH); return; }
      note_err(ZKE_D_BAD_LENGTH); continue;
    }
    // this signature reaches the hash stage
    const uint32_t my_cand = cand_count++;
    if (my_cand != round) continue;
    have_cand = true; err_after = 0;

    // ---- the b= value: decode, and locate its raw span for removal from the preimage
    const uint32_t b_rs = tagf(L, TG_B, 0), b_re = tagf(L, TG_B, 1);
    if (MODE == 0) {
      uint32_t sig_len = 0;
      const bool b64ok = decode_sig(L.tagbuf + tagf(L, TG_B, 2), tagf(L, TG_B, 3), J, sig_len);
      const uint32_t bh_o = tagf(L, TG_BH, 2), bh_l = tagf(L, TG_BH, 3);
      if (lane == 0) {
        M->sig_b64_ok = b64ok ? 1u : 0u;
        J->sig_len = sig_len;
        M->bh_len = bh_l;
      }
      for (uint32_t o = lane; o < 48; o += 64) M->bh[o] = o < bh_l ? L.tagbuf[bh_o + o] : 0;
    }
    // String::replace removes EVERY occurrence of the raw b= value (leftmost first, non-overlapping).  Normally the
    // tag's own span is the only one and the header is read through a one-excision view; when the value occurs
    // again (only short, hand-made b= values do) the excised header is written out once to region B of the scratch
    // slot — free until the body is canonicalised — and read back from there.
    const uint32_t bl = b_re - b_rs;
    uint8_t* const tmp = regA + (((size_t)raw.len + PRE_SLACK + 15) & ~(size_t)15);    // region B: raw.len + 16 bytes
    uint32_t tn = 0;
    bool copied = false;
    if (bl) {
      const uint32_t fl = bl < 8 ? bl : 8;
      auto next_occurrence = [&](uint32_t from, uint32_t skip_at) -> uint32_t {      // first match at >= from, != skip_at
        for (uint32_t base = from; base + bl <= v.len; base += 64) {
          const uint32_t p = base + lane;
          bool cand = p + bl <= v.len && p != skip_at;
          for (uint32_t t = 0; t < fl && cand; t++) cand = ldb(v, p + t) == ldb(v, b_rs + t);
          uint64_t m = __ballot(cand);
          while (m) {
            const uint32_t q = base + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            if (same_bytes(v, q, b_rs, bl)) return q;
          }
        }
        return NONE;
      };
      // STRICTNESS SITE b_removes_own_span_only (oracle: build_preimage, same name).  Default: String::replace — every occurrence
      // of the raw b= value goes.  ZKE_STRICT_B_OWN_SPAN: only the tag's own span is emptied.
      if (!(A.strict & ZKE_STRICT_B_OWN_SPAN) && next_occurrence(0, b_rs) != NONE) {
        if constexpr (HELPER) {
          // a later candidate (the posted one overflowed the preimage): the helper may still be writing region B — join first
          // (and what it left there is about to be overwritten: go = 0 makes the join below take the fallback)
          if (uni(H->posted)) {
            if (!uni(H->joined)) wg_barrier();
            if (lane == 0) { H->joined = 1; H->go = 0; }
          }
        }
        uint32_t pos = 0;
        while (pos < v.len) {
          const uint32_t q = next_occurrence(pos, NONE);
          const uint32_t end = (q == NONE) ? v.len : q;
          for (uint32_t base = pos; base < end; base += 64) { const uint32_t l = base + (uint32_t)lane; if (l < end) tmp[tn + (l - pos)] = (uint8_t)ldb(v, l); }
          tn += end - pos;
          if (q == NONE) break;
          pos = q + bl;
        }
        // the wave reads these bytes back with ordinary loads: make them visible past this CU's L1
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        copied = true;
      }
    }
    // The view is put together here, behind the branches, not inside them.  With `sv` assigned in both arms of the test above the
    // compiled code set the view's base to `tmp` on the "no second occurrence" path as well; bytes inside the staged head still
    // came from LDS, so only a signature header BEYOND the staged head was read from the (empty) region B and failed to verify
    // (tests/test_gpu_hdr_split.py, the S-hbm routes).  Check the join in the assembly when this is reshaped again.
    Str sv = v;
    if (copied) sv = mkstr(tmp, tn);
    else if (bl) { sv.len = v.len - bl; sv.cut = b_rs; sv.skip = bl; }
    ZKE_DEV_STOP(6);
    if constexpr (HELPER) {
      if (!uni(H->posted)) {
        // ---- hand-off: the body canonicalisation of this candidate starts on the helper wave, unless region B holds `tmp`
        if (lane == 0) {
          H->flags = flags; H->body_off = body_off; H->blen = raw.len - body_off;
          H->len_tag_lo = (uint32_t)len_tag; H->len_tag_hi = (uint32_t)(len_tag >> 32);
          H->go = copied ? 0u : 1u;
          H->posted = 1;
        }
        wg_barrier();
      }
    }
    // ---- header-hash preimage (cfdkim hash::compute_headers_hash)
    // (This block and the b= scan above stay written out in parse_email.  With the scan in a function that returns `copied`, the join
    // described above comes out wrong again: tests/test_gpu_hdr_split.py, the S-hbm routes, fail.)
    Out out{regA, 0, capA, false};
    const bool hrel = (flags & ZKE_F_HDR_RELAXED) != 0;
    const uint32_t hks_lane = hn.ks, hnl_lane = hn.nl;
    {
      const uint8_t* h = L.tagbuf + tagf(L, TG_H, 2);
      const uint32_t hl = tagf(L, TG_H, 3);
      // h= is split at every ':' (FWS is already stripped; empty entries count).  The ':' after position `from`, 64 bytes
      // of the value per step, instead of a scalar walk over its bytes.
      // (an h= value of at most 64 bytes — five to ten names — has its ':' in ONE mask: no loop, no further reads)
      const bool one_win = hl <= 64;
      const uint64_t colons = one_win ? __ballot((uint32_t)lane < hl && h[(uint32_t)lane < hl ? lane : 0] == ':') : 0ull;
      auto colon_after = [&](uint32_t from) -> uint32_t {
        if (one_win) { const uint64_t m = colons & bits_from(from); return m ? (uint32_t)__builtin_ctzll(m) : hl; }
        for (uint32_t base = from & ~63u; base < hl; base += 64) {
          const uint32_t l = base + (uint32_t)lane;
          const uint64_t m = __ballot(l < hl && l >= from && h[l] == ':');
          if (m) return base + (uint32_t)__builtin_ctzll(m);
        }
        return hl;
      };
      // the last header field in front of index `start` whose name is name[0, len) (case-insensitive), or NONE:
      // cfdkim walks the header list bottom-up with a cursor per name.  Fields 0..63 are tested by name LENGTH first, all
      // at once (lane x holds field x's), so only fields whose name has the right length are compared.
      auto find_last = [&](const uint8_t* name, uint32_t len, uint32_t start) -> uint32_t {
        for (uint32_t x = start; x-- > 64;) {
          const HdrSpan h2 = hdr_get(L, hdr_ovf, x);
          if (span_ieq(raw, h2.ks, h2.ke - h2.ks, name, len)) return x;
        }
        uint64_t m = __ballot((uint32_t)lane < start && (uint32_t)lane < nh && hnl_lane == len);
        while (m) {
          const uint32_t x = 63u - (uint32_t)__builtin_clzll(m);
          m &= ~(1ull << x);
          if (span_ieq(raw, __builtin_amdgcn_readlane(hks_lane, x), len, name, len)) return x;
        }
        return NONE;
      };
      uint32_t st = 0;
      for (;;) {
        const uint32_t e = colon_after(st);                  // entry [st, e)
        // bottom-up cursor per (lower-cased) name: replay the selection of the earlier entries of h= with the same name
        uint32_t cur = nh;
        for (uint32_t st2 = 0; st2 < st;) {
          const uint32_t e2 = colon_after(st2);              // < st: position st - 1 holds a ':'
          bool same = (e2 - st2) == (e - st);
          if (same) {
            bool bad = false;
            for (uint32_t base = 0; base < e - st; base += 64) { const uint32_t o = base + (uint32_t)lane; if (o < e - st) bad |= lower(h[st2 + o]) != lower(h[st + o]); }
            same = __ballot(bad) == 0;
          }
          if (same) {
            const uint32_t found = find_last(h + st2, e2 - st2, cur);
            cur = (found == NONE) ? 0 : found;
          }
          st2 = e2 + 1;
        }
        const uint32_t found = find_last(h + st, e - st, cur);
        if (found != NONE) {
          const HdrSpan sp = hdr_get(L, hdr_ovf, found);
          emit_header(out, substr(raw, sp.ks, sp.ke), substr(raw, sp.vs, sp.ve), hrel, true);
        }
        if (e >= hl) break;
        st = e + 1;
      }
    }
    // the DKIM-Signature header itself, b= emptied, no CRLF (cfdkim uses its own spelling of the name)
    if (hrel) { emit_lit(out, LIT("dkim-signature:")); emit_relaxed_value(out, sv); }
    else { emit_lit(out, LIT("DKIM-Signature: ")); emit_map(out, sv, 0, sv.len, [](uint32_t c) { return c; }); }
    if (out.overflow) {
      unsupported = ZKE_D_U_PREIMAGE_OVERFLOW;
      if (MODE == 1) { finish(ZKE_UNSUPPORTED, unsupported); return; }
      have_cand = false; cand_count--;
      // (HELPER: the only way on to a second hand-off point.  The post is behind this wave, so a later candidate posts nothing; its
      // copy into region B joins first, and the join at the end finds go = 0 or other (flags, l=) and takes the fallback.)
      continue;
    }
    cand_flags = flags; cand_len_tag = len_tag;
    if (lane == 0) {
      M->cand_sig_index = this_ix; M->cand_hdr = hx; M->flags = flags;
      M->len_tag_lo = (uint32_t)len_tag; M->len_tag_hi = (uint32_t)(len_tag >> 32);
      M->preimage_len = out.o;
      if (MODE == 0) { R->flags = flags; R->canon_header_len = out.o; R->sig_index = this_ix; }
    }
    if (MODE == 0) sha_job(1, regA, out.o, R->header_hash, (flags & ZKE_F_SHA1) ? 1u : 0u);
    cand_hdr_len = out.o;
    if (MODE == 1) break;
  }
  if (MODE == 1) {
    if (!have_cand) { finish(ZKE_CANON_FAIL, first_sig_hdr == NONE ? ZKE_D_NO_SIGNATURE : ZKE_D_SIG_SYNTAX); return; }
    if (lane == 0) { M->state = ST_CAND; M->first_sig_hdr = first_sig_hdr; }
    return;
  }
  if (lane == 0) {
    M->n_sigs = sig_ix; M->cand_total = cand_count; M->unsupported = unsupported; M->last_touched_sig = last_touched;
    M->post_err = err_after; M->pre_err = err_all; M->first_sig_hdr = first_sig_hdr;
  }
  if (!have_cand) {
    // nothing (more) to hash: neutral / last error / unsupported (core/src/circuits.rs:13 panics either way)
    if (lane == 0) R->sig_index = last_touched;
    if (unsupported) finish(ZKE_UNSUPPORTED, unsupported);
    else finish(ZKE_DKIM_NOT_PASS, err_all ? err_all : (round == 0 ? ZKE_D_NEUTRAL : M->cand_err));
    return;
  }
  ZKE_DEV_STOP(7);        // ablation: full parse, nothing downstream
  if (lane == 0) {
    M->state = ST_CAND;
    // an Ed25519 candidate leaves the RSA job inactive; ed25519_email_kernel verifies it
    const uint32_t jf = (cand_flags & ZKE_F_ED25519) ? 0u : (RSA_F_ACTIVE | ((cand_flags & ZKE_F_SHA1) ? (uint32_t)RSA_F_SHA1 : 0u) |
                                                                  (A.route_mask ? M->rsa_route & RSA_F_GROUPS : 0u));
    J->flags = jf;
    M->em_ok = 0;
    if ((jf & RSA_F_ACTIVE) && !(jf & RSA_F_GROUPS) && A.wave_list) A.wave_list[atomicAdd(A.wave_count, 1u)] = i;
  }
  // ---- body canonicalisation of the candidate (cfdkim hash::compute_body_hash), no launch boundary
  if constexpr (HELPER) {
    // ---- join (a candidate has passed the hand-off, so the post barrier is behind this wave)
    const bool posted = uni(H->posted) != 0;
    if (posted && !uni(H->joined)) wg_barrier();
    if (lane == 0 && posted) H->joined = 1;
    uint32_t full, src_is_raw;
    const CanonWhere W{raw.base + body_off, regA + (((size_t)raw.len + PRE_SLACK + 15) & ~(size_t)15)};      // (from registers: no look-up)
    if (posted && uni(H->go) && uni(H->flags) == cand_flags && uni(H->len_tag_lo) == (uint32_t)cand_len_tag && uni(H->len_tag_hi) == (uint32_t)(cand_len_tag >> 32)) {
      full = uni(H->full); src_is_raw = uni(H->src_is_raw);
    } else {
      // the fallback: the posted candidate is not the final one, or region B was in use — this wave, as in the one-wave front end
      canon_body_compute(W, cand_flags, raw.len - body_off, L.stage, full, src_is_raw);
    }
    canon_body_publish(B, i, W, 0, cand_flags, cand_len_tag, false, bucket, cand_hdr_len, full, src_is_raw);
  } else {
    canon_body_wave(B, i, 0, cand_flags, body_off, raw.len - body_off, cand_len_tag, L.stage, false, bucket, cand_hdr_len);   // parsing is over: the staged head is dead
  }
}

#ifndef ZKE_PARSE_PRIO
#define ZKE_PARSE_PRIO 3         // the front end's waves at the priority of the SHA-256 and RSA waves they share a SIMD with (ZKE_SHA_PRIO, ZKE_QUAD_PRIO):
                                 // those issue a three-operand instruction every 4.3 cycles, which leaves a wave at priority 0 next to nothing
#endif
#ifndef ZKE_PARSE_WAVES
#define ZKE_PARSE_WAVES 5        // waves per SIMD the front end is compiled for: 96 registers, no spills (at 6 — 80 registers — it spills 300 B per
                                 // lane since the strictness sites and the length buckets joined it: 28.5 M e-mails/s against 30.1 M; LDS allows 22 waves per CU)
#endif
// ZKE_PARSE_WG_WAVES = W: W e-mails per workgroup, still one per wavefront and nothing shared between them (no barrier,
// an LDS area each).  W only sets the granularity at which the chip hands out LDS and registers to the front end: with
// W = 8 a CU holds two workgroups (2 x 8 x 7.2 KB of LDS), i.e. four 80-register waves per SIMD, and 192 registers per SIMD
// + 44 KB of LDS are always left for the hash / modexp launches of earlier batches (fused.hip.h: 187 registers, 14.6 KB).
#ifndef ZKE_PARSE_WG_WAVES
#define ZKE_PARSE_WG_WAVES 1
#endif
constexpr size_t PARSE_DYN_LDS = ZKE_PARSE_WG_WAVES > 1 ? ZKE_PARSE_WG_WAVES * sizeof(ParseLds) : 0;     // launch argument
#ifdef ZKE_PARSE_NUM_VGPR      // with W > 1 the compiler sees an LDS-bound occupancy and takes more registers; this holds them
#define ZKE_PARSE_VGPR_ATTR __attribute__((amdgpu_num_vgpr(ZKE_PARSE_NUM_VGPR)))
#else
#define ZKE_PARSE_VGPR_ATTR
#endif
// ZKE_PARSE_HELPER: 1 (default) the pipeline launches parse_kernel<true>, two waves per e-mail (above), where the batch's plan takes it
// (stage_plan.hip.h, front_takes_helper); 0: parse_kernel<true> is not built (needed for ZKE_PARSE_WG_WAVES > 1).
#ifndef ZKE_PARSE_HELPER
#define ZKE_PARSE_HELPER 1
#endif
static_assert(sizeof(ParseLds) + CANON_LDS_BYTES + sizeof(HelperBox) == 10864, "LDS per workgroup of parse_kernel<true>: DESIGN §3, profiles/kernel_resource_usage.txt");
template <bool HELPER>
__global__ __launch_bounds__(HELPER ? 128 : 64 * ZKE_PARSE_WG_WAVES, ZKE_PARSE_WAVES) ZKE_PARSE_VGPR_ATTR void parse_kernel(ParseArgs A) {
  if constexpr (HELPER) {
    static_assert(!HELPER || ZKE_PARSE_WG_WAVES == 1, "the helper wave takes the place of a second e-mail in the workgroup");
    __shared__ ParseLds L;
    __shared__ __attribute__((aligned(16))) uint8_t canon_lds[CANON_LDS_BYTES];      // the helper's own: L.stage is alive in wave 0 until the join
    __shared__ HelperBox box;
    const uint32_t email = blockIdx.x;
    if (email >= A.b.n) return;                        // (the whole workgroup)
    if (ZKE_PARSE_PRIO) __builtin_amdgcn_s_setprio(ZKE_PARSE_PRIO);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Three barriers per wave on every path (two with ZKE_HELPER_KEYDEC = 0), in the order key, post, join: the helper's are the
    // ones below, straight-line; wave 0 executes here whichever of its own parse_email did not reach.
    if (wave == 0) {
      if (lane_id() == 0) { box.keyed = ZKE_HELPER_KEYDEC ? 0 : 1; box.key_go = 0; box.posted = 0; box.joined = 0; }      // (two-barrier build: the key counts as done)
      parse_email<true, 0, true>(A, email, L, &box);
      if (!uni(box.keyed)) wg_barrier();               // (key_go = 0 since the initialisation above)
      if (!uni(box.posted)) {
        if (lane_id() == 0) box.go = 0;
        wg_barrier();
      }
      if (!uni(box.joined)) wg_barrier();
    } else {
      if constexpr (ZKE_HELPER_KEYDEC) {
        // the key stage, on nothing but the batch's key columns: decoded and routed before wave 0 has split the headers
        Pkcs1 pk{0, 0, 0, 0};
        RsaModBytes mod{};
        uint32_t kr = 0;
        const bool rsa_key = uni(A.b.key_type[email]) == ZKE_KEY_RSA;
        if (rsa_key) {
          const uint64_t k0 = A.b.key_off[email], k1 = A.b.key_off[email + 1];
          const Str key = mkstr(A.b.key + k0, (uint32_t)(k1 - k0));
          uint32_t even = 0;
          kr = uni(decode_rsa_key_compute(key, pk, even, mod));
          uint32_t route = 0x800;         // no cache, no lane-group kernel in this launch, or an exponent / modulus they do not take
          if (!kr && A.cache && A.route_mask && pk.e == 65537 && !even) route = rsa_route(key, pk.np, pk.nl, pk.bits, A.cache, A.route_mask);
          if (lane_id() == 0) { box.kr = kr; box.bits = pk.bits; box.even = even; box.route = route; }
        }
        wg_barrier();                                    // key
        if (rsa_key && !kr && uni(box.key_go)) decode_rsa_key_store(A.b.rsa + email, pk, mod);
      }
      wg_barrier();                                    // post
      if (uni(box.go)) {
        uint32_t full, src_is_raw;
        canon_body_compute(canon_where(A.b, email, uni(box.body_off)), uni(box.flags), uni(box.blen), canon_lds, full, src_is_raw);
        if (lane_id() == 0) { box.full = full; box.src_is_raw = src_is_raw; }
        // region B is complete before wave 0 may write it (the fallback)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      wg_barrier();                                    // join
    }
  } else {
#if ZKE_PARSE_WG_WAVES > 1
    // dynamic LDS (W * sizeof(ParseLds), given at launch): with the size in sight the compiler takes the kernel's occupancy
    // for LDS-bound at 4 waves per SIMD and spends 109 registers — the point of W is that the front end stays at 80
    extern __shared__ __attribute__((aligned(16))) uint8_t parse_lds_raw[];
    ParseLds* L = reinterpret_cast<ParseLds*>(parse_lds_raw);
#else
    __shared__ ParseLds L[1];
#endif
    const uint32_t wave = ZKE_PARSE_WG_WAVES > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    const uint32_t email = blockIdx.x * ZKE_PARSE_WG_WAVES + wave;
    if (email >= A.b.n) return;
    if (ZKE_PARSE_PRIO) __builtin_amdgcn_s_setprio(ZKE_PARSE_PRIO);
    parse_email(A, email, L[wave]);
  }
}

// CSR (blob, off[n+1]) -> ShaJob list with digests packed 32 B apart (building-block entry point)
__global__ void sha_jobs_from_csr_kernel(const uint8_t* blob, const uint64_t* off, uint32_t n, uint8_t* digests, ShaJob* jobs) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ShaJob j;
  j.src = (uint64_t)(blob + off[i]);
  j.dst = (uint64_t)(digests + (size_t)i * 32);
  j.len = (uint32_t)(off[i + 1] - off[i]);
  j.pad = 0;
  jobs[i] = j;
}

}  // namespace zke
