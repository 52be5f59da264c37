// capture.hip.h — capture-group extraction behind the regex stage: the device half of helpers/src/regex.rs:16-51
// (meta::Regex::captures over the input, the groups named by capture_indices as strings).
//
// The DFA kernels have already found, per (e-mail, part), the one match span [start, end) — leftmost-first, as
// meta::Regex finds it.  What is missing is where the groups lie inside it.  Because the span is known, no thread list is
// needed:
//   1. backward pass over the span: R[pos] = the set of NFA states from which `match` is reachable consuming exactly
//      hay[pos, end).  One lane per state, 64 states per ballot; epsilon states (look, union, capture) are closed by
//      sweeping their words until nothing changes (the compiler numbers a state's successors below it, so one sweep and
//      a second for the loop edges is the rule).
//   2. forward walk, wave-uniform: from the start state take at each step the first successor in priority order that is
//      in R[pos] and was not visited at this position; capture states record `pos` on the way.  That is the path the
//      leftmost-first PikeVM's winning thread takes.
// R is kept for 64 positions at a time: spans longer than that store every 64th row in the first pass ("checkpoints") and
// recompute one block of rows from its checkpoint when the walk enters it.  Rows live in LDS while the program has at most
// CAP_LDS_STATES states, else in the wave's slice of the slot's capture workspace (same code: generic pointers).
// The walk disagrees loudly: a span it cannot reproduce is ZKE_UNSUPPORTED / ZKE_D_U_CAPTURE_WALK, never a guess.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "regex.hip.h"

namespace zke {

constexpr uint32_t CAP_K = 64;                                   // positions per block of rows
constexpr uint32_t CAP_CK_ROWS = ZKE_CAP_MAX_SPAN / CAP_K + 1;   // checkpoint rows (index = position / CAP_K; row 0 unused)
constexpr uint32_t CAP_ROWS = CAP_CK_ROWS + 2 + CAP_K + 1;       // + the first pass's two rolling rows + one block
constexpr uint32_t CAP_MAX_WORDS = ZKE_CAP_MAX_STATES / 64;      // 64-state words per row
constexpr uint32_t CAP_LDS_WORDS = 8;                            // programs of up to 512 states keep their rows in LDS
constexpr uint32_t CAP_LDS_STATES = CAP_LDS_WORDS * 64;
constexpr uint32_t CAP_MAX_PARTS = 16;                           // parts of one extraction batch (kernel-argument table)
constexpr size_t CAP_WORK_WORDS = (size_t)CAP_ROWS * CAP_MAX_WORDS;   // u64 words of one wave's slice
static_assert(ZKE_CAP_MAX_SPAN % CAP_K == 0 && ZKE_CAP_MAX_STATES % 64 == 0 && ZKE_CAP_MAX_PROGRAM_GROUPS * 2 <= 64, "capture limits");

// state kinds of the capture program (zkemail.rs_amd/regex_compile.py)
enum : uint32_t { CAP_FAIL = 0, CAP_MATCH = 1, CAP_RANGE = 2, CAP_SPARSE = 3, CAP_LOOK = 4, CAP_UNION = 5, CAP_CAPTURE = 6 };
constexpr uint32_t CAP_NONE = 0xFFFFFFFFu;
constexpr uint8_t CAPF_NOT_UTF8 = ZKE_CAPF_NOT_UTF8;

struct CapProgDev {             // a registered program on the device (validated on the host: every index is in range)
  uint32_t n_states, n_groups, start, words64;
  const uint32_t* off;          // [n_states + 1] word offsets into st
  const uint32_t* st;
  const uint64_t* eps;          // [words64] bit q & 63 of word q >> 6: state q is an epsilon state
};

struct CapPartDev {
  CapProgDev prog;
  uint32_t code;                // != 0: the part cannot run (program unregistered / undecodable / over a limit): this detail
  uint32_t n_groups, gbase;     // requested groups; their first column among the e-mail's G
  uint32_t groups[ZKE_CAP_MAX_GROUPS];
};

struct CapArgs {
  uint32_t plain;               // 0: the parts of a regex batch (haystacks as dfa_haystack picks them); 1: plain haystacks
  uint32_t n, P, G;
  DfaArgs d;                    // plain == 0: b, scratch_v, clean ... as the DFA launches had them
  uint32_t n_header_parts;
  const uint8_t* hay_blob; const uint64_t* hay_off;      // plain == 1
  const PartRes* parts;         // [n * P]
  uint32_t* spans;              // [n * G * 2]
  uint8_t* flags;               // [n * G]
  uint32_t* codes;              // [n * P] 0 or the ZKE_D_* that fails the part
  uint64_t* work;               // [waves * CAP_WORK_WORDS]
  CapPartDev part[CAP_MAX_PARTS];
};

__device__ __forceinline__ void cap_sync() {       // rows are handed from lane to lane of ONE wave through memory
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ uint64_t cap_uni64(uint64_t x) { return ((uint64_t)uni((uint32_t)(x >> 32)) << 32) | uni((uint32_t)x); }
__device__ __forceinline__ bool cap_bit(const uint64_t* row, uint32_t q) { return (row[q >> 6] >> (q & 63)) & 1; }
__device__ __forceinline__ bool cap_word_byte(uint32_t c) { return c == '_' || (c - '0') < 10u || ((c | 0x20) - 'a') < 26u; }
// Look::{Start, End, StartLF, EndLF, WordAscii, WordAsciiNegate} at `pos` of the WHOLE haystack (not of the span)
__device__ __forceinline__ bool cap_look(uint32_t look, const uint8_t* hay, uint32_t hlen, uint32_t pos) {
  switch (look) {
    case 1: return pos == 0;
    case 2: return pos == hlen;
    case 4: return pos == 0 || hay[pos - 1] == '\n';
    case 8: return pos == hlen || hay[pos] == '\n';
    default: {
      const bool l = pos > 0 && cap_word_byte(hay[pos - 1]), r = pos < hlen && cap_word_byte(hay[pos]);
      return look == 64 ? l != r : l == r;
    }
  }
}
// the transition of consuming state (offset o, count cnt) on byte b: its target, or CAP_NONE
__device__ __forceinline__ uint32_t cap_step(const uint32_t* st, uint32_t o, uint32_t cnt, uint32_t b) {
  for (uint32_t k = 0; k < cnt; k++) {
    const uint32_t r = st[o + 1 + 2 * k];
    if (b >= (r & 0xff) && b <= ((r >> 8) & 0xff)) return st[o + 2 + 2 * k];
  }
  return CAP_NONE;
}

// R[pos] into `cur` (nxt = R[pos + 1]; unread when pos == end)
__device__ __forceinline__ void cap_row(const CapProgDev& Pg, const uint8_t* hay, uint32_t hlen, uint32_t pos, uint32_t end,
                                        const uint64_t* nxt, uint64_t* cur, int lane) {
  const uint32_t W = Pg.words64;
  const uint32_t b = pos < end ? hay[pos] : 0;
  for (uint32_t w = 0; w < W; w++) {                 // match and consuming states: decided by R[pos + 1] alone
    const uint32_t q = w * 64 + lane;
    bool on = false;
    if (q < Pg.n_states) {
      const uint32_t o = Pg.off[q], h = Pg.st[o], kind = h & 0xff;
      if (kind == CAP_MATCH) on = pos == end;
      else if ((kind == CAP_RANGE || kind == CAP_SPARSE) && pos < end) {
        const uint32_t t = cap_step(Pg.st, o, h >> 8, b);
        on = t != CAP_NONE && cap_bit(nxt, t);
      }
    }
    const uint64_t word = __ballot(on);
    if (lane == 0) cur[w] = word;
  }
  cap_sync();
  for (bool changed = true; changed;) {              // epsilon states: to a fixed point
    changed = false;
    for (uint32_t w = 0; w < W; w++) {
      const uint64_t em = cap_uni64(Pg.eps[w]);
      if (!em) continue;
      uint64_t word = cap_uni64(cur[w]);
      bool grew = false;
      for (;;) {
        bool on = false;
        if (((em & ~word) >> lane) & 1) {
          const uint32_t q = w * 64 + lane, o = Pg.off[q], h = Pg.st[o], kind = h & 0xff;
          auto live = [&](uint32_t t) { return (t >> 6) == w ? (bool)((word >> (t & 63)) & 1) : cap_bit(cur, t); };
          if (kind == CAP_UNION) { for (uint32_t k = 0, c = h >> 8; k < c && !on; k++) on = live(Pg.st[o + 1 + k]); }
          else if (kind == CAP_CAPTURE) on = live(Pg.st[o + 2]);
          else on = cap_look(Pg.st[o + 1], hay, hlen, pos) && live(Pg.st[o + 2]);
        }
        const uint64_t add = __ballot(on);
        if (!add) break;
        word |= add; grew = true;
      }
      if (grew) {
        if (lane == 0) cur[w] = word;
        cap_sync();
        changed = true;
      }
    }
  }
}

// The groups of the match [s0, end) of haystack `hay`: lane s gets slot s (2 * group, + 1 for its end; CAP_NONE: not set).
// Returns 0, or ZKE_D_U_CAPTURE_WALK.  `rows`: CAP_ROWS rows of Pg.words64 words (LDS or global), this wave's alone.
__device__ __forceinline__ uint32_t cap_walk(const CapProgDev& Pg, const uint8_t* hay, uint32_t hlen, uint32_t s0, uint32_t end,
                                             uint64_t* rows, uint32_t& slot_out, int lane) {
  const uint32_t W = Pg.words64, L = end - s0;
  const uint32_t nb = L ? (L + CAP_K - 1) / CAP_K : 1;           // blocks; block j holds the rows of positions [j K, min((j + 1) K, L)]
  uint64_t* ck = rows;
  uint64_t* ring = rows + (size_t)CAP_CK_ROWS * W;
  uint64_t* blk = ring + 2 * (size_t)W;
  if (nb > 1) {                                                  // first pass: the checkpoints ck[1 .. nb - 1]
    const uint64_t* prev = nullptr;
    for (uint32_t r = L; r >= CAP_K; r--) {
      uint64_t* out = (r % CAP_K == 0) ? ck + (size_t)(r / CAP_K) * W : ring + (size_t)(r & 1) * W;
      cap_row(Pg, hay, hlen, s0 + r, end, prev, out, lane);
      prev = out;
    }
  }
  uint32_t slot = CAP_NONE;
  uint64_t vis0 = 0, vis1 = 0;                                   // visited at this position: lane l holds words l and l + 64
  auto visited = [&](uint32_t q) {
    const uint32_t w = q >> 6;
    const uint64_t a = __shfl(vis0, w & 63), b2 = __shfl(vis1, w & 63);
    return (bool)(((w < 64 ? a : b2) >> (q & 63)) & 1);
  };
  uint32_t q = Pg.start, pos = s0, cur_block = CAP_NONE;
  // every epsilon step visits a state not visited at this position, every other step consumes a byte: the bound is never the exit
  for (uint64_t steps = 0, max_steps = ((uint64_t)L + 1) * ((uint64_t)Pg.n_states + 1); steps <= max_steps; steps++) {
    const uint32_t r = pos - s0;
    const uint32_t j = r / CAP_K < nb ? r / CAP_K : nb - 1;
    if (j != cur_block) {
      const uint32_t lo = j * CAP_K, top = lo + CAP_K < L ? lo + CAP_K : L;
      if (top == L) cap_row(Pg, hay, hlen, end, end, nullptr, blk + (size_t)(top - lo) * W, lane);
      else {
        for (uint32_t w = lane; w < W; w += 64) blk[(size_t)(top - lo) * W + w] = ck[(size_t)(j + 1) * W + w];
        cap_sync();
      }
      for (uint32_t x = top; x-- > lo;) cap_row(Pg, hay, hlen, s0 + x, end, blk + (size_t)(x + 1 - lo) * W, blk + (size_t)(x - lo) * W, lane);
      cur_block = j;
    }
    const uint64_t* row = blk + (size_t)(r - j * CAP_K) * W;
    if (steps == 0 && !cap_bit(row, q)) return ZKE_D_U_CAPTURE_WALK;       // the program does not match the DFA pair's span
    const uint32_t o = uni(Pg.off[q]), h = uni(Pg.st[o]), kind = h & 0xff, cnt = h >> 8;
    if (kind == CAP_MATCH) { slot_out = slot; return pos == end ? 0u : (uint32_t)ZKE_D_U_CAPTURE_WALK; }
    if (kind == CAP_RANGE || kind == CAP_SPARSE) {
      if (pos >= end) return ZKE_D_U_CAPTURE_WALK;
      const uint32_t t = uni(cap_step(Pg.st, o, cnt, hay[pos]));
      if (t == CAP_NONE) return ZKE_D_U_CAPTURE_WALK;
      q = t; pos++; vis0 = 0; vis1 = 0;
      continue;
    }
    if (kind == CAP_FAIL) return ZKE_D_U_CAPTURE_WALK;
    {
      const uint32_t w = q >> 6;
      if ((uint32_t)lane == (w & 63)) { if (w < 64) vis0 |= 1ull << (q & 63); else vis1 |= 1ull << (q & 63); }
    }
    uint32_t nx = CAP_NONE;
    if (kind == CAP_UNION) {
      for (uint32_t base = 0; base < cnt && nx == CAP_NONE; base += 64) {
        const uint32_t k = base + lane;
        const uint32_t t = k < cnt ? Pg.st[o + 1 + k] : 0;
        const bool seen = visited(t);                  // (every lane takes part in the shuffle)
        const uint64_t m = __ballot(k < cnt && cap_bit(row, t) && !seen);
        if (m) nx = uni(Pg.st[o + 1 + base + (uint32_t)__builtin_ctzll(m)]);
      }
    } else {
      const uint32_t a = uni(Pg.st[o + 1]), t = uni(Pg.st[o + 2]);
      const bool seen = visited(t);
      bool ok = cap_bit(row, t) && !seen;
      if (kind == CAP_CAPTURE) { if ((uint32_t)lane == a) slot = pos; }
      else ok = ok && cap_look(a, hay, hlen, pos);
      if (ok) nx = t;
    }
    if (nx == CAP_NONE) return ZKE_D_U_CAPTURE_WALK;
    q = nx;
  }
  return ZKE_D_U_CAPTURE_WALK;
}

// Item `item` of a capture launch — one (e-mail, part) — by one wave: the walk over the match `pr` the search left, the requested
// groups into the part's columns (`row`: the e-mail's first column; the part's follow from its gbase), the capture verdict into
// codes[item].  hay_of(hay, hlen): the part's haystack, asked for only when the part is walked.  Rows: lds_rows for programs of at
// most CAP_LDS_STATES states, else this wave's slice of `work`.
template <class HayOf>
__device__ __forceinline__ void cap_item(const CapPartDev& part, const PartRes pr, HayOf hay_of, uint64_t* lds_rows, uint64_t* work,
                                         uint32_t* spans, uint8_t* flags, size_t row, uint32_t* codes, uint32_t item, int lane) {
  uint32_t code = 0;
  // every part the search left with exactly one match is walked, whatever the regex fold has written into the record meanwhile:
  // the fold of the gather launch needs the capture verdict of the parts IN FRONT of a part that fails on its match count
  const bool run = pr.code == 0 && pr.count == 1;
  uint32_t slot = CAP_NONE;
  const uint8_t* hay = nullptr; uint32_t hlen = 0;
  if (run) {
    if (part.code) code = part.code;
    else if (pr.end - pr.start > ZKE_CAP_MAX_SPAN) code = ZKE_D_U_CAPTURE_SPAN;
    else {
      hay_of(hay, hlen);
      uint64_t* rows = part.prog.words64 <= CAP_LDS_WORDS ? lds_rows : work + (size_t)blockIdx.x * CAP_WORK_WORDS;
      code = cap_walk(part.prog, hay, hlen, pr.start, pr.end, rows, slot, lane);
    }
  }
  // the requested groups: lane k answers for groups[k]
  const uint32_t ng = part.n_groups;
  uint32_t gs = CAP_NONE, ge = CAP_NONE;
  bool missing = false;
  {
    const uint32_t g = (uint32_t)lane < ng ? part.groups[lane] : 0;
    const bool inprog = g < part.prog.n_groups;
    const uint32_t a = __shfl(slot, (2 * g) & 63), b = __shfl(slot, (2 * g + 1) & 63);
    if (run && !code && (uint32_t)lane < ng) {
      if (inprog && a != CAP_NONE && b != CAP_NONE && a <= b) { gs = a; ge = b; }
      else missing = true;                         // "Capture group not found"  helpers/src/regex.rs:31
    }
  }
  if (run && !code && __ballot(missing)) code = ZKE_D_RE_GROUP_MISSING;
  if ((uint32_t)lane < ng) {
    const size_t col = row + part.gbase + lane;
    const bool have = run && !code;
    spans[2 * col] = have ? gs : CAP_NONE;
    spans[2 * col + 1] = have ? ge : CAP_NONE;
    flags[col] = have && !utf8_valid(hay + gs, ge - gs) ? CAPF_NOT_UTF8 : 0;
  }
  if (lane == 0) codes[item] = code;
  cap_sync();                                      // the next item reuses the rows
}

// One wave per (e-mail, part); the host bounds the grid (CAP_WORK_WAVES when rows live in the workspace) and each wave loops.  blockDim = 64.
__global__ __launch_bounds__(64) void capture_kernel(CapArgs A) {
  __shared__ uint64_t lds_rows[CAP_ROWS * CAP_LDS_WORDS];
  const int lane = threadIdx.x;
  const uint32_t items = A.n * A.P;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t i = item / A.P, p = item % A.P;
    const CapPartDev& part = A.part[p];
    cap_item(part, A.parts[item],
             [&](const uint8_t*& hay, uint32_t& hlen) {
               if (A.plain) { hay = A.hay_blob + A.hay_off[i]; hlen = (uint32_t)(A.hay_off[i + 1] - A.hay_off[i]); }
               else { DfaArgs D = A.d; D.is_body = p >= A.n_header_parts ? 1u : 0u; dfa_haystack(D, i, A.d.b.meta + i, hay, hlen); }
             },
             lds_rows, A.work, A.spans, A.flags, (size_t)i * A.G, A.codes, item, lane);
  }
}

// The match of every plain haystack (zke_capture_batch): process_regex_parts' search without a capture table, one haystack per lane.
struct CapFindArgs { DfaArgs d; const uint8_t* hay_blob; const uint64_t* hay_off; uint32_t n; };
__global__ __launch_bounds__(256) void capture_find_kernel(CapFindArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dlds[];
  DfaLds F{}, Rv{};
  const bool valid = dfa_stage(A.d, dlds, F, Rv);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  PartRes pr{PART_DECODE_FAIL, A.d.decode_detail, 0, 0};
  if (valid) pr = dfa_part(A.d, F, Rv, i, A.hay_blob + A.hay_off[i], (uint32_t)(A.hay_off[i + 1] - A.hay_off[i]), DfaAccel{0, 0, 0, false});
  A.d.out[i] = pr;
}

// The tables in the form the verify entry takes (zke_batch.cap_off / cap_str_off / cap_blob), and the capture verdict folded
// into the records.  ONE workgroup of 1024 threads: lengths -> exclusive scan -> gather.  hdr: [0] strings, [1] blob bytes needed.
struct CapGatherArgs {
  uint32_t plain, n, P, G, n_header_parts;
  DfaArgs d;
  const uint8_t* hay_blob; const uint64_t* hay_off;
  const PartRes* parts; const uint32_t* codes; uint32_t* spans;
  zke_result* results;          // plain == 0
  uint32_t* cap_off;            // [n * P + 1]
  uint32_t* cap_str_off;        // [n * G + 1]
  uint8_t* cap_blob; uint64_t blob_cap;
  uint64_t* hdr;
  uint32_t* tmp;                // [n * P + n * G] scratch: strings per (e-mail, part), bytes per column
  uint32_t gbase[CAP_MAX_PARTS + 1];
};

// exclusive scan of v[0, cnt) in place by the whole block; returns the total.  `sh`: 1024 + 1 words of LDS.
__device__ __forceinline__ uint64_t cap_block_scan(uint32_t* v, size_t cnt, uint64_t* sh) {
  const uint32_t T = blockDim.x, t = threadIdx.x;
  const size_t per = (cnt + T - 1) / T, lo = (size_t)t * per, hi = lo + per < cnt ? lo + per : cnt;
  uint64_t sum = 0;
  for (size_t k = lo; k < hi; k++) sum += v[k];
  sh[t] = sum;
  __syncthreads();
  if (t == 0) { uint64_t acc = 0; for (uint32_t k = 0; k < T; k++) { const uint64_t x = sh[k]; sh[k] = acc; acc += x; } sh[T] = acc; }
  __syncthreads();
  uint64_t acc = sh[t];
  for (size_t k = lo; k < hi; k++) { const uint32_t x = v[k]; v[k] = (uint32_t)acc; acc += x; }
  const uint64_t total = sh[T];
  __syncthreads();
  return total;
}

// Verdict of one e-mail, ONE fold over its P parts in verify order as compile_regex_parts walks them (helpers/src/regex.rs:21-47:
// the match count of a part, then its groups, then the next part).  The regex fold in front of the gather launch has named the first
// part whose SEARCH fails (decode, quit, match count); a part in front of that one whose capture fails takes the record over.
// regex_part == 0xFFFFFFFF: the regex fold never looked at a part (DKIM or canonicalisation failed) — the record stands.
// `parts`, `codes`: the e-mail's own P entries; nh: its config's header parts.  Returns whether the e-mail yields strings.
__device__ __forceinline__ bool cap_fold_email(zke_result* R, const PartRes* parts, const uint32_t* codes, uint32_t P, uint32_t nh) {
  bool ok = true;
  if (R->regex_part == CAP_NONE) ok = false;
  for (uint32_t p = 0; p < P && ok; p++) {
    const PartRes pr = parts[p];
    const uint32_t code = codes[p];
    if (pr.code != 0 || pr.count != 1) ok = false;            // the part the regex fold named (or one it skipped behind it)
    else if (code) {
      R->status = code == ZKE_D_RE_GROUP_MISSING ? (p < nh ? ZKE_HEADER_REGEX_FAIL : ZKE_BODY_REGEX_FAIL) : ZKE_UNSUPPORTED;
      R->detail = code;
      R->regex_part = p; R->match_count = pr.count; R->match_start = pr.start; R->match_end = pr.end;
      ok = false;
    }
  }
  return ok;
}
// The lengths of one (e-mail, part): the strings it yields into *nstr, the bytes of each of its ng columns into nbytes[0, ng);
// spans: the {start, end} pairs of those columns — a part that yields no strings yields no span either.
__device__ __forceinline__ void cap_part_lengths(bool part_ok, uint32_t ng, uint32_t* nstr, uint32_t* nbytes, uint32_t* spans) {
  *nstr = part_ok ? ng : 0;
  for (uint32_t c = 0; c < ng; c++) {
    const uint32_t s = spans[2 * c], e = spans[2 * c + 1];
    nbytes[c] = part_ok && s != CAP_NONE ? e - s : 0;
    if (!part_ok) { spans[2 * c] = CAP_NONE; spans[2 * c + 1] = CAP_NONE; }
  }
}
// One column's string into the tables: string `sidx` of `strings` starts at byte `at` of `bytes`; its bytes are hay[s, e) of the
// haystack hay_of() names (asked for only when the bytes fit the caller's blob).
template <class HayOf>
__device__ __forceinline__ void cap_put_string(uint32_t sidx, uint32_t at, uint32_t s, uint32_t e, uint64_t strings, uint64_t bytes,
                                               uint32_t* cap_str_off, uint8_t* cap_blob, uint64_t blob_cap, HayOf hay_of) {
  cap_str_off[sidx] = at;
  if (sidx + 1 == strings) cap_str_off[strings] = (uint32_t)bytes;
  const uint32_t len = e - s;
  if ((uint64_t)at + len > blob_cap) return;          // the caller's blob is too small: sizes are reported, nothing is cut short silently
  const uint8_t* hay = hay_of();
  for (uint32_t k = 0; k < len; k++) cap_blob[at + k] = hay[s + k];
}

__global__ __launch_bounds__(1024) void capture_gather_kernel(CapGatherArgs A) {
  __shared__ uint64_t sh[1025];
  const uint32_t T = blockDim.x, t = threadIdx.x;
  uint32_t* nstr = A.tmp;                              // [n * P]
  uint32_t* nbytes = A.tmp + (size_t)A.n * A.P;        // [n * G]
  for (uint32_t i = t; i < A.n; i += T) {
    const bool ok = A.plain ? true : cap_fold_email(A.results + i, A.parts + (size_t)i * A.P, A.codes + (size_t)i * A.P, A.P, A.n_header_parts);
    for (uint32_t p = 0; p < A.P; p++) {
      const bool part_ok = A.plain ? (A.codes[(size_t)i * A.P + p] == 0 && A.parts[(size_t)i * A.P + p].code == 0 && A.parts[(size_t)i * A.P + p].count == 1) : ok;
      const size_t col = (size_t)i * A.G + A.gbase[p];
      cap_part_lengths(part_ok, A.gbase[p + 1] - A.gbase[p], nstr + (size_t)i * A.P + p, nbytes + col, A.spans + 2 * col);
    }
  }
  __syncthreads();
  const size_t NP = (size_t)A.n * A.P, NG = (size_t)A.n * A.G;
  // which columns hold a string, before the scans overwrite the counts: a column is a string iff its part yields strings
  const uint64_t strings = cap_block_scan(nstr, NP, sh);
  for (size_t k = t; k < NP; k += T) A.cap_off[k] = nstr[k];
  if (t == 0) A.cap_off[NP] = (uint32_t)strings;
  const uint64_t bytes = cap_block_scan(nbytes, NG, sh);
  if (t == 0) { A.hdr[0] = strings; A.hdr[1] = bytes; }
  // strings in column order: string index = cap_off[i * P + p] + (c - gbase[p])
  for (size_t col = t; col < NG; col += T) {
    const uint32_t i = (uint32_t)(col / A.G), c = (uint32_t)(col % A.G);
    uint32_t p = 0;
    while (p + 1 < A.P && c >= A.gbase[p + 1]) p++;
    const size_t ip = (size_t)i * A.P + p;
    const uint32_t first = A.cap_off[ip], cnt = A.cap_off[ip + 1] - first;
    if (!cnt) continue;
    cap_put_string(first + (c - A.gbase[p]), nbytes[col], A.spans[2 * col], A.spans[2 * col + 1], strings, bytes, A.cap_str_off, A.cap_blob, A.blob_cap,
                   [&]() -> const uint8_t* {
                     const uint8_t* hay; uint32_t hlen;
                     if (A.plain) { hay = A.hay_blob + A.hay_off[i]; hlen = 0; }
                     else { DfaArgs D = A.d; D.is_body = p >= A.n_header_parts ? 1u : 0u; dfa_haystack(D, i, A.d.b.meta + i, hay, hlen); }
                     (void)hlen;
                     return hay;
                   });
  }
  if (t == 0 && strings == 0) A.cap_str_off[0] = 0;
}

}  // namespace zke
