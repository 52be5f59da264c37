// mixed_plan_fuzz.cpp — the host plan of a mixed regex batch (zkemail.rs_amd/csrc/mixed_plan.hip.h) over random config_of arrays
// and configs, under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_mixed_plan_sanitizers.py).  The header makes no
// HIP call, so this is plain C++ with its own main(): nothing is loaded into another process, nothing runs on a GPU.
//
// Checked for every accepted input: perm is a permutation of the e-mails that have a config, grouped by config and stable; the
// segments tile perm exactly once per (config, part); the block ranges of each launch are contiguous and sum to its grid; job_off
// is the prefix sum of P; configs without e-mails have no blocks; the LDS sizes and flags follow the cap.  Every refused input is
// refused before a write: the plan handed in comes back as it was.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../zkemail.rs_amd/csrc/mixed_plan.hip.h"

using namespace zke;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { if (g_fail++ < 20) fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static MixedPlan sentinel() {
  MixedPlan p;
  p.shape.m = 7; p.shape.J = 9; p.shape.n_segs = 11;
  p.job_off = {1, 2, 3}; p.email_cfg = {4}; p.perm = {5, 6}; p.cfg_first = {7};
  p.segs.resize(2); p.segs[1].part = 42;
  p.n_lane = 3; p.lane_blocks = 8; p.wave_blocks = 9; p.lane_lds = 77; p.wave_lds = 88;
  return p;
}
static bool untouched(const MixedPlan& p) {
  const MixedPlan s = sentinel();
  return p.shape.m == s.shape.m && p.shape.J == s.shape.J && p.shape.n_segs == s.shape.n_segs && p.job_off == s.job_off &&
         p.email_cfg == s.email_cfg && p.perm == s.perm && p.cfg_first == s.cfg_first && p.segs.size() == 2 && p.segs[1].part == 42 &&
         p.n_lane == 3 && p.lane_blocks == 8 && p.wave_blocks == 9 && p.lane_lds == 77 && p.wave_lds == 88;
}

static void check_plan(const std::vector<uint32_t>& config_of, const std::vector<MixedConfigIn>& cfgs, const std::vector<MixedPartIn>& parts,
                       uint32_t mapping, const MixedPlan& p) {
  const uint32_t n = (uint32_t)config_of.size(), C = (uint32_t)cfgs.size();
  auto P = [&](uint32_t c) { return cfgs[c].n_header_parts + cfgs[c].n_body_parts; };
  // job_off: the prefix sum of P; email_cfg
  CHECK(p.job_off.size() == (size_t)n + 1 && p.email_cfg.size() == n);
  uint32_t j = 0, m = 0;
  for (uint32_t i = 0; i < n; i++) {
    CHECK(p.job_off[i] == j);
    if (config_of[i] == MIXED_NONE) { CHECK(p.email_cfg[i] == MIXED_CFG_NONE); continue; }
    const MixedConfigIn& cf = cfgs[config_of[i]];
    CHECK(p.email_cfg[i] == (cf.n_header_parts | (cf.n_body_parts ? MIXED_CFG_HAS_BODY : 0u)));
    CHECK(p.email_cfg[i] != MIXED_CFG_NONE);
    j += P(config_of[i]); m++;
  }
  CHECK(p.job_off[n] == j && p.shape.J == j && p.shape.m == m);
  // perm: a permutation of the e-mails with a config, grouped by config, stable
  CHECK(p.perm.size() == m && p.cfg_first.size() == (size_t)C + 1 && p.cfg_first[0] == 0 && p.cfg_first[C] == m);
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t c = 0; c < C; c++) {
    CHECK(p.cfg_first[c] <= p.cfg_first[c + 1]);
    for (uint32_t k = p.cfg_first[c]; k < p.cfg_first[c + 1]; k++) {
      const uint32_t i = p.perm[k];
      CHECK(i < n);
      if (i >= n) continue;
      CHECK(config_of[i] == c && !seen[i]);
      seen[i] = 1;
      if (k > p.cfg_first[c]) CHECK(p.perm[k - 1] < i);            // stable: ascending inside a config
    }
  }
  for (uint32_t i = 0; i < n; i++) CHECK((seen[i] != 0) == (config_of[i] != MIXED_NONE));
  // segments: one per (config, part), each in exactly one launch; block ranges contiguous per launch and summing to its grid
  uint32_t S = 0;
  std::vector<uint32_t> base(C + 1, 0);
  for (uint32_t c = 0; c < C; c++) { S += P(c); base[c + 1] = S; }
  CHECK(p.segs.size() == S && p.shape.n_segs == S && p.n_lane <= S);
  std::vector<uint8_t> have(S, 0);
  size_t lds[2] = {1024, 1024};
  for (int wave = 0; wave < 2; wave++) {
    const uint32_t lo = wave ? p.n_lane : 0, hi = wave ? S : p.n_lane, per = wave ? MIXED_WAVE_BLOCK : MIXED_LANE_BLOCK;
    uint32_t block = 0;
    for (uint32_t k = lo; k < hi; k++) {
      const MixedSeg& s = p.segs[k];
      CHECK(s.config < C);
      if (s.config >= C) continue;
      const uint32_t nh = cfgs[s.config].n_header_parts;
      CHECK(s.part < P(s.config));
      if (s.part >= P(s.config)) continue;
      const uint32_t id = base[s.config] + s.part;
      CHECK(!have[id]);
      have[id] = 1;
      CHECK(s.is_body == (s.part >= nh ? 1u : 0u));
      CHECK((s.part >= mixed_wave_from(mapping, n, nh, P(s.config))) == (wave != 0));
      CHECK(s.first == p.cfg_first[s.config] && s.count == p.cfg_first[s.config + 1] - s.first);      // the config's whole range of perm
      CHECK(s.block0 == block && s.block_end == block + (s.count + per - 1) / per);
      if (!s.count) CHECK(s.block_end == s.block0);               // an empty config has no blocks
      if (s.count) CHECK((uint64_t)(s.block_end - s.block0) * per >= s.count && (uint64_t)(s.block_end - s.block0 - 1) * per < s.count);
      block = s.block_end;
      const MixedPartIn& pi = parts[id];
      CHECK(s.re == pi.dev && s.decode_detail == pi.detail);
      const bool fits = pi.dev && pi.lds_bytes + 1024 <= MIXED_LDS_CAP;
      CHECK(s.lds_tables == (fits ? 1u : 0u));
      CHECK(s.idle == ((pi.dev && wave) ? pi.idle : 0xFFFFFFFFu));
      if (s.count && fits) lds[wave] = std::max(lds[wave], pi.lds_bytes + 1024);
      if (k > lo) CHECK(p.segs[k - 1].config < s.config || (p.segs[k - 1].config == s.config && p.segs[k - 1].part < s.part));
    }
    CHECK((wave ? p.wave_blocks : p.lane_blocks) == block);
    // a block finds its segment as the kernels do: the first block_end beyond its index
    for (uint32_t b = 0; b < block; b += std::max<uint32_t>(1, block / 64)) {
      uint32_t a = lo, z = hi;
      while (a < z) { const uint32_t mid = (a + z) >> 1; if (p.segs[mid].block_end > b) z = mid; else a = mid + 1; }
      CHECK(a < hi && p.segs[a].block0 <= b && b < p.segs[a].block_end && p.segs[a].count);
    }
  }
  for (uint32_t id = 0; id < S; id++) CHECK(have[id]);
  CHECK(p.lane_lds == lds[0] && p.wave_lds == lds[1] && p.lane_lds <= MIXED_LDS_CAP && p.wave_lds <= MIXED_LDS_CAP);
  const MixedImage im = mixed_image(n, p.shape);
  CHECK(im.job_off % 16 == 0 && im.email_cfg % 16 == 0 && im.perm % 16 == 0 && im.segs % 16 == 0);
  CHECK(im.email_cfg >= im.job_off + ((size_t)n + 1) * 4 && im.perm >= im.email_cfg + (size_t)n * 4 && im.segs >= im.perm + (size_t)m * 4 &&
        im.total >= im.segs + (size_t)S * sizeof(MixedSeg));
}

int main() {
  std::mt19937 rng(20260917);
  auto rnd = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
  int accepted = 0, refused = 0;
  for (int round = 0; round < 6000; round++) {
    const uint32_t C = round % 97 == 0 ? MIXED_MAX_CONFIGS : rnd(0, round % 5 == 0 ? 64 : 6);
    std::vector<MixedConfigIn> cfgs(C);
    for (auto& c : cfgs) { c.n_header_parts = rnd(0, round % 7 == 0 ? 9 : 3); c.n_body_parts = rnd(0, round % 11 == 0 ? 9 : 2); }
    if (C && round % 13 == 0) cfgs[rnd(0, C - 1)] = MixedConfigIn{0, 0};                        // a zero-part config
    if (C && round % 211 == 0) cfgs[rnd(0, C - 1)] = MixedConfigIn{MIXED_MAX_PARTS - 3, 3};       // the part limit exactly
    uint32_t S = 0;
    for (auto& c : cfgs) S += c.n_header_parts + c.n_body_parts;
    std::vector<MixedPartIn> parts(S);
    for (auto& q : parts) {
      const uint32_t kind = rnd(0, 9);
      q.dev = kind == 0 ? 0 : 0x7f0000000000ull + 4096ull * rnd(1, 1000);
      q.lds_bytes = kind == 1 ? MIXED_LDS_CAP - 1024 + rnd(0, 2) - 1 : kind == 2 ? 900000 : rnd(16, 60000);
      q.idle = rnd(0, 3) ? 64 * rnd(1, 100) : 0xFFFFFFFFu;
      q.detail = q.dev ? 0 : rnd(1, 40);
    }
    const uint32_t sizes[] = {0, 1, 3, 4, 5, 255, 256, 257, 1024, 1025, 3000};
    const uint32_t n = round % 3 == 0 ? sizes[rnd(0, 10)] : rnd(0, 700);
    std::vector<uint32_t> config_of(n);
    const uint32_t skip = C ? rnd(0, C - 1) : 0;            // a config no e-mail names
    for (auto& c : config_of) {
      const uint32_t r = rnd(0, 9);
      c = (!C || r == 0) ? MIXED_NONE : rnd(0, C - 1);
      if (C > 1 && c == skip && round % 2) c = (skip + 1) % C;
    }
    if (round % 17 == 0) std::sort(config_of.begin(), config_of.end());
    const uint32_t mapping = rnd(0, 2);
    // refused variants first: each must leave the plan as it was
    {
      MixedPlan p = sentinel();
      if (n) {
        std::vector<uint32_t> bad = config_of;
        bad[rnd(0, n - 1)] = C + rnd(0, 5);                 // neither below n_configs nor ZKE_CONFIG_NONE
        CHECK(mixed_plan_build(bad.data(), n, cfgs.data(), C, parts.data(), mapping, p) != nullptr && untouched(p));
        bad[0] = 0xFFFFFFFEu;
        CHECK(mixed_plan_build(bad.data(), n, cfgs.data(), C, parts.data(), mapping, p) != nullptr && untouched(p));
        CHECK(mixed_plan_build(nullptr, n, cfgs.data(), C, parts.data(), mapping, p) != nullptr && untouched(p));
        refused += 3;
      }
      if (C) {
        std::vector<MixedConfigIn> big = cfgs;
        big[rnd(0, C - 1)] = MixedConfigIn{rnd(0, 1) ? MIXED_MAX_PARTS + 1 : 0xFFFFFFFFu, rnd(0, 1) ? 0u : 2u};
        std::vector<MixedPartIn> none(1);
        CHECK(mixed_plan_build(config_of.data(), n, big.data(), C, none.data(), mapping, p) != nullptr && untouched(p));
        CHECK(mixed_plan_build(config_of.data(), n, nullptr, C, parts.data(), mapping, p) != nullptr && untouched(p));
        if (S) CHECK(mixed_plan_build(config_of.data(), n, cfgs.data(), C, nullptr, mapping, p) != nullptr && untouched(p));
        refused += 2;
      }
      std::vector<MixedConfigIn> many(MIXED_MAX_CONFIGS + 1, MixedConfigIn{1, 0});
      std::vector<MixedPartIn> mp(MIXED_MAX_CONFIGS + 1, MixedPartIn{1, 16, 0, 0});
      CHECK(mixed_plan_build(config_of.data(), n, many.data(), MIXED_MAX_CONFIGS + 1, mp.data(), mapping, p) != nullptr && untouched(p));
      refused++;
    }
    MixedPlan p = round % 2 ? sentinel() : MixedPlan{};     // a plan is reusable: whatever it held is replaced
    const char* why = mixed_plan_build(config_of.data(), n, cfgs.data(), C, parts.data(), mapping, p);
    CHECK(why == nullptr);
    if (why) continue;
    MixedShape sh;
    CHECK(mixed_plan_check(config_of.data(), n, cfgs.data(), C, sh) == nullptr && sh.m == p.shape.m && sh.J == p.shape.J && sh.n_segs == p.shape.n_segs);
    check_plan(config_of, cfgs, parts, mapping, p);
    accepted++;
  }
  if (g_fail) { fprintf(stderr, "mixed_plan_fuzz: %d checks failed\n", g_fail); return 1; }
  printf("mixed_plan_fuzz ok: %d plans checked, %d inputs refused\n", accepted, refused);
  return 0;
}
