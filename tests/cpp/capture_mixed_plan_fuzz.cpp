// capture_mixed_plan_fuzz.cpp — the ragged half of the host plan of a mixed extraction (zke_extract_captures_mixed;
// zkemail.rs_amd/csrc/mixed_plan.hip.h: capmix_plan_check / capmix_plan_build / capmix_image) over random configs and config_of
// arrays, under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_capture_mixed_plan_sanitizers.py).  Plain C++ with its own
// main(): the header makes no HIP call.
//
// Checked for every accepted input, against a naive recomputation: col_off is the prefix sum of the configs' requested groups and
// agrees with job_off of the verify plan built from the same input; cap_cfg; per config {first part, header parts, G, first body
// column}; gbase per part; a column finds its e-mail and its part as the kernels do.  Every ZKE_E_ARG condition is refused before a
// write — the plan handed in comes back as it was —, and the column limit is exact: Gt = 2^20 - 1 passes, Gt = 2^20 does not.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../zkemail.rs_amd/csrc/mixed_plan.hip.h"

using namespace zke;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { if (g_fail++ < 20) fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static CapMixedPlan sentinel() {
  CapMixedPlan p;
  p.shape.J = 5; p.shape.Gt = 6; p.shape.n_parts = 7; p.shape.body_groups = true;
  p.col_off = {9, 8}; p.cap_cfg = {7}; p.gbase = {1, 2, 3};
  p.cfgs.resize(2); p.cfgs[1] = CapMixedCfg{11, 12, 13, 14};
  return p;
}
static bool untouched(const CapMixedPlan& p) {
  const CapMixedPlan s = sentinel();
  return p.shape.J == 5 && p.shape.Gt == 6 && p.shape.n_parts == 7 && p.shape.body_groups && p.col_off == s.col_off && p.cap_cfg == s.cap_cfg &&
         p.gbase == s.gbase && p.cfgs.size() == 2 && p.cfgs[1].part0 == 11 && p.cfgs[1].nh == 12 && p.cfgs[1].G == 13 && p.cfgs[1].gb0 == 14;
}
// the kernels' search: the first i with off[i + 1] > x
static uint32_t owner(const std::vector<uint32_t>& off, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (off[mid + 1] > x) hi = mid; else lo = mid + 1; }
  return lo;
}

static void check_plan(const std::vector<uint32_t>& config_of, const std::vector<MixedConfigIn>& cfgs, const std::vector<uint32_t>& groups,
                       const CapMixedPlan& p) {
  const uint32_t n = (uint32_t)config_of.size(), C = (uint32_t)cfgs.size();
  // naive: per config its parts' first index, G, gb0
  std::vector<uint32_t> part0(C), G(C), gb0(C), P(C);
  uint32_t at = 0;
  bool body_groups = false;
  for (uint32_t c = 0; c < C; c++) {
    part0[c] = at; P[c] = cfgs[c].n_header_parts + cfgs[c].n_body_parts; G[c] = 0; gb0[c] = 0;
    for (uint32_t q = 0; q < P[c]; q++) {
      if (q < cfgs[c].n_header_parts) gb0[c] += groups[at + q];
      else if (groups[at + q]) body_groups = true;
      G[c] += groups[at + q];
    }
    at += P[c];
  }
  CHECK(p.shape.n_parts == at && p.gbase.size() == at && p.cfgs.size() == C && p.shape.body_groups == body_groups);
  for (uint32_t c = 0; c < C; c++) {
    CHECK(p.cfgs[c].part0 == part0[c] && p.cfgs[c].nh == cfgs[c].n_header_parts && p.cfgs[c].G == G[c] && p.cfgs[c].gb0 == gb0[c]);
    uint32_t g = 0;
    for (uint32_t q = 0; q < P[c]; q++) { CHECK(p.gbase[part0[c] + q] == g); g += groups[part0[c] + q]; }
  }
  CHECK(p.col_off.size() == (size_t)n + 1 && p.cap_cfg.size() == n);
  uint64_t col = 0, job = 0;
  std::vector<uint32_t> job_off(n + 1);
  for (uint32_t i = 0; i < n; i++) {
    CHECK(p.col_off[i] == col);
    job_off[i] = (uint32_t)job;
    const uint32_t c = config_of[i];
    CHECK(p.cap_cfg[i] == c);
    if (c == MIXED_NONE) continue;
    col += G[c]; job += P[c];
  }
  job_off[n] = (uint32_t)job;
  CHECK(p.col_off[n] == col && p.shape.Gt == col && p.shape.J == job);
  // the verify plan of the same input numbers the jobs alike
  MixedShape vs;
  CHECK(mixed_plan_check(config_of.data(), n, cfgs.data(), C, vs) == nullptr && vs.J == p.shape.J);
  // a job and a column find their e-mail, the column its part, as the kernels do (sampled)
  const uint32_t Gt = p.shape.Gt, J = p.shape.J;
  for (uint32_t x = 0; x < J; x += std::max<uint32_t>(1, J / 97)) {
    const uint32_t i = owner(job_off, n, x);
    CHECK(i < n && job_off[i] <= x && x < job_off[i + 1] && config_of[i] != MIXED_NONE);
  }
  for (uint32_t x = 0; x < Gt; x += std::max<uint32_t>(1, Gt / 97)) {
    const uint32_t i = owner(p.col_off, n, x);
    CHECK(i < n && p.col_off[i] <= x && x < p.col_off[i + 1]);
    if (i >= n || config_of[i] == MIXED_NONE) { CHECK(false); continue; }
    const CapMixedCfg& cf = p.cfgs[config_of[i]];
    const uint32_t c = x - p.col_off[i], Pi = job_off[i + 1] - job_off[i];
    uint32_t q = 0;
    while (q + 1 < Pi && c >= p.gbase[cf.part0 + q + 1]) q++;
    CHECK(c >= p.gbase[cf.part0 + q] && c - p.gbase[cf.part0 + q] < groups[cf.part0 + q]);
  }
  const CapMixedImage im = capmix_image(n, C, p.shape, 120);
  CHECK(im.col_off % 16 == 0 && im.cap_cfg % 16 == 0 && im.cfgs % 16 == 0 && im.parts % 16 == 0);
  CHECK(im.cap_cfg >= im.col_off + ((size_t)n + 1) * 4 && im.cfgs >= im.cap_cfg + (size_t)n * 4 && im.parts >= im.cfgs + (size_t)C * sizeof(CapMixedCfg) &&
        im.total >= im.parts + (size_t)at * 120);
}

int main() {
  std::mt19937 rng(20261021);
  auto rnd = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
  int accepted = 0, refused = 0;
  for (int round = 0; round < 6000; round++) {
    const uint32_t C = round % 97 == 0 ? MIXED_MAX_CONFIGS : rnd(0, round % 5 == 0 ? 64 : 6);
    std::vector<MixedConfigIn> cfgs(C);
    for (auto& c : cfgs) {
      const uint32_t P = round % 7 == 0 ? rnd(1, CAPMIX_MAX_PARTS) : rnd(1, 5);
      c.n_header_parts = rnd(0, P); c.n_body_parts = P - c.n_header_parts;
    }
    uint32_t S = 0;
    for (auto& c : cfgs) S += c.n_header_parts + c.n_body_parts;
    std::vector<uint32_t> groups(S + 1);
    for (auto& g : groups) g = rnd(0, 3) == 0 ? 0 : rnd(0, round % 11 == 0 ? CAPMIX_MAX_GROUPS : 3);
    if (C && round % 13 == 0) {                              // a config with no requested group at all
      const uint32_t c = rnd(0, C - 1);
      uint32_t at = 0;
      for (uint32_t k = 0; k < c; k++) at += cfgs[k].n_header_parts + cfgs[k].n_body_parts;
      for (uint32_t q = 0; q < cfgs[c].n_header_parts + cfgs[c].n_body_parts; q++) groups[at + q] = 0;
    }
    const uint32_t sizes[] = {0, 1, 3, 64, 255, 256, 257, 1024, 1025, 3000};
    const uint32_t n = round % 3 == 0 ? sizes[rnd(0, 9)] : rnd(0, 700);
    std::vector<uint32_t> config_of(n);
    const uint32_t skip = C ? rnd(0, C - 1) : 0;             // a config no e-mail names
    for (auto& c : config_of) {
      c = (!C || rnd(0, 9) == 0) ? MIXED_NONE : rnd(0, C - 1);
      if (C > 1 && c == skip && round % 2) c = (skip + 1) % C;
    }
    // every ZKE_E_ARG condition: refused, the plan as it was
    {
      CapMixedPlan p = sentinel();
      if (n) {
        std::vector<uint32_t> bad = config_of;
        bad[rnd(0, n - 1)] = C + rnd(0, 5);
        CHECK(capmix_plan_build(bad.data(), n, cfgs.data(), C, groups.data(), p) != nullptr && untouched(p));
        bad[0] = 0xFFFFFFFEu;
        CHECK(capmix_plan_build(bad.data(), n, cfgs.data(), C, groups.data(), p) != nullptr && untouched(p));
        CHECK(capmix_plan_build(nullptr, n, cfgs.data(), C, groups.data(), p) != nullptr && untouched(p));
        refused += 3;
      }
      if (C) {
        const uint32_t c = rnd(0, C - 1);
        std::vector<MixedConfigIn> bad = cfgs;
        const uint32_t kind = rnd(0, 3);
        bad[c] = kind == 0 ? MixedConfigIn{0, 0} : kind == 1 ? MixedConfigIn{CAPMIX_MAX_PARTS + 1, 0} : kind == 2 ? MixedConfigIn{9, 8} : MixedConfigIn{0xFFFFFFFFu, 2};
        std::vector<uint32_t> g2(S + 64, 1);
        CHECK(capmix_plan_build(config_of.data(), n, bad.data(), C, g2.data(), p) != nullptr && untouched(p));
        std::vector<uint32_t> many = groups;
        many[rnd(0, S - 1)] = CAPMIX_MAX_GROUPS + 1 + (rnd(0, 1) ? 0xFFFFFF00u : 0u);
        CHECK(capmix_plan_build(config_of.data(), n, cfgs.data(), C, many.data(), p) != nullptr && untouched(p));
        CHECK(capmix_plan_build(config_of.data(), n, nullptr, C, groups.data(), p) != nullptr && untouched(p));
        CHECK(capmix_plan_build(config_of.data(), n, cfgs.data(), C, nullptr, p) != nullptr && untouched(p));
        refused += 4;
      }
      std::vector<MixedConfigIn> many(MIXED_MAX_CONFIGS + 1, MixedConfigIn{1, 0});
      std::vector<uint32_t> mg(MIXED_MAX_CONFIGS + 1, 1);
      CHECK(capmix_plan_build(config_of.data(), n, many.data(), MIXED_MAX_CONFIGS + 1, mg.data(), p) != nullptr && untouched(p));
      refused++;
    }
    CapMixedPlan p = round % 2 ? sentinel() : CapMixedPlan{};
    const char* why = capmix_plan_build(config_of.data(), n, cfgs.data(), C, groups.data(), p);
    CHECK(why == nullptr);
    if (why) continue;
    CapMixedShape sh;
    CHECK(capmix_plan_check(config_of.data(), n, cfgs.data(), C, groups.data(), sh) == nullptr && sh.J == p.shape.J && sh.Gt == p.shape.Gt &&
          sh.n_parts == p.shape.n_parts && sh.body_groups == p.shape.body_groups);
    check_plan(config_of, cfgs, groups, p);
    accepted++;
  }
  // the column limit, exactly: 4 096 e-mails of one config of 16 parts x 16 groups are 2^20 columns; one group fewer in ONE other
  // config named once gives 2^20 - 1
  {
    const std::vector<MixedConfigIn> cfgs = {MixedConfigIn{16, 0}, MixedConfigIn{8, 8}};
    std::vector<uint32_t> groups(32, CAPMIX_MAX_GROUPS);
    groups[31] = CAPMIX_MAX_GROUPS - 1;
    std::vector<uint32_t> config_of(4096, 0);
    CapMixedPlan p = sentinel();
    CHECK(capmix_plan_build(config_of.data(), 4096, cfgs.data(), 2, groups.data(), p) != nullptr && untouched(p));
    config_of[1234] = 1;
    CHECK(capmix_plan_build(config_of.data(), 4096, cfgs.data(), 2, groups.data(), p) == nullptr && p.shape.Gt == (1u << 20) - 1 && p.shape.J == 4096 * 16);
    check_plan(config_of, cfgs, groups, p);
    refused++; accepted++;
  }
  if (g_fail) { fprintf(stderr, "capture_mixed_plan_fuzz: %d checks failed\n", g_fail); return 1; }
  printf("capture_mixed_plan_fuzz ok: %d plans checked, %d inputs refused\n", accepted, refused);
  return 0;
}
