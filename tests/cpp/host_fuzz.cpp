// host_fuzz.cpp — the host-side parsers of the engine under AddressSanitizer / UndefinedBehaviorSanitizer, on the CPU, no GPU:
// the whole C-ABI translation unit compiled host-only (hipcc --cuda-host-only -fsanitize=address,undefined) with this main().
//   * parse_dfa_blob: the regex-automata wire format (untrusted caller bytes) — the two golden blobs cut at every length,
//     with every byte of their headers flipped, and random word substitutions;
//   * zke_wire_decode: borsh / bincode records cut at every length and with random byte flips;
//   * CopyPool: several callers at once, odd sizes and alignments, results compared with memcpy (also under -fsanitize=thread);
//   * zke_abi_encode into buffers of exactly the size it asks for, and one byte less;
//   * host_batch (the host entries' batch descriptor): both shapes of one batch agree, malformed ones are refused;
//   * deliver_scan and fold_selection (what a retired scan / key selection hands its caller): random results in the device layout
//     into exact-size caller buffers, every capacity from none to plenty;
//   * deliver_pending (a slot's pending-delivery record paid in one call) against those individual calls, every kind of batch, and
//     the shortfall rule with each variable-size buffer one byte too small;
//   * zke_shard_bounds, image_layout, pair_hash on edge sizes;
//   * the hash / modexp stage's plan (stage_plan.hip.h) and the launches made from it, over a fixed grid of engines and batches:
//     kernel launches are recorded instead of made, one line per case, and `--stage-plan OUT` writes the lines to OUT, which
//     tests/test_host_sanitizers.py compares with tests/golden/stage_plan.txt (recorded before the plan had a module of its own).
// tests/test_host_sanitizers.py builds and runs it.  (The same source with -fsanitize=thread instead: clean as well, run by hand —
// the second 40 s build is not worth a place in the suite.)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <string>
#include <utility>

// Every kernel launch of the translation unit is recorded, not made: the kernel by name, grid x block, the dynamic LDS bytes and,
// for a launch that takes StageArgs, the workgroups per role.  hipGetLastError() has no device to ask here and would end a
// sequence of launches after the first.
namespace plan_rec {
std::string line;                                    // the launches of the case at hand
const char* kernel_name(const void* k);              // (defined below, where the kernels are)
template <class T> auto describe(const T& a, int) -> decltype((void)a.g_oct9, void()) {
  line += " sha=" + std::to_string(a.g_sha) + " wave=" + std::to_string(a.g_wave) + " quad=" + std::to_string(a.g_quad) +
          " oct=" + std::to_string(a.g_oct) + " oct9=" + std::to_string(a.g_oct9) + " twin=" + std::to_string(a.twin_kinds);
}
template <class T> void describe(const T&, long) {}
template <class... A> void launch(const void* k, dim3 grid, dim3 block, size_t lds, const A&... a) {
  line += std::string(" | ") + kernel_name(k) + " " + std::to_string(grid.x) + "x" + std::to_string(block.x) + " lds=" + std::to_string(lds);
  (describe(a, 0), ...);
}
}  // namespace plan_rec
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, lds, stream, ...) plan_rec::launch(reinterpret_cast<const void*>(k), grid, block, lds, __VA_ARGS__)
#define hipGetLastError() hipSuccess

#include "../../zkemail.rs_amd/csrc/engine.hip"

#include <array>
#include <random>
#include <thread>

const char* plan_rec::kernel_name(const void* k) {
#define NAMED(kernel) {reinterpret_cast<const void*>(kernel<SHA_TILE>), #kernel}
  static const std::pair<const void*, const char*> names[] = {
      NAMED(sha256_batch_kernel), NAMED(sha256_pair_kernel), NAMED(sha256_ring_kernel), NAMED(sha256_twin_kernel),
      NAMED(hash_modexp_kernel), NAMED(hash_modexp_ring_kernel), NAMED(hash_modexp_twin_kernel)};
#undef NAMED
  for (const auto& nm : names) if (nm.first == k) return nm.second;
  return "another kernel";
}

// One engine of the grid: what the plan depends on besides the batch.
struct PlanCase { uint32_t slots, queues; int oct9, ring, twin; uint32_t kinds, lanes, sha_mapping, cache; };
static void plan_engine(zke_engine& eng, const PlanCase& c) {
  StageEnv& v = eng.stage;
  v.slots = c.slots; v.hw_queues = c.queues;
  v.rsa_oct9 = c.oct9; v.sha_ring = c.ring; v.sha_twin = c.twin; v.twin_kinds = c.kinds;
  v.rsa_lane_groups = c.lanes; v.sha_mapping = c.sha_mapping; v.key_cache = c.cache != 0;
}
// A batch of n e-mails through the plan and the stage's launches, as run_device_pipeline does it; returns the route mask
static uint32_t plan_run_stage(zke_engine& eng, uint32_t n, bool any_big, bool have_order, uint32_t last_wave_jobs) {
  static const uint32_t some_words[4] = {};
  const uint32_t n_pad = (n + 63) & ~63u;
  const StagePlan plan = plan_stage(eng.stage, n, 4 * n_pad, any_big, have_order, last_wave_jobs);
  if (launch_hash_modexp(&eng, plan, nullptr, 4 * n_pad, nullptr, n, nullptr, nullptr, some_words, some_words, have_order ? some_words : nullptr, nullptr)) exit(1);
  return plan.route_mask;
}
static void plan_run_sha(zke_engine& eng, uint32_t n) {
  if (launch_sha(&eng, plan_sha(eng.stage, n), nullptr, n, nullptr)) exit(1);
}
// The grid.  The option axes vary one at a time around the defaults, on both sides of the in-flight bound.
static std::string stage_plan_table() {
  const uint32_t U = 0xFFFFFFFFu;
  std::vector<PlanCase> engines;
  for (auto sq : {std::pair<uint32_t, uint32_t>{1, 4}, {4, 23}, {5, 4}, {5, 8}, {22, 23}}) engines.push_back({sq.first, sq.second, -1, -1, -1, 3, 0, 0, 1});
  for (auto sq : {std::pair<uint32_t, uint32_t>{1, 4}, {22, 23}}) {
    const PlanCase d{sq.first, sq.second, -1, -1, -1, 3, 0, 0, 1};
    auto with = [&](auto change) { PlanCase c = d; change(c); engines.push_back(c); };
    for (int f : {0, 1}) { with([&](PlanCase& c) { c.oct9 = f; }); with([&](PlanCase& c) { c.ring = f; }); with([&](PlanCase& c) { c.twin = f; }); }
    with([](PlanCase& c) { c.ring = 0; c.twin = 1; });
    with([](PlanCase& c) { c.ring = 1; c.twin = 0; });
    for (uint32_t k : {1u, 0u}) { with([&](PlanCase& c) { c.kinds = k; }); with([&](PlanCase& c) { c.kinds = k; c.ring = 1; c.twin = 1; }); }
    for (uint32_t l : {1u, 2u}) with([&](PlanCase& c) { c.lanes = l; });
    for (int f : {0, 1}) with([&](PlanCase& c) { c.lanes = 2; c.oct9 = f; });
    for (uint32_t m : {1u, 2u}) with([&](PlanCase& c) { c.sha_mapping = m; });
    with([](PlanCase& c) { c.cache = 0; });
  }
  std::string table = "# e = slots / hardware queues / forced oct9 / ring / twin (-1: not forced) / twin_kinds / rsa_lane_groups / sha_mapping / key cache;"
                      " last = -1: nothing known; ring, twin: zke_engine_sha_ring / _twin; then the launches: kernel grid x block, LDS bytes, StageArgs\n";
  char buf[160];
  for (size_t k = 0; k < engines.size(); k++) {
    const PlanCase& c = engines[k];
    zke_engine eng;
    plan_engine(eng, c);
    snprintf(buf, sizeof buf, "e=%u/%u/%d/%d/%d/%u/%u/%u/%u", c.slots, c.queues, c.oct9, c.ring, c.twin, c.kinds, c.lanes, c.sha_mapping, c.cache);
    const std::string env = buf;
    snprintf(buf, sizeof buf, " ring=%d twin=%d", zke_engine_sha_ring(&eng), zke_engine_sha_twin(&eng));
    const std::string abi = buf;
    auto stage = [&](uint32_t n, int big, int order, uint32_t last) {
      plan_rec::line.clear();
      const uint32_t mask = plan_run_stage(eng, n, big != 0, order != 0, last);
      snprintf(buf, sizeof buf, " n=%u big=%d order=%d last=%d mask=%u", n, big, order, (int)last, mask);
      table += "stage " + env + buf + abi + plan_rec::line + "\n";
    };
    for (uint32_t n : {1u, 127u, 128u, 255u, 256u, 1000u, 8192u, 8256u}) {
      stage(n, 0, 1, U); stage(n, 1, 1, U); stage(n, 0, 0, U);
      if (k < 5) { stage(n, 1, 0, U); for (uint32_t last : {0u, 5u, 100000u}) stage(n, 0, 1, last); }       // (the walkers' count depends on nothing else)
    }
    for (uint32_t n : {0u, 1u, 32u, 33u, 64u, 32768u, 32769u}) {
      plan_rec::line.clear();
      plan_run_sha(eng, n);
      snprintf(buf, sizeof buf, " n=%u", n);
      table += "sha " + env + buf + abi + plan_rec::line + "\n";
    }
  }
  return table;
}

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  uint8_t buf[4096]; size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  // ---- the stage plan over its grid (`--stage-plan OUT` alone: only this section, to regenerate the table)
  {
    const std::string table = stage_plan_table();
    if (argc >= 3 && !strcmp(argv[1], "--stage-plan")) {
      FILE* f = fopen(argv[2], "wb");
      if (!f || fwrite(table.data(), 1, table.size(), f) != table.size() || fclose(f)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
      if (argc == 3) return 0;
      argv += 2; argc -= 2;
    }
  }
  // ---- the environment's part of a StageEnv: each variable alone, unreadable queue counts, the two thresholds in builds with the knobs only
  {
    const char* const names[] = {"GPU_MAX_HW_QUEUES", "ZKE_RSA_OCT9", "ZKE_SHA_RING", "ZKE_SHA_TWIN", "ZKE_SHA_TWIN_KINDS", "ZKE_RSA_QUAD_MIN", "ZKE_RSA_OCT_MIN"};
    std::vector<std::pair<const char*, std::string>> kept;
    for (const char* nm : names) if (const char* v = getenv(nm)) kept.emplace_back(nm, v);
    auto read = [&](const char* name, const char* value) {
      for (const char* nm : names) unsetenv(nm);
      if (name) setenv(name, value, 1);
      StageEnv v;
      stage_env_from_environment(v);
      return v;
    };
    auto same = [](const StageEnv& a, const StageEnv& b) {
      return a.slots == b.slots && a.hw_queues == b.hw_queues && a.rsa_oct9 == b.rsa_oct9 && a.sha_ring == b.sha_ring && a.sha_twin == b.sha_twin && a.twin_kinds == b.twin_kinds &&
             a.rsa_quad_min == b.rsa_quad_min && a.rsa_oct_min == b.rsa_oct_min && a.sha_mapping == b.sha_mapping && a.rsa_lane_groups == b.rsa_lane_groups && a.key_cache == b.key_cache;
    };
    auto expect = [&](const char* name, const char* value, auto change) {
      StageEnv want; change(want);
      if (!same(read(name, value), want)) { fprintf(stderr, "stage_env_from_environment: %s=%s\n", name ? name : "(nothing set)", value ? value : ""); exit(1); }
    };
    expect(nullptr, nullptr, [](StageEnv&) {});
    expect("GPU_MAX_HW_QUEUES", "23", [](StageEnv& v) { v.hw_queues = 23; });
    for (const char* bad : {"", "0", "-3", "many"}) expect("GPU_MAX_HW_QUEUES", bad, [](StageEnv& v) { v.hw_queues = 4; });
    for (int f : {0, 1}) {
      const char* val = f ? "1" : "0";
      expect("ZKE_RSA_OCT9", val, [&](StageEnv& v) { v.rsa_oct9 = f; });
      expect("ZKE_SHA_RING", val, [&](StageEnv& v) { v.sha_ring = f; });
      expect("ZKE_SHA_TWIN", val, [&](StageEnv& v) { v.sha_twin = f; });
    }
    expect("ZKE_SHA_RING", "7", [](StageEnv& v) { v.sha_ring = 1; });
    expect("ZKE_SHA_TWIN_KINDS", "0", [](StageEnv& v) { v.twin_kinds = 0; });
    expect("ZKE_SHA_TWIN_KINDS", "6", [](StageEnv& v) { v.twin_kinds = 2; });
#ifdef ZKE_DEV_KNOBS
    expect("ZKE_RSA_QUAD_MIN", "64", [](StageEnv& v) { v.rsa_quad_min = 64; });
    expect("ZKE_RSA_OCT_MIN", "32", [](StageEnv& v) { v.rsa_oct_min = 32; });
#else
    expect("ZKE_RSA_QUAD_MIN", "64", [](StageEnv&) {});
    expect("ZKE_RSA_OCT_MIN", "32", [](StageEnv&) {});
#endif
    for (const char* nm : names) unsetenv(nm);
    for (const auto& kv : kept) setenv(kv.first, kv.second.c_str(), 1);
  }
  if (argc < 4) { fprintf(stderr, "usage: host_fuzz [--stage-plan out.txt] fwd.dfa rev.dfa record.bin [record2.bin ...]\n"); return 2; }
  std::mt19937_64 rng(12345);
  size_t cases = 0;
  // ---- dense DFA blobs
  for (int k = 1; k <= 2; k++) {
    const std::vector<uint8_t> good = slurp(argv[k]);
    { HostDfa h; if (parse_dfa_blob(good.data(), good.size(), h) != 0) { fprintf(stderr, "golden blob %d does not parse\n", k); return 1; } }
    for (size_t cut = 0; cut < good.size(); cut += (cut < 600 ? 1 : 37)) {          // every prefix is an exact-size heap buffer: a read past it trips ASan
      std::vector<uint8_t> b(good.begin(), good.begin() + cut);
      HostDfa h; if (parse_dfa_blob(b.data(), b.size(), h) == 0) { fprintf(stderr, "a proper prefix (%zu) parsed\n", cut); return 1; }
      cases++;
    }
    for (size_t at = 0; at < std::min<size_t>(good.size(), 400); at++)
      for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xFF}) {
        std::vector<uint8_t> b = good; b[at] ^= x;
        HostDfa h; (void)parse_dfa_blob(b.data(), b.size(), h); cases++;
      }
    for (int it = 0; it < 100000; it++) {                                            // random words anywhere (ids, counts, bounds)
      std::vector<uint8_t> b = good;
      const int m = 1 + (int)(rng() % 3);
      for (int j = 0; j < m; j++) {
        const size_t at = (rng() % (b.size() / 4)) * 4;
        const uint32_t v = (rng() & 1) ? (uint32_t)rng() : (uint32_t)(rng() % 4096);
        memcpy(b.data() + at, &v, 4);
      }
      HostDfa h;
      if (parse_dfa_blob(b.data(), b.size(), h) == 0) {
        // whatever still parses must be walkable without leaving the table: the id checks are what guarantees it
        const DfaDev& d = h.d;
        uint32_t sid = d.starts[2];
        for (int step = 0; step < 300; step++) { if (sid + d.classes[step & 255] >= h.table.size()) { fprintf(stderr, "walk leaves the table\n"); return 1; } sid = h.table[sid + d.classes[step & 255]]; }
        (void)dfa_idle_state(h);
      }
      cases++;
    }
  }
  // ---- borsh / bincode records (argv[3..]: alternately borsh EmailWithRegex, bincode EmailWithRegex)
  for (int k = 3; k < argc; k++) {
    const std::vector<uint8_t> good = slurp(argv[k]);
    const uint32_t fmt = (k - 3) & 1;
    zke_wire_doc* d = nullptr; size_t used = 0;
    if (zke_wire_decode(fmt, good.data(), good.size(), 1, &d, &used) != 0 || used != good.size()) { fprintf(stderr, "record %d does not decode\n", k); return 1; }
    zke_wire_free(d);
    for (size_t cut = 0; cut < good.size(); cut++) {
      std::vector<uint8_t> b(good.begin(), good.begin() + cut);
      if (zke_wire_decode(fmt, b.data(), b.size(), 1, &d, &used) == 0) { fprintf(stderr, "a truncated record (%zu) decoded\n", cut); return 1; }
      cases++;
    }
    for (int it = 0; it < 20000; it++) {
      std::vector<uint8_t> b = good;
      const int m = 1 + (int)(rng() % 4);
      for (int j = 0; j < m; j++) b[rng() % b.size()] = (uint8_t)rng();
      if (zke_wire_decode(fmt, b.data(), b.size(), 1, &d, &used) == 0) {
        zke_wire_email v; (void)zke_wire_view(d, &v);
        size_t sum = v.raw_len + v.domain_len + v.key_len;                           // every span lies inside the buffer
        for (uint32_t p = 0; p < v.n_header_parts; p++) { sum += v.header_parts[p].fwd_len; for (uint32_t c = 0; c < v.header_parts[p].n_captures; c++) sum += v.header_parts[p].capture_lens[c]; }
        for (uint32_t p = 0; p < v.n_body_parts; p++) sum += v.body_parts[p].bwd_len;
        if (sum > b.size()) { fprintf(stderr, "spans exceed the buffer\n"); return 1; }
        zke_wire_free(d);
      }
      cases++;
    }
  }
  // ---- CopyPool: four callers, odd sizes / alignments
  {
    CopyPool pool(3);
    std::vector<std::thread> ths;
    std::atomic<int> bad{0};
    for (int t = 0; t < 4; t++) ths.emplace_back([&, t] {
      std::mt19937_64 r(99 + t);
      for (int it = 0; it < 60; it++) {
        const size_t n = (size_t)(r() % (3u << 20)) + 1, so = r() % 61, dof = (r() % 3) * 64;
        std::vector<uint8_t> src(n + 64), dst(n + 256, 0xEE), ref(n + 256, 0xEE);
        for (size_t i = 0; i < src.size(); i += 97) src[i] = (uint8_t)r();
        CopyPool::Piece pc[2] = {{dst.data() + dof, src.data() + so, n - n / 3}, {dst.data() + dof + (n - n / 3), src.data() + so + (n - n / 3), n / 3}};
        pool.copy(pc, 2);
        memcpy(ref.data() + dof, src.data() + so, n);
        if (dst != ref) bad++;
      }
    });
    for (auto& t : ths) t.join();
    if (bad) { fprintf(stderr, "CopyPool: %d copies differ from memcpy\n", bad.load()); return 1; }
    cases += 240;
    // gather: thousands of small pieces with consecutive destinations (zke_verify_emails), from two callers at once
    std::vector<std::thread> th2;
    for (int t = 0; t < 2; t++) th2.emplace_back([&, t] {
      std::mt19937_64 r(7 + t);
      for (int it = 0; it < 12; it++) {
        const size_t np = (size_t)(r() % 3000) + 1;
        std::vector<std::vector<uint8_t>> srcs(np);
        std::vector<CopyPool::Piece> pc(np);
        size_t total = 0;
        for (auto& v : srcs) { v.resize((size_t)(r() % 5 == 0 ? r() % 20000 : r() % 600)); for (size_t i = 0; i < v.size(); i += 31) v[i] = (uint8_t)r(); total += v.size(); }
        std::vector<uint8_t> dst(total + 64, 0xEE), ref(total + 64, 0xEE);
        size_t o = r() % 64 == 0 ? 0 : r() % 48;
        for (size_t i = 0; i < np; i++) { pc[i] = CopyPool::Piece{dst.data() + o, srcs[i].empty() ? nullptr : srcs[i].data(), srcs[i].size()}; if (!srcs[i].empty()) memcpy(ref.data() + o, srcs[i].data(), srcs[i].size()); o += srcs[i].size(); if (o > total + 16) break; }
        if (o > total + 48) continue;
        dst.resize(std::max(dst.size(), o)); ref.resize(dst.size(), 0xEE);
        pool.gather(pc.data(), np);
        if (dst != ref) bad++;
      }
    });
    for (auto& t : th2) t.join();
    if (bad) { fprintf(stderr, "CopyPool::gather: %d results differ from memcpy\n", bad.load()); return 1; }
    cases += 24;
  }
  // ---- zke_abi_encode: string tables of random sizes into heap buffers of exactly the size asked for, one byte less, and none
  for (int it = 0; it < 3000; it++) {
    uint8_t h1[32], h2[32];
    for (int i = 0; i < 32; i++) { h1[i] = (uint8_t)rng(); h2[i] = (uint8_t)rng(); }
    auto table = [&](std::vector<std::vector<uint8_t>>& store, std::vector<const uint8_t*>& ptr, std::vector<size_t>& len) {
      const int n = (int)(rng() % 5);
      for (int i = 0; i < n; i++) { store.emplace_back((size_t)(rng() % 3 == 0 ? rng() % 100 : rng() % 34)); for (auto& c : store.back()) c = (uint8_t)rng(); }
      for (auto& v : store) { ptr.push_back(v.empty() ? nullptr : v.data()); len.push_back(v.size()); }
    };
    std::vector<std::vector<uint8_t>> s1, s2; std::vector<const uint8_t*> p1, p2; std::vector<size_t> l1, l2;
    table(s1, p1, l1); table(s2, p2, l2);
    const uint32_t wm = (uint32_t)(rng() & 1);
    size_t need = 0, got = 0;
    if (zke_abi_encode(h1, h2, p1.data(), l1.data(), (uint32_t)p1.size(), wm, p2.data(), l2.data(), (uint32_t)p2.size(), nullptr, 0, &need) != 0 || need % 32) { fprintf(stderr, "abi size query\n"); return 1; }
    std::vector<uint8_t> exact(need), tight(need - 1);
    if (zke_abi_encode(h1, h2, p1.data(), l1.data(), (uint32_t)p1.size(), wm, p2.data(), l2.data(), (uint32_t)p2.size(), exact.data(), exact.size(), &got) != 0 || got != need) { fprintf(stderr, "abi exact\n"); return 1; }
    if (zke_abi_encode(h1, h2, p1.data(), l1.data(), (uint32_t)p1.size(), wm, p2.data(), l2.data(), (uint32_t)p2.size(), tight.data(), tight.size(), &got) != ZKE_E_NOMEM) { fprintf(stderr, "abi tight\n"); return 1; }
    cases++;
  }
  // ---- host_batch: the host entries' batch descriptor, packed (zke_batch) and gathered (zke_email_ref[n] + zke_regex_lists), every
  // array in a heap buffer of exactly its size
  {
    const uint32_t n = 6, NP = n * 3;                                                // 2 header parts + 1 body part
    auto exact = [](const auto& v) { return std::vector<typename std::decay_t<decltype(v)>::value_type>(v.begin(), v.end()); };
    std::vector<std::vector<uint8_t>> raw(n), dom(n), key(n);
    std::vector<zke_email_ref> refs(n);
    for (uint32_t i = 0; i < n; i++) {
      raw[i].resize(i == 4 ? 0 : 1 + rng() % 700); dom[i].resize(i == 1 ? 0 : 1 + rng() % 20); key[i].resize(1 + rng() % 300);
      for (auto* v : {&raw[i], &dom[i], &key[i]}) for (auto& c : *v) c = (uint8_t)rng();
      refs[i] = zke_email_ref{raw[i].data(), raw[i].size(), reinterpret_cast<const char*>(dom[i].data()), dom[i].size(), key[i].data(),
                              key[i].size(), i % 3, i & 1};
    }
    // the same e-mails packed, each blob behind `base` bytes of something else (off[0] = base)
    auto pack = [&](const std::vector<std::vector<uint8_t>>& v, size_t base, std::vector<uint8_t>& blob, std::vector<uint64_t>& off) {
      std::vector<uint8_t> b(base, 0xAB);
      off.assign(n + 1, base);
      for (uint32_t i = 0; i < n; i++) { b.insert(b.end(), v[i].begin(), v[i].end()); off[i + 1] = b.size(); }
      blob = exact(b);
    };
    std::vector<uint8_t> rb, db, kb, kt(n), xn(n);
    std::vector<uint64_t> ro, dof, ko;
    pack(raw, 3, rb, ro); pack(dom, 0, db, dof); pack(key, 17, kb, ko);
    std::vector<uint32_t> hids{4, 9}, bids{2}, co{0}, so{0};
    std::vector<uint8_t> cb;
    for (uint32_t k = 0; k < NP; k++) {
      for (uint32_t c = 0; c < k % 3; c++) { cb.insert(cb.end(), 1 + rng() % 8, (uint8_t)('a' + c)); so.push_back((uint32_t)cb.size()); }
      co.push_back((uint32_t)so.size() - 1);
    }
    const std::vector<uint32_t> cap_off = exact(co), cap_str_off = exact(so), zeros(NP + 1, 0);
    const std::vector<uint8_t> cap_blob = exact(cb);
    std::vector<zke_result> out(n);
    zke_batch pb{};
    pb.n = n; pb.raw_blob = rb.data(); pb.raw_off = ro.data(); pb.domain_blob = db.data(); pb.domain_off = dof.data();
    pb.key_blob = kb.data(); pb.key_off = ko.data(); pb.key_type = kt.data(); pb.ext_null = xn.data();
    pb.with_regex = 1; pb.n_header_parts = 2; pb.n_body_parts = 1; pb.header_part_ids = hids.data(); pb.body_part_ids = bids.data();
    pb.cap_off = cap_off.data(); pb.cap_str_off = cap_str_off.data(); pb.cap_blob = cap_blob.data();
    zke_regex_lists rl{2, hids.data(), 1, bids.data(), cap_off.data(), cap_str_off.data(), cap_blob.data()};
    auto packed = [&](HostBatch& d) { return host_batch(d, "packed", out.data(), &pb); };
    auto gathered = [&](HostBatch& d) { return host_batch(d, "gathered", out.data(), refs.data(), n, &rl); };
    auto refused = [&](int r, const char* what) {
      if (r != ZKE_E_ARG || !strstr(g_err.c_str(), what)) { fprintf(stderr, "host_batch: '%s' not refused (%d, '%s')\n", what, r, g_err.c_str()); exit(1); }
      cases++;
    };
    // one batch, two shapes: the same totals, capture tables and image layout
    HostBatch a, b;
    if (packed(a) || gathered(b)) { fprintf(stderr, "host_batch: a valid batch refused: %s\n", g_err.c_str()); return 1; }
    if (a.raw_total != ro[n] - 3 || a.raw_total != b.raw_total || a.dom_total != b.dom_total || a.key_total != b.key_total ||
        a.raw_base != 3 || a.key_base != 17 || b.raw_base || a.cap_words != NP + 1 || a.cap_words != b.cap_words ||
        a.cap_strs != b.cap_strs || a.cap_bytes != cb.size() || a.cap_bytes != b.cap_bytes || memcmp(&a.L, &b.L, sizeof a.L) ||
        a.refs || b.refs != refs.data()) { fprintf(stderr, "host_batch: the two shapes of one batch differ\n"); return 1; }
    // each offset array of the packed shape made decreasing
    for (std::vector<uint64_t>* off : {&ro, &dof, &ko}) {
      const std::vector<uint64_t> keep = *off;
      (*off)[2] = (*off)[3] + 1;
      refused(packed(a), "non-decreasing");
      *off = keep;
    }
    // capture tables without a string, cap_str_off and cap_blob NULL: no tables, in both shapes
    pb.cap_off = rl.cap_off = zeros.data(); pb.cap_str_off = rl.cap_str_off = nullptr; pb.cap_blob = rl.cap_blob = nullptr;
    const ImageLayout none = image_layout(n, b.raw_total, b.dom_total, b.key_total, 0, 0, 0);
    for (int shape = 0; shape < 2; shape++)
      if ((shape ? gathered(a) : packed(a)) || a.cap_words || a.b.cap_off || a.b.cap_str_off || memcmp(&a.L, &none, sizeof none)) { fprintf(stderr, "host_batch: string-less tables\n"); return 1; }
    // ... while tables that hold strings need cap_str_off (and cap_blob)
    pb.cap_off = rl.cap_off = cap_off.data();
    pb.cap_blob = rl.cap_blob = cap_blob.data();
    refused(packed(a), "cap_str_off"); refused(gathered(a), "cap_str_off");
    pb.cap_str_off = rl.cap_str_off = cap_str_off.data();
    pb.cap_blob = rl.cap_blob = nullptr;
    refused(packed(a), "cap_blob"); refused(gathered(a), "cap_blob");
    pb.cap_blob = rl.cap_blob = cap_blob.data();
    // gathered: a null buffer with a length, implausible lengths, more than 1 TiB in all
    for (int k = 0; k < 3; k++) {
      zke_email_ref keep = refs[3];
      if (k == 0) refs[3].raw = nullptr; else if (k == 1) refs[3].from_domain = nullptr; else refs[3].key = nullptr;
      refused(gathered(a), "null buffer");
      refs[3] = keep;
      if (k == 0) refs[3].raw_len = (1ull << 40) + 1; else if (k == 1) refs[3].domain_len = (1ull << 32) + 1; else refs[3].key_len = (1ull << 32) + 1;
      refused(gathered(a), "implausible length");
      refs[3] = keep;
    }
    refs[0].raw_len = refs[1].raw_len = 1ull << 40;
    refused(gathered(a), "1 TiB");
  }
  // ---- deliver_scan: random scans in the device layout (the pinned twin is an exact-size heap vector, as every caller buffer is);
  // sigs and sel_blob each at no capacity, one short, exact and generous
  for (int it = 0; it < 150; it++) {
    const uint32_t n = 1 + (uint32_t)(rng() % 9), max_sigs = 1 + (uint32_t)(rng() % 5);
    std::vector<uint32_t> st(4 * (size_t)n), want_off(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) {
      st[4 * i] = (uint32_t)(rng() % 3); st[4 * i + 1] = (uint32_t)rng(); st[4 * i + 3] = (uint32_t)(rng() % 4);
      st[4 * i + 2] = rng() % 3 == 0 ? 0u : (uint32_t)(rng() % (max_sigs + 3));                 // n_signatures: also beyond max_sigs
      want_off[i + 1] = want_off[i] + std::min(st[4 * i + 2], max_sigs);
    }
    const size_t total = want_off[n], used = rng() % 4 == 0 ? 0 : (size_t)(rng() % (40 * (size_t)n * max_sigs));
    std::vector<zke_sig_info> recs((size_t)n * max_sigs);
    for (auto& r : recs) { uint8_t* p = reinterpret_cast<uint8_t*>(&r); for (size_t k = 0; k < sizeof r; k++) p[k] = (uint8_t)rng(); }
    std::vector<uint8_t> sel(used);
    for (auto& c : sel) c = (uint8_t)rng();
    for (size_t sigs_cap : {(size_t)0, total ? total - 1 : 0, total, total + 3})
      for (size_t blob_cap : {(size_t)0, used ? used - 1 : 0, used, used + 9}) {
        ScanBufs b;
        b.L = scan_layout(n, max_sigs, std::min<size_t>(blob_cap, (size_t)n * max_sigs * ZKE_MAX_TAGBUF));      // as submit_host sizes it
        std::vector<uint8_t> twin(b.L.total, 0xEE);
        const uint32_t used32 = (uint32_t)used;
        memcpy(twin.data(), &used32, 4);
        memcpy(twin.data() + b.L.status, st.data(), st.size() * 4);
        memcpy(twin.data() + b.L.recs, recs.data(), recs.size() * sizeof(zke_sig_info));
        if (std::min(used, b.L.blob_cap)) memcpy(twin.data() + b.L.blob, sel.data(), std::min(used, b.L.blob_cap));
        b.t.h.p = twin.data(); b.t.h.cap = twin.size();
        std::vector<uint32_t> status(4 * (size_t)n, 7u), off(n + 1, 7u);
        std::vector<zke_sig_info> sigs(sigs_cap);
        std::vector<uint8_t> blob(blob_cap, 0xCC);
        zke_sig_scan o{status.data(), status.size(), off.data(), off.size(), sigs_cap ? sigs.data() : nullptr, sigs_cap,
                       blob_cap ? blob.data() : nullptr, blob_cap, 4 * (size_t)n, (size_t)n + 1, 99, 99, 99};
        zke_engine eng;
        const int r = deliver_scan(&eng, b, &o);
        b.t.h.p = nullptr; b.t.h.cap = 0;
        const bool sigs_short = sigs_cap < total, blob_short = blob_cap < used;
        bool ok = r == (sigs_short || blob_short ? ZKE_E_NOMEM : 0) && o.sigs_need == total && o.sel_blob_need == used && off == want_off &&
                  status == st && o.n_sigs == (sigs_short ? 0 : total);
        for (uint32_t i = 0; ok && !sigs_short && i < n; i++)
          ok = want_off[i + 1] == want_off[i] ||
               !memcmp(sigs.data() + want_off[i], recs.data() + (size_t)i * max_sigs, (want_off[i + 1] - want_off[i]) * sizeof(zke_sig_info));
        if (ok && !r && used) ok = !memcmp(blob.data(), sel.data(), used);
        if (!ok) { fprintf(stderr, "deliver_scan: n %u max_sigs %u sigs %zu/%zu blob %zu/%zu -> %d\n", n, max_sigs, sigs_cap, total, blob_cap, used, r); return 1; }
        cases++;
      }
  }
  // ---- fold_selection against its rule restated: the first ZKE_OK record of a row wins, flagged when a ZKE_UNSUPPORTED one precedes
  // it; no ZKE_OK: the row's last record, ZKE_SEL_NONE; an empty row: a zeroed record, ZKE_DKIM_NOT_PASS / ZKE_D_NEUTRAL, ZKE_SEL_NONE
  for (int it = 0; it < 400; it++) {
    const uint32_t n = (uint32_t)(rng() % 12);
    std::vector<uint32_t> off(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) off[i + 1] = off[i] + (rng() % 3 == 0 ? 0u : (uint32_t)(rng() % 5));
    std::vector<zke_result> R(off[n]), out(n), want(n);
    std::vector<uint32_t> chosen(n, 7u), want_chosen(n);
    for (auto& x : R) {
      uint8_t* p = reinterpret_cast<uint8_t*>(&x); for (size_t k = 0; k < sizeof x; k++) p[k] = (uint8_t)rng();
      x.status = std::array<uint32_t, 4>{ZKE_OK, ZKE_UNSUPPORTED, ZKE_DKIM_NOT_PASS, ZKE_KEY_DECODE_FAIL}[rng() % 4];
    }
    for (uint32_t i = 0; i < n; i++) {
      uint32_t k = off[i], flag = 0;
      for (; k < off[i + 1] && R[k].status != ZKE_OK; k++) if (R[k].status == ZKE_UNSUPPORTED) flag = ZKE_SEL_AFTER_UNSUPPORTED;
      want_chosen[i] = k < off[i + 1] ? ((k - off[i]) | flag) : ZKE_SEL_NONE;
      if (off[i] == off[i + 1]) { memset(&want[i], 0, sizeof want[i]); want[i].status = ZKE_DKIM_NOT_PASS; want[i].detail = ZKE_D_NEUTRAL; }
      else want[i] = R[k < off[i + 1] ? k : off[i + 1] - 1];
    }
    fold_selection(R.data(), off, out.data(), chosen.data());
    if (chosen != want_chosen || (n && memcmp(out.data(), want.data(), n * sizeof(zke_result)))) { fprintf(stderr, "fold_selection differs from its rule\n"); return 1; }
    cases++;
  }
  // ---- deliver_pending (what a slot owes for a finished batch) against the individual deliver_* / fold_selection calls, byte for
  // byte: a default-constructed Slot — no stream, no event, no device — whose pinned twins are exact-size heap vectors, and two
  // callers with buffers of the same sizes, one served by deliver_pending, the other by the calls it stands for, in its order.
  // Then every output that can fall short with its variable-size buffer one byte too small: ZKE_E_NOMEM to cap_rc where there is
  // one, zke_last_error left alone where there is none, 0 returned, the fixed-size outputs and every *_need exact either way.
  {
    const uint32_t n = 3, max_sigs = 2, P = 2, G = 3, NP = n * P, NG = n * G;
    struct Caps { size_t sigs, sel_blob, keys, bytes, cap_blob; };
    struct Caller {                                                                   // every buffer of exactly its capacity
      std::vector<zke_result> rec, sel;
      std::vector<uint32_t> chosen, st, off, spans, cap_off, cap_str_off, ospans;
      std::vector<zke_sig_info> sigs;
      std::vector<zke_key_info> kinfos;
      std::vector<zke_body_info> binfos;
      std::vector<uint8_t> blob, keys, bytes, flags, cblob, oflags;
      zke_sig_scan scan; zke_keyrec_out keyrec; zke_body_out body; zke_capture_out caps; zke_capture_origin org;
      Caller(const Caps& c, uint32_t m)
          : rec(m), sel(n), chosen(n, 7u), st(4 * n, 7u), off(n + 1, 7u), spans(NG * 2, 7u), cap_off(NP + 1, 7u), cap_str_off(NG + 1, 7u), ospans(NG * 2, 7u),
            sigs(c.sigs), kinfos(m), binfos(n), blob(c.sel_blob, 0xCC), keys(c.keys, 0xCC), bytes(c.bytes, 0xCC), flags(NG, 0xCC), cblob(c.cap_blob, 0xCC), oflags(NG, 0xCC) {
        for (auto* v : {&rec, &sel}) memset(v->data(), 0xCC, v->size() * sizeof(zke_result));
        memset(sigs.data(), 0xCC, sigs.size() * sizeof(zke_sig_info)); memset(kinfos.data(), 0xCC, kinfos.size() * sizeof(zke_key_info));
        memset(binfos.data(), 0xCC, binfos.size() * sizeof(zke_body_info));
        scan = zke_sig_scan{st.data(), st.size(), off.data(), off.size(), c.sigs ? sigs.data() : nullptr, c.sigs, c.sel_blob ? blob.data() : nullptr, c.sel_blob, 4 * (size_t)n, (size_t)n + 1, 99, 99, 99};
        keyrec = zke_keyrec_out{kinfos.data(), m, c.keys ? keys.data() : nullptr, c.keys, m, 99};
        body = zke_body_out{binfos.data(), n, c.bytes ? bytes.data() : nullptr, c.bytes, n, 99};
        caps = zke_capture_out{spans.data(), spans.size(), flags.data(), flags.size(), cap_off.data(), cap_off.size(), cap_str_off.data(), cap_str_off.size(),
                               c.cap_blob ? cblob.data() : nullptr, c.cap_blob, (size_t)NG * 2, NG, (size_t)NP + 1, (size_t)NG + 1, 99, 99};
        org = zke_capture_origin{ospans.data(), ospans.size(), oflags.data(), oflags.size(), (size_t)NG * 2, NG};
      }
      bool same(const Caller& o) const {
        auto eq = [](const auto& a, const auto& b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof a[0])); };
        return eq(rec, o.rec) && eq(sel, o.sel) && eq(chosen, o.chosen) && eq(st, o.st) && eq(off, o.off) && eq(spans, o.spans) && eq(cap_off, o.cap_off) &&
               eq(cap_str_off, o.cap_str_off) && eq(ospans, o.ospans) && eq(sigs, o.sigs) && eq(kinfos, o.kinfos) && eq(binfos, o.binfos) && eq(blob, o.blob) &&
               eq(keys, o.keys) && eq(bytes, o.bytes) && eq(flags, o.flags) && eq(cblob, o.cblob) && eq(oflags, o.oflags) &&
               scan.sigs_need == o.scan.sigs_need && scan.sel_blob_need == o.scan.sel_blob_need && scan.n_sigs == o.scan.n_sigs && keyrec.keys_need == o.keyrec.keys_need &&
               body.bytes_need == o.body.bytes_need && caps.cap_blob_need == o.caps.cap_blob_need && caps.n_strings == o.caps.n_strings;
      }
    };
    enum : uint32_t { REC = 1, SEL = 2, SCAN = 4, KEYREC = 8, BODY = 16, CAPS = 32 };
    for (int it = 0; it < 60; it++) {
      // what the device left behind, in the pinned twins' layouts
      const std::vector<uint32_t> sel_off{0, 2, 2, 5};                                 // 5 (e-mail, candidate) pairs; their records are also "the records"
      const uint32_t m = sel_off[n];
      std::vector<zke_result> R(m);
      for (auto& x : R) { uint8_t* q = reinterpret_cast<uint8_t*>(&x); for (size_t k = 0; k < sizeof x; k++) q[k] = (uint8_t)rng(); x.status = rng() % 2 ? ZKE_OK : ZKE_DKIM_NOT_PASS; }
      std::vector<uint32_t> st(4 * n);
      size_t total_sigs = 0;
      for (uint32_t i = 0; i < n; i++) { st[4 * i] = 0; st[4 * i + 1] = (uint32_t)rng(); st[4 * i + 2] = 1 + (uint32_t)(rng() % 3); st[4 * i + 3] = 1; total_sigs += std::min(st[4 * i + 2], max_sigs); }
      const uint32_t sel_used = 1 + (uint32_t)(rng() % 40);
      std::vector<uint32_t> rec_off(m + 1, 0), key_len(m);
      size_t total_keys = 0;
      for (uint32_t i = 0; i < m; i++) { rec_off[i + 1] = rec_off[i] + 8 + (uint32_t)(rng() % 300); key_len[i] = 1 + (uint32_t)(rng() % (rec_off[i + 1] - rec_off[i])); total_keys += key_len[i]; }
      std::vector<uint32_t> raw_off(n + 1, 0), body_len(n);
      size_t total_body = 0;
      for (uint32_t i = 0; i < n; i++) { raw_off[i + 1] = raw_off[i] + 4 + (uint32_t)(rng() % 500); body_len[i] = 1 + (uint32_t)(rng() % (raw_off[i + 1] - raw_off[i])); total_body += body_len[i]; }      // none outgrows its place
      std::vector<uint8_t> scan_twin, keyrec_twin, body_twin, cap_twin;
      Slot w;
      zke_engine eng;
      auto stage = [&](const Caps& c, size_t cap_bytes) {                              // cap_bytes: the capture strings' bytes (0: an empty blob)
        auto noise = [&](std::vector<uint8_t>& v, size_t bytes) { v.resize(bytes); for (auto& x : v) x = (uint8_t)rng(); };
        w.h_results.p = R.data(); w.h_results.cap = R.size() * sizeof(zke_result);
        w.sb.L = scan_layout(n, max_sigs, std::min<size_t>(c.sel_blob, (size_t)n * max_sigs * ZKE_MAX_TAGBUF));
        noise(scan_twin, w.sb.L.total);
        memcpy(scan_twin.data(), &sel_used, 4);
        memcpy(scan_twin.data() + w.sb.L.status, st.data(), st.size() * 4);
        w.sb.t.h.p = scan_twin.data(); w.sb.t.h.cap = scan_twin.size();
        w.kb.L = keyrec_layout(m, rec_off[m]);
        noise(keyrec_twin, w.kb.L.total);
        for (uint32_t i = 0; i < m; i++) reinterpret_cast<zke_key_info*>(keyrec_twin.data())[i] = zke_key_info{0, ZKE_KEY_RSA, rec_off[i], key_len[i]};
        w.kb.t.h.p = keyrec_twin.data(); w.kb.t.h.cap = keyrec_twin.size();
        w.bb.L = body_layout(n, raw_off[n]);
        noise(body_twin, w.bb.L.first_copy);                                           // the second places are not there: nothing may read them
        for (uint32_t i = 0; i < n; i++)
          reinterpret_cast<zke_body_info*>(body_twin.data())[i] = zke_body_info{ZKE_OK, 0, 1, 0, 0, body_len[i], body_len[i], raw_off[i + 1] - raw_off[i], (uint64_t)raw_off[i]};
        w.bb.t.h.p = body_twin.data(); w.bb.t.h.cap = body_twin.size();
        w.cb.L = cap_layout(n, P, G, c.cap_blob);
        noise(cap_twin, w.cb.L.fixed_end);                                             // the twin ends in front of the blob
        const uint64_t hdr[2] = {NG, cap_bytes};
        memcpy(cap_twin.data() + w.cb.L.hdr, hdr, sizeof hdr);
        w.cb.t.h.p = cap_twin.data(); w.cb.t.h.cap = cap_twin.size();
        w.ob.L = origin_layout(n, G); w.ob.launched = false;                           // no body part asks for a group: the origins are the spans
      };
      auto owed = [&](uint32_t kinds, Caller& c) {
        PendingDelivery p;
        if (kinds & REC) { p.records = c.rec.data(); p.n = m; }
        if (kinds & SEL) { p.sel_off = sel_off; p.sel_out = c.sel.data(); p.sel_chosen = c.chosen.data(); }
        if (kinds & SCAN) p.scan = &c.scan;
        if (kinds & KEYREC) p.keyrec = &c.keyrec;
        if (kinds & BODY) p.body = &c.body;
        if (kinds & CAPS) { p.caps = &c.caps; p.org = &c.org; }
        return p;
      };
      // the calls deliver_pending stands for, in its order; a shortfall in *rc, anything else returned
      auto one_by_one = [&](uint32_t kinds, Caller& c, int* rc) {
        if (kinds & REC) memcpy(c.rec.data(), R.data(), m * sizeof(zke_result));
        if (kinds & SEL) fold_selection(R.data(), sel_off, c.sel.data(), c.chosen.data());
        int r = 0;
        if ((kinds & SCAN) && (r = deliver_scan(&eng, w.sb, &c.scan))) { if (r != ZKE_E_NOMEM) return r; *rc = r; }
        if ((kinds & KEYREC) && (r = deliver_keyrec(&eng, w.kb, &c.keyrec))) { if (r != ZKE_E_NOMEM) return r; *rc = r; }
        if ((kinds & BODY) && (r = deliver_body(&eng, w.bb, &c.body, nullptr))) { if (r != ZKE_E_NOMEM) return r; *rc = r; }
        if ((kinds & CAPS) && (r = deliver_captures(&eng, w.cb, &c.caps, nullptr))) { if (r != ZKE_E_NOMEM) return r; *rc = r; }
        if (kinds & CAPS) deliver_origins(w.cb, w.ob, &c.org);
        return 0;
      };
      auto needs_exact = [&](uint32_t kinds, const Caller& c, size_t cap_bytes) {
        return (!(kinds & SCAN) || (c.scan.sigs_need == total_sigs && c.scan.sel_blob_need == sel_used && c.st == st && c.off[n] == total_sigs)) &&
               (!(kinds & KEYREC) || (c.keyrec.keys_need == total_keys && c.kinfos[m - 1].key_off + c.kinfos[m - 1].key_len == total_keys)) &&
               (!(kinds & BODY) || (c.body.bytes_need == total_body && c.binfos[n - 1].body_off + c.binfos[n - 1].body_len == total_body)) &&
               (!(kinds & CAPS) || (c.caps.cap_blob_need == cap_bytes && c.caps.n_strings == NG && !memcmp(c.spans.data(), cap_twin.data() + w.cb.L.spans, NG * 8) &&
                                    c.ospans == c.spans && c.oflags == std::vector<uint8_t>(NG, 0)));
      };
      const Caps exact{total_sigs, sel_used, total_keys, total_body, 0};
      // records only; a selection; a scan; a lone key-record decode; a selection with key records; a body extraction that did not spill;
      // captures with an empty blob, origins not launched (an extraction's records come as they are)
      for (uint32_t kinds : {(uint32_t)REC, (uint32_t)SEL, (uint32_t)SCAN, (uint32_t)KEYREC, SEL | KEYREC, (uint32_t)BODY, REC | CAPS}) {
        stage(exact, 0);
        Caller a(exact, m), b(exact, m);
        int rc_a = 0, rc_b = 0;
        const int ra = deliver_pending(&eng, w, owed(kinds, a), &rc_a), rb = one_by_one(kinds, b, &rc_b);
        if (ra || rb || rc_a || rc_b || !a.same(b) || !needs_exact(kinds, a, 0)) { fprintf(stderr, "deliver_pending: kinds %u: %d/%d, cap_rc %d/%d, or the outputs differ\n", kinds, ra, rb, rc_a, rc_b); return 1; }
        cases++;
      }
      // one byte too small: sigs, sel_blob, keys, bytes, cap_blob (one string byte, no capacity: nothing is left to fetch from HBM)
      struct Short { uint32_t kinds; Caps caps; size_t cap_bytes; };
      const Short shorts[] = {{SCAN, {total_sigs - 1, sel_used, total_keys, total_body, 0}, 0}, {SCAN, {total_sigs, sel_used - 1u, total_keys, total_body, 0}, 0},
                              {KEYREC, {total_sigs, sel_used, total_keys - 1, total_body, 0}, 0}, {SEL | KEYREC, {total_sigs, sel_used, total_keys - 1, total_body, 0}, 0},
                              {BODY, {total_sigs, sel_used, total_keys, total_body - 1, 0}, 0}, {REC | CAPS, exact, 1}};
      for (const Short& sh : shorts)
        for (int told = 0; told < 2; told++) {
          stage(sh.caps, sh.cap_bytes);
          Caller a(sh.caps, m), b(sh.caps, m);
          int rc_a = 0, rc_b = 0;
          g_err = "sentinel";
          const int ra = deliver_pending(&eng, w, owed(sh.kinds, a), told ? &rc_a : nullptr);
          const bool err_ok = told ? g_err != "sentinel" : g_err == "sentinel";
          const int rb = one_by_one(sh.kinds, b, &rc_b);
          if (ra || rb || rc_b != ZKE_E_NOMEM || rc_a != (told ? ZKE_E_NOMEM : 0) || !err_ok || !a.same(b) || !needs_exact(sh.kinds, a, sh.cap_bytes)) {
            fprintf(stderr, "deliver_pending: kinds %u one byte short, %s: %d/%d, cap_rc %d/%d, last error '%s', or the outputs differ\n", sh.kinds,
                    told ? "with cap_rc" : "nobody to tell", ra, rb, rc_a, rc_b, g_err.c_str());
            return 1;
          }
          cases++;
        }
      w.h_results = PinnedBuf{}; w.sb.t.h = PinnedBuf{}; w.kb.t.h = PinnedBuf{}; w.bb.t.h = PinnedBuf{}; w.cb.t.h = PinnedBuf{};      // (the vectors own the memory)
    }
  }
  // ---- small pure functions on edge sizes
  {
    uint32_t bounds[9];
    uint64_t off1[1] = {7};
    if (zke_shard_bounds(off1, 0, 8, bounds) != 0 || bounds[8] != 0) return 1;
    std::vector<uint64_t> off(1001); off[0] = 1ull << 62;
    for (int i = 1; i <= 1000; i++) off[i] = off[i - 1] + (rng() % 3 == 0 ? 0 : rng() % 100000);
    for (uint32_t w : {1u, 2u, 3u, 8u}) { if (zke_shard_bounds(off.data(), 1000, w, bounds) != 0 || bounds[w] != 1000) return 1; for (uint32_t r = 0; r < w; r++) if (bounds[r] > bounds[r + 1]) return 1; }
    (void)image_layout(0, 0, 0, 0, 0, 0, 0);
    // ---- the plan sections of an image (host_stage.hip.h): {no plan, a mixed batch, a mixed batch + a mixed extraction} x {no encoding,
    // a host-planned one, a device-planned one} over n = 0, 1, 2, 65, with and without external inputs; the mixed batch alone has a
    // config without parts (an extraction's configs cannot).  The descriptor is built as the entries build it, laid out once, and then:
    // the sections lie inside [L.mixed, L.raw) one behind the other, the encoding's starts 64-byte aligned, and what stage_* puts into a
    // heap buffer of exactly the section's size, *_view on the same base hands back: equal to the plan's arrays.  The same through ONE
    // buffer of exactly the sections' total, each section at its offset: no stage_* writes into a neighbour.
    for (uint32_t n : {0u, 1u, 2u, 65u})
      for (int plan_kind = 0; plan_kind < 3; plan_kind++)
        for (int enc_kind = 0; enc_kind < 3; enc_kind++)
          for (uint32_t ext_strs : {0u, 5u}) {
            if ((!enc_kind || !n) && ext_strs) continue;                               // (the strings are the e-mails': ext_off[n] of them)
            auto bad = [&](const char* what) { fprintf(stderr, "plan sections: n %u plan %d enc %d ext %u: %s\n", n, plan_kind, enc_kind, ext_strs, what); exit(1); };
            // the e-mails, and configs of {2 header + 1 body parts, none (an extraction: 1 header part), 2 body parts}; every fourth e-mail has no config
            std::vector<std::vector<uint8_t>> raw(n);
            std::vector<zke_email_ref> refs(n);
            std::vector<zke_result> out(n);
            for (uint32_t i = 0; i < n; i++) { raw[i].assign(1 + rng() % 90, (uint8_t)i); refs[i] = zke_email_ref{raw[i].data(), raw[i].size(), nullptr, 0, nullptr, 0, ZKE_KEY_RSA, 0}; }
            const std::vector<MixedConfigIn> counts{{2, 1}, {plan_kind == 2 ? 1u : 0u, 0}, {0, 2}};
            const std::vector<uint32_t> ids{3, 1, 4, 1, 5, 9};
            std::vector<zke_regex_config> cfgs;
            for (size_t c = 0, at = 0; c < counts.size(); at += counts[c].n_header_parts + counts[c].n_body_parts, c++)
              cfgs.push_back(zke_regex_config{counts[c].n_header_parts, ids.data() + at, counts[c].n_body_parts, ids.data() + at + counts[c].n_header_parts});
            std::vector<uint32_t> config_of(n);
            for (uint32_t i = 0; i < n; i++) config_of[i] = i % 4 == 3 ? ZKE_CONFIG_NONE : i % 3;
            const zke_regex_mixed zm{(uint32_t)cfgs.size(), cfgs.data(), config_of.data(), nullptr, nullptr, nullptr};
            zke_engine eng;                                                            // an empty registry: every part resolves to "not registered"
            CapMixedReq cq;
            MixedReq& mq = cq.verify;
            if (plan_kind && (mixed_request("plan sections", &zm, n, mq) || mixed_resolve(&eng, mq))) bad(g_err.c_str());
            if (plan_kind == 2) {
              std::vector<uint32_t> groups(mq.shape.n_segs);
              for (auto& g : groups) g = (uint32_t)(rng() % 4);
              if (const char* why = capmix_plan_build(config_of.data(), n, counts.data(), zm.n_configs, groups.data(), cq.plan)) bad(why);
              cq.lists = zm;
              cq.part.resize(cq.plan.shape.n_parts);
              for (auto& p : cq.part) { uint8_t* q = reinterpret_cast<uint8_t*>(&p); for (size_t k = 0; k < sizeof p; k++) q[k] = (uint8_t)rng(); }
            }
            // the encoding: five external strings in all (or none), n jobs of a host plan or ext_off[n + 1] of a device plan
            EncodeReq eq;
            std::vector<uint32_t> ext_off(n + 1, 0), ext_str_off(ext_strs + 1, 0);
            for (uint32_t i = 0; i < n; i++) ext_off[i + 1] = i + 1 == n ? ext_strs : std::min(ext_strs, ext_off[i] + (uint32_t)(rng() % 3));
            for (uint32_t k = 0; k < ext_strs; k++) ext_str_off[k + 1] = ext_str_off[k] + (uint32_t)(rng() % 40);
            std::vector<uint8_t> ext_blob(ext_str_off[ext_strs]);
            for (auto& c : ext_blob) c = (uint8_t)rng();
            eq.ext_str_off = ext_str_off.data(); eq.ext_blob = ext_blob.data();
            eq.plan.ext_strs = ext_strs; eq.plan.ext_bytes = (uint32_t)ext_blob.size();
            eq.device_plan = enc_kind == 2; eq.n = n; eq.ext_off = ext_off.data();
            if (enc_kind == 1) { eq.plan.jobs.resize(n); for (auto& j : eq.plan.jobs) { j = EncodeJob{}; j.enc_off = rng(); } }
            HostBatch d;
            // (an entry with an encoding lays the image out itself, once d.enc is set; every other one leaves that to host_batch)
            if (host_batch(d, "plan sections", out.data(), refs.data(), n, nullptr, plan_kind ? &mq : nullptr, plan_kind == 2 ? &cq : nullptr, !enc_kind)) bad(g_err.c_str());
            if (enc_kind) { d.enc = &eq; layout_host_batch(d); }
            // where the sections lie
            const PlanSections& S = d.S;
            const ImageLayout& L = d.L;
            if (L.mixed + S.total > L.raw || S.mixed.total > S.capmix_at || S.capmix_at + S.capmix.total > S.enc_at || S.enc_at + S.enc.total != S.total)
              bad("a section leaves [L.mixed, L.raw) or overlaps its neighbour");
            if ((L.mixed + S.enc_at) % 64) bad("the encoding's section does not start 64-byte aligned");
            if ((!plan_kind && S.mixed.total) || (plan_kind != 2 && S.capmix.total) || (!enc_kind && S.enc.total)) bad("a section has bytes without a request");
            const ImageLayout bare = image_layout(n, d.raw_total, 0, 0, 0, 0, 0);
            if (!plan_kind && !enc_kind && (S.total || memcmp(&L, &bare, sizeof L))) bad("an image without a plan has plan bytes");
            // the round trip: what *_view names from a section's base against the plan's arrays
            auto same = [](const void* got, const auto& want) { return want.empty() || !memcmp(got, want.data(), want.size() * sizeof want[0]); };
            auto mixed_back = [&](const uint8_t* base) {
              const MixedLaunch ml = mixed_view(base, S.mixed, &mq.plan);
              return ml.plan == &mq.plan && same(ml.job_off, mq.plan.job_off) && same(ml.email_cfg, mq.plan.email_cfg) && same(ml.perm, mq.plan.perm) &&
                     same(ml.segs, mq.plan.segs) && mq.plan.job_off.size() == (size_t)n + 1 && mq.plan.segs.size() == mq.shape.n_segs;
            };
            auto capmix_back = [&](const uint8_t* base) {
              const uint32_t* job_off = mq.plan.job_off.data();
              const CapMixedTables t = capmix_view(base, S.capmix, job_off);
              return t.job_off == job_off && same(t.col_off, cq.plan.col_off) && same(t.cap_cfg, cq.plan.cap_cfg) && same(t.cfgs, cq.plan.cfgs) && same(t.part, cq.part) &&
                     cq.part.size() == mq.shape.n_segs;
            };
            auto enc_back = [&](const uint8_t* base) {
              const EncodeArgs a = enc_view(base, S.enc);
              return (enc_kind != 1 || (same(a.jobs, eq.plan.jobs) && eq.plan.jobs.size() == n)) && (enc_kind != 2 || !ext_strs || same(a.jobs, ext_off)) &&
                     (!ext_strs || same(a.ext_str_off, ext_str_off)) && same(a.ext_blob, ext_blob);
            };
            auto stage_enc_of = [&](uint8_t* base) { stage_enc(base, S.enc, eq.plan, eq.device_plan, eq.ext_off, n, eq.ext_str_off, eq.ext_blob); };
            // ... each section alone in a heap buffer of exactly its size (a write or a read past it trips ASan) ...
            std::vector<uint8_t> bm(S.mixed.total, 0xEE), bc(S.capmix.total, 0xEE), be(S.enc.total, 0xEE);
            if (plan_kind) { stage_mixed(bm.data(), S.mixed, mq.plan); if (!mixed_back(bm.data())) bad("the mixed plan's round trip"); }
            if (plan_kind == 2) { stage_capmix(bc.data(), S.capmix, cq.plan, cq.part); if (!capmix_back(bc.data())) bad("the mixed extraction's round trip"); }
            if (enc_kind) { stage_enc_of(be.data()); if (!enc_back(be.data())) bad("the encoding's round trip"); }
            // ... and all of them in one buffer of exactly their total, each at its offset: first everything is staged, then everything is read
            std::vector<uint8_t> all(S.total, 0xEE);
            if (plan_kind) stage_mixed(all.data(), S.mixed, mq.plan);
            if (plan_kind == 2) stage_capmix(all.data() + S.capmix_at, S.capmix, cq.plan, cq.part);
            if (enc_kind) stage_enc_of(all.data() + S.enc_at);
            if ((plan_kind && !mixed_back(all.data())) || (plan_kind == 2 && !capmix_back(all.data() + S.capmix_at)) || (enc_kind && !enc_back(all.data() + S.enc_at)))
              bad("a section staged at its offset was overwritten by a neighbour");
            cases++;
          }
    (void)pair_hash(nullptr, 0, nullptr, 0);
    uint8_t x[17] = {1, 2, 3};
    if (pair_hash(x, 17, x, 3) == pair_hash(x, 16, x, 3)) return 1;
  }
  printf("host_fuzz ok: %zu cases\n", cases);
  return 0;
}
