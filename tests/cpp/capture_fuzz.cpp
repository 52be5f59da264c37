// capture_fuzz.cpp — the host-side reader of capture programs (parse_capture_program, behind zke_capture_register /
// zke_capture_validate) under AddressSanitizer / UndefinedBehaviorSanitizer, on the CPU, no GPU: the C-ABI translation unit
// compiled with host sanitizers (device code is built, never run) and this main().  The golden programs of tests/golden cut at
// every length (each prefix an exact-size heap buffer: a read past it trips ASan), every header byte flipped, and random word
// substitutions; whatever the reader still accepts is walked here the way capture.hip.h walks it — every offset, target, slot
// and epsilon-mask word it would touch — inside exact-size vectors.  tests/test_capture_sanitizers.py builds and runs it.
#include "../../zkemail.rs_amd/csrc/engine.hip"

#include <random>

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  uint8_t buf[4096]; size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

// every index the kernels form from an accepted program, checked against the tables' sizes
static bool walk_inside(const HostCapture& h) {
  const uint32_t N = h.n_states;
  if (h.table.size() != (size_t)N + 1 + h.n_words || h.eps.size() != (N + 63) / 64 || h.start >= N) return false;
  const std::vector<uint32_t> off(h.table.begin(), h.table.begin() + N + 1), st(h.table.begin() + N + 1, h.table.end());
  for (uint32_t q = 0; q < N; q++) {
    const uint32_t o = off.at(q), hd = st.at(o), kind = hd & 0xff, cnt = hd >> 8;
    const bool eps = (h.eps.at(q >> 6) >> (q & 63)) & 1;
    if (eps != (kind == CAP_LOOK || kind == CAP_UNION || kind == CAP_CAPTURE)) return false;
    if (kind == CAP_RANGE || kind == CAP_SPARSE) { for (uint32_t k = 0; k < cnt; k++) { (void)st.at(o + 1 + 2 * k); if (st.at(o + 2 + 2 * k) >= N) return false; } }
    else if (kind == CAP_UNION) { for (uint32_t k = 0; k < cnt; k++) if (st.at(o + 1 + k) >= N) return false; }
    else if (kind == CAP_LOOK) { if (st.at(o + 2) >= N) return false; }
    else if (kind == CAP_CAPTURE) { if (st.at(o + 1) >= 64 || st.at(o + 1) >= 2 * h.n_groups || st.at(o + 2) >= N) return false; }
    else if (kind > CAP_CAPTURE) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: capture_fuzz program.zkcp [...]\n"); return 2; }
  std::mt19937_64 rng(4242);
  size_t cases = 0, accepted = 0;
  for (int k = 1; k < argc; k++) {
    const std::vector<uint8_t> good = slurp(argv[k]);
    { HostCapture h; if (parse_capture_program(good.data(), good.size(), h) != 0 || !walk_inside(h)) { fprintf(stderr, "golden program %d does not parse\n", k); return 1; } }
    for (size_t cut = 0; cut < good.size(); cut++) {
      std::vector<uint8_t> b(good.begin(), good.begin() + cut);
      HostCapture h;
      uint32_t detail = 0;
      if (parse_capture_program(b.data(), b.size(), h) == 0) { fprintf(stderr, "a proper prefix (%zu) parsed\n", cut); return 1; }
      if (zke_capture_validate(b.empty() ? nullptr : b.data(), b.size(), &detail) != 0 || detail != ZKE_D_U_CAPTURE_PROGRAM) { fprintf(stderr, "prefix %zu: detail %u\n", cut, detail); return 1; }
      cases++;
    }
    for (size_t at = 0; at < good.size(); at++)
      for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xFF}) {
        std::vector<uint8_t> b = good; b[at] ^= x;
        HostCapture h;
        if (parse_capture_program(b.data(), b.size(), h) == 0) { accepted++; if (!walk_inside(h)) { fprintf(stderr, "flip at %zu: walk leaves the tables\n", at); return 1; } }
        cases++;
      }
    const uint32_t n_states = rd32(good.data() + 8);
    for (int it = 0; it < 100000; it++) {
      std::vector<uint8_t> b = good;
      const int m = 1 + (int)(rng() % 3);
      for (int j = 0; j < m; j++) {
        const size_t at = (rng() % (b.size() / 4)) * 4;
        const uint32_t pick = (uint32_t)(rng() % 4);
        const uint32_t v = pick == 0 ? (uint32_t)rng() : pick == 1 ? (uint32_t)(rng() % (n_states + 2)) : pick == 2 ? (uint32_t)(rng() % 8) | ((uint32_t)(rng() % 4) << 8)
                                                                                                     : ((uint32_t)(rng() % 256) | ((uint32_t)(rng() % 256) << 8));
        memcpy(b.data() + at, &v, 4);
      }
      HostCapture h;
      if (parse_capture_program(b.data(), b.size(), h) == 0) { accepted++; if (!walk_inside(h)) { fprintf(stderr, "substitution %d: walk leaves the tables\n", it); return 1; } }
      cases++;
    }
  }
  // headers that promise more than the blob holds, or more than the engine takes
  {
    std::vector<uint32_t> w{0x50434B5Au, 1, 0xFFFFFFFFu, 1, 0, 0, 0xFFFFFFFFu, 0};
    HostCapture h;
    if (parse_capture_program(reinterpret_cast<const uint8_t*>(w.data()), w.size() * 4, h) != ZKE_D_U_CAPTURE_PROGRAM) return 1;
    w[2] = ZKE_CAP_MAX_STATES + 1; w[6] = 0;
    std::vector<uint32_t> big(8 + ZKE_CAP_MAX_STATES + 2, 0);
    memcpy(big.data(), w.data(), 32);
    if (parse_capture_program(reinterpret_cast<const uint8_t*>(big.data()), big.size() * 4, h) != ZKE_D_U_CAPTURE_STATES) return 1;
    cases += 2;
  }
  if (accepted < 1000) { fprintf(stderr, "only %zu mutations were accepted: the walk was hardly exercised\n", accepted); return 1; }
  printf("capture_fuzz ok: %zu cases, %zu accepted and walked\n", cases, accepted);
  return 0;
}
