// body_fuzz.cpp — the host side of zke_extract_bodies under AddressSanitizer / UndefinedBehaviorSanitizer, on the CPU, no GPU: the
// C-ABI translation unit compiled with host sanitizers (device code is built, never run) and this main().  Host code there: the
// argument checks, which come before anything is staged, the layout, and the compaction of a finished extraction into the caller's
// buffers (host_stage.hip.h: body_measure, body_compact — infos rewritten to packed offsets, bodies compacted out of their first
// and second places, ZKE_E_NOMEM with the exact need).  Every buffer is an exact-size heap vector: a read or write past it trips
// ASan.  Hostile tables — offsets that overlap, lengths past the buffer — must be refused or served without leaving the twin.
// tests/test_body_sanitizers.py builds and runs it.
#include "../../zkemail.rs_amd/csrc/engine.hip"

#include <random>

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "body_fuzz: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  std::mt19937_64 rng(20261020);
  size_t cases = 0;

  // ---- argument checks: an engine object that owns nothing (the checks must not look at it)
  {
    zke_engine eng;
    zke_engine* e = &eng;
    const uint8_t raw[] = "From: a@example.com\r\n\r\nx\r\n";
    std::vector<zke_email_ref> ems(3, zke_email_ref{raw, sizeof raw - 1, nullptr, 0, nullptr, 0, 0, 0});
    std::vector<zke_body_info> infos(3);
    std::vector<uint8_t> bytes(256);
    zke_body_out out{infos.data(), infos.size(), bytes.data(), bytes.size(), 0, 0};
    uint64_t t = 0;
    EXPECT(zke_extract_bodies(nullptr, ems.data(), 3, 0, &out) == ZKE_E_ARG);
    EXPECT(zke_extract_bodies_async(e, ems.data(), 3, 0, &out, nullptr) == ZKE_E_ARG);
    EXPECT(zke_extract_bodies(e, nullptr, 3, 0, &out) == ZKE_E_ARG);
    EXPECT(zke_extract_bodies(e, ems.data(), 3, 0, nullptr) == ZKE_E_ARG);
    EXPECT(zke_extract_bodies(e, ems.data(), 3, 2, &out) == ZKE_E_ARG);
    EXPECT(zke_extract_bodies_async(e, ems.data(), 3, 0x80000000u, &out, &t) == ZKE_E_ARG);
    { auto bad = ems; bad[1].raw = nullptr; EXPECT(zke_extract_bodies(e, bad.data(), 3, 1, &out) == ZKE_E_ARG); }
    { auto bad = ems; bad[2].raw_len = (size_t)1 << 31; EXPECT(zke_extract_bodies(e, bad.data(), 3, 0, &out) == ZKE_E_ARG); }      // never read: refused by its length
    { zke_body_out o = out; o.infos_cap = 2; o.infos_need = 99; o.bytes_need = 99; EXPECT(zke_extract_bodies(e, ems.data(), 3, 0, &o) == ZKE_E_NOMEM && o.infos_need == 3 && o.bytes_need == 0); }
    { zke_body_out o = out; o.infos = nullptr; EXPECT(zke_extract_bodies(e, ems.data(), 3, 0, &o) == ZKE_E_ARG); }
    { zke_body_out o = out; o.bytes = nullptr; EXPECT(zke_extract_bodies(e, ems.data(), 3, 0, &o) == ZKE_E_ARG); }
    EXPECT(strstr(zke_last_error(e), "zke_extract_bodies") != nullptr);
    cases += 11;
  }

  // ---- the layout: the sections do not overlap and hold what the kernel writes
  for (uint32_t n : {0u, 1u, 3u, 64u, 1000u}) {
    const size_t raw_total = (size_t)n * 4097;
    const BodyLayout L = body_layout(n, raw_total);
    EXPECT(L.bytes >= (size_t)n * sizeof(zke_body_info) && L.region >= raw_total && L.first_copy == L.bytes + L.region && L.total == L.first_copy + L.region);
    cases++;
  }

  // ---- compaction: random extractions in the device layout, every byte capacity from none to plenty
  for (int it = 0; it < 400; it++) {
    const uint32_t n = (uint32_t)(rng() % 40);
    std::vector<uint32_t> len(n), off(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) { len[i] = (uint32_t)(rng() % 6 == 0 ? 0 : rng() % 700); off[i + 1] = off[i] + len[i]; }
    const BodyLayout L = body_layout(n, off[n]);
    std::vector<uint8_t> twin(L.total);                  // stands for the pinned twin: exact size
    for (auto& x : twin) x = (uint8_t)rng();
    zke_body_info* dev = reinterpret_cast<zke_body_info*>(twin.data());
    std::vector<std::vector<uint8_t>> want(n);
    size_t total = 0;
    bool any_spill = false;
    for (uint32_t i = 0; i < n; i++) {
      const bool ok = rng() % 4 != 0;
      const uint32_t blen = ok ? (uint32_t)(rng() % (2 * (size_t)len[i] + 1)) : (uint32_t)(rng() % 9);      // a failed e-mail's body_len is not looked at ... within bounds
      dev[i] = zke_body_info{ok ? 0u : (uint32_t)(1 + rng() % 11), (uint32_t)(rng() % 200), (uint32_t)rng(), (uint32_t)(rng() % 3), (uint32_t)rng(), (uint32_t)rng(),
                             ok ? blen : std::min<uint32_t>(blen, 2 * len[i]), len[i], (uint64_t)off[i]};
      if (ok) {
        const size_t a = std::min<size_t>(blen, len[i]);
        want[i].assign(twin.begin() + L.bytes + off[i], twin.begin() + L.bytes + off[i] + a);
        want[i].insert(want[i].end(), twin.begin() + L.first_copy + off[i], twin.begin() + L.first_copy + off[i] + (blen - a));
        total += blen;
        any_spill = any_spill || blen > len[i];
      }
    }
    for (size_t cap : {(size_t)0, total ? total - 1 : 0, total, total + 5}) {
      std::vector<zke_body_info> infos(n);
      std::vector<uint8_t> bytes(cap);
      zke_body_out o{infos.data(), n, cap ? bytes.data() : nullptr, cap, n, 12345};
      bool spilled = !any_spill;
      const int r = body_measure(L, twin.data(), &o, spilled);
      EXPECT(o.bytes_need == total && spilled == any_spill);
      EXPECT(r == (cap < total ? ZKE_E_NOMEM : 0));
      if (!r) body_compact(L, twin.data(), &o);
      size_t at = 0;
      for (uint32_t i = 0; i < n; i++) {             // the infos arrive either way
        EXPECT(infos[i].status == dev[i].status && infos[i].detail == dev[i].detail && infos[i].part == dev[i].part && infos[i].body_off == at && infos[i].reserved == 0);
        EXPECT(infos[i].body_len == (dev[i].status ? 0u : dev[i].body_len));
        if (!r && infos[i].body_len) EXPECT(!memcmp(bytes.data() + at, want[i].data(), want[i].size()));
        at += infos[i].body_len;
      }
      cases++;
    }

    // hostile tables: one info of an otherwise good table points outside its place — a length beyond twice the place, a place beyond the
    // region, an offset past it.  Refused as a whole (ZKE_E_DEVICE), nothing read through it.  Overlapping places are served: every
    // read stays inside the twin.
    if (n) {
      const uint32_t v = (uint32_t)(rng() % n);
      const zke_body_info keep = dev[v];
      std::vector<zke_body_info> infos(n);
      std::vector<uint8_t> bytes(2 * (size_t)off[n] + 16);
      zke_body_out o{infos.data(), n, bytes.data(), bytes.size(), 0, 0};
      bool spilled = false;
      dev[v].status = 0; dev[v].body_len = 2 * len[v] + 1 + (uint32_t)(rng() % 1000);
      EXPECT(body_measure(L, twin.data(), &o, spilled) == ZKE_E_DEVICE);
      dev[v] = keep; dev[v].reserved = (uint32_t)(L.region - off[v]) + 1 + (uint32_t)(rng() % 1000);
      EXPECT(body_measure(L, twin.data(), &o, spilled) == ZKE_E_DEVICE);
      dev[v] = keep; dev[v].body_off = L.region + 1 + rng() % 1000;
      EXPECT(body_measure(L, twin.data(), &o, spilled) == ZKE_E_DEVICE);
      dev[v] = keep; dev[v].body_off = ~0ull - rng() % 64;
      EXPECT(body_measure(L, twin.data(), &o, spilled) == ZKE_E_DEVICE);
      dev[v] = keep;
      for (uint32_t i = 0; i < n; i++) { dev[i].status = 0; dev[i].body_off = 0; dev[i].reserved = (uint32_t)L.region; dev[i].body_len = (uint32_t)(rng() % (2 * L.region + 1)); }
      size_t sum = 0;
      for (uint32_t i = 0; i < n; i++) sum += dev[i].body_len;
      std::vector<uint8_t> big(sum);
      zke_body_out o2{infos.data(), n, big.data(), big.size(), 0, 0};
      EXPECT(body_measure(L, twin.data(), &o2, spilled) == 0 && o2.bytes_need == sum);
      body_compact(L, twin.data(), &o2);
      cases += 5;
    }
  }
  printf("body_fuzz ok: %zu cases\n", cases);
  return 0;
}
