// keyrec_fuzz.cpp — the host side of the key-record entry points (zke_decode_key_records, zke_select_keys_from_records) under
// AddressSanitizer / UndefinedBehaviorSanitizer, on the CPU, no GPU: the C-ABI translation unit compiled with host sanitizers
// (device code is built, never run) and this main().  Two things are host code there: the argument checks, which come before
// anything is staged, and the delivery of a finished decode into the caller's buffers (deliver_keyrec: infos rewritten to packed
// offsets, keys compacted, ZKE_E_NOMEM with the exact need).  Every buffer is an exact-size heap vector: a read or write past it
// trips ASan.  tests/test_keyrec_sanitizers.py builds and runs it.
#include "../../zkemail.rs_amd/csrc/engine.hip"

#include <random>

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "keyrec_fuzz: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  std::mt19937_64 rng(20261017);
  size_t cases = 0;

  // ---- argument checks: an engine object that owns nothing (the checks must not look at it)
  {
    zke_engine eng;
    zke_engine* e = &eng;
    const uint8_t txt[] = "v=DKIM1; p=AAAA";
    std::vector<zke_keyrec_ref> recs(3, zke_keyrec_ref{txt, sizeof txt - 1});
    std::vector<zke_key_info> infos(3);
    std::vector<uint8_t> keys(64);
    zke_keyrec_out out{infos.data(), infos.size(), keys.data(), keys.size(), 0, 0};
    uint64_t t = 0;
    EXPECT(zke_decode_key_records(nullptr, recs.data(), 3, 0, &out) == ZKE_E_ARG);
    EXPECT(zke_decode_key_records_async(e, recs.data(), 3, 0, &out, nullptr) == ZKE_E_ARG);
    EXPECT(zke_decode_key_records(e, nullptr, 3, 0, &out) == ZKE_E_ARG);
    EXPECT(zke_decode_key_records(e, recs.data(), 3, 0, nullptr) == ZKE_E_ARG);
    EXPECT(zke_decode_key_records(e, recs.data(), 3, 2, &out) == ZKE_E_ARG);
    EXPECT(zke_decode_key_records(e, recs.data(), 1u << 19, 0, &out) == ZKE_E_ARG);
    { auto bad = recs; bad[1].txt = nullptr; EXPECT(zke_decode_key_records(e, bad.data(), 3, 1, &out) == ZKE_E_ARG); }
    { zke_keyrec_out o = out; o.infos_cap = 2; o.infos_need = 99; EXPECT(zke_decode_key_records(e, recs.data(), 3, 1, &o) == ZKE_E_NOMEM && o.infos_need == 3 && o.keys_need == 0); }
    { zke_keyrec_out o = out; o.infos = nullptr; EXPECT(zke_decode_key_records(e, recs.data(), 3, 1, &o) == ZKE_E_ARG); }
    { zke_keyrec_out o = out; o.keys = nullptr; EXPECT(zke_decode_key_records(e, recs.data(), 3, 1, &o) == ZKE_E_ARG); }
    EXPECT(strstr(zke_last_error(e), "zke_decode_key_records") != nullptr);

    const uint8_t raw[] = "From: a@example.com\r\n\r\nx\r\n";
    std::vector<zke_email_ref> ems(2, zke_email_ref{raw, sizeof raw - 1, "example.com", 11, nullptr, 0, 0, 0});
    std::vector<zke_result> res(2);
    std::vector<uint32_t> chosen(2), off{0, 2, 3};
    EXPECT(zke_select_keys_from_records(nullptr, ems.data(), 2, off.data(), recs.data(), 1, res.data(), chosen.data(), &out) == ZKE_E_ARG);
    EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, off.data(), recs.data(), 1, res.data(), chosen.data(), &out, nullptr) == ZKE_E_ARG);
    EXPECT(zke_select_keys_from_records_async(e, nullptr, 2, off.data(), recs.data(), 1, res.data(), chosen.data(), &out, &t) == ZKE_E_ARG);
    EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, nullptr, recs.data(), 1, res.data(), chosen.data(), &out, &t) == ZKE_E_ARG);
    EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, off.data(), nullptr, 1, res.data(), chosen.data(), &out, &t) == ZKE_E_ARG);
    EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, off.data(), recs.data(), 1, nullptr, chosen.data(), &out, &t) == ZKE_E_ARG);
    EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, off.data(), recs.data(), 1, res.data(), nullptr, &out, &t) == ZKE_E_ARG);
    EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, off.data(), recs.data(), 1, res.data(), chosen.data(), nullptr, &t) == ZKE_E_ARG);
    EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, off.data(), recs.data(), 7, res.data(), chosen.data(), &out, &t) == ZKE_E_ARG);
    { std::vector<uint32_t> dec{0, 2, 1}; EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, dec.data(), recs.data(), 1, res.data(), chosen.data(), &out, &t) == ZKE_E_ARG); }
    { zke_keyrec_out o = out; o.infos_cap = 2; EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, off.data(), recs.data(), 1, res.data(), chosen.data(), &o, &t) == ZKE_E_NOMEM && o.infos_need == 3); }
    { std::vector<uint32_t> o1{1, 2, 3}; zke_keyrec_out o = out; o.infos_cap = 1;       // cand_off[0] != 0: two candidates in all
      EXPECT(zke_select_keys_from_records_async(e, ems.data(), 2, o1.data(), recs.data(), 1, res.data(), chosen.data(), &o, &t) == ZKE_E_NOMEM && o.infos_need == 2); }
    cases += 22;
  }

  // ---- the layout: the sections do not overlap and hold what the kernels write
  for (uint32_t m : {0u, 1u, 3u, 64u, 1000u}) {
    const size_t rec_total = (size_t)m * 411;
    const KeyrecLayout L = keyrec_layout(m, rec_total);
    EXPECT(L.keys >= (size_t)m * sizeof(zke_key_info) && L.total == L.keys + rec_total);
    EXPECT(L.p_type >= ((size_t)m + 1) * 8 && L.p_blob >= L.p_type + m && L.p_total >= L.p_blob + rec_total);
    cases++;
  }

  // ---- delivery: random decodes in the device layout, every key capacity from none to plenty
  for (int it = 0; it < 400; it++) {
    const uint32_t m = (uint32_t)(rng() % 40);
    std::vector<uint32_t> rec_len(m), rec_off(m + 1, 0);
    for (uint32_t i = 0; i < m; i++) { rec_len[i] = (uint32_t)(rng() % 5 == 0 ? 0 : rng() % 900); rec_off[i + 1] = rec_off[i] + rec_len[i]; }
    KeyrecBufs b;
    b.L = keyrec_layout(m, rec_off[m]);
    std::vector<uint8_t> twin(b.L.total);                 // stands for the pinned twin: exact size
    for (auto& x : twin) x = (uint8_t)rng();
    b.t.h.p = twin.data(); b.t.h.cap = twin.size();
    zke_key_info* dev = reinterpret_cast<zke_key_info*>(twin.data());
    std::vector<std::vector<uint8_t>> want(m);
    size_t total = 0;
    for (uint32_t i = 0; i < m; i++) {
      const bool ok = rec_len[i] >= 4 && rng() % 3 != 0;
      const uint32_t kl = ok ? (uint32_t)(rng() % (rec_len[i] * 3 / 4) + 1) : (uint32_t)(rng() % 7);     // a failed record's key_len is not looked at
      dev[i] = zke_key_info{ok ? 0u : (uint32_t)(100 + rng() % 10), (uint32_t)(rng() % 3), rec_off[i], kl};
      if (ok) { want[i].assign(twin.begin() + b.L.keys + rec_off[i], twin.begin() + b.L.keys + rec_off[i] + kl); total += kl; }
    }
    for (size_t cap : {(size_t)0, total ? total - 1 : 0, total, total + 5}) {
      std::vector<zke_key_info> infos(m);
      std::vector<uint8_t> keys(cap);
      zke_keyrec_out o{infos.data(), m, cap ? keys.data() : nullptr, cap, m, 12345};
      zke_engine eng;
      const int r = deliver_keyrec(&eng, b, &o);
      EXPECT(o.keys_need == total);
      EXPECT(r == (cap < total ? ZKE_E_NOMEM : 0));
      size_t at = 0;
      for (uint32_t i = 0; i < m; i++) {           // the infos arrive either way
        EXPECT(infos[i].code == dev[i].code && infos[i].key_type == dev[i].key_type && infos[i].key_off == at);
        EXPECT(infos[i].key_len == (dev[i].code ? 0u : dev[i].key_len));
        if (!r && infos[i].key_len) EXPECT(!memcmp(keys.data() + at, want[i].data(), want[i].size()));
        at += infos[i].key_len;
      }
      cases++;
    }
    b.t.h.p = nullptr; b.t.h.cap = 0;
  }
  printf("keyrec_fuzz ok: %zu cases\n", cases);
  return 0;
}
