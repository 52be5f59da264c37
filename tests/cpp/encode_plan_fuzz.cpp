// encode_plan_fuzz.cpp — the host plan of an output encoding (zkemail.rs_amd/csrc/encode_plan.hip.h) and its argument checks over
// random and damaged tables, under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_encode_plan_sanitizers.py).  The header
// makes no HIP call, so this is plain C++ with its own main(): nothing is loaded into another process, nothing runs on a GPU.
//
// Checked for every accepted input: a job names exactly its e-mail's strings, len is what a writer that lays the encoding out word by
// word produces (the layout of zke_abi_encode, restated here), places follow each other without a gap, total is their sum — and
// buffers of EXACTLY those sizes hold every encoding (the writer runs inside them under AddressSanitizer).  Every refused input —
// decreasing offsets, a null table with a non-zero tail, both list forms, a kind above 1, an encoding that reaches 2^32 bytes, a total
// that leaves 64 bits — is refused before a write: the plan handed in comes back as it was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../zkemail.rs_amd/csrc/encode_plan.hip.h"

using namespace zke;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { if (g_fail++ < 20) fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static EncodePlan sentinel() {
  EncodePlan p;
  p.jobs.resize(2); p.jobs[1].enc_off = 42; p.len = {7, 8, 9}; p.total = 77; p.ext_strs = 5; p.match_strs = 6; p.ext_bytes = 3; p.match_bytes = 4;
  return p;
}
static bool untouched(const EncodePlan& p) {
  return p.jobs.size() == 2 && p.jobs[1].enc_off == 42 && p.len == std::vector<uint32_t>{7, 8, 9} && p.total == 77 && p.ext_strs == 5 &&
         p.match_strs == 6 && p.ext_bytes == 3 && p.match_bytes == 4;
}

// A CSR string table over `rows` rows.
struct Table {
  std::vector<uint32_t> off{0}, str_off{0};
  std::vector<uint8_t> blob;
  void row(std::mt19937& rng, uint32_t strings, uint32_t max_len) {
    static const uint32_t edge[] = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65};
    for (uint32_t s = 0; s < strings; s++) {
      const uint32_t len = rng() % 3 == 0 ? edge[rng() % 11] : rng() % (max_len + 1);
      for (uint32_t b = 0; b < len; b++) blob.push_back((uint8_t)(1 + rng() % 255));
      str_off.push_back((uint32_t)blob.size());
    }
    off.push_back((uint32_t)str_off.size() - 1);
  }
};

// The layout of zke_abi_encode, restated: writes into out[0, cap) and returns the size.  Every byte it writes is inside [0, cap) or
// AddressSanitizer says so (out is a heap block of exactly cap bytes).
struct Writer {
  uint8_t* out; size_t cap, len = 0;
  void word(uint64_t v) { uint8_t* p = out + len; memset(p, 0, 24); for (int i = 0; i < 8; i++) p[24 + i] = (uint8_t)(v >> (56 - 8 * i)); len += 32; }
  void bytes(const uint8_t* s, size_t n) { const size_t pad = (n + 31) & ~(size_t)31; if (n) memcpy(out + len, s, n); memset(out + len + n, 0, pad - n); len += pad; }
  void array(const Table& t, uint32_t lo, uint32_t hi) {
    word(hi - lo);
    uint64_t o = 32 * (uint64_t)(hi - lo);
    for (uint32_t s = lo; s < hi; s++) { word(o); o += 32 + (((uint64_t)t.str_off[s + 1] - t.str_off[s] + 31) & ~31ull); }
    for (uint32_t s = lo; s < hi; s++) { word(t.str_off[s + 1] - t.str_off[s]); bytes(t.blob.data() + t.str_off[s], t.str_off[s + 1] - t.str_off[s]); }
  }
};

static void check_plan(uint32_t n, const std::vector<uint32_t>& kinds, const Table& ext, const Table& mat, const std::vector<uint32_t>* row_off,
                       uint32_t stride, const EncodePlan& p) {
  CHECK(p.jobs.size() == n && p.len.size() == n);
  CHECK(p.ext_strs == ext.off.back() && p.match_strs == mat.off.back());
  CHECK(p.ext_bytes == (p.ext_strs ? ext.str_off[p.ext_strs] : 0u) && p.match_bytes == (p.match_strs ? mat.str_off[p.match_strs] : 0u));
  uint64_t total = 0;
  std::vector<uint32_t> ext_cnt, mat_cnt;
  for (uint32_t i = 0; i < n; i++) {
    const EncodeJob& j = p.jobs[i];
    CHECK(j.kind == kinds[i] && j.enc_off == total && j.reserved == 0 && total % 32 == 0 && p.len[i] % 32 == 0);
    const uint32_t elo = ext.off[i], ehi = ext.off[i + 1];
    CHECK(j.ext_hi - j.ext_lo == ehi - elo && (ehi == elo || (j.ext_lo == elo && j.ext_hi == ehi)) && (p.ext_strs || j.ext_hi == 0));
    const uint64_t r0 = row_off ? (*row_off)[i] : (uint64_t)i * stride, r1 = row_off ? (*row_off)[i + 1] : r0 + stride;
    const uint32_t mlo = kinds[i] ? mat.off[r0] : 0, mhi = kinds[i] ? mat.off[r1] : 0;
    CHECK(j.match_hi - j.match_lo == mhi - mlo && (mhi == mlo || (j.match_lo == mlo && j.match_hi == mhi)));
    total += p.len[i];
  }
  CHECK(p.total == total);
  // exact-size caller buffers: the whole batch written into a heap block of exactly `total` bytes, each e-mail inside its place
  uint8_t* blob = (uint8_t*)malloc(total ? total : 1);
  for (uint32_t i = 0; i < n; i++) {
    const EncodeJob& j = p.jobs[i];
    Writer w{blob + j.enc_off, p.len[i]};
    uint8_t hash[32] = {0};
    w.word(0x20);
    size_t tuple_at = 0;
    if (j.kind) { w.word(0x40); tuple_at = w.len; w.word(0); }
    const size_t t0 = w.len;
    w.bytes(hash, 32); w.bytes(hash, 32); w.word(0x60);
    w.array(ext, ext.off[i], ext.off[i + 1]);
    if (j.kind) {
      const size_t end = w.len;
      w.len = tuple_at; w.word(0x40 + (end - t0)); w.len = end;
      const uint64_t r0 = row_off ? (*row_off)[i] : (uint64_t)i * stride, r1 = row_off ? (*row_off)[i + 1] : r0 + stride;
      w.array(mat, mat.off[r0], mat.off[r1]);
    }
    CHECK(w.len == p.len[i]);
  }
  free(blob);
}

int main() {
  std::mt19937 rng(20250607);
  // ---- accepted inputs
  for (int round = 0; round < 400; round++) {
    const uint32_t n = round < 8 ? (uint32_t)round : (uint32_t)(rng() % 70);
    const int shape = round % 3;                    // 0: one row per e-mail; 1: a part list per batch (stride P); 2: ragged rows (job_off)
    const uint32_t stride = shape == 1 ? rng() % 4 : 1;
    std::vector<uint32_t> kinds(n), row_off;
    Table ext, mat;
    for (uint32_t i = 0; i < n; i++) { kinds[i] = shape == 1 ? 1 : rng() % 2; ext.row(rng, rng() % 8 == 0 ? 130 : rng() % 5, 90); }
    uint64_t rows = (uint64_t)n * stride;
    if (shape == 2) {
      row_off.push_back(0);
      for (uint32_t i = 0; i < n; i++) row_off.push_back(row_off.back() + (kinds[i] ? rng() % 4 : 0));
      rows = row_off.back();
    }
    for (uint64_t r = 0; r < rows; r++) mat.row(rng, rng() % 16 == 0 ? 70 : rng() % 3, 70);
    EncodeTables t;
    t.ext_off = ext.off.data(); t.ext_str_off = ext.str_off.data(); t.ext_blob = ext.blob.data();
    t.match_off = mat.off.data(); t.match_str_off = mat.str_off.data(); t.match_blob = mat.blob.data();
    t.row_stride = stride; t.row_off = shape == 2 ? row_off.data() : nullptr;
    if (ext.blob.empty()) t.ext_blob = nullptr;      // (no byte anywhere: a null blob is fine)
    if (mat.blob.empty()) t.match_blob = nullptr;
    EncodePlan p = sentinel();
    const char* why = encode_plan_build(n, kinds.data(), t, p);
    CHECK(why == nullptr);
    if (!why) check_plan(n, kinds, ext, mat, shape == 2 ? &row_off : nullptr, stride, p);
    if (n == 0) continue;
    // ---- the same tables, damaged: each refusal leaves the plan as it was
    auto refused = [&](const EncodeTables& bad, const std::vector<uint32_t>& k, const char* needle) {
      EncodePlan q = sentinel();
      const char* w = encode_plan_build(n, k.data(), bad, q);
      CHECK(w != nullptr && strstr(w, needle) != nullptr && untouched(q));
    };
    { std::vector<uint32_t> k = kinds; k[rng() % n] = 2 + rng() % 100; refused(t, k, "kind"); }
    if (ext.off.back() >= 2) {
      std::vector<uint32_t> d = ext.str_off; d[1 + rng() % (d.size() - 2)] = d.back() + 1 + rng() % 9;
      EncodeTables bad = t; bad.ext_str_off = d.data(); refused(bad, kinds, "decrease");
      bad = t; bad.ext_str_off = nullptr; refused(bad, kinds, "non-zero tail");
      if (!ext.blob.empty()) { bad = t; bad.ext_blob = nullptr; refused(bad, kinds, "non-zero tail"); }
    }
    if (n >= 2 && ext.off.back()) {
      std::vector<uint32_t> d = ext.off; d[rng() % n] = d.back() + 1;
      EncodeTables bad = t; bad.ext_off = d.data(); refused(bad, kinds, "decrease");
    }
    if (rows >= 2 && mat.off.back()) {
      std::vector<uint32_t> d = mat.off; d[rng() % rows] = d.back() + 1;
      EncodeTables bad = t; bad.match_off = d.data(); refused(bad, kinds, "decrease");
      bad = t; bad.match_str_off = nullptr; refused(bad, kinds, "non-zero tail");
    }
    // null tables altogether are "no string anywhere", whatever the other pointers say
    EncodeTables none = t; none.ext_off = nullptr; none.match_off = nullptr; none.ext_str_off = nullptr; none.match_blob = nullptr;
    EncodePlan q = sentinel();
    CHECK(encode_plan_build(n, kinds.data(), none, q) == nullptr && q.ext_strs == 0 && q.match_strs == 0);
    for (uint32_t i = 0; i < n; i++) CHECK(q.len[i] == (kinds[i] ? 32u + 64 + 96 + 32 + 32 : 32u + 96 + 32));
  }
  // ---- both list forms set
  int a = 0, b = 0;
  CHECK(encode_lists_check(&a, &b) != nullptr && !encode_lists_check(&a, nullptr) && !encode_lists_check(nullptr, &b) && !encode_lists_check(nullptr, nullptr));
  // ---- an encoding that reaches 2^32 bytes: offsets alone say so, no byte of a blob exists or is read
  {
    const uint32_t kinds[2] = {0, 0}, off[3] = {0, 1, 3};
    const uint8_t byte = 0;
    // 32 + 96 + 32 + 64 + pad32(L) + 64 + pad32(M) reaches 2^32 exactly when pad32(L) + pad32(M) == 2^32 - 288
    const uint32_t L = 0x80000000u - 288, M = 0x80000000u;
    uint32_t str_off[4] = {0, 5, 5 + L, 0};
    EncodeTables t;
    t.ext_off = off; t.ext_str_off = str_off; t.ext_blob = &byte;
    str_off[3] = str_off[2] + (M - 32);                                   // one word short of the limit: accepted, len = 2^32 - 32
    EncodePlan p = sentinel();
    CHECK(encode_plan_build(2, kinds, t, p) == nullptr && p.len[1] == 0xFFFFFFE0u && p.jobs[1].enc_off == 32 + 96 + 32 + 64 + 32 && p.total == p.jobs[1].enc_off + 0xFFFFFFE0ull);
    str_off[3] = str_off[2] + (M - 31);                                   // one byte more pads to the limit: refused
    p = sentinel();
    const char* why = encode_plan_build(2, kinds, t, p);
    CHECK(why && strstr(why, "2^32") && untouched(p));
    // many strings: 2^21 of 2 016 bytes are less than 2^32 bytes of blob and more than 2^32 with their two words each
    std::vector<uint32_t> many((size_t)(1u << 21) + 1);
    for (size_t s = 0; s < many.size(); s++) many[s] = (uint32_t)(s * 2016);
    const uint32_t one[2] = {0, 1u << 21}, k1[1] = {1};
    EncodeTables m;
    m.match_off = one; m.match_str_off = many.data(); m.match_blob = &byte;
    p = sentinel();
    why = encode_plan_build(1, k1, m, p);
    CHECK(why && strstr(why, "2^32") && untouched(p));
  }
  // ---- a total that leaves 64 bits: n < 2^32 encodings below 2^32 bytes cannot reach it, so the guard is driven directly
  {
    uint64_t total = ~0ull - 31;
    CHECK(enc_place(total, 31) && total == ~0ull &&!enc_place(total, 1));
    total = 1ull << 63;
    CHECK(!enc_place(total, 1ull << 63));
    total = 5;
    CHECK(enc_place(total, 0xFFFFFFE0ull) && total == 5 + 0xFFFFFFE0ull);
  }
  if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
  printf("encode_plan_fuzz ok\n");
  return 0;
}
