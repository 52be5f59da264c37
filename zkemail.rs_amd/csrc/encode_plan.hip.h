// encode_plan.hip.h — the host plan of an output encoding (zke_verify_emails_encoded, zke_encode_outputs): where each e-mail's
// VerificationOutput::from_parts(email, matches).abi_encode() (core/src/io.rs:28-44) goes in the batch's byte blob and how long it
// is.  The size of an encoding depends on the kind and on the string LENGTHS alone, so it is known before the batch runs: a pure
// function of the tables' offsets — no HIP call, no engine state, no byte of a blob is read.  It compiles as plain C++
// (tests/cpp/encode_plan_fuzz.cpp).
//
//   abi.encode(SolEmailOutput)           32 (0x20) + tuple;  tuple = 32 + 32 + 32 (0x60) + array(external_inputs)
//   abi.encode(SolEmailWithRegexOutput)  32 (0x20) + 64 (the two member offsets) + tuple + array(matches)
//   array(strings)                       32 (count) + 32 per string (its offset) + per string 32 (length) + its bytes padded to 32
//
// Every place is a multiple of 32, so is every length: e-mail i's encoding starts at enc_off[i] = the sum of the lengths in front of
// it, whatever the verdicts turn out to be — an e-mail that is not ZKE_OK leaves its place unused (no compaction, no counter).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace zke {

constexpr uint32_t ENC_KIND_EMAIL = 0;          // SolEmailOutput
constexpr uint32_t ENC_KIND_WITH_REGEX = 1;     // SolEmailWithRegexOutput
constexpr uint64_t ENC_MAX_LEN = 1ull << 32;    // an encoding is shorter than this (zke_encoded_info.len is 32 bits)

// Device image of one e-mail's job (32 bytes; read by encode_outputs_kernel).  The string ranges index the two str_off tables.
struct EncodeJob {
  uint32_t kind;                  // ENC_KIND_*
  uint32_t ext_lo, ext_hi;        // external inputs: strings [ext_lo, ext_hi) of the external-input table
  uint32_t match_lo, match_hi;    // matches: strings [match_lo, match_hi) of the match table (empty for ENC_KIND_EMAIL)
  uint32_t reserved;
  uint64_t enc_off;               // the e-mail's place in the byte blob
};
static_assert(sizeof(EncodeJob) == 32, "EncodeJob is a device image");

// The tables as the caller holds them (host memory).  Strings are CSR: string s is blob[str_off[s], str_off[s + 1]).
//   external inputs  e-mail i's are the strings ext_off[i] .. ext_off[i + 1]; ext_off == nullptr: none anywhere
//   matches          e-mail i's are the strings match_off[r0] .. match_off[r1], r0 / r1 = row_off[i] / row_off[i + 1] (a mixed batch's
//                    job_off) or, with row_off == nullptr, i * row_stride / (i + 1) * row_stride (one part list per batch: rows are
//                    (e-mail, part) pairs; row_stride 1: one row per e-mail); match_off == nullptr: none anywhere
struct EncodeTables {
  const uint32_t* ext_off = nullptr;
  const uint32_t* ext_str_off = nullptr;
  const uint8_t* ext_blob = nullptr;
  const uint32_t* row_off = nullptr;
  uint32_t row_stride = 1;
  const uint32_t* match_off = nullptr;
  const uint32_t* match_str_off = nullptr;
  const uint8_t* match_blob = nullptr;
};

struct EncodePlan {
  std::vector<EncodeJob> jobs;    // [n]
  std::vector<uint32_t> len;      // [n] bytes of e-mail i's encoding (whether or not it will be written)
  uint64_t total = 0;             // bytes of the blob = the sum of len
  uint32_t ext_strs = 0, match_strs = 0;      // strings of the two tables that the jobs can name (the tables' tails)
  uint32_t ext_bytes = 0, match_bytes = 0;    // ... and bytes of their blobs
};

inline uint64_t enc_pad32(uint64_t n) { return (n + 31) & ~(uint64_t)31; }
// total += len unless that leaves 64 bits
inline bool enc_place(uint64_t& total, uint64_t len) { return !__builtin_add_overflow(total, len, &total); }
// array(strings [lo, hi)) added to `size`; false as soon as the encoding reaches ENC_MAX_LEN
inline bool enc_add_array(const uint32_t* str_off, uint32_t lo, uint32_t hi, uint64_t& size) {
  size += 32 + 64 * (uint64_t)(hi - lo);
  if (size >= ENC_MAX_LEN) return false;
  for (uint32_t s = lo; s < hi; s++) {
    size += enc_pad32((uint64_t)str_off[s + 1] - str_off[s]);
    if (size >= ENC_MAX_LEN) return false;
  }
  return true;
}

// at most one of the two list forms of a zke_encode_in
inline const char* encode_lists_check(const void* lists, const void* mixed) {
  return lists && mixed ? "both lists and mixed are set (at most one)" : nullptr;
}

// A CSR pair, checked: idx[0 .. rows] and, when it names a string, str_off[0 .. idx[rows]] do not decrease; a table that names strings
// has its str_off, and its blob when a string has a byte.  0, or a message.
inline const char* encode_table_check(const uint32_t* idx, uint64_t rows, const uint32_t* str_off, const uint8_t* blob, uint32_t& strs,
                                      uint32_t& bytes) {
  strs = 0; bytes = 0;
  if (!idx) return nullptr;
  for (uint64_t r = 0; r < rows; r++) if (idx[r + 1] < idx[r]) return "offsets decrease";
  const uint32_t tail = idx[rows];
  if (!tail) return nullptr;
  if (!str_off) return "a null table has a non-zero tail";
  for (uint32_t s = 0; s < tail; s++) if (str_off[s + 1] < str_off[s]) return "offsets decrease";
  if (str_off[tail] && !blob) return "a null table has a non-zero tail";
  strs = tail; bytes = str_off[tail];
  return nullptr;
}

// The plan of n e-mails of kinds[n].  0, or a message — then `out` is as it was.
inline const char* encode_plan_build(uint32_t n, const uint32_t* kinds, const EncodeTables& t, EncodePlan& out) {
  if (n && !kinds) return "null pointer";
  EncodePlan p;
  const uint64_t rows = t.row_off ? (n ? t.row_off[n] : 0) : (uint64_t)n * t.row_stride;
  if (const char* why = encode_table_check(t.ext_off, n, t.ext_str_off, t.ext_blob, p.ext_strs, p.ext_bytes)) return why;
  if (const char* why = encode_table_check(t.match_off, rows, t.match_str_off, t.match_blob, p.match_strs, p.match_bytes)) return why;
  p.jobs.resize(n); p.len.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    if (kinds[i] > ENC_KIND_WITH_REGEX) return "kind is neither 0 (SolEmailOutput) nor 1 (SolEmailWithRegexOutput)";
    EncodeJob& j = p.jobs[i];
    j = EncodeJob{};
    j.kind = kinds[i];
    if (p.ext_strs) { j.ext_lo = t.ext_off[i]; j.ext_hi = t.ext_off[i + 1]; }
    if (p.match_strs && j.kind == ENC_KIND_WITH_REGEX) {
      const uint64_t r0 = t.row_off ? t.row_off[i] : (uint64_t)i * t.row_stride, r1 = t.row_off ? t.row_off[i + 1] : r0 + t.row_stride;
      j.match_lo = t.match_off[r0]; j.match_hi = t.match_off[r1];
    }
    uint64_t size = 32 + 96 + (j.kind == ENC_KIND_WITH_REGEX ? 64 : 0);
    if (!enc_add_array(t.ext_str_off, j.ext_lo, j.ext_hi, size) ||
        (j.kind == ENC_KIND_WITH_REGEX && !enc_add_array(t.match_str_off, j.match_lo, j.match_hi, size)))
      return "an encoding of 2^32 bytes or more";
    j.enc_off = p.total;
    p.len[i] = (uint32_t)size;
    if (!enc_place(p.total, size)) return "the encodings exceed 2^64 bytes";
  }
  out = std::move(p);
  return nullptr;
}

}  // namespace zke
