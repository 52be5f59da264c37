// zkemail_core.hpp — C++ mirror of zkemail_core's public surface (core/src/lib.rs:1-13) over the
// C-ABI in zkemail_amd.h.  Header-only; link with libzkemail_amd.so.
//
// Same type names, field names and function names as the reference (core/src/structs.rs:8-75,
// core/src/circuits.rs:9,31).  Where the reference panics (assert!/unwrap/expect, an abort under
// its release profile, Cargo.toml:35) these functions throw zkemail::VerifyPanic carrying the
// status that names the panic site; a caller that wants drop-in abort semantics lets it propagate
// to std::terminate.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "zkemail_amd.h"

namespace zkemail {

struct PublicKey {                         // structs.rs:8-11
  std::vector<uint8_t> key;
  std::string key_type;                    // "rsa" | "ed25519"
};
struct DFA {                               // structs.rs:16-19
  std::vector<uint8_t> fwd, bwd;
};
struct CompiledRegex {                     // structs.rs:24-27
  DFA verify_re;
  std::optional<std::vector<std::string>> captures;
};
struct RegexInfo {                         // structs.rs:32-35
  std::optional<std::vector<CompiledRegex>> header_parts, body_parts;
};
struct ExternalInput {                     // structs.rs:40-44
  std::string name;
  std::optional<std::string> value;
  size_t max_length = 0;
};
struct Email {                             // structs.rs:49-54
  std::string from_domain;
  std::vector<uint8_t> raw_email;
  PublicKey public_key;
  std::vector<ExternalInput> external_inputs;
};
struct EmailWithRegex {                    // structs.rs:59-62
  Email email;
  RegexInfo regex_info;
};
struct EmailVerifierOutput {               // structs.rs:65-69
  std::vector<uint8_t> from_domain_hash, public_key_hash;
  std::vector<std::string> external_inputs;
};
struct EmailWithRegexVerifierOutput {      // structs.rs:72-75
  EmailVerifierOutput email;
  std::vector<std::string> regex_matches;
};

struct EngineError : std::runtime_error { using std::runtime_error::runtime_error; };

// core/src/io.rs:18-44: the on-the-wire form of the witness (Solidity abi.encode of SolEmailOutput /
// SolEmailWithRegexOutput), through the C entry point zke_abi_encode.
struct VerificationOutput {
  EmailVerifierOutput email;
  std::optional<std::vector<std::string>> matches;      // nullopt: EmailOnly; a value: WithRegex
  static VerificationOutput from_parts(EmailVerifierOutput email, std::optional<std::vector<std::string>> matches) {   // io.rs:28-33
    return VerificationOutput{std::move(email), std::move(matches)};
  }
  std::vector<uint8_t> abi_encode() const {                                                                                // io.rs:35-44
    if (email.from_domain_hash.size() != 32 || email.public_key_hash.size() != 32)
      throw std::length_error("hashes must be 32 bytes");                                                                // io.rs:49-50 try_into().unwrap()
    auto table = [](const std::vector<std::string>& v, std::vector<const uint8_t*>& p, std::vector<size_t>& l) {
      for (const auto& s : v) { p.push_back(reinterpret_cast<const uint8_t*>(s.data())); l.push_back(s.size()); }
    };
    std::vector<const uint8_t*> p1, p2;
    std::vector<size_t> l1, l2;
    table(email.external_inputs, p1, l1);
    if (matches) table(*matches, p2, l2);
    size_t need = 0;
    auto call = [&](uint8_t* out, size_t cap) {
      return zke_abi_encode(email.from_domain_hash.data(), email.public_key_hash.data(), p1.data(), l1.data(), (uint32_t)p1.size(),
                            matches ? 1u : 0u, p2.data(), l2.data(), (uint32_t)p2.size(), out, cap, &need);
    };
    if (int rc = call(nullptr, 0)) throw EngineError("zke_abi_encode: " + std::to_string(rc));
    std::vector<uint8_t> out(need);
    if (int rc = call(out.data(), out.size())) throw EngineError("zke_abi_encode: " + std::to_string(rc));
    return out;
  }
};

// The reference would have panicked here.
struct VerifyPanic : std::runtime_error {
  uint32_t status, detail;
  VerifyPanic(uint32_t s, uint32_t d)
      : std::runtime_error("zkemail_core panic site status=" + std::to_string(s) + " detail=" + std::to_string(d)),
        status(s), detail(d) {}
  // ... at a site the status alone does not name (extract_email_body: email.rs:26 the parse, :17 / :21 get_body_raw)
  VerifyPanic(uint32_t s, uint32_t d, const std::string& site)
      : std::runtime_error("zkemail_core panic site " + site + " status=" + std::to_string(s) + " detail=" + std::to_string(d)),
        status(s), detail(d) {}
};

// One DKIM-Signature header as a scan reports it (zke_sig_info, the selector as a string).
struct SigInfo {
  uint32_t header_index, code, algo;       // code: 0 candidate | ZKE_D_NEUTRAL other domain | ZKE_D_* why validate_header refuses it
  std::string selector;
  uint32_t val_start, val_end;             // the header's value in raw_email
};
// A scan's answer for one e-mail; `sigs` holds the first max_sigs headers, the counts are the true ones.
struct SigScan {
  uint32_t status, detail, n_signatures, n_candidates;
  std::vector<SigInfo> sigs;
};
// The caller's resolver of generate_email_inputs: (from_domain, selector) -> the key, or nullopt when the fetch fails
// (helpers/src/dkim.rs fetch_dkim_key; DNS stays with the caller).
using FetchKey = std::function<std::optional<PublicKey>(const std::string& domain, const std::string& selector)>;
// One DKIM key record as a decode reports it (zke_key_info, the key as bytes): code 0 and the key, or ZKE_D_KEYREC_* and none.
struct KeyInfo {
  uint32_t code, key_type;                 // key_type: ZKE_KEY_* as far as the record got
  std::vector<uint8_t> key;                // PKCS#1 DER or 32 raw bytes
  PublicKey public_key() const { return PublicKey{key, key_type == ZKE_KEY_ED25519 ? "ed25519" : "rsa"}; }
};
// One e-mail's extract_email_body as an extraction reports it (zke_body_info, the decoded body as bytes).
struct BodyInfo {
  uint32_t status, detail;                 // ZKE_OK | ZKE_PARSE_FAIL | ZKE_BODY_DECODE_FAIL | ZKE_UNSUPPORTED
  uint32_t part, encoding;                 // 0 the message, k its k-th direct subpart, bit 31: chosen as text/html; ZKE_CTE_*
  uint32_t src_off, src_len;               // body_bytes of the chosen part in the raw e-mail, before decoding
  std::vector<uint8_t> body;               // empty unless status is ZKE_OK
};
// One e-mail's verifier output as a batch encodes it on the device (zke_encoded_info, the encoding as bytes): the record's verdict
// and, when that is ZKE_OK, VerificationOutput::from_parts(..).abi_encode() and its SHA-256; else no bytes and a zero digest.
struct EncodedOutput {
  uint32_t status, detail;                 // of the e-mail's record
  uint32_t kind;                           // 0 SolEmailOutput, 1 SolEmailWithRegexOutput
  std::vector<uint8_t> bytes;
  std::array<uint8_t, 32> digest;
};
// The resolver of generate_email_inputs_from_records: (from_domain, selector) -> the RAW answer — the TXT record of
// selector._domainkey.domain (its character-strings joined) or the archive's value —, or nullopt when the fetch fails.
using FetchRecord = std::function<std::optional<std::string>(const std::string& domain, const std::string& selector)>;

// One part of an extraction (zke_capture_part): the registered DFA pair that finds the match, the registered capture program of the
// same pattern, the groups wanted (RegexPattern.capture_indices).
struct CapturePart {
  uint32_t dfa_id, prog_id;
  std::vector<uint32_t> groups;
};
// What an extraction delivers (zke_capture_out): spans {start, end} and flags per (e-mail, requested group), and the capture tables
// in the form the verify entries take.
struct CaptureTables {
  std::vector<uint32_t> spans;
  std::vector<uint8_t> flags;
  std::vector<uint32_t> cap_off, cap_str_off;
  std::vector<uint8_t> cap_blob;
};
// Where the spans lie before the QP filter (zke_capture_origin): {start, end} in the canonical body as it was signed, ZKE_ORGF_* each.
struct CaptureOrigins {
  std::vector<uint32_t> spans;
  std::vector<uint8_t> flags;
};

class Engine {
 public:
  explicit Engine(int device = -1) {
    zke_options o{};
    o.device = device;
    if (int r = zke_engine_create(&o, &e_)) throw EngineError("zke_engine_create failed: " + std::to_string(r) + " " + zke_last_error(nullptr));
  }
  // every field of zke_options by name (ABI 0.3): slots, host threads, kernel variants, the strictness flags
  explicit Engine(const zke_options& o) {
    if (int r = zke_engine_create(&o, &e_)) throw EngineError("zke_engine_create failed: " + std::to_string(r) + " " + zke_last_error(nullptr));
  }
  ~Engine() { zke_engine_destroy(e_); }
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;
  zke_engine* raw() { return e_; }

  // core/src/circuits.rs:9-29
  EmailVerifierOutput verify_email(const Email& email) {
    zke_result r = run(email, nullptr);
    if (r.status != ZKE_OK) throw VerifyPanic(r.status, r.detail);
    return output(email, r);
  }
  // core/src/circuits.rs:31-68
  EmailWithRegexVerifierOutput verify_email_with_regex(const EmailWithRegex& in) {
    zke_result r = run(in.email, &in.regex_info);
    if (r.status != ZKE_OK) throw VerifyPanic(r.status, r.detail);
    EmailWithRegexVerifierOutput out{output(in.email, r), {}};
    for (const auto* parts : {&in.regex_info.header_parts, &in.regex_info.body_parts})    // circuits.rs:58-62
      if (*parts)
        for (const auto& p : **parts)
          if (p.captures) out.regex_matches.insert(out.regex_matches.end(), p.captures->begin(), p.captures->end());
    return out;
  }

  // verify_email over a vector of e-mails, each where it is (zke_verify_emails: the engine gathers the buffers itself):
  // one record per e-mail, never a throw for a bad e-mail — `status` / `detail` say what the reference would have done.
  std::vector<zke_result> verify_emails(const std::vector<Email>& emails) {
    std::vector<zke_email_ref> refs(emails.size());
    for (size_t i = 0; i < emails.size(); i++) {
      const Email& em = emails[i];
      uint32_t ext = 0;
      for (const auto& x : em.external_inputs) if (!x.value) ext = 1;                    // circuits.rs:24
      refs[i] = zke_email_ref{em.raw_email.data(), em.raw_email.size(), em.from_domain.data(), em.from_domain.size(),
                              em.public_key.key.data(), em.public_key.key.size(), key_type_code(em.public_key.key_type), ext};
    }
    std::vector<zke_result> out(emails.size());
    if (int r = zke_verify_emails(e_, refs.data(), (uint32_t)refs.size(), out.data()))
      throw EngineError("zke_verify_emails failed: " + std::to_string(r) + " " + zke_last_error(e_));
    return out;
  }

  // verify_email_with_regex over a vector that shares one part list (one regex_config per batch; the captures are per e-mail):
  // the pairs are registered once (zke_dfa_register), the e-mails stay where they are (zke_verify_emails_with_regex).
  std::vector<zke_result> verify_emails_with_regex(const std::vector<EmailWithRegex>& in) {
    if (in.empty()) return {};
    ListsPack p;
    pack_lists(in, p);
    std::vector<zke_result> out(in.size());
    if (int r = zke_verify_emails_with_regex(e_, p.refs.data(), (uint32_t)p.refs.size(), &p.lists, out.data()))
      throw EngineError("zke_verify_emails_with_regex failed: " + std::to_string(r) + " " + zke_last_error(e_));
    return out;
  }

  // verify_email over a vector of e-mails with the outputs encoded on the device (zke_verify_emails_encoded): per e-mail the record's
  // verdict and, where it is ZKE_OK, VerificationOutput::from_parts(email, None).abi_encode() (core/src/io.rs:28-44) and its SHA-256 —
  // what abi_encode(verify_email(email)) gives, for the whole batch.  Never a throw for a bad e-mail.
  std::vector<EncodedOutput> verify_emails_encoded(const std::vector<Email>& emails) {
    std::vector<zke_email_ref> refs(emails.size());
    std::vector<const Email*> ems(emails.size());
    for (size_t i = 0; i < emails.size(); i++) { refs[i] = ref_of(emails[i]); ems[i] = &emails[i]; }
    return encoded_call(refs, ems, nullptr);
  }
  // ... and verify_email_with_regex over a vector that shares one part list: SolEmailWithRegexOutput, the matches the e-mail's captures
  std::vector<EncodedOutput> verify_emails_with_regex_encoded(const std::vector<EmailWithRegex>& in) {
    if (in.empty()) return {};
    ListsPack p;
    pack_lists(in, p);
    std::vector<const Email*> ems(in.size());
    for (size_t i = 0; i < in.size(); i++) ems[i] = &in[i].email;
    return encoded_call(p.refs, ems, &p.lists);
  }

  // verify_email_with_regex over a vector as the reference has it — every value with a RegexInfo of its own — and verify_email for
  // the entries without one (nullopt), in ONE batch (zke_verify_emails_mixed): the pairs are registered, the configs are the distinct
  // id lists in order of first appearance, the capture tables are e-mail-major.  Record i is what verify_emails_with_regex gives
  // input i in a batch of its own config, or what verify_emails gives it.
  std::vector<zke_result> verify_emails_mixed(const std::vector<std::pair<Email, std::optional<RegexInfo>>>& in) {
    if (in.empty()) return {};
    auto ids_of = [&](const std::optional<std::vector<CompiledRegex>>& parts) {
      std::vector<uint32_t> v;
      if (parts)
        for (const auto& p : *parts) {
          uint32_t id = 0;
          if (int r = zke_dfa_register(e_, p.verify_re.fwd.data(), p.verify_re.fwd.size(), p.verify_re.bwd.data(), p.verify_re.bwd.size(), &id))
            throw EngineError("zke_dfa_register failed: " + std::to_string(r) + " " + zke_last_error(e_));
          v.push_back(id);
        }
      return v;
    };
    std::vector<std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> lists;       // the configs' id lists (stable addresses below)
    std::vector<zke_email_ref> refs(in.size());
    std::vector<uint32_t> config_of(in.size()), cap_off{0}, cap_str_off{0};
    std::vector<uint8_t> cap_blob;
    for (size_t i = 0; i < in.size(); i++) {
      const Email& em = in[i].first;
      uint32_t ext = 0;
      for (const auto& x : em.external_inputs) if (!x.value) ext = 1;
      refs[i] = zke_email_ref{em.raw_email.data(), em.raw_email.size(), em.from_domain.data(), em.from_domain.size(),
                              em.public_key.key.data(), em.public_key.key.size(), key_type_code(em.public_key.key_type), ext};
      if (!in[i].second) { config_of[i] = ZKE_CONFIG_NONE; continue; }
      const RegexInfo& ri = *in[i].second;
      auto key = std::make_pair(ids_of(ri.header_parts), ids_of(ri.body_parts));
      size_t c = 0;
      while (c < lists.size() && lists[c] != key) c++;
      if (c == lists.size()) {
        if (c == ZKE_MIXED_MAX_CONFIGS) throw EngineError("more than ZKE_MIXED_MAX_CONFIGS regex configs in one batch; split it");
        lists.push_back(std::move(key));
      }
      config_of[i] = (uint32_t)c;
      for (const auto* parts : {&ri.header_parts, &ri.body_parts})
        if (*parts)
          for (const auto& p : **parts) {
            if (p.captures)
              for (const auto& s : *p.captures) { cap_blob.insert(cap_blob.end(), s.begin(), s.end()); cap_str_off.push_back((uint32_t)cap_blob.size()); }
            cap_off.push_back((uint32_t)cap_str_off.size() - 1);
          }
    }
    if (cap_blob.empty()) cap_blob.push_back(0);
    std::vector<zke_regex_config> configs(lists.size());
    for (size_t c = 0; c < lists.size(); c++)
      configs[c] = zke_regex_config{(uint32_t)lists[c].first.size(), lists[c].first.data(), (uint32_t)lists[c].second.size(), lists[c].second.data()};
    zke_regex_mixed mixed{(uint32_t)configs.size(), configs.data(), config_of.data(), cap_off.size() > 1 ? cap_off.data() : nullptr,
                          cap_str_off.data(), cap_blob.data()};
    std::vector<zke_result> out(in.size());
    if (int r = zke_verify_emails_mixed(e_, refs.data(), (uint32_t)refs.size(), &mixed, out.data()))
      throw EngineError("zke_verify_emails_mixed failed: " + std::to_string(r) + " " + zke_last_error(e_));
    return out;
  }

  // zke_extract_captures over a vector of e-mails that share one part list: verify_email + canonicalise + QP clean + exactly one
  // match per part + the requested groups.  One record per e-mail; `caps` as zke_capture_out describes it.
  std::vector<zke_result> extract_captures(const std::vector<Email>& emails, const std::vector<CapturePart>& header_parts,
                                           const std::vector<CapturePart>& body_parts, CaptureTables& caps) {
    return extract(emails, header_parts, body_parts, caps, nullptr);
  }
  // ... and (zke_extract_captures_mapped) where every span lies in its haystack BEFORE the QP filter: what a circuit that is given
  // the signed body needs to place a capture there, or to learn that a soft break cuts it in two (ZKE_ORGF_SPLIT).
  std::vector<zke_result> extract_captures(const std::vector<Email>& emails, const std::vector<CapturePart>& header_parts,
                                           const std::vector<CapturePart>& body_parts, CaptureTables& caps, CaptureOrigins& origins) {
    return extract(emails, header_parts, body_parts, caps, &origins);
  }
  // zke_extract_captures_encoded: the extraction, String::from_utf8_lossy, abi_encode and SHA-256 in ONE batch — from raw e-mails,
  // keys and a part list to the public values.  Per e-mail the record's verdict and, when that is ZKE_OK, the bytes of
  // EmailWithRegexVerifierOutput.abi_encode() and their digest.  `caps`: nullptr, or the tables as zke_capture_out describes them,
  // the strings REPAIRED (helpers/src/regex.rs:35) — CompiledRegex.captures as the reference holds them.  The external inputs are
  // the e-mails' own, flattened [name, value, ...].  One call when the first guess of the two variable-size buffers holds, else a
  // second with the exact needs the first reported.
  std::vector<EncodedOutput> extract_captures_encoded(const std::vector<Email>& emails, const std::vector<CapturePart>& header_parts,
                                                      const std::vector<CapturePart>& body_parts, CaptureTables* caps = nullptr) {
    const uint32_t n = (uint32_t)emails.size();
    std::vector<zke_email_ref> refs(n);
    for (uint32_t i = 0; i < n; i++) refs[i] = ref_of(emails[i]);
    std::vector<zke_capture_part> hp, bp;
    size_t G = 0;
    for (const auto& p : header_parts) { hp.push_back(zke_capture_part{p.dfa_id, p.prog_id, (uint32_t)p.groups.size(), p.groups.data()}); G += p.groups.size(); }
    for (const auto& p : body_parts) { bp.push_back(zke_capture_part{p.dfa_id, p.prog_id, (uint32_t)p.groups.size(), p.groups.data()}); G += p.groups.size(); }
    std::vector<uint32_t> ext_off{0}, ext_str_off{0};
    std::vector<uint8_t> ext_blob;
    for (const Email& em : emails) {
      for (const auto& x : em.external_inputs)
        for (const std::string* s : {&x.name, x.value ? &*x.value : nullptr}) {
          if (s) ext_blob.insert(ext_blob.end(), s->begin(), s->end());
          ext_str_off.push_back((uint32_t)ext_blob.size());
        }
      ext_off.push_back((uint32_t)ext_str_off.size() - 1);
    }
    if (ext_blob.empty()) ext_blob.push_back(0);
    const size_t NP = (size_t)n * (hp.size() + bp.size()), NG = (size_t)n * G;
    CaptureTables own;
    CaptureTables& t = caps ? *caps : own;
    if (caps) { t.spans.assign(NG * 2 + 1, 0); t.flags.assign(NG + 1, 0); t.cap_off.assign(NP + 1, 0); t.cap_str_off.assign(NG + 1, 0); t.cap_blob.assign(NG * 64 + 1, 0); }
    std::vector<zke_result> recs(n);
    std::vector<zke_encoded_info> infos(n + 1);
    std::vector<uint8_t> bytes((size_t)n * 512 + 2 * ext_blob.size() + 64 * ext_str_off.size() + NG * 160 + 1);
    zke_capture_out o{};
    zke_encoded_out enc{};
    for (int attempt = 0; attempt < 2; attempt++) {
      if (caps) o = zke_capture_out{t.spans.data(), NG * 2, t.flags.data(), NG, t.cap_off.data(), NP + 1, t.cap_str_off.data(), NG + 1,
                                    t.cap_blob.data(), t.cap_blob.size(), 0, 0, 0, 0, 0, 0};
      enc = zke_encoded_out{infos.data(), n, bytes.data(), bytes.size(), 0, 0};
      const int r = zke_extract_captures_encoded(e_, refs.data(), n, hp.data(), (uint32_t)hp.size(), bp.data(), (uint32_t)bp.size(), recs.data(),
                                                 caps ? &o : nullptr, ext_off.data(), ext_str_off.data(), ext_blob.data(), &enc);
      if (r == ZKE_E_NOMEM && attempt == 0) {      // the needs are exact: one second call suffices
        if (caps && o.cap_blob_need > t.cap_blob.size()) t.cap_blob.resize(o.cap_blob_need);
        if (enc.bytes_need > bytes.size()) bytes.resize(enc.bytes_need);
        continue;
      }
      if (r) throw EngineError("zke_extract_captures_encoded failed: " + std::to_string(r) + " " + zke_last_error(e_));
      break;
    }
    if (caps) { t.spans.resize(NG * 2); t.flags.resize(NG); t.cap_str_off.resize(o.n_strings + 1); t.cap_blob.resize(o.cap_blob_need); }
    std::vector<EncodedOutput> out(n);
    for (uint32_t i = 0; i < n; i++) {
      out[i].status = recs[i].status; out[i].detail = recs[i].detail; out[i].kind = infos[i].kind;
      out[i].bytes.assign(bytes.begin() + infos[i].off, bytes.begin() + infos[i].off + infos[i].len);
      std::copy(infos[i].digest, infos[i].digest + 32, out[i].digest.begin());
    }
    return out;
  }
  // zke_utf8_lossy_batch: String::from_utf8_lossy over byte strings — every ill-formed chunk one U+FFFD.  `changed` (optional): per
  // string whether it was not valid UTF-8.
  std::vector<std::vector<uint8_t>> utf8_lossy(const std::vector<std::vector<uint8_t>>& strings, std::vector<uint8_t>* changed = nullptr) {
    const uint32_t n = (uint32_t)strings.size();
    std::vector<uint64_t> off{0};
    std::vector<uint8_t> blob;
    for (const auto& s : strings) { blob.insert(blob.end(), s.begin(), s.end()); off.push_back(blob.size()); }
    std::vector<uint32_t> out_off(n + 1);
    std::vector<uint8_t> out(blob.size() + blob.size() / 8 + 64), flags(n + 1);
    size_t need = 0;
    int r = zke_utf8_lossy_batch(e_, blob.data(), off.data(), n, out_off.data(), out.data(), out.size(), &need, flags.data());
    if (r == ZKE_E_NOMEM) { out.resize(need); r = zke_utf8_lossy_batch(e_, blob.data(), off.data(), n, out_off.data(), out.data(), out.size(), &need, flags.data()); }
    if (r) throw EngineError("zke_utf8_lossy_batch failed: " + std::to_string(r) + " " + zke_last_error(e_));
    std::vector<std::vector<uint8_t>> res(n);
    for (uint32_t i = 0; i < n; i++) res[i].assign(out.begin() + out_off[i], out.begin() + out_off[i + 1]);
    if (changed) { changed->resize(n); for (uint32_t i = 0; i < n; i++) (*changed)[i] = flags[i] & 1; }
    return res;
  }
  // zke_extract_captures_mixed: the extraction over e-mails that carry different regex configs, in ONE batch.  `configs`: the
  // distinct configs (header parts, body parts); config_of[i]: e-mail i's, or ZKE_CONFIG_NONE (verify_email only).  `caps` is ragged:
  // cap_off has J + 1 entries, spans / flags / cap_str_off are indexed by column (the header's job_off / col_off) — the tables
  // zke_verify_emails_mixed takes.  origins: nullptr, or where the spans lie before the QP filter (the same columns).
  std::vector<zke_result> extract_captures_mixed(const std::vector<Email>& emails,
                                                 const std::vector<std::pair<std::vector<CapturePart>, std::vector<CapturePart>>>& configs,
                                                 const std::vector<uint32_t>& config_of, CaptureTables& caps, CaptureOrigins* origins = nullptr) {
    if (config_of.size() != emails.size()) throw EngineError("one config index (or ZKE_CONFIG_NONE) per e-mail");
    const uint32_t n = (uint32_t)emails.size();
    std::vector<zke_email_ref> refs(n);
    for (uint32_t i = 0; i < n; i++) {
      const Email& em = emails[i];
      uint32_t ext = 0;
      for (const auto& x : em.external_inputs) if (!x.value) ext = 1;
      refs[i] = zke_email_ref{em.raw_email.data(), em.raw_email.size(), em.from_domain.data(), em.from_domain.size(),
                              em.public_key.key.data(), em.public_key.key.size(), key_type_code(em.public_key.key_type), ext};
    }
    std::vector<std::vector<zke_capture_part>> parts(configs.size());
    std::vector<zke_capture_config> cfgs(configs.size());
    std::vector<size_t> P(configs.size()), G(configs.size(), 0);
    for (size_t c = 0; c < configs.size(); c++) {
      for (const auto* side : {&configs[c].first, &configs[c].second})
        for (const auto& p : *side) { parts[c].push_back(zke_capture_part{p.dfa_id, p.prog_id, (uint32_t)p.groups.size(), p.groups.data()}); G[c] += p.groups.size(); }
      P[c] = parts[c].size();
      cfgs[c] = zke_capture_config{(uint32_t)configs[c].first.size(), parts[c].data(), (uint32_t)configs[c].second.size(),
                                   parts[c].data() + configs[c].first.size()};
    }
    size_t J = 0, Gt = 0;
    for (uint32_t c : config_of) {
      if (c == ZKE_CONFIG_NONE) continue;
      if (c >= configs.size()) throw EngineError("config_of names no config");
      J += P[c]; Gt += G[c];
    }
    caps.spans.assign(Gt * 2 + 1, 0); caps.flags.assign(Gt + 1, 0); caps.cap_off.assign(J + 1, 0); caps.cap_str_off.assign(Gt + 1, 0);
    caps.cap_blob.assign(Gt * 32 + 1, 0);
    zke_capture_origin org{};
    if (origins) {
      origins->spans.assign(Gt * 2 + 1, 0); origins->flags.assign(Gt + 1, 0);
      org = zke_capture_origin{origins->spans.data(), Gt * 2, origins->flags.data(), Gt, 0, 0};
    }
    const zke_capture_mixed mixed{(uint32_t)cfgs.size(), cfgs.data(), config_of.data()};
    std::vector<zke_result> out(n);
    zke_capture_out o{};
    for (int attempt = 0; attempt < 2; attempt++) {
      o = zke_capture_out{caps.spans.data(), Gt * 2, caps.flags.data(), Gt, caps.cap_off.data(), J + 1, caps.cap_str_off.data(), Gt + 1,
                          caps.cap_blob.data(), caps.cap_blob.size(), 0, 0, 0, 0, 0, 0};
      const int r = zke_extract_captures_mixed(e_, refs.data(), n, &mixed, out.data(), &o, origins ? &org : nullptr);
      if (r == ZKE_E_NOMEM && attempt == 0 && o.cap_blob_need > caps.cap_blob.size()) { caps.cap_blob.resize(o.cap_blob_need); continue; }
      if (r) throw EngineError("zke_extract_captures_mixed failed: " + std::to_string(r) + " " + zke_last_error(e_));
      break;
    }
    caps.spans.resize(Gt * 2); caps.flags.resize(Gt); caps.cap_str_off.resize(o.n_strings + 1); caps.cap_blob.resize(o.cap_blob_need);
    if (origins) { origins->spans.resize(Gt * 2); origins->flags.resize(Gt); }
    return out;
  }

  // helpers/src/generator.rs:17-30 for a batch (zke_scan_signatures): every DKIM-Signature header of every e-mail with
  // validate_header's verdict, whether d= names from_domain, a= classified and the selector.
  std::vector<SigScan> scan_signatures(const std::vector<std::vector<uint8_t>>& raw_emails, const std::vector<std::string>& from_domains,
                                       uint32_t max_sigs = 8) {
    if (raw_emails.size() != from_domains.size()) throw EngineError("one from_domain per raw e-mail");
    const uint32_t n = (uint32_t)raw_emails.size();
    std::vector<zke_email_ref> refs(n);
    for (uint32_t i = 0; i < n; i++)
      refs[i] = zke_email_ref{raw_emails[i].data(), raw_emails[i].size(), from_domains[i].data(), from_domains[i].size(), nullptr, 0, 0, 0};
    std::vector<uint32_t> status((size_t)n * 4 + 1), off((size_t)n + 1);
    std::vector<zke_sig_info> sigs((size_t)n * max_sigs + 1);
    std::vector<uint8_t> blob((size_t)n * max_sigs * 32 + 1);
    zke_sig_scan o{};
    for (int attempt = 0; attempt < 2; attempt++) {
      o = zke_sig_scan{status.data(), (size_t)n * 4, off.data(), (size_t)n + 1, sigs.data(), (size_t)n * max_sigs, blob.data(), blob.size(), 0, 0, 0, 0, 0};
      const int r = zke_scan_signatures(e_, refs.data(), n, max_sigs, &o);
      if (r == ZKE_E_NOMEM && attempt == 0 && o.sel_blob_need > blob.size()) { blob.resize(o.sel_blob_need); continue; }
      if (r) throw EngineError("zke_scan_signatures failed: " + std::to_string(r) + " " + zke_last_error(e_));
      break;
    }
    std::vector<SigScan> out(n);
    for (uint32_t i = 0; i < n; i++) {
      out[i] = SigScan{status[4 * (size_t)i], status[4 * (size_t)i + 1], status[4 * (size_t)i + 2], status[4 * (size_t)i + 3], {}};
      for (uint32_t k = off[i]; k < off[i + 1]; k++) {
        const zke_sig_info& s = sigs[k];
        out[i].sigs.push_back(SigInfo{s.header_index, s.code, s.algo, std::string(reinterpret_cast<const char*>(blob.data()) + s.sel_off, s.sel_len),
                                      s.val_start, s.val_end});
      }
    }
    return out;
  }

  // helpers/src/generator.rs:31-45 for a batch (zke_select_keys): candidate_keys[i] = the keys fetched for e-mail i's candidates
  // in the scan's order (nullopt: the fetch failed).  Returns the records; chosen[i] = the first key under which e-mail i
  // verifies (bit 31: ZKE_SEL_AFTER_UNSUPPORTED) or ZKE_SEL_NONE.  The e-mails' own public_key fields are ignored.
  std::vector<zke_result> select_keys(const std::vector<Email>& emails, const std::vector<std::vector<std::optional<PublicKey>>>& candidate_keys,
                                      std::vector<uint32_t>& chosen) {
    if (emails.size() != candidate_keys.size()) throw EngineError("one candidate list per e-mail");
    const uint32_t n = (uint32_t)emails.size();
    std::vector<zke_email_ref> refs(n);
    std::vector<uint32_t> off{0};
    std::vector<zke_key_ref> keys;
    for (uint32_t i = 0; i < n; i++) {
      const Email& em = emails[i];
      uint32_t ext = 0;
      for (const auto& x : em.external_inputs) if (!x.value) ext = 1;
      refs[i] = zke_email_ref{em.raw_email.data(), em.raw_email.size(), em.from_domain.data(), em.from_domain.size(), nullptr, 0, 0, ext};
      for (const auto& k : candidate_keys[i])
        keys.push_back(k ? zke_key_ref{k->key.data(), k->key.size(), key_type_code(k->key_type), 0} : zke_key_ref{nullptr, 0, ZKE_KEY_RSA, 0});
      off.push_back((uint32_t)keys.size());
    }
    std::vector<zke_result> out(n);
    chosen.assign(n, ZKE_SEL_NONE);
    if (int r = zke_select_keys(e_, refs.data(), n, off.data(), keys.data(), out.data(), chosen.data()))
      throw EngineError("zke_select_keys failed: " + std::to_string(r) + " " + zke_last_error(e_));
    return out;
  }

  // helpers/src/generator.rs:11-53 generate_email_inputs for a batch: scan, `fetch_key` once per distinct (from_domain, selector)
  // of a candidate, keep the first key under which the e-mail verifies.  Throws VerifyPanic for the first e-mail where the
  // reference returns Err — a parse_mail error (the scan's status), "No DKIM signatures found" (ZKE_DKIM_NOT_PASS /
  // ZKE_D_NO_SIGNATURE), "No valid DKIM key found for any signature" (ZKE_DKIM_NOT_PASS with the last candidate's detail) — and
  // with ZKE_UNSUPPORTED where the engine cannot give the reference's answer.
  std::vector<Email> generate_email_inputs(const std::vector<std::string>& from_domains, const std::vector<std::vector<uint8_t>>& raw_emails,
                                           const FetchKey& fetch_key, const std::vector<std::vector<ExternalInput>>* external_inputs = nullptr,
                                           uint32_t max_sigs = ZKE_SCAN_MAX_SIGS) {
    const std::vector<SigScan> scans = scan_signatures(raw_emails, from_domains, max_sigs);
    std::map<std::pair<std::string, std::string>, std::optional<PublicKey>> cache;
    std::vector<std::vector<std::optional<PublicKey>>> cands(scans.size());
    std::vector<Email> probe(scans.size());
    for (size_t i = 0; i < scans.size(); i++) {
      probe[i] = Email{from_domains[i], raw_emails[i], PublicKey{}, {}};
      for (const SigInfo& s : scans[i].sigs) {
        if (s.code != 0) continue;
        auto key = std::make_pair(from_domains[i], s.selector);
        auto it = cache.find(key);
        if (it == cache.end()) it = cache.emplace(key, fetch_key(from_domains[i], s.selector)).first;
        cands[i].push_back(it->second);
      }
    }
    std::vector<uint32_t> chosen;
    const std::vector<zke_result> recs = select_keys(probe, cands, chosen);
    return emails_of_selection(scans, probe, recs, chosen, external_inputs, [&](size_t i) { return cands[i].size(); },
                               [&](size_t i, uint32_t k) { return *cands[i][k]; });
  }

  // helpers/src/dkim.rs:67-111 for a batch (zke_decode_key_records): what a resolver returns -> the (key, key_type) pair of
  // Email.public_key.  mode: ZKE_KEYREC_DNS (RFC 6376 3.6.1 TXT record) or ZKE_KEYREC_ARCHIVE (the archive's value as dkim.rs reads
  // it); nullopt or an empty record: the fetch failed.
  std::vector<KeyInfo> decode_key_records(const std::vector<std::optional<std::string>>& records, uint32_t mode = ZKE_KEYREC_DNS) {
    KeyrecCall c(records);
    if (int r = zke_decode_key_records(e_, c.refs.data(), (uint32_t)c.refs.size(), mode, &c.out))
      throw EngineError("zke_decode_key_records failed: " + std::to_string(r) + " " + zke_last_error(e_));
    return c.result();
  }

  // core/src/email.rs:7-23 for a batch (zke_extract_bodies): parse_mail, the text/html subpart (else the first, else the message),
  // its Content-Transfer-Encoding undone.  part_keeps_eol: ZKE_BODYF_PART_KEEPS_EOL.
  std::vector<BodyInfo> extract_email_bodies(const std::vector<std::vector<uint8_t>>& raw_emails, bool part_keeps_eol = false) {
    const uint32_t n = (uint32_t)raw_emails.size();
    std::vector<zke_email_ref> refs(n);
    size_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
      refs[i] = zke_email_ref{};
      refs[i].raw = raw_emails[i].data(); refs[i].raw_len = raw_emails[i].size();
      total += raw_emails[i].size();
    }
    std::vector<zke_body_info> infos(n);
    std::vector<uint8_t> bytes(2 * total + 1);           // a decoded body is at most twice its source (lone LF becomes CRLF)
    zke_body_out out{infos.data(), n, bytes.data(), bytes.size(), 0, 0};
    if (int r = zke_extract_bodies(e_, refs.data(), n, part_keeps_eol ? ZKE_BODYF_PART_KEEPS_EOL : 0u, &out))
      throw EngineError("zke_extract_bodies failed: " + std::to_string(r) + " " + zke_last_error(e_));
    std::vector<BodyInfo> res(n);
    for (uint32_t i = 0; i < n; i++) {
      const zke_body_info& f = infos[i];
      res[i] = BodyInfo{f.status, f.detail, f.part, f.encoding, f.src_off, f.src_len,
                        std::vector<uint8_t>(bytes.begin() + (size_t)f.body_off, bytes.begin() + (size_t)f.body_off + f.body_len)};
    }
    return res;
  }

  // zke_select_keys_from_records: select_keys with the resolver's raw answers in place of keys; the records are decoded on the GPU in
  // front of the verify launches.  infos[i][k]: what candidate k of e-mail i decoded to.
  std::vector<zke_result> select_keys_from_records(const std::vector<Email>& emails, const std::vector<std::vector<std::optional<std::string>>>& candidate_records,
                                                   std::vector<uint32_t>& chosen, std::vector<std::vector<KeyInfo>>& infos, uint32_t mode = ZKE_KEYREC_DNS) {
    if (emails.size() != candidate_records.size()) throw EngineError("one candidate list per e-mail");
    const uint32_t n = (uint32_t)emails.size();
    std::vector<zke_email_ref> refs(n);
    std::vector<uint32_t> off{0};
    std::vector<std::optional<std::string>> flat;
    for (uint32_t i = 0; i < n; i++) {
      const Email& em = emails[i];
      uint32_t ext = 0;
      for (const auto& x : em.external_inputs) if (!x.value) ext = 1;
      refs[i] = zke_email_ref{em.raw_email.data(), em.raw_email.size(), em.from_domain.data(), em.from_domain.size(), nullptr, 0, 0, ext};
      flat.insert(flat.end(), candidate_records[i].begin(), candidate_records[i].end());
      off.push_back((uint32_t)flat.size());
    }
    KeyrecCall c(flat);
    std::vector<zke_result> out(n);
    chosen.assign(n, ZKE_SEL_NONE);
    if (int r = zke_select_keys_from_records(e_, refs.data(), n, off.data(), c.refs.data(), mode, out.data(), chosen.data(), &c.out))
      throw EngineError("zke_select_keys_from_records failed: " + std::to_string(r) + " " + zke_last_error(e_));
    const std::vector<KeyInfo> all = c.result();
    infos.assign(n, {});
    for (uint32_t i = 0; i < n; i++) infos[i].assign(all.begin() + off[i], all.begin() + off[i + 1]);
    return out;
  }

  // generate_email_inputs with the resolver's RAW answers: "raw e-mails + the records in, Email values out" — the caller is left
  // with network code only.  Errors as generate_email_inputs.
  std::vector<Email> generate_email_inputs_from_records(const std::vector<std::string>& from_domains, const std::vector<std::vector<uint8_t>>& raw_emails,
                                                        const FetchRecord& fetch_record, uint32_t mode = ZKE_KEYREC_DNS,
                                                        const std::vector<std::vector<ExternalInput>>* external_inputs = nullptr,
                                                        uint32_t max_sigs = ZKE_SCAN_MAX_SIGS) {
    const std::vector<SigScan> scans = scan_signatures(raw_emails, from_domains, max_sigs);
    std::map<std::pair<std::string, std::string>, std::optional<std::string>> cache;
    std::vector<std::vector<std::optional<std::string>>> cands(scans.size());
    std::vector<Email> probe(scans.size());
    for (size_t i = 0; i < scans.size(); i++) {
      probe[i] = Email{from_domains[i], raw_emails[i], PublicKey{}, {}};
      for (const SigInfo& s : scans[i].sigs) {
        if (s.code != 0) continue;
        auto key = std::make_pair(from_domains[i], s.selector);
        auto it = cache.find(key);
        if (it == cache.end()) it = cache.emplace(key, fetch_record(from_domains[i], s.selector)).first;
        cands[i].push_back(it->second);
      }
    }
    std::vector<uint32_t> chosen;
    std::vector<std::vector<KeyInfo>> infos;
    const std::vector<zke_result> recs = select_keys_from_records(probe, cands, chosen, infos, mode);
    return emails_of_selection(scans, probe, recs, chosen, external_inputs, [&](size_t i) { return cands[i].size(); },
                               [&](size_t i, uint32_t k) { return infos[i][k].public_key(); });
  }

 private:
  // generator.rs:36-52 over a selection's answer: one Email per e-mail under key_of(i, chosen[i]), or the reference's Err
  template <class Count, class KeyOf>
  static std::vector<Email> emails_of_selection(const std::vector<SigScan>& scans, const std::vector<Email>& probe, const std::vector<zke_result>& recs,
                                                const std::vector<uint32_t>& chosen, const std::vector<std::vector<ExternalInput>>* external_inputs,
                                                Count n_cands, KeyOf key_of) {
    std::vector<Email> out;
    for (size_t i = 0; i < scans.size(); i++) {
      const SigScan& sc = scans[i];
      if (sc.status != ZKE_OK) throw VerifyPanic(sc.status, sc.detail);
      if (sc.n_signatures == 0) throw VerifyPanic(ZKE_DKIM_NOT_PASS, ZKE_D_NO_SIGNATURE);                       // generator.rs:21
      if (chosen[i] == ZKE_SEL_NONE) {
        if (sc.n_candidates > n_cands(i)) throw VerifyPanic(ZKE_UNSUPPORTED, ZKE_D_U_TOO_MANY_SIGS);            // the list was cut
        throw VerifyPanic(recs[i].status == ZKE_UNSUPPORTED ? ZKE_UNSUPPORTED : ZKE_DKIM_NOT_PASS, recs[i].detail);   // generator.rs:52
      }
      if (chosen[i] & ZKE_SEL_AFTER_UNSUPPORTED) throw VerifyPanic(ZKE_UNSUPPORTED, ZKE_D_U_ALGO_ED25519);
      Email em = probe[i];
      em.public_key = key_of(i, chosen[i]);
      if (external_inputs) em.external_inputs = (*external_inputs)[i];
      out.push_back(std::move(em));
    }
    return out;
  }
  // The records of one call as zke_keyrec_ref[m] and the buffers of its zke_keyrec_out (3/4 of the records' bytes hold every key)
  struct KeyrecCall {
    std::vector<zke_keyrec_ref> refs;
    std::vector<zke_key_info> infos;
    std::vector<uint8_t> keys;
    zke_keyrec_out out{};
    explicit KeyrecCall(const std::vector<std::optional<std::string>>& records) {
      size_t total = 0;
      for (const auto& r : records) {
        refs.push_back(r && !r->empty() ? zke_keyrec_ref{reinterpret_cast<const uint8_t*>(r->data()), r->size()} : zke_keyrec_ref{nullptr, 0});
        total += refs.back().len;
      }
      infos.resize(records.size() + 1);
      keys.resize(total * 3 / 4 + 1);
      out.infos = infos.data(); out.infos_cap = records.size(); out.keys = keys.data(); out.keys_cap = keys.size();
    }
    std::vector<KeyInfo> result() const {
      std::vector<KeyInfo> v;
      for (size_t i = 0; i < refs.size(); i++)
        v.push_back(KeyInfo{infos[i].code, infos[i].key_type, std::vector<uint8_t>(keys.begin() + infos[i].key_off, keys.begin() + infos[i].key_off + infos[i].key_len)});
      return v;
    }
  };
  std::vector<zke_result> extract(const std::vector<Email>& emails, const std::vector<CapturePart>& header_parts,
                                  const std::vector<CapturePart>& body_parts, CaptureTables& caps, CaptureOrigins* origins) {
    const uint32_t n = (uint32_t)emails.size();
    std::vector<zke_email_ref> refs(n);
    for (uint32_t i = 0; i < n; i++) {
      const Email& em = emails[i];
      uint32_t ext = 0;
      for (const auto& x : em.external_inputs) if (!x.value) ext = 1;
      refs[i] = zke_email_ref{em.raw_email.data(), em.raw_email.size(), em.from_domain.data(), em.from_domain.size(),
                              em.public_key.key.data(), em.public_key.key.size(), key_type_code(em.public_key.key_type), ext};
    }
    std::vector<zke_capture_part> hp, bp;
    size_t G = 0;
    for (const auto& p : header_parts) { hp.push_back(zke_capture_part{p.dfa_id, p.prog_id, (uint32_t)p.groups.size(), p.groups.data()}); G += p.groups.size(); }
    for (const auto& p : body_parts) { bp.push_back(zke_capture_part{p.dfa_id, p.prog_id, (uint32_t)p.groups.size(), p.groups.data()}); G += p.groups.size(); }
    const size_t NP = (size_t)n * (hp.size() + bp.size()), NG = (size_t)n * G;
    caps.spans.assign(NG * 2 + 1, 0); caps.flags.assign(NG + 1, 0); caps.cap_off.assign(NP + 1, 0); caps.cap_str_off.assign(NG + 1, 0);
    caps.cap_blob.assign(NG * 32 + 1, 0);
    zke_capture_origin org{};
    if (origins) {
      origins->spans.assign(NG * 2 + 1, 0); origins->flags.assign(NG + 1, 0);
      org = zke_capture_origin{origins->spans.data(), NG * 2, origins->flags.data(), NG, 0, 0};
    }
    std::vector<zke_result> out(n);
    zke_capture_out o{};
    for (int attempt = 0; attempt < 2; attempt++) {
      o = zke_capture_out{caps.spans.data(), NG * 2, caps.flags.data(), NG, caps.cap_off.data(), NP + 1, caps.cap_str_off.data(), NG + 1,
                          caps.cap_blob.data(), caps.cap_blob.size(), 0, 0, 0, 0, 0, 0};
      const int r = origins ? zke_extract_captures_mapped(e_, refs.data(), n, hp.data(), (uint32_t)hp.size(), bp.data(), (uint32_t)bp.size(), out.data(), &o, &org)
                            : zke_extract_captures(e_, refs.data(), n, hp.data(), (uint32_t)hp.size(), bp.data(), (uint32_t)bp.size(), out.data(), &o);
      if (r == ZKE_E_NOMEM && attempt == 0 && o.cap_blob_need > caps.cap_blob.size()) { caps.cap_blob.resize(o.cap_blob_need); continue; }
      if (r) throw EngineError("zke_extract_captures failed: " + std::to_string(r) + " " + zke_last_error(e_));
      break;
    }
    caps.spans.resize(NG * 2); caps.flags.resize(NG); caps.cap_str_off.resize(o.n_strings + 1); caps.cap_blob.resize(o.cap_blob_need);
    if (origins) { origins->spans.resize(NG * 2); origins->flags.resize(NG); }
    return out;
  }
  static uint32_t key_type_code(const std::string& t) {
    return t == "rsa" ? ZKE_KEY_RSA : (t == "ed25519" ? ZKE_KEY_ED25519 : ZKE_KEY_OTHER);
  }
  static zke_email_ref ref_of(const Email& em) {
    uint32_t ext = 0;
    for (const auto& x : em.external_inputs) if (!x.value) ext = 1;                      // circuits.rs:24
    return zke_email_ref{em.raw_email.data(), em.raw_email.size(), em.from_domain.data(), em.from_domain.size(),
                         em.public_key.key.data(), em.public_key.key.size(), key_type_code(em.public_key.key_type), ext};
  }
  // A vector of EmailWithRegex that shares one part list as zke_verify_emails_with_regex takes it: the pairs registered, the e-mails
  // where they are, the captures as CSR tables.  `lists` points into the pack.
  struct ListsPack {
    std::vector<uint32_t> hids, bids, cap_off{0}, cap_str_off{0};
    std::vector<uint8_t> cap_blob;
    std::vector<zke_email_ref> refs;
    zke_regex_lists lists{};
  };
  void pack_lists(const std::vector<EmailWithRegex>& in, ListsPack& p) {
    auto ids_of = [&](const std::optional<std::vector<CompiledRegex>>& parts) {
      std::vector<uint32_t> v;
      if (parts)
        for (const auto& q : *parts) {
          uint32_t id = 0;
          if (int r = zke_dfa_register(e_, q.verify_re.fwd.data(), q.verify_re.fwd.size(), q.verify_re.bwd.data(), q.verify_re.bwd.size(), &id))
            throw EngineError("zke_dfa_register failed: " + std::to_string(r) + " " + zke_last_error(e_));
          v.push_back(id);                       // an equal pair registered again gets the id it already has
        }
      return v;
    };
    p.hids = ids_of(in[0].regex_info.header_parts);
    p.bids = ids_of(in[0].regex_info.body_parts);
    p.refs.resize(in.size());
    for (size_t i = 0; i < in.size(); i++) {
      if (ids_of(in[i].regex_info.header_parts) != p.hids || ids_of(in[i].regex_info.body_parts) != p.bids)
        throw EngineError("a batch must share one part list; split it per regex_config");
      p.refs[i] = ref_of(in[i].email);
      for (const auto* parts : {&in[i].regex_info.header_parts, &in[i].regex_info.body_parts})
        if (*parts)
          for (const auto& q : **parts) {
            if (q.captures)
              for (const auto& s : *q.captures) { p.cap_blob.insert(p.cap_blob.end(), s.begin(), s.end()); p.cap_str_off.push_back((uint32_t)p.cap_blob.size()); }
            p.cap_off.push_back((uint32_t)p.cap_str_off.size() - 1);
          }
    }
    if (p.cap_blob.empty()) p.cap_blob.push_back(0);
    p.lists = zke_regex_lists{(uint32_t)p.hids.size(), p.hids.data(), (uint32_t)p.bids.size(), p.bids.data(),
                              p.hids.size() + p.bids.size() ? p.cap_off.data() : nullptr, p.cap_str_off.data(), p.cap_blob.data()};
  }
  // zke_verify_emails_encoded over refs (and `lists`, or nullptr for verify_email): the external inputs flattened [name, value, ...]
  // (circuits.rs:18-27; a None value travels as "": its e-mail reports ZKE_EXTERNAL_INPUT_NULL and is not encoded), a first call
  // that asks for the sizes — they are exact and known before anything runs —, the call itself.
  std::vector<EncodedOutput> encoded_call(const std::vector<zke_email_ref>& refs, const std::vector<const Email*>& ems, const zke_regex_lists* lists) {
    const uint32_t n = (uint32_t)refs.size();
    std::vector<uint32_t> ext_off{0}, ext_str_off{0};
    std::vector<uint8_t> ext_blob;
    for (const Email* em : ems) {
      for (const auto& x : em->external_inputs)
        for (const std::string* s : {&x.name, x.value ? &*x.value : nullptr}) {
          if (s) ext_blob.insert(ext_blob.end(), s->begin(), s->end());
          ext_str_off.push_back((uint32_t)ext_blob.size());
        }
      ext_off.push_back((uint32_t)ext_str_off.size() - 1);
    }
    if (ext_blob.empty()) ext_blob.push_back(0);
    const zke_encode_in in{lists, nullptr, ext_off.data(), ext_str_off.data(), ext_blob.data()};
    std::vector<zke_result> recs(n);
    zke_encoded_out enc{};
    int r = zke_verify_emails_encoded(e_, refs.data(), n, &in, recs.data(), &enc);
    if (r && r != ZKE_E_NOMEM) throw EngineError("zke_verify_emails_encoded failed: " + std::to_string(r) + " " + zke_last_error(e_));
    std::vector<zke_encoded_info> infos(enc.infos_need + 1);
    std::vector<uint8_t> bytes(enc.bytes_need + 1);
    enc = zke_encoded_out{infos.data(), enc.infos_need, bytes.data(), enc.bytes_need, 0, 0};
    if ((r = zke_verify_emails_encoded(e_, refs.data(), n, &in, recs.data(), &enc)))
      throw EngineError("zke_verify_emails_encoded failed: " + std::to_string(r) + " " + zke_last_error(e_));
    std::vector<EncodedOutput> out(n);
    for (uint32_t i = 0; i < n; i++) {
      out[i].status = recs[i].status; out[i].detail = recs[i].detail; out[i].kind = infos[i].kind;
      out[i].bytes.assign(bytes.begin() + infos[i].off, bytes.begin() + infos[i].off + infos[i].len);
      std::copy(infos[i].digest, infos[i].digest + 32, out[i].digest.begin());
    }
    return out;
  }
  // One e-mail through the single-e-mail entry points of the C-ABI (zke_verify_email / zke_verify_email_with_regex).
  zke_result run(const Email& em, const RegexInfo* ri) {
    uint32_t ext = 0;
    for (const auto& x : em.external_inputs) if (!x.value) ext = 1;                      // circuits.rs:24
    const uint32_t kt = key_type_code(em.public_key.key_type);
    zke_result r{};
    int rc;
    if (!ri) {
      rc = zke_verify_email(e_, em.raw_email.data(), em.raw_email.size(), em.from_domain.data(), em.from_domain.size(),
                            em.public_key.key.data(), em.public_key.key.size(), kt, ext, &r);
    } else {
      // RegexInfo -> two zke_regex_part lists; the pointer tables live until the call returns
      std::vector<zke_regex_part> hp, bp;
      std::vector<std::vector<const uint8_t*>> ptrs;
      std::vector<std::vector<size_t>> lens;
      size_t total = 0;
      for (const auto* parts : {&ri->header_parts, &ri->body_parts}) if (*parts) total += (*parts)->size();
      ptrs.reserve(total); lens.reserve(total);
      for (const auto* parts : {&ri->header_parts, &ri->body_parts}) {
        if (!*parts) continue;
        for (const auto& p : **parts) {
          ptrs.emplace_back(); lens.emplace_back();
          if (p.captures)
            for (const auto& s : *p.captures) { ptrs.back().push_back(reinterpret_cast<const uint8_t*>(s.data())); lens.back().push_back(s.size()); }
          zke_regex_part q{};
          q.fwd = p.verify_re.fwd.data(); q.fwd_len = p.verify_re.fwd.size();
          q.bwd = p.verify_re.bwd.data(); q.bwd_len = p.verify_re.bwd.size();
          q.n_captures = (uint32_t)ptrs.back().size();
          q.captures = ptrs.back().data(); q.capture_lens = lens.back().data();
          (parts == &ri->header_parts ? hp : bp).push_back(q);
        }
      }
      rc = zke_verify_email_with_regex(e_, em.raw_email.data(), em.raw_email.size(), em.from_domain.data(), em.from_domain.size(),
                                       em.public_key.key.data(), em.public_key.key.size(), kt, ext, hp.data(), (uint32_t)hp.size(),
                                       bp.data(), (uint32_t)bp.size(), &r);
    }
    if (rc) throw EngineError(std::string("zke_verify_email: ") + zke_last_error(e_) + " (" + std::to_string(rc) + ")");
    return r;
  }
  static EmailVerifierOutput output(const Email& em, const zke_result& r) {
    EmailVerifierOutput o;
    o.from_domain_hash.assign(r.from_domain_hash, r.from_domain_hash + 32);            // circuits.rs:16
    o.public_key_hash.assign(r.public_key_hash, r.public_key_hash + 32);               // circuits.rs:17
    for (const auto& x : em.external_inputs) { o.external_inputs.push_back(x.name); o.external_inputs.push_back(*x.value); }
    return o;
  }
  zke_engine* e_ = nullptr;
};

inline Engine& default_engine() {
  static Engine e;
  return e;
}
inline EmailVerifierOutput verify_email(const Email& email) { return default_engine().verify_email(email); }
// core/src/email.rs:61-86 remove_quoted_printable_soft_breaks, both return values (zke_qp_clean_batch on a batch of one): the body
// without its "=\r\n" soft breaks, zero-padded to its length, and index_map — the position in `body` of every cleaned byte,
// usize::MAX over the padding.
inline std::pair<std::vector<uint8_t>, std::vector<size_t>> remove_quoted_printable_soft_breaks(Engine& engine, const std::vector<uint8_t>& body) {
  const uint64_t off[2] = {0, body.size()};
  std::vector<uint8_t> cleaned(body.size());
  std::vector<uint32_t> map32(body.size());
  uint32_t kept = 0;
  if (int r = zke_qp_clean_batch(engine.raw(), body.data(), off, 1, cleaned.data(), map32.data(), &kept))
    throw EngineError("zke_qp_clean_batch failed: " + std::to_string(r) + " " + zke_last_error(engine.raw()));
  std::vector<size_t> index_map(body.size());
  for (size_t j = 0; j < body.size(); j++) index_map[j] = map32[j] == ZKE_QP_NO_INDEX ? SIZE_MAX : (size_t)map32[j];
  return {std::move(cleaned), std::move(index_map)};
}
inline EmailWithRegexVerifierOutput verify_email_with_regex(const EmailWithRegex& in) {
  return default_engine().verify_email_with_regex(in);
}
// core/src/email.rs:7 extract_email_body(&parse_mail(raw).unwrap()): the decoded body.  Throws VerifyPanic naming the site where the
// reference panics — core/src/email.rs:26 (parse_mail), :21 (get_body_raw of the text/html part), :17 (of the first part or the
// message) — or, for an input the engine does not decide (ZKE_UNSUPPORTED), the site it stopped in front of.
inline std::vector<uint8_t> extract_email_body(Engine& engine, const std::vector<uint8_t>& raw) {
  BodyInfo f = engine.extract_email_bodies({raw})[0];
  if (f.status == ZKE_OK) return std::move(f.body);
  const bool parse = f.status == ZKE_PARSE_FAIL || (f.status == ZKE_UNSUPPORTED && f.detail != ZKE_D_U_BODY_CTE);
  throw VerifyPanic(f.status, f.detail, parse ? "core/src/email.rs:26" : (f.part >> 31) ? "core/src/email.rs:21" : "core/src/email.rs:17");
}
inline std::vector<uint8_t> extract_email_body(const std::vector<uint8_t>& raw) { return extract_email_body(default_engine(), raw); }
// helpers/src/generator.rs:11 generate_email_inputs(from_domain, raw_email, external_inputs) with the key fetch as a callback
inline Email generate_email_inputs(const std::string& from_domain, const std::vector<uint8_t>& raw_email, const FetchKey& fetch_key,
                                   std::optional<std::vector<ExternalInput>> external_inputs = std::nullopt) {
  std::vector<std::vector<ExternalInput>> ext{external_inputs.value_or(std::vector<ExternalInput>{})};
  return default_engine().generate_email_inputs({from_domain}, {raw_email}, fetch_key, &ext)[0];
}
// ... and with the resolver's raw answer (TXT record or archive value) in place of the key: dkim.rs:67-111 runs on the GPU
inline Email generate_email_inputs_from_records(const std::string& from_domain, const std::vector<uint8_t>& raw_email, const FetchRecord& fetch_record,
                                                uint32_t mode = ZKE_KEYREC_DNS, std::optional<std::vector<ExternalInput>> external_inputs = std::nullopt) {
  std::vector<std::vector<ExternalInput>> ext{external_inputs.value_or(std::vector<ExternalInput>{})};
  return default_engine().generate_email_inputs_from_records({from_domain}, {raw_email}, fetch_record, mode, &ext)[0];
}

}  // namespace zkemail
