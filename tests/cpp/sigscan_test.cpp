// Exercises the generator half of include/zkemail_core.hpp: scan_signatures, select_keys, generate_email_inputs.
// usage: sigscan_test <raw.eml> <from_domain> <max_sigs> [<selector> <key.der> <key_type>]...
// prints one line "SCAN <status> <detail> <n_signatures> <n_candidates>", one line "SIG <header_index> <code> <algo> <selector>
// <val_start> <val_end>" per record, then — generate_email_inputs with a resolver made of the (selector, key, type) triples of the
// command line — "GEN <resolver calls> <chosen key's type> <its length> <domain/selector asked, in order>" and "VERIFIED <2 bytes
// of public_key_hash>" (verify_email of the generated Email), or "PANIC <status> <detail> <resolver calls>".
#include <cstdio>
#include <fstream>
#include <iterator>
#include <map>

#include "zkemail_core.hpp"

static std::vector<uint8_t> slurp(const char* p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 4) % 3) return 2;
  const std::vector<uint8_t> raw = slurp(argv[1]);
  const std::string dom = argv[2];
  const uint32_t max_sigs = (uint32_t)std::atoi(argv[3]);
  std::map<std::string, zkemail::PublicKey> keys;
  for (int a = 4; a + 2 < argc; a += 3) keys[argv[a]] = zkemail::PublicKey{slurp(argv[a + 1]), argv[a + 2]};
  zkemail::Engine eng;
  const auto scans = eng.scan_signatures({raw, raw}, {dom, dom}, max_sigs);
  const zkemail::SigScan& sc = scans[1];
  std::printf("SCAN %u %u %u %u\n", sc.status, sc.detail, sc.n_signatures, sc.n_candidates);
  for (const auto& s : sc.sigs) std::printf("SIG %u %u %u %s %u %u\n", s.header_index, s.code, s.algo, s.selector.c_str(), s.val_start, s.val_end);
  int calls = 0;
  std::string asked;
  auto fetch = [&](const std::string& d, const std::string& sel) -> std::optional<zkemail::PublicKey> {
    calls++;
    asked += (asked.empty() ? "" : ",") + d + "/" + sel;
    auto it = keys.find(sel);
    if (it == keys.end()) return std::nullopt;
    return it->second;
  };
  try {
    const auto ems = eng.generate_email_inputs({dom, dom}, {raw, raw}, fetch, nullptr, max_sigs);
    std::printf("GEN %d %s %zu %s\n", calls, ems[1].public_key.key_type.c_str(), ems[1].public_key.key.size(), asked.c_str());
    const auto out = eng.verify_email(ems[0]);            // what the generator returns is what verify_email takes
    std::printf("VERIFIED %02x%02x\n", out.public_key_hash[0], out.public_key_hash[1]);
  } catch (const zkemail::VerifyPanic& p) {
    std::printf("PANIC %u %u %d\n", p.status, p.detail, calls);
    return 1;
  }
  return 0;
}
