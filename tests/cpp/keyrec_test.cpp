// Exercises the key-record part of include/zkemail_core.hpp: decode_key_records, select_keys_from_records (through
// generate_email_inputs_from_records) and the free function.
// usage: keyrec_test <mode> <raw.eml> <from_domain> [<selector> <record file>]...
// prints one line "KEY <code> <key_type> <key length> <first two key bytes, hex>" per record of the command line (decoded as one
// batch, a failed fetch appended), then — generate_email_inputs_from_records with a resolver made of the (selector, record) pairs —
// "GEN <resolver calls> <chosen key's type> <its length>" and "VERIFIED <2 bytes of public_key_hash>" (verify_email of the
// generated Email), or "PANIC <status> <detail> <resolver calls>".
#include <cstdio>
#include <fstream>
#include <iterator>
#include <map>

#include "zkemail_core.hpp"

static std::string slurp(const char* p) {
  std::ifstream f(p, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 4) % 2) return 2;
  const uint32_t mode = (uint32_t)std::atoi(argv[1]);
  const std::string rs = slurp(argv[2]);
  const std::vector<uint8_t> raw(rs.begin(), rs.end());
  const std::string dom = argv[3];
  std::map<std::string, std::string> records;
  std::vector<std::optional<std::string>> flat;
  for (int a = 4; a + 1 < argc; a += 2) { records[argv[a]] = slurp(argv[a + 1]); flat.push_back(records[argv[a]]); }
  flat.push_back(std::nullopt);
  zkemail::Engine eng;
  for (const zkemail::KeyInfo& k : eng.decode_key_records(flat, mode))
    std::printf("KEY %u %u %zu %02x%02x\n", k.code, k.key_type, k.key.size(), k.key.size() > 0 ? k.key[0] : 0, k.key.size() > 1 ? k.key[1] : 0);
  int calls = 0;
  auto fetch = [&](const std::string&, const std::string& sel) -> std::optional<std::string> {
    calls++;
    auto it = records.find(sel);
    if (it == records.end()) return std::nullopt;
    return it->second;
  };
  try {
    const auto ems = eng.generate_email_inputs_from_records({dom, dom}, {raw, raw}, fetch, mode);
    std::printf("GEN %d %s %zu\n", calls, ems[1].public_key.key_type.c_str(), ems[1].public_key.key.size());
    const auto out = eng.verify_email(ems[0]);            // what the generator returns is what verify_email takes
    std::printf("VERIFIED %02x%02x\n", out.public_key_hash[0], out.public_key_hash[1]);
  } catch (const zkemail::VerifyPanic& p) {
    std::printf("PANIC %u %u %d\n", p.status, p.detail, calls);
    return 1;
  }
  return 0;
}
