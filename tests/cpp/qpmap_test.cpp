// Exercises the index-map part of include/zkemail_core.hpp: remove_quoted_printable_soft_breaks and the extract_captures
// overload that fills origins.
// usage: qpmap_test <body file> [<raw.eml> <from_domain> <key.der> <fwd dfa> <bwd dfa> <capture program> <group>...]
// prints "QP <kept bytes> <cleaned, hex>" and "MAP <index_map entries, MAX for usize::MAX>" for the body; then, for the e-mail with the
// pattern as its one body part, "REC <status> <detail>" and per requested group "ORG <span start> <span end> <origin start>
// <origin end> <flags>", and "SAME <1 if the overload without origins delivers the same record and tables>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

#include "zkemail_core.hpp"

static std::vector<uint8_t> slurp(const char* p) {
  std::ifstream f(p, std::ios::binary);
  const std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  return std::vector<uint8_t>(s.begin(), s.end());
}

int main(int argc, char** argv) {
  if (argc != 2 && argc < 9) return 2;
  zkemail::Engine eng;
  const std::vector<uint8_t> body = slurp(argv[1]);
  const auto [cleaned, index_map] = zkemail::remove_quoted_printable_soft_breaks(eng, body);
  size_t kept = 0;
  while (kept < index_map.size() && index_map[kept] != SIZE_MAX) kept++;
  std::printf("QP %zu ", kept);
  for (uint8_t c : cleaned) std::printf("%02x", c);
  std::printf("\nMAP");
  for (size_t x : index_map) { if (x == SIZE_MAX) std::printf(" MAX"); else std::printf(" %zu", x); }
  std::printf("\n");
  if (argc == 2) return 0;

  const std::vector<uint8_t> fwd = slurp(argv[5]), bwd = slurp(argv[6]), prog = slurp(argv[7]);
  zkemail::CapturePart part{};
  if (zke_dfa_register(eng.raw(), fwd.data(), fwd.size(), bwd.data(), bwd.size(), &part.dfa_id) ||
      zke_capture_register(eng.raw(), prog.data(), prog.size(), &part.prog_id))
    return 3;
  for (int a = 8; a < argc; a++) part.groups.push_back((uint32_t)std::atoi(argv[a]));
  const zkemail::Email em{argv[3], slurp(argv[2]), zkemail::PublicKey{slurp(argv[4]), "rsa"}, {}};
  zkemail::CaptureTables caps, plain;
  zkemail::CaptureOrigins org;
  const auto recs = eng.extract_captures({em}, {}, {part}, caps, org);
  std::printf("REC %u %u\n", recs[0].status, recs[0].detail);
  for (size_t g = 0; g < part.groups.size(); g++)
    std::printf("ORG %u %u %u %u %u\n", caps.spans[2 * g], caps.spans[2 * g + 1], org.spans[2 * g], org.spans[2 * g + 1], org.flags[g]);
  const auto recs2 = eng.extract_captures({em}, {}, {part}, plain);
  const bool same = !std::memcmp(&recs[0], &recs2[0], sizeof(zke_result)) && plain.spans == caps.spans && plain.flags == caps.flags &&
                    plain.cap_off == caps.cap_off && plain.cap_str_off == caps.cap_str_off && plain.cap_blob == caps.cap_blob;
  std::printf("SAME %d\n", same ? 1 : 0);
  return 0;
}
