// Exercises Engine::extract_captures_encoded and Engine::utf8_lossy of include/zkemail_core.hpp.
// usage: extract_encoded_test <h0> <b0> -- <m0> <m1> ...     (each part <x> is the triple x.fwd / x.bwd / x.prog — the DFA pair and the
//        capture program of one pattern —, each <m> the pair m.eml / m.key; from_domain is example.com)
// Every e-mail gets the part list {header part h0: group 1, body part b0: groups 0 and 1}.  E-mail i carries the external input
// ("name<i>", "value<i>") when i is even.
// prints per e-mail "enc <i> <status> <kind> <digest hex> <encoding hex>", then per e-mail "str <i> <hex> <hex> ..." (its strings as
// the tables hold them), then "same 1" when a second call without tables gave the same outputs, then "lossy <hex> <changed>" for
// the Unicode standard's example through utf8_lossy.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

#include "zkemail_core.hpp"

static std::vector<uint8_t> slurp(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void hex(const uint8_t* p, size_t n) { for (size_t k = 0; k < n; k++) std::printf("%02x", p[k]); }

int main(int argc, char** argv) {
  if (argc < 5 || std::strcmp(argv[3], "--")) return 2;
  try {
    zkemail::Engine eng;
    auto part_of = [&](const char* base, std::vector<uint32_t> groups) {
      const auto fwd = slurp(std::string(base) + ".fwd"), bwd = slurp(std::string(base) + ".bwd"), prog = slurp(std::string(base) + ".prog");
      zkemail::CapturePart part{0, 0, std::move(groups)};
      if (zke_dfa_register(eng.raw(), fwd.data(), fwd.size(), bwd.data(), bwd.size(), &part.dfa_id) ||
          zke_capture_register(eng.raw(), prog.data(), prog.size(), &part.prog_id))
        throw zkemail::EngineError(std::string("registration failed: ") + zke_last_error(eng.raw()));
      return part;
    };
    const std::vector<zkemail::CapturePart> hp{part_of(argv[1], {1})}, bp{part_of(argv[2], {0, 1})};
    std::vector<zkemail::Email> emails;
    for (int k = 4; k < argc; k++) {
      const int i = k - 4;
      zkemail::Email em;
      em.raw_email = slurp(std::string(argv[k]) + ".eml");
      em.public_key = {slurp(std::string(argv[k]) + ".key"), "rsa"};
      em.from_domain = "example.com";
      if (i % 2 == 0) em.external_inputs.push_back({"name" + std::to_string(i), "value" + std::to_string(i), 0});
      emails.push_back(std::move(em));
    }
    zkemail::CaptureTables caps;
    const auto outs = eng.extract_captures_encoded(emails, hp, bp, &caps);
    for (size_t i = 0; i < outs.size(); i++) {
      std::printf("enc %zu %u %u ", i, outs[i].status, outs[i].kind);
      hex(outs[i].digest.data(), 32);
      std::printf(" ");
      hex(outs[i].bytes.data(), outs[i].bytes.size());
      std::printf("\n");
    }
    const size_t P = 2;
    for (size_t i = 0; i < outs.size(); i++) {
      std::printf("str %zu", i);
      for (uint32_t s = caps.cap_off[i * P]; s < caps.cap_off[(i + 1) * P]; s++) {
        std::printf(" x");
        hex(caps.cap_blob.data() + caps.cap_str_off[s], caps.cap_str_off[s + 1] - caps.cap_str_off[s]);
      }
      std::printf("\n");
    }
    const auto bare = eng.extract_captures_encoded(emails, hp, bp);
    bool same = bare.size() == outs.size();
    for (size_t i = 0; same && i < outs.size(); i++)
      same = bare[i].status == outs[i].status && bare[i].bytes == outs[i].bytes && bare[i].digest == outs[i].digest;
    std::printf("same %d\n", same ? 1 : 0);
    std::vector<uint8_t> changed;
    const std::vector<uint8_t> example{0x61, 0xF1, 0x80, 0x80, 0xE1, 0x80, 0xC2, 0x62, 0x80, 0x63, 0x80, 0xBF, 0x64};
    const auto fixed = eng.utf8_lossy({example, {'o', 'k'}}, &changed);
    std::printf("lossy ");
    hex(fixed[0].data(), fixed[0].size());
    std::printf(" %u %u\n", (unsigned)changed[0], (unsigned)changed[1]);
  } catch (const zkemail::EngineError& e) {
    std::printf("ERROR %s\n", e.what());
    return 1;
  }
  return 0;
}
