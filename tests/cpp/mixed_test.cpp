// Exercises zkemail::Engine::verify_emails_mixed of include/zkemail_core.hpp: one batch whose e-mails carry different regex configs.
// usage: mixed_test <caps.txt> <a0.dfa> <a1.dfa> <d0.dfa> -- <m0> <m1> ...      (each <x.dfa> is the pair x.dfa.fwd / x.dfa.bwd,
//        each <m> the pair m.eml / m.key; from_domain is example.com)
// The first three e-mails get the config {header parts a0, a1}, the next three {body part d0}, the rest none.  caps.txt holds one
// line per (e-mail, part) in order, the part's capture strings separated by tabs.
// prints one line per e-mail: "record <i> <status> <detail> <regex_part> <match_count> <match_start> <match_end> <header_hash hex>"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>

#include "zkemail_core.hpp"

static std::vector<uint8_t> slurp(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 7 || std::strcmp(argv[5], "--")) return 2;
  std::ifstream caps(argv[1]);
  auto next_caps = [&]() {
    std::string line, s;
    std::getline(caps, line);
    std::vector<std::string> out;
    std::stringstream ss(line);
    while (std::getline(ss, s, '\t')) out.push_back(s);
    return out;
  };
  auto pair_of = [&](const char* base) { return zkemail::DFA{slurp(std::string(base) + ".fwd"), slurp(std::string(base) + ".bwd")}; };
  const zkemail::DFA a0 = pair_of(argv[2]), a1 = pair_of(argv[3]), d0 = pair_of(argv[4]);
  std::vector<std::pair<zkemail::Email, std::optional<zkemail::RegexInfo>>> in;
  for (int k = 6; k < argc; k++) {
    zkemail::Email em;
    em.raw_email = slurp(std::string(argv[k]) + ".eml");
    em.public_key = {slurp(std::string(argv[k]) + ".key"), "rsa"};
    em.from_domain = "example.com";
    const int i = k - 6;
    std::optional<zkemail::RegexInfo> ri;
    if (i < 3) {
      ri = zkemail::RegexInfo{};
      zkemail::CompiledRegex p0{a0, next_caps()};
      zkemail::CompiledRegex p1{a1, next_caps()};
      ri->header_parts = std::vector<zkemail::CompiledRegex>{p0, p1};
    } else if (i < 6) {
      ri = zkemail::RegexInfo{};
      ri->body_parts = std::vector<zkemail::CompiledRegex>{zkemail::CompiledRegex{d0, next_caps()}};
    }
    in.emplace_back(std::move(em), std::move(ri));
  }
  try {
    zkemail::Engine eng;
    const auto recs = eng.verify_emails_mixed(in);
    for (size_t i = 0; i < recs.size(); i++) {
      const zke_result& r = recs[i];
      std::printf("record %zu %u %u %u %u %u %u ", i, r.status, r.detail, r.regex_part, r.match_count, r.match_start, r.match_end);
      for (int b = 0; b < 32; b++) std::printf("%02x", r.header_hash[b]);
      std::printf("\n");
    }
  } catch (const zkemail::EngineError& e) {
    std::printf("ERROR %s\n", e.what());
    return 1;
  }
  return 0;
}
