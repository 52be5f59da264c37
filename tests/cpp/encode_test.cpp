// Exercises the encoded batch calls of include/zkemail_core.hpp: Engine::verify_emails_encoded and verify_emails_with_regex_encoded.
// usage: encode_test <caps.txt> <h0.dfa> <b0.dfa> -- <m0> <m1> ...      (each <x.dfa> is the pair x.dfa.fwd / x.dfa.bwd, each <m> the
//        pair m.eml / m.key; from_domain is example.com)
// Every e-mail gets the config {header part h0, body part b0}; caps.txt holds one line per (e-mail, part) in order, the part's capture
// strings separated by tabs.  E-mail i carries the external inputs ("name<i>", "value<i>") when i is even, ("a", "") and ("", "b") on
// top when i is a multiple of 4, and a null value when i is 3.
// prints per e-mail "plain <i> <status> <kind> <digest hex> <encoding hex>", then "regex <i> ..." likewise for the second call.
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
static void show(const char* tag, const std::vector<zkemail::EncodedOutput>& outs) {
  for (size_t i = 0; i < outs.size(); i++) {
    std::printf("%s %zu %u %u ", tag, i, outs[i].status, outs[i].kind);
    for (uint8_t c : outs[i].digest) std::printf("%02x", c);
    std::printf(" ");
    for (uint8_t c : outs[i].bytes) std::printf("%02x", c);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc < 6 || std::strcmp(argv[4], "--")) return 2;
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
  const zkemail::DFA h0 = pair_of(argv[2]), b0 = pair_of(argv[3]);
  std::vector<zkemail::Email> emails;
  std::vector<zkemail::EmailWithRegex> inputs;
  for (int k = 5; k < argc; k++) {
    const int i = k - 5;
    zkemail::Email em;
    em.raw_email = slurp(std::string(argv[k]) + ".eml");
    em.public_key = {slurp(std::string(argv[k]) + ".key"), "rsa"};
    em.from_domain = "example.com";
    if (i % 2 == 0) em.external_inputs.push_back({"name" + std::to_string(i), "value" + std::to_string(i), 0});
    if (i % 4 == 0) { em.external_inputs.push_back({"a", "", 0}); em.external_inputs.push_back({"", "b", 0}); }
    if (i == 3) em.external_inputs.push_back({"absent", std::nullopt, 0});
    zkemail::RegexInfo ri;
    ri.header_parts = std::vector<zkemail::CompiledRegex>{zkemail::CompiledRegex{h0, next_caps()}};
    ri.body_parts = std::vector<zkemail::CompiledRegex>{zkemail::CompiledRegex{b0, next_caps()}};
    emails.push_back(em);
    inputs.push_back(zkemail::EmailWithRegex{std::move(em), std::move(ri)});
  }
  try {
    zkemail::Engine eng;
    show("plain", eng.verify_emails_encoded(emails));
    show("regex", eng.verify_emails_with_regex_encoded(inputs));
  } catch (const zkemail::EngineError& e) {
    std::printf("ERROR %s\n", e.what());
    return 1;
  }
  return 0;
}
