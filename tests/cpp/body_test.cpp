// Exercises the body part of include/zkemail_core.hpp: Engine::extract_email_bodies and the free extract_email_body.
// usage: body_test <keep_eol 0|1> <raw.eml>...
// prints per e-mail "INFO <status> <detail> <part> <encoding> <src_off> <src_len> <body, hex>" (the batch call), then per e-mail
// "BODY <hex>" or "PANIC <status> <detail> <what()>" (the reference's call, one e-mail at a time).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "zkemail_core.hpp"

static std::vector<uint8_t> slurp(const char* p) {
  std::ifstream f(p, std::ios::binary);
  const std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  return std::vector<uint8_t>(s.begin(), s.end());
}
static void hex(const std::vector<uint8_t>& v) { for (uint8_t c : v) std::printf("%02x", c); }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  zkemail::Engine eng;
  std::vector<std::vector<uint8_t>> raws;
  for (int a = 2; a < argc; a++) raws.push_back(slurp(argv[a]));
  for (const zkemail::BodyInfo& f : eng.extract_email_bodies(raws, std::atoi(argv[1]) != 0)) {
    std::printf("INFO %u %u %u %u %u %u ", f.status, f.detail, f.part, f.encoding, f.src_off, f.src_len);
    hex(f.body);
    std::printf("\n");
  }
  for (const auto& raw : raws) {
    try {
      const std::vector<uint8_t> body = zkemail::extract_email_body(eng, raw);
      std::printf("BODY ");
      hex(body);
      std::printf("\n");
    } catch (const zkemail::VerifyPanic& p) {
      std::printf("PANIC %u %u %s\n", p.status, p.detail, p.what());
    }
  }
  return 0;
}
