// utf8_lossy_fuzz — the serial routines of zkemail.rs_amd/csrc/utf8_lossy.hip.h (utf8_lossy_len, utf8_lossy_write) over the cases
// on stdin, for tests/test_utf8_lossy_sanitizers.py to compare with Python's decode("utf-8", "replace").  Built with
// -fsanitize=address,undefined: every case is read from a heap block of exactly its length and written into one of exactly the
// length utf8_lossy_len reported, so a read or write one byte outside either is a report, not a wrong answer.
//   stdin    per case: u32 length (little endian), the bytes
//   stdout   per case: u32 repaired length, the repaired bytes; then the line "utf8_lossy_fuzz ok <cases>"
#define ZKE_UTF8_LOSSY_SCALAR_ONLY
#include "../../zkemail.rs_amd/csrc/utf8_lossy.hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool read_exact(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

int main() {
  std::vector<uint8_t> out;
  size_t cases = 0;
  for (;;) {
    uint8_t lb[4];
    const size_t got = fread(lb, 1, 4, stdin);
    if (got == 0) break;
    if (got != 4) { fprintf(stderr, "truncated length\n"); return 2; }
    const uint32_t n = (uint32_t)lb[0] | (uint32_t)lb[1] << 8 | (uint32_t)lb[2] << 16 | (uint32_t)lb[3] << 24;
    uint8_t* src = static_cast<uint8_t*>(malloc(n ? n : 1));      // (n == 0: a block nothing may be read from but its address)
    if (!src || !read_exact(src, n)) { fprintf(stderr, "truncated case\n"); return 2; }
    const size_t len = zke::utf8_lossy_len(src, n);
    if (len > 3 * (size_t)n) { fprintf(stderr, "case %zu: length %zu beyond three times %u\n", cases, len, n); return 1; }
    uint8_t* dst = static_cast<uint8_t*>(malloc(len ? len : 1));
    if (!dst) return 2;
    const size_t wrote = zke::utf8_lossy_write(src, n, dst);
    if (wrote != len) { fprintf(stderr, "case %zu: wrote %zu, measured %zu\n", cases, wrote, len); return 1; }
    const uint32_t l32 = (uint32_t)len;
    const uint8_t ob[4] = {(uint8_t)l32, (uint8_t)(l32 >> 8), (uint8_t)(l32 >> 16), (uint8_t)(l32 >> 24)};
    out.insert(out.end(), ob, ob + 4);
    out.insert(out.end(), dst, dst + len);
    free(dst);
    free(src);
    cases++;
  }
  if (!out.empty() && fwrite(out.data(), 1, out.size(), stdout) != out.size()) return 2;
  printf("utf8_lossy_fuzz ok %zu\n", cases);
  return 0;
}
