// Host check that h84_repair4 of codec_math.h -- the form the repairing attention
// kernels use: the XOR and the counts read off h_code4 -- equals h84_scrub4, the
// scrubber's decode / re-encode form: every byte value in every byte lane of a
// word (with several fillers in the other lanes), and every 16-bit pattern in
// both halves.  The XOR, and each of the three counters, must agree.
// Built and run by tests/test_attention_repair.py; prints "mismatches N".
#include <cstdio>
#include "codec_math.h"

using namespace kvecc;

static long g_bad = 0;

static void check(uint32_t w) {
  uint32_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
  const uint32_t want = h84_scrub4(w, a[0], a[1], a[2]);
  const uint32_t got = h84_repair4(w, b[0], b[1], b[2]);
  const bool ok = want == got && a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
  if (!ok && g_bad++ < 8)
    std::printf("mismatch at %08x: xor %08x / %08x, counts %u %u %u / %u %u %u\n", w, want, got, a[0], a[1], a[2],
                b[0], b[1], b[2]);
}

int main() {
  const uint32_t fills[] = {0x00u, 0x5Au, 0xFFu, 0x33u, 0x80u, 0x0Fu, 0x01u};
  for (uint32_t lane = 0; lane < 4; ++lane)
    for (uint32_t fill : fills)
      for (uint32_t b = 0; b < 256; ++b) check(((fill * 0x01010101u) & ~(0xFFu << (8 * lane))) | b << (8 * lane));
  for (uint32_t v = 0; v < (1u << 16); ++v) {
    check(v | v << 16);
    check(v << 8 | (v * 0x9E37u & 0xFFu) | (v * 0x85EBu & 0xFF00u) << 16);
  }
  std::printf("mismatches %ld\n", g_bad);
  return g_bad != 0;
}
