// TEST PROGRAM (CPU) for the portable core of leo_erasure_amd/csrc/
// gfw_heal_tile.hpp: gfwheal::mac_in<W> and gfwheal::from_domain<W>, the
// per-lane arithmetic "acc ^= c * x" and the way back to bytes that
// gfw_heal_list runs on the GPU, against field arithmetic taken from the
// oracle.  Stand-alone (its own main), so it can also be built with
// -fsanitize=address,undefined and run directly.  Not part of the product.
//
//   gfw_heal_core_test VECTORS
//
// VECTORS (written by tests/test_scrub_gfw_cpu.py from oracle.gf_mul), little
// endian u32 words: the number of records, then per record: w, n, n inputs of
// 17 words each (the coefficient c, a lane's 16 registers of words x), and the
// 16 registers of the XOR of the n products c * x.
// Built with codes.cpp: the reduction byte of w = 8 comes from field(8), as in
// scrub.hip.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../leo_erasure_amd/csrc/codes.hpp"
#include "../leo_erasure_amd/csrc/gfw_heal_tile.hpp"

namespace {

using leoec::gfwheal::kRegs;

template <int W>
bool check(const uint32_t* in, uint32_t n, const uint32_t* want, uint32_t red) {
  uint32_t acc[1][kRegs];
  for (int r = 0; r < kRegs; ++r) acc[0][r] = 0u;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t x[kRegs];
    std::memcpy(x, in + (size_t)i * 17 + 1, sizeof x);
    leoec::gfwheal::mac_in<W>(in[(size_t)i * 17], x, acc, red);
  }
  leoec::gfwheal::from_domain<W>(acc);
  return std::memcmp(acc[0], want, sizeof acc[0]) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s VECTORS\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<uint32_t> v;
  uint32_t word;
  while (std::fread(&word, sizeof word, 1, f) == 1) v.push_back(word);
  std::fclose(f);
  const uint32_t red = leoec::field(8).mul(0x80u, 2u);
  int failures = 0;
  unsigned done[3] = {0, 0, 0};
  size_t at = 1;
  bool ok = !v.empty() && v[0] <= 100000;
  for (uint32_t r = 0; ok && r < v[0]; ++r) {
    if (at + 2 > v.size()) {
      ok = false;
      break;
    }
    const uint32_t w = v[at], n = v[at + 1];
    at += 2;
    if ((w != 8 && w != 16 && w != 32) || n == 0 || n > 64 || at + (size_t)n * 17 + kRegs > v.size()) {
      ok = false;
      break;
    }
    const uint32_t* in = &v[at];
    const uint32_t* want = in + (size_t)n * 17;
    at += (size_t)n * 17 + kRegs;
    const bool good = w == 8 ? check<8>(in, n, want, red)
                             : w == 16 ? check<16>(in, n, want, 0u) : check<32>(in, n, want, 0u);
    ++done[w == 8 ? 0 : w == 16 ? 1 : 2];
    if (!good && ++failures <= 10)
      std::fprintf(stderr, "record %u: w %u, %u inputs, first c %#x: wrong sum\n", r, w, n, in[0]);
  }
  if (!ok || at != v.size()) {
    std::fprintf(stderr, "%s: short or malformed\n", argv[1]);
    return 2;
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("ok: %u records of w 8, %u of w 16, %u of w 32\n", done[0], done[1], done[2]);
  return 0;
}
