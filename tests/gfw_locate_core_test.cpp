// TEST PROGRAM (CPU) for the portable core of leo_erasure_amd/csrc/
// locate_gfw_impl.hpp: gfwloc::misfit<W>, the per-lane test "does c * s_0
// equal s_i" that gfw_locate runs on the GPU, against field arithmetic taken
// from the oracle.  Stand-alone (its own main), so it can also be built with
// -fsanitize=address,undefined and run directly.  Not part of the product.
//
//   gfw_locate_core_test VECTORS
//
// VECTORS (written by tests/test_locate_gfw_cpu.py from oracle.gf_mul), little
// endian: u32 n16, u32 n32; 65,536 bytes, byte c * 256 + x = c * x in GF(2^8);
// n16 records, then n32 records, of 33 u32 each: the coefficient c, a lane's
// 16 registers of words x (w = 16: two words per register), the 16 registers
// of c * x.
// Built with codes.cpp: the reduction byte of w = 8 comes from field(8), as in
// locate.hip.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../leo_erasure_amd/csrc/codes.hpp"
#include "../leo_erasure_amd/csrc/locate_gfw_impl.hpp"

namespace {

using leoec::gfwloc::kRegs;

int failures = 0;

void fail(const char* what, int w, uint32_t c, int at) {
  if (++failures <= 10) std::fprintf(stderr, "w %d c %#x: %s (at %d)\n", w, c, what, at);
}

// s0 = x, si = prod must fit; prod with one bit flipped must not.
template <int W>
void check(uint32_t c, const uint32_t* x, const uint32_t* prod, uint32_t red, int at) {
  uint32_t s0[kRegs], si[kRegs];
  std::memcpy(s0, x, sizeof s0);
  std::memcpy(si, prod, sizeof si);
  leoec::gfwloc::to_domain<W>(s0);
  leoec::gfwloc::to_domain<W>(si);
  uint32_t before[kRegs];
  std::memcpy(before, s0, sizeof s0);
  if (leoec::gfwloc::misfit<W>(c, s0, si, red) != 0u) fail("the product does not fit", W, c, at);
  if (std::memcmp(before, s0, sizeof s0) != 0) fail("s0 was changed", W, c, at);
  const int bit = (at * 37 + (int)(c % 97u)) % (kRegs * 32);
  std::memcpy(si, prod, sizeof si);
  si[bit / 32] ^= 1u << (bit % 32);
  leoec::gfwloc::to_domain<W>(si);
  if (leoec::gfwloc::misfit<W>(c, s0, si, red) == 0u) fail("a wrong product fits", W, c, at);
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
  uint32_t n[2];
  std::vector<uint8_t> mul8(65536);
  bool ok = std::fread(n, sizeof n, 1, f) == 1 && std::fread(mul8.data(), 1, 65536, f) == 65536 &&
            n[0] <= 100000 && n[1] <= 100000;
  std::vector<uint32_t> rec((size_t)(ok ? n[0] + n[1] : 0) * 33);
  ok = ok && (rec.empty() || std::fread(rec.data(), sizeof(uint32_t), rec.size(), f) == rec.size());
  std::fclose(f);
  if (!ok) {
    std::fprintf(stderr, "%s: short or malformed\n", argv[1]);
    return 2;
  }
  // w = 8: every product; a lane's 64 bytes hold x = 64 q .. 64 q + 63
  const uint32_t red = leoec::field(8).mul(0x80u, 2u);
  for (uint32_t c = 0; c < 256; ++c)
    for (int q = 0; q < 4; ++q) {
      uint8_t xb[64], pb[64];
      for (int i = 0; i < 64; ++i) {
        xb[i] = (uint8_t)(64 * q + i);
        pb[i] = mul8[c * 256 + xb[i]];
      }
      uint32_t x[kRegs], p[kRegs];
      std::memcpy(x, xb, sizeof x);
      std::memcpy(p, pb, sizeof p);
      check<8>(c, x, p, red, q);
    }
  for (uint32_t r = 0; r < n[0]; ++r) {
    const uint32_t* v = &rec[(size_t)r * 33];
    check<16>(v[0], v + 1, v + 17, 0u, (int)r);
  }
  for (uint32_t r = 0; r < n[1]; ++r) {
    const uint32_t* v = &rec[(size_t)(n[0] + r) * 33];
    check<32>(v[0], v + 1, v + 17, 0u, (int)r);
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("ok: 65536 products of w 8, %u records of w 16, %u of w 32\n", n[0], n[1]);
  return 0;
}
