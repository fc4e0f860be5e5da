// update_core_test.cpp — the arithmetic of leoec_update_dev that needs no
// device (leo_erasure_amd/csrc/update_core.hpp), as a stand-alone program:
//   * split_range against a brute-force byte map: every offset and length of a
//     3-block object with w = 4, ps = 16 (bs = 64), and of one with bs = 96;
//   * lane_bytes against the bytes themselves;
//   * packet_positions and touched_packets against the byte map: every
//     position with a touched lane is listed once, and no other;
//   * mul_dword<8|16|32> against the library's field (codes.cpp);
//   * the lanes of gf_update and bit_update replayed on the host, over buffers
//     that hold exactly the bytes the contract allows to be read (so a
//     sanitizer build catches a byte read or written outside the range): the
//     patched object, and parity = parity before ^ encoding of the delta, from
//     consistent and from random parity, with the rows of a launch chunked (the
//     new bytes stored by the last chunk only).
// Built by tests/test_update_cpu.py, once more with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../leo_erasure_amd/csrc/codes.hpp"
#include "../leo_erasure_amd/csrc/update_core.hpp"

using namespace leoec;

static int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (++failures <= 20) {                 \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
    }                                         \
  } while (0)

static uint32_t rng_state = 0x1E0Eu;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

static long test_split(uint64_t bs, int k) {
  long n = 0;
  const uint64_t size = bs * k;
  for (uint64_t off = 0; off < size; ++off)
    for (uint64_t len = 1; off + len <= size; ++len, ++n) {
      std::vector<upd::Seg> segs((size_t)k);
      const int ns = upd::split_range(bs, off, len, segs.data(), k);
      CHECK(ns >= 1, "split %llu+%llu: %d", (unsigned long long)off, (unsigned long long)len, ns);
      std::vector<int> hit(size, 0);
      for (int i = 0; i < ns; ++i) {
        const upd::Seg& g = segs[(size_t)i];
        CHECK(g.lo < g.hi && g.hi <= bs && g.block < (uint32_t)k, "segment shape");
        CHECK(i == 0 || g.block == segs[(size_t)i - 1].block + 1, "segments ascend");
        for (uint64_t x = g.lo; x < g.hi; ++x) ++hit[g.block * bs + x];
      }
      for (uint64_t p = 0; p < size; ++p)
        CHECK(hit[p] == (p >= off && p < off + len ? 1 : 0), "split %llu+%llu byte %llu",
              (unsigned long long)off, (unsigned long long)len, (unsigned long long)p);
      // one segment too few: refused
      if (ns > 1) CHECK(upd::split_range(bs, off, len, segs.data(), ns - 1) == -1, "cap");
    }
  return n;
}

static long test_lane_bytes() {
  long n = 0;
  for (uint64_t lo = 0; lo < 48; ++lo)
    for (uint64_t hi = lo + 1; hi <= 48; ++hi)
      for (uint64_t at = 0; at < 48; at += 16, ++n) {
        const uint32_t b = upd::lane_bytes(at, lo, hi);
        for (int i = 0; i < 16; ++i)
          CHECK(((b >> i) & 1u) == (at + i >= lo && at + i < hi ? 1u : 0u), "lane_bytes");
        CHECK((b >> 16) == 0u, "lane_bytes high bits");
      }
  return n;
}

static long test_packets(uint32_t w, uint32_t ps) {
  long n = 0;
  const uint64_t bs = (uint64_t)w * ps;
  const uint32_t per = ps / 16;
  for (uint64_t lo = 0; lo < bs; ++lo)
    for (uint64_t hi = lo + 1; hi <= bs; ++hi, ++n) {
      const upd::Positions pos = upd::packet_positions(lo, hi, ps);
      std::vector<int> listed(per, 0);
      for (uint32_t t = 0; t < pos.count; ++t) ++listed[(pos.first + t) % per];
      CHECK(pos.first < per && pos.count <= per, "positions shape");
      for (uint32_t y = 0; y < per; ++y) {
        uint32_t want = 0;
        for (uint32_t c = 0; c < w; ++c)
          for (uint32_t i = 0; i < 16; ++i) {
            const uint64_t x = (uint64_t)c * ps + y * 16 + i;
            if (x >= lo && x < hi) want |= 1u << c;
          }
        CHECK(upd::touched_packets(y * 16, ps, w, lo, hi) == want, "touched_packets");
        CHECK(listed[y] == (want ? 1 : 0), "positions [%llu,%llu) y %u: listed %d touched %x",
              (unsigned long long)lo, (unsigned long long)hi, y, listed[y], want);
      }
    }
  return n;
}

template <int W>
static long test_mul() {
  const Field& f = field(W);
  long n = 0;
  for (int it = 0; it < 400; ++it, ++n) {
    const uint32_t c = it < 3 ? (uint32_t)it : rnd() & upd::ones<W>();
    uint32_t t[W];
    for (int b = 0; b < W; ++b) t[b] = upd::spread<W>(f.mul(c, 1u << b));
    for (int j = 0; j < 16; ++j) {
      const uint32_t x = j == 0 ? 0xFFFFFFFFu : rnd();
      const uint32_t got = upd::mul_dword<W>(x, t);
      for (int s = 0; s < 32; s += W) {
        const uint32_t xw = W == 32 ? x : (x >> s) & upd::ones<W>();
        const uint32_t gw = W == 32 ? got : (got >> s) & upd::ones<W>();
        CHECK(gw == f.mul(c, xw), "mul_dword<%d> c %x x %x", W, c, xw);
      }
    }
  }
  return n;
}

// An exact-size copy of [lo, hi) of a row, addressed with the row's offsets
// (a sanitizer build sees any access outside).
struct Window {
  std::vector<uint8_t> bytes;
  uint64_t lo;
  Window(const std::vector<uint8_t>& row, uint64_t lo_, uint64_t hi) : bytes(row.begin() + lo_, row.begin() + hi), lo(lo_) {}
  uint8_t* at(uint64_t x) { return bytes.data() + (x - lo); }  // (pointer arithmetic only)
};

static uint32_t load_word(const uint8_t* p, int w) {
  uint32_t v = 0;
  for (int i = 0; i < w / 8; ++i) v |= (uint32_t)p[i] << (8 * i);
  return v;
}

// gf_update's lanes on the host: k = 3 data blocks, m coding blocks, bs = 64.
template <int W>
static long test_gf_lanes() {
  constexpr int K = 3, M = 5, R = 2;  // rows in chunks of 2: 2, 2, 1
  constexpr uint64_t BS = 64, SIZE = K * BS - 5;
  const Field& f = field(W);
  uint32_t C[M][K];
  for (auto& row : C)
    for (auto& c : row) c = rnd() & upd::ones<W>();
  auto encode = [&](const std::vector<uint8_t>& obj, std::vector<uint8_t>& par) {
    std::vector<uint8_t> padded(K * BS, 0);
    std::memcpy(padded.data(), obj.data(), SIZE);
    par.assign(M * BS, 0);
    for (int i = 0; i < M; ++i)
      for (uint64_t x = 0; x < BS; x += W / 8) {
        uint32_t v = 0;
        for (int j = 0; j < K; ++j) v ^= f.mul(C[i][j], load_word(&padded[j * BS + x], W));
        for (int b = 0; b < W / 8; ++b) par[i * BS + x + b] = (uint8_t)(v >> (8 * b));
      }
  };
  long n = 0;
  for (uint64_t off = 0; off < SIZE; off += (off < 40 ? 1 : 7))
    for (uint64_t len = 1; off + len <= SIZE; len += (len < 36 ? 1 : 13))
      for (int random_parity = 0; random_parity < 2; ++random_parity, ++n) {
        std::vector<uint8_t> obj(SIZE), nw(SIZE), par, par_new, par_d;
        for (auto& b : obj) b = (uint8_t)rnd();
        nw = obj;
        for (uint64_t p = off; p < off + len; ++p) nw[p] = (uint8_t)(obj[p] ^ (1 + p % 255));
        encode(obj, par);
        encode(nw, par_new);
        if (random_parity) {
          std::vector<uint8_t> d(SIZE, 0);
          for (uint64_t p = off; p < off + len; ++p) d[p] = (uint8_t)(obj[p] ^ nw[p]);
          encode(d, par_d);
          for (auto& b : par) b = (uint8_t)rnd();
          for (size_t i = 0; i < par.size(); ++i) par_new[i] = (uint8_t)(par[i] ^ par_d[i]);
        }
        Window objw(obj, off, off + len);
        Window patw(nw, off, off + len);  // patch byte lead + (p - off) is nw[p]
        std::vector<upd::Seg> segs(K);
        const int ns = upd::split_range(BS, off, len, segs.data(), K);
        for (int s = 0; s < ns; ++s) {
          const upd::Seg& g = segs[(size_t)s];
          for (int row0 = 0; row0 < M; row0 += R) {
            const int rows = M - row0 < R ? M - row0 : R;
            const bool store = row0 + rows == M;
            const uint64_t l0 = upd::first_lane(g.lo), nl = upd::lane_count(g.lo, g.hi);
            for (uint64_t l = 0; l < nl; ++l) {
              const uint64_t x = (l0 + l) * 16;
              const uint32_t bytes = upd::lane_bytes(x, g.lo, g.hi);
              CHECK(bytes != 0, "an idle lane");
              uint32_t o[4], v[4];
              upd::gather16(objw.at(g.block * BS + x), bytes, o);
              upd::gather16(patw.at(g.block * BS + x), bytes, v);
              if (store) upd::scatter16(objw.at(g.block * BS + x), bytes, v);
              for (int r = 0; r < rows; ++r) {
                uint32_t t[W];
                for (int b = 0; b < W; ++b) t[b] = upd::spread<W>(f.mul(C[row0 + r][g.block], 1u << b));
                uint8_t* p = &par[(row0 + r) * BS + x];
                for (int d = 0; d < 4; ++d) {
                  const uint32_t q = upd::mul_dword<W>(o[d] ^ v[d], t);
                  for (int b = 0; b < 4; ++b) p[4 * d + b] ^= (uint8_t)(q >> (8 * b));
                }
              }
            }
          }
        }
        CHECK(par == par_new, "gf lanes w %d [%llu,+%llu) random %d", W, (unsigned long long)off,
              (unsigned long long)len, random_parity);
        CHECK(std::memcmp(objw.bytes.data(), &nw[off], len) == 0, "gf lanes: objs");
      }
  return n;
}

// bit_update's lanes on the host: k = 3, m = 2, w = 4, ps = 16 (bs = 64) and
// w = 3, ps = 32 (bs = 96), a random bitmatrix, bit-rows in chunks of 3.
static long test_bit_lanes(uint32_t w, uint32_t ps) {
  constexpr int K = 3, M = 2, RCH = 3;
  const uint64_t BS = (uint64_t)w * ps, SIZE = K * BS - 21;
  std::vector<uint32_t> B((size_t)M * w * K);  // [coding packet][data block]: bit c
  for (auto& x : B) x = rnd() & ((1u << w) - 1u) & (rnd() | rnd());
  B[0] = 0;  // a row that reaches nothing of block 0
  auto encode = [&](const std::vector<uint8_t>& obj, std::vector<uint8_t>& par) {
    std::vector<uint8_t> padded(K * BS, 0);
    std::memcpy(padded.data(), obj.data(), SIZE);
    par.assign(M * BS, 0);
    for (uint32_t q = 0; q < M * w; ++q)
      for (int j = 0; j < K; ++j)
        for (uint32_t c = 0; c < w; ++c)
          if ((B[(size_t)q * K + j] >> c) & 1u)
            for (uint32_t y = 0; y < ps; ++y) par[q * ps + y] ^= padded[j * BS + c * ps + y];
  };
  long n = 0;
  for (uint64_t off = 0; off < SIZE; off += (off < 40 ? 1 : 5))
    for (uint64_t len = 1; off + len <= SIZE; len += (len < 40 ? 1 : 11), ++n) {
      std::vector<uint8_t> obj(SIZE), nw, par, par_d, want;
      for (auto& b : obj) b = (uint8_t)rnd();
      nw = obj;
      std::vector<uint8_t> d(SIZE, 0);
      for (uint64_t p = off; p < off + len; ++p) {
        nw[p] = (uint8_t)(obj[p] ^ (1 + p % 255));
        d[p] = (uint8_t)(obj[p] ^ nw[p]);
      }
      encode(d, par_d);
      par.resize(M * BS);
      for (auto& b : par) b = (uint8_t)rnd();
      want = par;
      for (size_t i = 0; i < par.size(); ++i) want[i] ^= par_d[i];
      std::vector<uint8_t> touched_lane(M * BS / 16, 0);  // parity lanes read or written
      Window objw(obj, off, off + len), patw(nw, off, off + len);
      std::vector<upd::Seg> segs(K);
      const int ns = upd::split_range(BS, off, len, segs.data(), K);
      for (int s = 0; s < ns; ++s) {
        const upd::Seg& g = segs[(size_t)s];
        const upd::Positions pos = upd::packet_positions(g.lo, g.hi, ps);
        const int total = M * (int)w;
        for (int row0 = 0; row0 < total; row0 += RCH) {
          const int rows = total - row0 < RCH ? total - row0 : RCH;
          const bool store = row0 + rows == total;
          for (uint32_t t = 0; t < pos.count; ++t) {
            const uint32_t y = (pos.first + t) % (ps / 16) * 16;
            uint32_t delta[32][4], touched = 0;
            for (uint32_t c = 0; c < w; ++c) {
              const uint64_t at = (uint64_t)c * ps + y;
              const uint32_t bytes = upd::lane_bytes(at, g.lo, g.hi);
              if (!bytes) continue;
              touched |= 1u << c;
              uint32_t o[4], v[4];
              upd::gather16(objw.at(g.block * BS + at), bytes, o);
              upd::gather16(patw.at(g.block * BS + at), bytes, v);
              for (int i = 0; i < 4; ++i) delta[c][i] = o[i] ^ v[i];
            }
            CHECK(touched == upd::touched_packets(y, ps, w, g.lo, g.hi) && touched, "touched");
            for (int q = 0; q < rows; ++q) {
              const uint32_t row = B[(size_t)(row0 + q) * K + g.block];
              if (!upd::row_meets(row, touched)) continue;
              touched_lane[((uint64_t)(row0 + q) * ps + y) / 16] = 1;
              for (uint32_t c = 0; c < w; ++c)
                if ((row & touched) >> c & 1u)
                  for (int i = 0; i < 16; ++i)
                    par[(uint64_t)(row0 + q) * ps + y + i] ^= (uint8_t)(delta[c][i / 4] >> (8 * (i % 4)));
            }
            if (!store) continue;
            for (uint32_t c = 0; c < w; ++c) {
              if (!((touched >> c) & 1u)) continue;
              const uint64_t at = (uint64_t)c * ps + y;
              const uint32_t bytes = upd::lane_bytes(at, g.lo, g.hi);
              uint32_t v[4];
              upd::gather16(patw.at(g.block * BS + at), bytes, v);
              upd::scatter16(objw.at(g.block * BS + at), bytes, v);
            }
          }
        }
      }
      CHECK(par == want, "bit lanes w %u [%llu,+%llu)", w, (unsigned long long)off, (unsigned long long)len);
      CHECK(std::memcmp(objw.bytes.data(), &nw[off], len) == 0, "bit lanes: objs");
      // a parity lane is touched only where the delta's encoding can be non-zero
      for (size_t l = 0; l < touched_lane.size(); ++l) {
        bool reach = false;
        const uint64_t q = l * 16 / ps, y = l * 16 % ps;
        for (int j = 0; j < K; ++j)
          for (uint32_t c = 0; c < w; ++c)
            if ((B[q * K + j] >> c) & 1u)
              for (int i = 0; i < 16; ++i) {
                const uint64_t p = j * BS + c * ps + y + i;
                if (p >= off && p < off + len) reach = true;
              }
        CHECK((touched_lane[l] != 0) == reach, "bit lanes: parity lane %zu touched %d reach %d", l,
              touched_lane[l], (int)reach);
      }
    }
  return n;
}

int main() {
  const long splits = test_split(64, 3) + test_split(96, 3);
  const long lanes = test_lane_bytes();
  const long packets = test_packets(4, 16) + test_packets(3, 32);
  const long muls = test_mul<8>() + test_mul<16>() + test_mul<32>();
  const long gf = test_gf_lanes<8>() + test_gf_lanes<16>() + test_gf_lanes<32>();
  const long bit = test_bit_lanes(4, 16) + test_bit_lanes(3, 32);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok: %ld splits, %ld lanes, %ld packet ranges, %ld coefficients, %ld word updates, %ld packet updates\n",
              splits, lanes, packets, muls, gf, bit);
  return 0;
}
