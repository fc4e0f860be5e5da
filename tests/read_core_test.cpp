// read_core_test.cpp — the arithmetic of leoec_read_dev that needs no device
// (leo_erasure_amd/csrc/read_core.hpp over update_core.hpp), as a stand-alone
// program:
//   * group_segments over every erased mask of a 4-block object and every run
//     of segments: lost blocks alone, intact runs maximal, nothing left out;
//   * valid_bytes / block_valid against the bytes, part() against the list;
//   * gf_read's lanes replayed on the host for vandrs(6,3,8), vandrs(4,2,16) and
//     vandrs(4,2,32), bit_read's for cauchyrs(4,2,5) and liberation(4,2,5):
//     random stripes (a ragged last block; an empty last block), consistent and
//     with random coding blocks, every lost data block under three erased sets
//     (alone; with the next data block; with coding block 0, so the survivors
//     use coding blocks from 1 up), every range lo < hi of a block of 16 w bytes
//     (and of 32 w for the packet classes) on the ragged stripe with random
//     coding blocks and a sample of them on the others, the survivors split
//     into launches of 2 and of 3 (the first stores, the later ones XOR into out), against a
//     brute-force decode with the host field of codes.cpp: one multiply per
//     word, one XOR per set bit.  A lane's accumulators depend on its position
//     and the launch's survivors only, never on the range: they are computed
//     once per (stripe, erased set, lost block, launch) with the kernel's own
//     steps (the valid-byte clip, gather16, gf_accumulate), and every range
//     replays the emission (lane masks, store or XOR, scatter16).
//     The object is a buffer of exactly `size` bytes, out one of exactly
//     lead + length, and every erased block holds other bytes than the stripe's:
//     a sanitizer build catches a byte read past the object or written outside
//     the range, a read of an erased block gives wrong bytes;
//   * transpose_rows against the bit-rows it was built from, and the survivor
//     packets bit_read skips: exactly those whose column misses the packets of
//     the lost block that hold a byte of the range (from the byte map).
// Built by tests/test_read_cpu.py, once more with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../leo_erasure_amd/csrc/codes.hpp"
#include "../leo_erasure_amd/csrc/read_core.hpp"

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

static uint32_t rng_state = 0x5EADu;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

// Every range of a block on the stripe with a ragged last block and random
// coding blocks; on the other three stripes every short range and head, and a
// sample of the long ones.
static uint64_t step(bool every, uint64_t at, uint64_t sparse) { return every || at < 20 ? 1 : sparse; }

// A whole lane in one access, as the kernels' rd_load / rd_store; any other
// lane byte by byte.
static void load_lane(const uint8_t* p, uint32_t bytes, uint32_t (&d)[4]) {
  if (bytes == 0xFFFFu) std::memcpy(d, p, 16);
  else upd::gather16(p, bytes, d);
}
static void store_lane(uint8_t* p, uint32_t bytes, const uint32_t (&d)[4]) {
  if (bytes == 0xFFFFu) std::memcpy(p, d, 16);
  else upd::scatter16(p, bytes, d);
}

static long test_groups() {
  constexpr int K = 4;
  long n = 0;
  for (uint32_t mask = 0; mask < (1u << K); ++mask) {
    char gone[K + 2] = {0};
    for (int b = 0; b < K; ++b) gone[b] = (char)((mask >> b) & 1u);
    for (int b0 = 0; b0 < K; ++b0)
      for (int b1 = b0; b1 < K; ++b1, ++n) {
        std::vector<upd::Seg> segs;
        for (int b = b0; b <= b1; ++b) segs.push_back(upd::Seg{(uint32_t)b, b == b0 ? 5u : 0u, b == b1 ? 9u : 64u});
        const int ns = (int)segs.size();
        std::vector<rd::Group> g((size_t)ns);
        const int ng = rd::group_segments(segs.data(), ns, gone, g.data(), ns);
        CHECK(ng >= 1, "groups: %d", ng);
        uint32_t next = 0;
        for (int i = 0; i < ng; ++i) {
          CHECK(g[(size_t)i].first == next && g[(size_t)i].count >= 1, "groups tile the segments");
          next = g[(size_t)i].first + g[(size_t)i].count;
          for (uint32_t s = g[(size_t)i].first; s < next && s < (uint32_t)ns; ++s)
            CHECK((gone[segs[s].block] != 0) == g[(size_t)i].lost, "a group is all lost or all intact");
          if (g[(size_t)i].lost) CHECK(g[(size_t)i].count == 1, "a lost block is its own group");
          if (i > 0) CHECK(g[(size_t)i].lost || g[(size_t)i - 1].lost, "intact runs are maximal");
        }
        CHECK(next == (uint32_t)ns, "every segment is in a group");
        if (ng > 1) CHECK(rd::group_segments(segs.data(), ns, gone, g.data(), ng - 1) == -1, "cap");
      }
  }
  return n;
}

static long test_clip_and_parts() {
  long n = 0;
  for (uint64_t valid = 0; valid <= 48; ++valid)
    for (uint64_t at = 0; at < 64; at += 16, ++n) {
      const uint32_t b = rd::valid_bytes(at, valid);
      for (int i = 0; i < 16; ++i) CHECK(((b >> i) & 1u) == (at + i < valid ? 1u : 0u), "valid_bytes");
    }
  for (uint64_t size = 0; size <= 200; ++size)
    for (uint32_t id = 0; id < 5; ++id, ++n) {
      uint64_t want = 64;
      if (id < 3) {
        want = 0;
        for (uint64_t p = id * 64; p < (id + 1) * 64; ++p) want += p < size;
      }
      CHECK(rd::block_valid(id, 3, 64, size) == want, "block_valid");
    }
  for (uint32_t total = 1; total <= 40; ++total)
    for (uint32_t per = 1; per <= 17; ++per, ++n) {
      uint32_t next = 0;
      const uint32_t parts = rd::part_count(total, per);
      for (uint32_t i = 0; i < parts; ++i) {
        const rd::Part p = rd::part(total, per, i);
        CHECK(p.first == next && p.count >= 1 && p.count <= per, "part");
        CHECK(i + 1 == parts || p.count == per, "only the last launch is short");
        next += p.count;
      }
      CHECK(next == total, "parts cover the survivors");
    }
  return n;
}

// A random stripe of k data blocks of bs bytes, `size` bytes of them the
// object, and m coding blocks; erased blocks overwritten in the working copy.
struct Stripe {
  int k, m;
  uint64_t bs, size;
  std::vector<uint8_t> obj;                  // exactly `size` bytes
  std::vector<std::vector<uint8_t>> coding;  // m x bs
  std::vector<uint8_t> padded() const {
    std::vector<uint8_t> p((size_t)k * bs, 0);
    std::memcpy(p.data(), obj.data(), size);
    return p;
  }
  // block `id` at byte x (a pointer only: nothing is read here)
  const uint8_t* at(uint32_t id, uint64_t x) const {
    return id < (uint32_t)k ? obj.data() + (uint64_t)id * bs + x : coding[id - k].data() + x;
  }
};

static std::vector<int> survivors(int k, int m, const std::vector<int>& erased) {
  std::vector<int> s;
  for (int id = 0; id < k + m && (int)s.size() < k; ++id) {
    bool gone = false;
    for (int e : erased) gone |= e == id;
    if (!gone) s.push_back(id);
  }
  return s;
}

static std::vector<std::vector<int>> erased_sets(int k, int j) {
  return {{j}, {j, (j + 1) % k}, {j, k}};
}

// The survivors' blocks as the decoder sees them (data zero past `size`), then
// the erased blocks of the working copy spoiled.
static void spoil(Stripe* s, const std::vector<int>& erased) {
  for (int e : erased)
    for (uint64_t x = 0; x < s->bs; ++x) {
      if (e < s->k) {
        if ((uint64_t)e * s->bs + x < s->size) s->obj[(size_t)e * s->bs + x] ^= (uint8_t)(1 + x % 255);
      } else {
        s->coding[(size_t)e - s->k][x] ^= (uint8_t)(1 + x % 255);
      }
    }
}

// Every range of the lost block's valid bytes: the emission of the lanes
// (parts x lanes x 4 dwords, block-local) against want (the block, bs bytes).
static long replay_ranges(const std::vector<std::vector<uint32_t>>& lane_acc, uint32_t parts, uint64_t bs,
                          uint64_t valid, const std::vector<uint8_t>& want, bool every, const char* what) {
  long n = 0;
  for (uint64_t lo = 0; lo < valid; lo += step(every, lo, 7))
    for (uint64_t hi = lo + 1; hi <= valid; hi += step(every, hi - lo, 11), ++n) {
      const uint64_t lead = lo % 16, length = hi - lo;
      std::vector<uint8_t> out(lead + length, 0xA5);  // exactly the row's bytes
      const int64_t shift = -(int64_t)(lo - lead);      // block byte x is out byte x + shift
      const uint64_t l0 = upd::first_lane(lo), nl = upd::lane_count(lo, hi);
      for (uint32_t p = 0; p < parts; ++p)
        for (uint64_t l = 0; l < nl; ++l) {
          const uint64_t x = (l0 + l) * 16;
          const uint32_t bytes = upd::lane_bytes(x, lo, hi);
          CHECK(bytes != 0, "an idle lane");
          uint32_t v[4];
          std::memcpy(v, &lane_acc[p][(size_t)(x / 16) * 4], sizeof v);
          uint8_t* const op = out.data() + ((int64_t)x + shift);  // (pointer arithmetic only)
          if (p != 0) {
            uint32_t old[4];
            load_lane(op, bytes, old);
            for (int d = 0; d < 4; ++d) v[d] ^= old[d];
          }
          store_lane(op, bytes, v);
        }
      bool head = true;
      for (uint64_t i = 0; i < lead; ++i) head &= out[i] == 0xA5;
      CHECK(head, "%s [%llu,%llu): the lead bytes were written", what, (unsigned long long)lo, (unsigned long long)hi);
      CHECK(std::memcmp(out.data() + lead, want.data() + lo, length) == 0, "%s [%llu,%llu)", what,
            (unsigned long long)lo, (unsigned long long)hi);
      (void)bs;
    }
  return n;
}

static uint32_t load_word(const uint8_t* p, int w) {
  uint32_t v = 0;
  for (int i = 0; i < w / 8; ++i) v |= (uint32_t)p[i] << (8 * i);
  return v;
}

template <int W>
static long test_gf(int k, int m) {
  const Field& f = field(W);
  GfMatrix C;
  if (vandermonde_coding_matrix(k, m, W, &C)) {
    CHECK(false, "no coding matrix");
    return 0;
  }
  const uint64_t bs = 16 * W;
  long n = 0;
  for (int shape = 0; shape < 2; ++shape)
    for (int random_coding = 0; random_coding < 2; ++random_coding) {
      Stripe s;
      s.k = k; s.m = m; s.bs = bs;
      s.size = shape == 0 ? (uint64_t)k * bs - 21 : (uint64_t)(k - 2) * bs + 5;
      s.obj.resize(s.size);
      for (auto& b : s.obj) b = (uint8_t)rnd();
      const std::vector<uint8_t> data = s.padded();
      s.coding.assign((size_t)m, std::vector<uint8_t>(bs, 0));
      for (int i = 0; i < m; ++i)
        for (uint64_t x = 0; x < bs; x += W / 8) {
          uint32_t v = 0;
          for (int j = 0; j < k; ++j) v ^= f.mul(C.at(i, j), load_word(&data[j * bs + x], W));
          if (random_coding) v = rnd();
          for (int b = 0; b < W / 8; ++b) s.coding[(size_t)i][x + b] = (uint8_t)(v >> (8 * b));
        }
      for (int j = 0; j < k; ++j) {
        const uint64_t valid = rd::block_valid((uint32_t)j, (uint32_t)k, bs, s.size);
        if (!valid) continue;
        for (const auto& erased : erased_sets(k, j)) {
          const std::vector<int> surv = survivors(k, m, erased);
          CHECK((int)surv.size() == k, "survivors");
          // row j of the inverse of the survivors' generator rows
          GfMatrix G, inv;
          G.rows = G.cols = k;
          G.a.assign((size_t)k * k, 0);
          for (int i = 0; i < k; ++i)
            for (int c = 0; c < k; ++c)
              G.at(i, c) = surv[(size_t)i] < k ? (uint32_t)(surv[(size_t)i] == c) : C.at(surv[(size_t)i] - k, c);
          if (gf_invert(G, W, &inv)) {
            CHECK(false, "singular");
            continue;
          }
          // brute force: one field multiply per word of the survivors as the decoder sees them
          std::vector<uint8_t> want(bs, 0);
          for (uint64_t x = 0; x < bs; x += W / 8) {
            uint32_t v = 0;
            for (int i = 0; i < k; ++i) {
              const uint8_t* src = surv[(size_t)i] < k ? &data[(size_t)surv[(size_t)i] * bs + x]
                                                       : &s.coding[(size_t)surv[(size_t)i] - k][x];
              v ^= f.mul(inv.at(j, i), load_word(src, W));
            }
            for (int b = 0; b < W / 8; ++b) want[x + b] = (uint8_t)(v >> (8 * b));
          }
          if (!random_coding) CHECK(std::memcmp(want.data(), &data[(size_t)j * bs], bs) == 0, "the decode row");
          Stripe work = s;
          spoil(&work, erased);
          for (uint32_t per = 2; per <= 3; ++per) {
            const uint32_t parts = rd::part_count((uint32_t)k, per);
            std::vector<std::vector<uint32_t>> lane_acc(parts, std::vector<uint32_t>(bs / 16 * 4, 0));
            for (uint32_t p = 0; p < parts; ++p) {
              const rd::Part pt = rd::part((uint32_t)k, per, p);
              for (uint64_t x = 0; x < bs; x += 16) {
                uint32_t acc[4] = {0, 0, 0, 0};
                for (uint32_t i = pt.first; i < pt.first + pt.count; ++i) {
                  const uint32_t id = (uint32_t)surv[i];
                  const uint32_t have = rd::valid_bytes(x, rd::block_valid(id, (uint32_t)k, bs, work.size));
                  if (!have) continue;
                  uint32_t v[4], t[W];
                  load_lane(work.at(id, x), have, v);
                  for (int b = 0; b < W; ++b) t[b] = upd::spread<W>(f.mul(inv.at(j, (int)i), 1u << b));
                  rd::gf_accumulate<W>(acc, v, t);
                }
                std::memcpy(&lane_acc[p][(size_t)(x / 16) * 4], acc, sizeof acc);
              }
            }
            n += replay_ranges(lane_acc, parts, bs, valid, want, shape == 0 && random_coding == 1, "gf_read");
          }
        }
      }
    }
  return n;
}

// The decode bit-rows of data block j over the survivors (engine.cpp bit_rows,
// one wanted id): rows[r * k w + i w + c].
static bool decode_bit_rows(const BitMatrix& B, int k, int w, const std::vector<int>& surv, int j,
                            std::vector<uint8_t>* rows) {
  const int n = k * w;
  BitMatrix G, inv;
  G.resize(n, n);
  for (int i = 0; i < k; ++i)
    for (int r = 0; r < w; ++r)
      for (int col = 0; col < n; ++col)
        if (surv[(size_t)i] < k ? col == surv[(size_t)i] * w + r : B.get((surv[(size_t)i] - k) * w + r, col))
          G.set(i * w + r, col, true);
  if (bit_invert(G, &inv)) return false;
  rows->assign((size_t)w * n, 0);
  for (int r = 0; r < w; ++r)
    for (int col = 0; col < n; ++col) (*rows)[(size_t)r * n + col] = inv.get(j * w + r, col);
  return true;
}

static long test_bit(const BitMatrix& B, int k, int m, int w, uint32_t ps, long* skipped_total) {
  const uint64_t bs = (uint64_t)w * ps;
  const uint32_t per_packet = ps / 16;
  const int n = k * w;
  long count = 0;
  for (int shape = 0; shape < 2; ++shape)
    for (int random_coding = 0; random_coding < 2; ++random_coding) {
      Stripe s;
      s.k = k; s.m = m; s.bs = bs;
      s.size = shape == 0 ? (uint64_t)k * bs - 21 : (uint64_t)(k - 2) * bs + 5;
      s.obj.resize(s.size);
      for (auto& b : s.obj) b = (uint8_t)rnd();
      const std::vector<uint8_t> data = s.padded();
      s.coding.assign((size_t)m, std::vector<uint8_t>(bs, 0));
      for (int q = 0; q < m * w; ++q)
        for (uint32_t y = 0; y < ps; ++y) {
          uint8_t v = 0;
          for (int col = 0; col < n; ++col)
            if (B.get(q, col)) v ^= data[(size_t)(col / w) * bs + (size_t)(col % w) * ps + y];
          s.coding[(size_t)(q / w)][(size_t)(q % w) * ps + y] = random_coding ? (uint8_t)rnd() : v;
        }
      for (int j = 0; j < k; ++j) {
        const uint64_t valid = rd::block_valid((uint32_t)j, (uint32_t)k, bs, s.size);
        if (!valid) continue;
        for (const auto& erased : erased_sets(k, j)) {
          const std::vector<int> surv = survivors(k, m, erased);
          std::vector<uint8_t> rows;
          if (!decode_bit_rows(B, k, w, surv, j, &rows)) {
            CHECK(false, "singular");
            continue;
          }
          std::vector<uint32_t> cols((size_t)n);
          rd::transpose_rows(rows.data(), (uint32_t)k, (uint32_t)w, cols.data());
          for (int r = 0; r < w; ++r)
            for (int q = 0; q < n; ++q)
              CHECK(((cols[(size_t)q] >> r) & 1u) == (rows[(size_t)r * n + q] ? 1u : 0u), "transpose");
          for (int q = 0; q < n; ++q) CHECK((cols[(size_t)q] >> w) == 0u, "transpose high bits");
          // brute force: one XOR per set bit, over the survivors as the decoder sees them
          std::vector<uint8_t> want(bs, 0);
          for (int r = 0; r < w; ++r)
            for (int q = 0; q < n; ++q) {
              if (!rows[(size_t)r * n + q]) continue;
              const int id = surv[(size_t)(q / w)];
              const uint8_t* src = id < k ? &data[(size_t)id * bs + (size_t)(q % w) * ps]
                                          : &s.coding[(size_t)id - k][(size_t)(q % w) * ps];
              for (uint32_t y = 0; y < ps; ++y) want[(size_t)r * ps + y] ^= src[y];
            }
          if (!random_coding) CHECK(std::memcmp(want.data(), &data[(size_t)j * bs], bs) == 0, "the decode rows");
          Stripe work = s;
          spoil(&work, erased);
          for (uint32_t per = 2; per <= 3; ++per) {
            const uint32_t parts = rd::part_count((uint32_t)k, per);
            const bool every = shape == 0 && random_coding == 1;
            for (uint64_t lo = 0; lo < valid; lo += step(every, lo, 7))
              for (uint64_t hi = lo + 1; hi <= valid; hi += step(every, hi - lo, 11), ++count) {
                const uint64_t lead = lo % 16, length = hi - lo;
                std::vector<uint8_t> out(lead + length, 0xA5);
                const int64_t shift = -(int64_t)(lo - lead);
                const upd::Positions pos = upd::packet_positions(lo, hi, ps);
                std::vector<char> loaded((size_t)n * per_packet, 0);
                for (uint32_t p = 0; p < parts; ++p) {
                  const rd::Part pt = rd::part((uint32_t)k, per, p);
                  for (uint32_t t = 0; t < pos.count; ++t) {
                    const uint32_t y = (pos.first + t) % per_packet * 16;
                    const uint32_t touched = upd::touched_packets(y, ps, (uint32_t)w, lo, hi);
                    uint32_t acc[32][4];
                    for (int r = 0; r < w; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0u;
                    for (uint32_t i = pt.first; i < pt.first + pt.count; ++i) {
                      const uint32_t id = (uint32_t)surv[i];
                      const uint64_t sv = rd::block_valid(id, (uint32_t)k, bs, work.size);
                      for (int c = 0; c < w; ++c) {
                        const uint32_t hit = rd::column_hits(cols[(size_t)i * w + c], touched);
                        if (!hit) continue;
                        loaded[((size_t)i * w + c) * per_packet + y / 16] = 1;
                        const uint64_t at = (uint64_t)c * ps + y;
                        const uint32_t have = rd::valid_bytes(at, sv);
                        if (!have) continue;
                        uint32_t v[4];
                        load_lane(work.at(id, at), have, v);
                        for (int r = 0; r < w; ++r)
                          if ((hit >> r) & 1u)
                            for (int d = 0; d < 4; ++d) acc[r][d] ^= v[d];
                      }
                    }
                    for (int r = 0; r < w; ++r) {
                      if (!((touched >> r) & 1u)) continue;
                      const uint64_t at = (uint64_t)r * ps + y;
                      const uint32_t bytes = upd::lane_bytes(at, lo, hi);
                      uint8_t* const op = out.data() + ((int64_t)at + shift);
                      if (p != 0) {
                        uint32_t old[4];
                        load_lane(op, bytes, old);
                        for (int d = 0; d < 4; ++d) acc[r][d] ^= old[d];
                      }
                      store_lane(op, bytes, acc[r]);
                    }
                  }
                }
                bool head = true;
                for (uint64_t i = 0; i < lead; ++i) head &= out[i] == 0xA5;
                CHECK(head, "bit_read [%llu,%llu): the lead bytes were written", (unsigned long long)lo,
                      (unsigned long long)hi);
                CHECK(std::memcmp(out.data() + lead, want.data() + lo, length) == 0, "bit_read w %d ps %u [%llu,%llu)",
                      w, ps, (unsigned long long)lo, (unsigned long long)hi);
                // loaded: exactly the survivor packets that feed a packet of block j holding a byte
                // of the range, at the lane positions where it does
                for (uint32_t yl = 0; yl < per_packet; ++yl) {
                  uint32_t holds = 0;  // packets of block j with a byte of the range at this lane
                  for (int r = 0; r < w; ++r)
                    for (uint32_t b = 0; b < 16; ++b) {
                      const uint64_t x = (uint64_t)r * ps + yl * 16 + b;
                      if (x >= lo && x < hi) holds |= 1u << r;
                    }
                  for (int q = 0; q < n; ++q) {
                    bool need = false;
                    for (int r = 0; r < w; ++r) need |= ((holds >> r) & 1u) && rows[(size_t)r * n + q];
                    CHECK((loaded[(size_t)q * per_packet + yl] != 0) == need, "survivor packet %d at lane %u: loaded %d needed %d",
                          q, yl, loaded[(size_t)q * per_packet + yl], (int)need);
                    *skipped_total += !need;
                  }
                }
              }
          }
        }
      }
    }
  return count;
}

int main() {
  const long groups = test_groups();
  const long clips = test_clip_and_parts();
  const long gf = test_gf<8>(6, 3) + test_gf<16>(4, 2) + test_gf<32>(4, 2);
  long skipped = 0;
  long bit = 0;
  {
    GfMatrix C;
    BitMatrix B;
    if (cauchy_good_coding_matrix(4, 2, 5, &C)) CHECK(false, "no cauchy matrix");
    expand_to_bitmatrix(C, 5, &B);
    bit += test_bit(B, 4, 2, 5, 16, &skipped) + test_bit(B, 4, 2, 5, 32, &skipped);
  }
  {
    BitMatrix B;
    if (liberation_coding_bitmatrix(4, 5, &B)) CHECK(false, "no liberation matrix");
    bit += test_bit(B, 4, 2, 5, 16, &skipped) + test_bit(B, 4, 2, 5, 32, &skipped);
  }
  CHECK(skipped > 0, "no survivor packet was ever skipped");
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok: %ld groupings, %ld clips and parts, %ld word ranges, %ld packet ranges, %ld survivor lanes skipped\n",
              groups, clips, gf, bit, skipped);
  return 0;
}
