// locate.hip — leoec_locate_dev: which one block of each object of a device
// batch is damaged?  One word per object, already a `lost` mask for
// leoec_heal_dev; and leoec_locate_rows, the ratios the answer rests on.
//
// Served: GF(2^8) matrix codes with k <= 16, 2 <= m <= 4 (vandrs w = 8,
// isars), the configurations of verify.hip's fused path with a second coding
// block to tell the data blocks apart.  Three steps on the stream, nothing
// allocated, uploaded or waited for:
//   memset          every word to all ones ("every block is a candidate");
//   gf8_locate      (locate_impl.hpp) reads the k + m blocks once; every dirty
//                   wave ANDs its candidate mask into its object's word;
//   locate_finish   all ones -> 0, exactly one bit -> kept, anything else ->
//                   LEOEC_LOCATE_MANY.
// leoec_locate_ws_dev adds the bitmatrix classes (cauchyrs, liberation), which
// have no fused check: the chunked encode pass (ws_pass.hpp, as verify.hip's
// two-pass path), and per chunk of objects that the caller's workspace holds,
//   encode plan     the pass's: the class's ordinary encode into the workspace;
//   memset          the chunk's words to all ones;
//   bit_locate      below: syndromes = workspace ^ stored coding blocks, the
//                   packet form of the test (locate_bitrows.hpp);
//   locate_finish.
// Everything leoec_locate_dev serves is forwarded to it.
// leoec_locate_gfw_dev adds the GF(2^w) word classes in the same way (vandrs
// w = 16 / 32; vandrs / isars w = 8 with k > 16 or m > 4): the same pass and
// the same four steps with gfw_locate (locate_gfw_impl.hpp) in bit_locate's
// place, the word form of the test (locate_wrows.hpp).  Everything
// leoec_locate_ws_dev serves is forwarded to it.
// The memset and the last step are one pair of helpers in all three calls
// (locate_reset, locate_tail).
// leoec_scrub_dev (scrub.hip) runs op_locate_dev with its own steps in it
// (scrub_steps.hpp): its kernel stands in locate_finish's place;
// leoec_scrub_ws_dev does the same with op_locate_ws_dev's bitmatrix branch,
// leoec_scrub_gfw_dev with op_locate_gfw_dev's word branch.
// This unit is kept out of engine.cpp / capi.cpp for verify.hip's reason: the
// host sanitizer harness links those against stand-in kernels.  The gf_init
// warm-up does not load this unit's kernels either.
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "engine.hpp"
#include "locate_bitrows.hpp"
#include "locate_gfw_impl.hpp"
#include "locate_impl.hpp"
#include "locate_rows.hpp"
#include "locate_wrows.hpp"
#include "scrub_steps.hpp"
#include "ws_pass.hpp"

namespace leoec {

using namespace detail;

namespace {

template <std::size_t... I>
LocateFn gf8_locate_pick(std::index_sequence<I...>, int k, int r) {
  static LocateFn (*const sel[])(int) = {&gf8_locate_launcher<(int)I + 1>...};
  return sel[k - 1](r);
}

bool locate_served(int coding, int k, int m, int w) {
  return gf8_fused_config(coding, k, m, w) && m >= 2;
}

// One word per lane, in place.
__global__ void __launch_bounds__(kThreads) locate_finish(uint32_t* __restrict__ lost, uint32_t n) {
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = lost[i];
  lost[i] = v == 0xFFFFFFFFu ? 0u : (v != 0u && (v & (v - 1u)) == 0u) ? v : LEOEC_LOCATE_MANY;
}

// The two ends of a chunk of `no` objects from object o0, in all three calls:
// before its locate kernel, every word to all ones;
int locate_reset(uint32_t* lost, uint64_t o0, uint64_t no, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(lost + o0, 0xFF, no * sizeof(uint32_t), s);
  return e == hipSuccess ? LEOEC_OK : LEOEC_E_HIP;
}

// after it, the caller's own step or locate_finish (no <= 2^31 - 1 words: one grid).
int locate_tail(LocateSteps* steps, uint32_t* lost, uint64_t o0, uint64_t no, hipStream_t s) {
  if (steps) return steps->finish(o0, no, s);
  return launch_kernel(locate_finish, dim3((uint32_t)((no + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, lost + o0, (uint32_t)no);
}

// The tail of leoec_locate_rows, _bitrows and _wrows: `need` words of room.
int copy_rows(const std::vector<uint32_t>& t, uint32_t* out, int cap, int need) {
  if (!out || cap < need) return LEOEC_E_ARG;
  for (size_t i = 0; i < t.size(); ++i) out[i] = t[i];
  return LEOEC_OK;
}

// The code and its ratio table; needs no device.
int locate_code(int coding, int k, int m, int w, const Code** c, std::vector<uint32_t>* ratio) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (!locate_served(coding, k, m, w)) return LEOEC_E_UNSUPPORTED;
  if ((rc = get_code(coding, k, m, w, c))) return rc;
  if ((*c)->C.a.size() != (size_t)m * k) return LEOEC_E_UNSUPPORTED;
  return locate_build_rows((*c)->C.a.data(), k, m, ratio);
}

int op_locate_rows(int coding, int k, int m, int w, uint32_t* ratio, int cap) {
  const Code* c;
  std::vector<uint32_t> t;
  const int rc = locate_code(coding, k, m, w, &c, &t);
  if (rc) return rc;
  return copy_rows(t, ratio, cap, (m - 1) * k);
}

}  // namespace

// steps (scrub_steps.hpp): leoec_scrub_dev's share of the call; none for
// leoec_locate_dev itself.
int op_locate_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                  uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                  uint32_t* lost, hipStream_t s, LocateSteps* steps) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  const Code* c;
  std::vector<uint32_t> ratio;
  if ((rc = locate_code(coding, k, m, w, &c, &ratio))) return rc;
  if (nobj == 0 || bs == 0) return LEOEC_OK;
  if (!lost || ((uintptr_t)lost & 3u)) return LEOEC_E_ARG;
  if (steps && (rc = steps->check(bs))) return rc;
  if ((rc = check_dev_batch(objs, obj_stride, size, parity, parity_stride, m, bs))) return rc;
  if ((rc = device_init())) return rc;
  if (steps && (rc = steps->begin(*c, s))) return rc;
  GfApply a;
  a.w = w;
  a.K = k;
  a.R = m;
  a.coef = c->C.a;  // the encoding rows: data blocks 0..k-1 in, coding blocks out
  EncodeShards sh = encode_shards(k, m, bs, size, objs, obj_stride, parity, parity_stride);
  a.in = std::move(sh.in);
  a.out = std::move(sh.par);
  a.block_size = bs;
  a.nobj = nobj;
  const LocateFn fn = gf8_locate_pick(std::make_index_sequence<kMaxK>{}, k, m);
  const uint64_t max_obj = gf8_max_objects(bs);
  for (uint64_t o0 = 0; o0 < nobj; o0 += max_obj) {
    const uint64_t no = nobj - o0 < max_obj ? nobj - o0 : max_obj;
    if ((rc = locate_reset(lost, o0, no, s))) return rc;
    if ((rc = fn(a, ratio.data(), o0, no, lost, s))) return rc;
    if ((rc = locate_tail(steps, lost, o0, no, s))) return rc;
  }
  return LEOEC_OK;
}

namespace {

// ---------------------------------------------------------------------------
// The bitmatrix classes: leoec_locate_ws_dev.

constexpr int kBitLocLanes = 64;                       // one wave per workgroup
constexpr uint32_t kBitLocTile = kBitLocLanes * 16u;   // bytes of every packet per workgroup
constexpr int kBitLocWords = 768;                      // (m - 1) k w at most: 3 KiB of argument

// ws: the chunk's freshly encoded coding blocks, object o at o * per
// (per = m bs, packed: row q = i w + r at q * ps is packet r of coding block
// i); parity: the stored ones, object o at o * parity_stride, the same rows.
struct BitLocArgs {
  const uint8_t* ws;
  const uint8_t* parity;
  uint64_t parity_stride;
  uint64_t per;
  uint32_t ps, tiles, k, m, w;
  uint32_t rows[kBitLocWords];  // locate_build_bitrows' words
};
static_assert(sizeof(BitLocArgs) + sizeof(uint32_t*) <= 3200, "kernel argument segment");

// One workgroup (one wave) per (object, 1 KiB of packet offsets), one 16-byte
// column per lane, w a runtime value.  Lanes past the packet read the tile's
// first column and count as zero syndromes, which fit every block.
// Clean path: the m w syndrome rows ORed per coding block, one ballot per
// block; a wave with no non-zero syndrome ends there and writes nothing.
// Dirty path: coding block i is a candidate when no syndrome but s_i is
// non-zero; data blocks only when every syndrome is (every B[i][j] is
// invertible: a column that fits a data block is non-zero in every syndrome
// or in none).  Then the w packets of s_0 go to LDS (each lane reads back only
// what it wrote: no barrier), every s_i[r] is loaded once and compared with
// the XOR of the s_0 packets its row word names, for every data block still
// in the running (row words by scalar loads from the argument).  lost[o]: the
// word of object o of this launch (all ones beforehand).
__global__ void __launch_bounds__(kBitLocLanes)
bit_locate(const BitLocArgs a, uint32_t* __restrict__ lost) {
  extern __shared__ u32x4 bit_locate_s0[];  // [w][kBitLocLanes]
  const uint32_t obj = blockIdx.x / a.tiles;
  const uint32_t tile = blockIdx.x - obj * a.tiles;
  const uint32_t t0 = tile * kBitLocTile;  // < ps
  const uint32_t off = t0 + threadIdx.x * 16u;
  const bool in = off < a.ps;  // ps is a multiple of 16: the column lies inside the packet
  const uint32_t o = in ? off : t0;
  const uint8_t* const x = a.ws + (uint64_t)obj * a.per + o;
  const uint8_t* const y = a.parity + (uint64_t)obj * a.parity_stride + o;
  const uint32_t rows = a.m * a.w;
  uint32_t dirty = 0;  // wave-uniform: bit i set when any lane's syndrome of block i is non-zero
  for (uint32_t i = 0, q = 0; i < a.m; ++i) {
    uint32_t nz = 0;
#pragma unroll 4
    for (uint32_t r = 0; r < a.w; ++r, ++q) {
      const u32x4 e = ld16<false>(x + (uint64_t)q * a.ps);
      const u32x4 p = ld16<true>(y + (uint64_t)q * a.ps);
      nz |= (e[0] ^ p[0]) | (e[1] ^ p[1]) | (e[2] ^ p[2]) | (e[3] ^ p[3]);
    }
    if (__builtin_amdgcn_ballot_w64(in && nz != 0u) != 0ull) dirty |= 1u << i;
  }
  if (dirty == 0u) return;
  // The cold branch.
  auto syndrome = [&](uint32_t q) {
    const u32x4 e = ld16<false>(x + (uint64_t)q * a.ps);
    const u32x4 p = ld16<true>(y + (uint64_t)q * a.ps);
    const uint32_t keep = in ? ~0u : 0u;
    return u32x4{(e[0] ^ p[0]) & keep, (e[1] ^ p[1]) & keep, (e[2] ^ p[2]) & keep,
                 (e[3] ^ p[3]) & keep};
  };
  uint32_t mask = 0;
  for (uint32_t i = 0; i < a.m; ++i)
    if ((dirty & ~(1u << i)) == 0u) mask |= 1u << (a.k + i);
  if (dirty == (1u << a.m) - 1u) {  // m <= 31
    u32x4* const s0 = bit_locate_s0 + threadIdx.x;
    for (uint32_t c = 0; c < a.w; ++c) s0[c * kBitLocLanes] = syndrome(c);
    const uint32_t all = (1u << a.k) - 1u;  // k <= 30
    uint32_t notfit = 0;                    // wave-uniform: data blocks some column does not fit
    for (uint32_t q = a.w; q < rows && notfit != all; ++q) {
      const uint32_t i = q / a.w, r = q - i * a.w;
      const u32x4 s = syndrome(q);
      for (uint32_t j = 0; j < a.k; ++j) {
        if ((notfit >> j) & 1u) continue;
        u32x4 p = s;
        for (uint32_t t = a.rows[((i - 1u) * a.k + j) * a.w + r]; t != 0u; t &= t - 1u) {
          const u32x4 v = s0[(uint32_t)__builtin_ctz(t) * kBitLocLanes];
          p[0] ^= v[0];
          p[1] ^= v[1];
          p[2] ^= v[2];
          p[3] ^= v[3];
        }
        if (__builtin_amdgcn_ballot_w64((p[0] | p[1] | p[2] | p[3]) != 0u) != 0ull) notfit |= 1u << j;
      }
    }
    mask |= ~notfit & all;
  }
  if (threadIdx.x == 0u) atomicAnd(&lost[obj], mask);
}

}  // namespace

// (scrub_steps.hpp: scrub.hip asks too)
bool bit_class(int coding) { return coding == LEOEC_CAUCHYRS || coding == LEOEC_LIBERATION; }

namespace {

bool bit_locate_served(int coding, int k, int m, int w) {
  return bit_class(coding) && m >= 2 && k + m <= 32 && (m - 1) * k * w <= kBitLocWords;
}

// The code and its row words; needs no device.
int bit_locate_code(int coding, int k, int m, int w, const Code** c, std::vector<uint32_t>* rows) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (!bit_locate_served(coding, k, m, w)) return LEOEC_E_UNSUPPORTED;
  if ((rc = get_code(coding, k, m, w, c))) return rc;
  if (!(*c)->bitmatrix) return LEOEC_E_UNSUPPORTED;
  return locate_build_bitrows((*c)->B, k, m, w, rows);
}

int op_locate_bitrows(int coding, int k, int m, int w, uint32_t* rows, int cap) {
  const Code* c;
  std::vector<uint32_t> t;
  const int rc = bit_locate_code(coding, k, m, w, &c, &t);
  if (rc) return rc;
  return copy_rows(t, rows, cap, (m - 1) * k * w);
}

int op_locate_ws_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                               uint64_t* bytes) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  const Code* c;
  std::vector<uint32_t> t;
  const bool bit = bit_class(coding);
  if ((rc = bit ? bit_locate_code(coding, k, m, w, &c, &t) : locate_code(coding, k, m, w, &c, &t)))
    return rc;
  if (!bytes) return LEOEC_E_ARG;
  uint64_t all;
  if (!encode_region_bytes(m, bs, nobj, &all)) return LEOEC_E_BAD_SIZE;
  *bytes = bit ? all : 0;
  return LEOEC_OK;
}

}  // namespace

// steps (scrub_steps.hpp): leoec_scrub_ws_dev's share of the bitmatrix branch,
// with `workspace` its encode region alone (the chunk size comes from
// workspace_bytes); none for leoec_locate_ws_dev itself.
int op_locate_ws_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                     uint32_t* lost, void* workspace, uint64_t workspace_bytes, hipStream_t s,
                     LocateSteps* steps) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  if (!bit_class(coding))  // served or LEOEC_E_UNSUPPORTED there; no workspace
    return op_locate_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride, lost,
                         s, nullptr);
  const Code* c;
  std::vector<uint32_t> rows;
  if ((rc = bit_locate_code(coding, k, m, w, &c, &rows))) return rc;
  if (nobj == 0 || bs == 0) return LEOEC_OK;
  if (!lost || ((uintptr_t)lost & 3u)) return LEOEC_E_ARG;
  if (steps && (rc = steps->check(bs))) return rc;
  if ((rc = check_dev_batch(objs, obj_stride, size, parity, parity_stride, m, bs))) return rc;
  if ((rc = WsPass::check(workspace, workspace_bytes, m, bs))) return rc;
  if ((rc = device_init())) return rc;
  if (steps && (rc = steps->begin(*c, s))) return rc;
  WsPass pass;
  if ((rc = pass.prepare(*c, bs, size, objs, obj_stride, parity, parity_stride))) return rc;
  BitLocArgs a;
  a.ws = static_cast<const uint8_t*>(workspace);
  a.parity_stride = parity_stride;
  a.per = (uint64_t)m * bs;
  a.ps = (uint32_t)(bs / (uint64_t)w);  // bs < 2^32 (check_dev_batch), a multiple of 16 w
  a.tiles = (a.ps + kBitLocTile - 1u) / kBitLocTile;
  a.k = (uint32_t)k;
  a.m = (uint32_t)m;
  a.w = (uint32_t)w;
  for (size_t i = 0; i < (size_t)kBitLocWords; ++i) a.rows[i] = i < rows.size() ? rows[i] : 0u;
  const size_t lds = (size_t)w * kBitLocLanes * sizeof(u32x4);  // <= 32 KiB
  const auto chunk = [&](uint64_t o0, uint64_t no) {
    int rc = locate_reset(lost, o0, no, s);
    if (rc) return rc;
    a.parity = parity + o0 * parity_stride;
    if ((rc = launch_kernel(bit_locate, dim3((uint32_t)(no * a.tiles)), dim3(kBitLocLanes), lds, s,
                            a, lost + o0)))
      return rc;
    return locate_tail(steps, lost, o0, no, s);
  };
  return pass.run(workspace, workspace_bytes, nobj, a.tiles, s, chunk);
}

namespace {

// ---------------------------------------------------------------------------
// The GF(2^w) word classes: leoec_locate_gfw_dev.

// What neither leoec_locate_dev nor leoec_locate_ws_dev serves of the matrix
// classes, with a second coding block and a bit for every block.
bool gfw_locate_served(int coding, int k, int m, int w) {
  return (coding == LEOEC_VANDRS || coding == LEOEC_ISARS) && (w == 8 || w == 16 || w == 32) &&
         !locate_served(coding, k, m, w) && m >= 2 && k + m <= 32;
}

// The ratio table of a code, built once and kept with the cached Code (get_code
// never frees one): at (16,16,32) the build is 240 divisions and 28,800
// products bit by bit, milliseconds, which a call's host time would show.
int gfw_ratio(const Code* c, const std::vector<uint32_t>** out) {
  struct Entry {
    int rc;
    std::vector<uint32_t> ratio;
  };
  static std::mutex mu;
  static std::map<const Code*, Entry> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(c);
  if (it == cache.end()) {
    Entry e;
    e.rc = locate_build_wrows(c->C.a.data(), c->k, c->m, c->w, &e.ratio);
    it = cache.emplace(c, std::move(e)).first;
  }
  *out = &it->second.ratio;
  return it->second.rc;
}

// The code and its ratio table; needs no device.
int gfw_locate_code(int coding, int k, int m, int w, const Code** c,
                    const std::vector<uint32_t>** ratio) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (!gfw_locate_served(coding, k, m, w)) return LEOEC_E_UNSUPPORTED;
  if ((rc = get_code(coding, k, m, w, c))) return rc;
  if ((*c)->bitmatrix || (*c)->C.a.size() != (size_t)m * k) return LEOEC_E_UNSUPPORTED;
  return gfw_ratio(*c, ratio);
}

}  // namespace

// Class (a) of leoec_locate_gfw_dev: what leoec_locate_ws_dev serves, and the
// bitmatrix configurations it refuses, which stay refused.
// (scrub_steps.hpp: scrub.hip asks too)
bool gfw_forwarded(int coding, int k, int m, int w) {
  return bit_class(coding) || locate_served(coding, k, m, w);
}

namespace {

int op_locate_wrows(int coding, int k, int m, int w, uint32_t* ratio, int cap) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (gfw_forwarded(coding, k, m, w)) return LEOEC_E_UNSUPPORTED;
  const Code* c;
  const std::vector<uint32_t>* t;
  if ((rc = gfw_locate_code(coding, k, m, w, &c, &t))) return rc;
  return copy_rows(*t, ratio, cap, (m - 1) * k);
}

int op_locate_gfw_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                uint64_t* bytes) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  if (gfw_forwarded(coding, k, m, w))
    return op_locate_ws_dev_workspace(coding, k, m, w, size, nobj, bytes);
  const Code* c;
  const std::vector<uint32_t>* t;
  if ((rc = gfw_locate_code(coding, k, m, w, &c, &t))) return rc;
  if (!bytes) return LEOEC_E_ARG;
  return encode_region_bytes(m, bs, nobj, bytes) ? LEOEC_OK : LEOEC_E_BAD_SIZE;
}

int launch_gfw_locate(int w, const GfwLocArgs& a, uint64_t no, uint32_t* lost, hipStream_t s) {
  const dim3 grid((uint32_t)(no * a.tiles)), block(kGfwLocLanes);
  if (w == 8) return launch_kernel(gfw_locate<8>, grid, block, 0, s, a, lost);
  if (w == 16) return launch_kernel(gfw_locate<16>, grid, block, 0, s, a, lost);
  return launch_kernel(gfw_locate<32>, grid, block, 0, s, a, lost);
}

}  // namespace

// steps (scrub_steps.hpp): leoec_scrub_gfw_dev's share of the word branch,
// with `workspace` its encode region alone (the chunk size comes from
// workspace_bytes); none for leoec_locate_gfw_dev itself.
int op_locate_gfw_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                      uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                      uint32_t* lost, void* workspace, uint64_t workspace_bytes, hipStream_t s,
                      LocateSteps* steps) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  if (gfw_forwarded(coding, k, m, w))
    return op_locate_ws_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride,
                            lost, workspace, workspace_bytes, s, nullptr);
  const Code* c;
  const std::vector<uint32_t>* ratio;
  if ((rc = gfw_locate_code(coding, k, m, w, &c, &ratio))) return rc;
  if (nobj == 0 || bs == 0) return LEOEC_OK;
  if (!lost || ((uintptr_t)lost & 3u)) return LEOEC_E_ARG;
  if (steps && (rc = steps->check(bs))) return rc;
  if ((rc = check_dev_batch(objs, obj_stride, size, parity, parity_stride, m, bs))) return rc;
  if ((rc = WsPass::check(workspace, workspace_bytes, m, bs))) return rc;
  if (ratio->size() > (size_t)kGfwLocWords) return LEOEC_E_UNSUPPORTED;  // (k + m <= 32: never)
  if ((rc = device_init())) return rc;
  if (steps && (rc = steps->begin(*c, s))) return rc;
  WsPass pass;
  if ((rc = pass.prepare(*c, bs, size, objs, obj_stride, parity, parity_stride))) return rc;
  GfwLocArgs a;
  a.ws = static_cast<const uint8_t*>(workspace);
  a.parity_stride = parity_stride;
  a.per = (uint64_t)m * bs;
  a.bs = (uint32_t)bs;  // bs < 2^32 (check_dev_batch), a multiple of 16 w
  a.tiles = (uint32_t)((bs + kGfwLocTile - 1) / kGfwLocTile);  // one 4 KiB tile of every block
  a.k = (uint32_t)k;
  a.m = (uint32_t)m;
  a.red = field(8).mul(0x80u, 2u);  // alpha^8 reduced: the polynomial's low byte
  a.pad = 0;
  for (size_t i = 0; i < (size_t)kGfwLocWords; ++i) a.ratio[i] = i < ratio->size() ? (*ratio)[i] : 0u;
  const auto chunk = [&](uint64_t o0, uint64_t no) {
    int rc = locate_reset(lost, o0, no, s);
    if (rc) return rc;
    a.parity = parity + o0 * parity_stride;
    if ((rc = launch_gfw_locate(w, a, no, lost + o0, s))) return rc;
    return locate_tail(steps, lost, o0, no, s);
  };
  return pass.run(workspace, workspace_bytes, nobj, a.tiles, s, chunk);
}

}  // namespace leoec

extern "C" {

int leoec_locate_gfw_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                   uint64_t* bytes) {
  return leoec::guarded(
      [&] { return leoec::op_locate_gfw_dev_workspace(coding, k, m, w, size, nobj, bytes); });
}

int leoec_locate_gfw_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                         uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                         uint32_t* lost, void* workspace, uint64_t workspace_bytes, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_locate_gfw_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                    parity_stride, lost, workspace, workspace_bytes,
                                    (hipStream_t)stream, nullptr);
  });
}

int leoec_locate_wrows(int coding, int k, int m, int w, uint32_t* ratio, int cap) {
  return leoec::guarded([&] { return leoec::op_locate_wrows(coding, k, m, w, ratio, cap); });
}

int leoec_locate_ws_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                  uint64_t* bytes) {
  return leoec::guarded(
      [&] { return leoec::op_locate_ws_dev_workspace(coding, k, m, w, size, nobj, bytes); });
}

int leoec_locate_ws_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                        uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                        uint32_t* lost, void* workspace, uint64_t workspace_bytes, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_locate_ws_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                   parity_stride, lost, workspace, workspace_bytes,
                                   (hipStream_t)stream, nullptr);
  });
}

int leoec_locate_bitrows(int coding, int k, int m, int w, uint32_t* rows, int cap) {
  return leoec::guarded([&] { return leoec::op_locate_bitrows(coding, k, m, w, rows, cap); });
}

int leoec_locate_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                     uint32_t* lost, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_locate_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                parity_stride, lost, (hipStream_t)stream, nullptr);
  });
}

int leoec_locate_rows(int coding, int k, int m, int w, uint32_t* ratio, int cap) {
  return leoec::guarded([&] { return leoec::op_locate_rows(coding, k, m, w, ratio, cap); });
}

}  // extern "C"
