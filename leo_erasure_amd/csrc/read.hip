// read.hip — leoec_read_dev: a byte range of every object of a degraded batch
// written to `out`, the bytes leoec_decode_dev would leave in objs, without
// rebuilding a block and without writing objs or parity.
//
// The range is split at data-block boundaries (upd::split_range) and grouped
// (rd::group_segments); per group, on the stream, nothing allocated, uploaded
// or waited for:
//   range_copy    a maximal run of intact data blocks: the range's bytes are
//                 contiguous in the object row, one lane per 16-byte lane.
//   gf_read<W>    one lost block, vandrs w = 8 / 16 / 32 and isars: one lane
//                 per 16-byte lane of the segment, out = XOR_i coef[i] *
//                 surv_i[x] with row j of the decode map (engine.cpp gf_rows)
//                 as the coefficients, whose products coef[i] * alpha^b travel
//                 as kernel arguments, 16 survivors a launch.
//   bit_read      one lost block, cauchyrs and liberation: one lane per object
//                 and lane position y of a packet; accumulators of the touched
//                 packets of the lost block in LDS (every lane its own slots: no
//                 barrier, no register array indexed by a runtime w); per
//                 survivor packet whose column of the decode bit-rows (engine.cpp
//                 bit_rows, transposed on the host) meets a touched packet one
//                 load of its lane at y.  A survivor travels as its id and its
//                 w column masks, 768 argument words a launch.
// When the survivors of a lost block take several launches, the first stores
// the range's bytes of out and the later ones XOR into them (`first`): the
// mirror of update's `store`.  Stream order makes every later launch see the
// earlier one's bytes; what out held before the call is never read by the
// first launch, so it never reaches the result.
// An erased block is never read: the survivors are intact ids by construction
// and a copy run holds intact blocks only.  A survivor lane that reaches past
// its block's valid bytes is gathered bytewise and zero-filled (rd::valid_bytes);
// head and tail lanes of a segment scatter only the range's bytes.
// The decode rows of a (code, survivors, lost block) are inverted on the host
// at the first call and kept in a bounded cache (read_rows).
// A chunk of objects exists only to keep a launch's grid below 2^31.
// This unit is kept out of engine.cpp / capi.cpp for verify.hip's reason: the
// host sanitizer harness links those against stand-in kernels.
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "engine.hpp"
#include "knobs.hpp"
#include "read_core.hpp"

namespace leoec {
namespace detail {

typedef uint32_t rd_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kCopyLanes = 256;     // 4 KiB of the run per workgroup
constexpr int kGfRdLanes = 256;     // 4 KiB of the segment per workgroup
constexpr int kGfRdSurv = 16;       // survivors per launch
constexpr int kBitRdLanes = 64;     // 1 KiB of every packet per workgroup
constexpr int kBitRdWords = 768;    // argument words per launch: a survivor takes 1 + w

// One group of one chunk of objects.
struct RdArgs {
  const uint8_t* objs;    // the chunk's first row
  const uint8_t* parity;  // the chunk's first row
  uint8_t* out;           // the chunk's first row
  uint64_t obj_stride, parity_stride, out_stride;
  uint64_t size;
  int64_t out_shift;  // byte x of the group's base (the lost block, or the object) is out byte x + out_shift (a multiple of 16)
  uint32_t lo, hi;    // the segment, block-local bytes (gf_read, bit_read)
  uint32_t bs, k;
  uint32_t tiles;     // workgroups per object
  uint32_t first;     // the first launch of the segment: store; a later one: XOR into out
};

struct CopyArgs {
  RdArgs u;
  uint64_t p0, p1;  // the run, object bytes
};

template <int W>
struct GfRdArgs {
  RdArgs u;
  uint32_t lane0, lanes;  // first 16-byte lane of the block, and how many
  uint32_t nsurv, pad;
  uint32_t id[kGfRdSurv];    // survivor block ids (< k: data, in objs; else coding, in parity)
  uint32_t t[kGfRdSurv][W];  // spread(coef[i] * alpha^b)
};

struct BitRdArgs {
  RdArgs u;
  uint32_t w, ps;
  uint32_t pos0, npos;  // upd::Positions
  uint32_t nsurv, pad;
  uint32_t words[kBitRdWords];  // per survivor: its id, then w column masks (bit r: feeds packet r of the lost block)
};
static_assert(sizeof(GfRdArgs<32>) <= 3200 && sizeof(BitRdArgs) <= 3200, "kernel argument segment");

// A whole lane in one access; any other lane byte by byte (upd::gather16 /
// scatter16: zero outside `bytes`, nothing else touched).
__device__ __forceinline__ rd_u32x4 rd_load(const uint8_t* p, uint32_t bytes) {
  if (bytes == 0xFFFFu) return *reinterpret_cast<const rd_u32x4*>(p);
  uint32_t d[4];
  upd::gather16(p, bytes, d);
  return rd_u32x4{d[0], d[1], d[2], d[3]};
}

__device__ __forceinline__ void rd_store(uint8_t* p, uint32_t bytes, rd_u32x4 v) {
  if (bytes == 0xFFFFu) {
    *reinterpret_cast<rd_u32x4*>(p) = v;
    return;
  }
  const uint32_t d[4] = {v[0], v[1], v[2], v[3]};
  upd::scatter16(p, bytes, d);
}

// The range's bytes of a lane stored (the first launch) or XORed into out.
__device__ __forceinline__ void rd_emit(uint8_t* p, uint32_t bytes, rd_u32x4 v, uint32_t first) {
  if (!first) v ^= rd_load(p, bytes);
  rd_store(p, bytes, v);
}

// Block `id` of object row (ob, pb): where it starts and its valid bytes.
__device__ __forceinline__ const uint8_t* rd_block(const RdArgs& u, const uint8_t* ob, const uint8_t* pb,
                                                   uint32_t id, uint32_t* valid) {
  *valid = (uint32_t)rd::block_valid(id, u.k, u.bs, u.size);
  return id < u.k ? ob + (uint64_t)id * u.bs : pb + (uint64_t)(id - u.k) * u.bs;
}

// grid: objects x tiles; a workgroup is 256 consecutive lanes of one object's
// run.  Every lane holds a byte of the run.
__global__ void __launch_bounds__(kCopyLanes) range_copy(const CopyArgs a) {
  const uint32_t o = blockIdx.x / a.u.tiles;
  const uint64_t l = (uint64_t)(blockIdx.x - o * a.u.tiles) * (uint32_t)kCopyLanes + threadIdx.x;
  const uint64_t at = (a.p0 / 16u + l) * 16u;
  if (at >= a.p1) return;
  const uint32_t bytes = upd::lane_bytes(at, a.p0, a.p1);
  const uint8_t* const src = a.u.objs + (uint64_t)o * a.u.obj_stride + at;
  uint8_t* const dst = a.u.out + (uint64_t)o * a.u.out_stride + ((int64_t)at + a.u.out_shift);
  rd_store(dst, bytes, rd_load(src, bytes));
}

// grid: objects x tiles; a workgroup is 256 consecutive lanes of one object's
// segment.  Every lane of the segment holds a byte of the range.
template <int W>
__global__ void __launch_bounds__(kGfRdLanes) gf_read(const GfRdArgs<W> a) {
  const uint32_t o = blockIdx.x / a.u.tiles;
  const uint32_t l = (blockIdx.x - o * a.u.tiles) * (uint32_t)kGfRdLanes + threadIdx.x;
  if (l >= a.lanes) return;
  const uint32_t x = (a.lane0 + l) * 16u;  // < bs
  const uint8_t* const ob = a.u.objs + (uint64_t)o * a.u.obj_stride;
  const uint8_t* const pb = a.u.parity + (uint64_t)o * a.u.parity_stride;
  uint32_t acc[4] = {0u, 0u, 0u, 0u};
  for (uint32_t i = 0; i < a.nsurv; ++i) {  // uniform: id and t come from the argument segment
    uint32_t valid;
    const uint8_t* const sp = rd_block(a.u, ob, pb, a.id[i], &valid);
    const uint32_t have = rd::valid_bytes(x, valid);
    if (!have) continue;  // wholly past the survivor's bytes: zero
    const rd_u32x4 v4 = rd_load(sp + x, have);
    const uint32_t v[4] = {v4[0], v4[1], v4[2], v4[3]};
    rd::gf_accumulate<W>(acc, v, a.t[i]);
  }
  uint8_t* const op = a.u.out + (uint64_t)o * a.u.out_stride + ((int64_t)x + a.u.out_shift);
  rd_emit(op, upd::lane_bytes(x, a.u.lo, a.u.hi), rd_u32x4{acc[0], acc[1], acc[2], acc[3]}, a.u.first);
}

// grid: objects x tiles; a workgroup is one wave, 64 lane positions of one
// object.  Dynamic LDS: [w][64] accumulators.
__global__ void __launch_bounds__(kBitRdLanes) bit_read(const BitRdArgs a) {
  extern __shared__ rd_u32x4 bit_read_acc[];  // [w][kBitRdLanes]
  rd_u32x4* const acc = bit_read_acc + threadIdx.x;
  const uint32_t o = blockIdx.x / a.u.tiles;
  const uint32_t t = (blockIdx.x - o * a.u.tiles) * (uint32_t)kBitRdLanes + threadIdx.x;
  if (t >= a.npos) return;  // (no barrier below)
  const uint32_t per = a.ps / 16u;
  uint32_t pos = a.pos0 + t;  // < 2 per
  if (pos >= per) pos -= per;
  const uint32_t y = pos * 16u;
  const uint32_t touched = upd::touched_packets(y, a.ps, a.w, a.u.lo, a.u.hi);
  for (uint32_t rest = touched; rest != 0u; rest &= rest - 1u)
    acc[(uint32_t)__builtin_ctz(rest) * kBitRdLanes] = rd_u32x4{0u, 0u, 0u, 0u};
  const uint8_t* const ob = a.u.objs + (uint64_t)o * a.u.obj_stride;
  const uint8_t* const pb = a.u.parity + (uint64_t)o * a.u.parity_stride;
  for (uint32_t i = 0; i < a.nsurv; ++i) {  // uniform: the words come from the argument segment
    const uint32_t sw = i * (a.w + 1u);
    uint32_t valid;
    const uint8_t* const sp = rd_block(a.u, ob, pb, a.words[sw], &valid);
    for (uint32_t c = 0; c < a.w; ++c) {
      uint32_t hit = rd::column_hits(a.words[sw + 1u + c], touched);
      if (!hit) continue;  // feeds no touched packet: not loaded
      const uint32_t at = c * a.ps + y;  // < bs
      const uint32_t have = rd::valid_bytes(at, valid);
      if (!have) continue;
      const rd_u32x4 v = rd_load(sp + at, have);
      for (; hit != 0u; hit &= hit - 1u) acc[(uint32_t)__builtin_ctz(hit) * kBitRdLanes] ^= v;
    }
  }
  uint8_t* const op = a.u.out + (uint64_t)o * a.u.out_stride + a.u.out_shift;
  for (uint32_t rest = touched; rest != 0u; rest &= rest - 1u) {
    const uint32_t r = (uint32_t)__builtin_ctz(rest);
    const uint32_t at = r * a.ps + y;
    rd_emit(op + at, upd::lane_bytes(at, a.u.lo, a.u.hi), acc[r * kBitRdLanes], a.u.first);
  }
}

// The decode rows of one lost block j over the survivors, as the kernels take
// them: the k coefficients of row j (word classes), or the k w column masks
// (packet classes).  Inverted on the host once per (code, survivors, j) and
// kept: keyed like the plan cache (engine.cpp make_plan), bounded by entries
// and bytes, started over when full (rows in use live on through their
// shared_ptr).
int read_rows(const Code& c, const std::vector<int>& surv, int j,
              std::shared_ptr<const std::vector<uint32_t>>* out) {
  static std::mutex mu;
  static std::map<std::vector<intptr_t>, std::shared_ptr<const std::vector<uint32_t>>> cache;
  static size_t cached_bytes = 0;
  constexpr size_t kMaxEntries = 4096, kMaxBytes = (size_t)16 << 20;
  std::vector<intptr_t> key;
  key.reserve(2 + surv.size());
  key.push_back((intptr_t)&c);
  key.push_back(j);
  key.insert(key.end(), surv.begin(), surv.end());
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) {
      *out = it->second;
      return LEOEC_OK;
    }
  }
  auto rows = std::make_shared<std::vector<uint32_t>>();  // built outside the lock
  int rc;
  if (c.bitmatrix) {
    std::vector<uint8_t> bits;
    if ((rc = bit_rows(c, surv.data(), &j, 1, &bits))) return rc;
    rows->resize((size_t)c.k * c.w);
    rd::transpose_rows(bits.data(), (uint32_t)c.k, (uint32_t)c.w, rows->data());
  } else if ((rc = gf_rows(c, surv.data(), &j, 1, rows.get()))) {
    return rc;
  }
  const size_t nb = rows->size() * sizeof(uint32_t) + key.size() * sizeof(intptr_t);
  std::lock_guard<std::mutex> lock(mu);
  if (cache.size() >= kMaxEntries || cached_bytes + nb > kMaxBytes) {
    cache.clear();
    cached_bytes = 0;
  }
  auto ins = cache.emplace(std::move(key), std::move(rows));
  if (ins.second) cached_bytes += nb;
  *out = ins.first->second;
  return LEOEC_OK;
}

template <int W>
int launch_gf_read(const RdArgs& u, const std::vector<int>& surv, const std::vector<uint32_t>& coef,
                   rd::Part p, uint32_t lane0, uint32_t lanes, uint32_t nobj, hipStream_t s) {
  GfRdArgs<W> a;
  a.u = u;
  a.u.first = p.first == 0;
  a.lane0 = lane0;
  a.lanes = lanes;
  a.nsurv = p.count;
  a.pad = 0;
  const Field& f = field(W);
  for (uint32_t i = 0; i < (uint32_t)kGfRdSurv; ++i) {
    const bool on = i < p.count;
    a.id[i] = on ? (uint32_t)surv[p.first + i] : 0u;
    for (int b = 0; b < W; ++b)
      a.t[i][b] = on ? upd::spread<W>(f.mul(coef[p.first + i], 1u << b)) : 0u;
  }
  return launch_kernel(gf_read<W>, dim3(nobj * u.tiles), dim3(kGfRdLanes), 0, s, a);
}

// One lost block of the word classes over one chunk of objects.
int gf_read_segment(RdArgs u, const Code& c, const std::vector<int>& surv,
                    const std::vector<uint32_t>& coef, const upd::Seg& g, uint32_t nobj, hipStream_t s) {
  const uint32_t lane0 = (uint32_t)upd::first_lane(g.lo);
  const uint32_t lanes = (uint32_t)upd::lane_count(g.lo, g.hi);
  u.tiles = (lanes + kGfRdLanes - 1) / kGfRdLanes;
  const uint32_t parts = rd::part_count((uint32_t)c.k, kGfRdSurv);
  for (uint32_t n = 0; n < parts; ++n) {
    const rd::Part p = rd::part((uint32_t)c.k, kGfRdSurv, n);
    const int rc = c.w == 8    ? launch_gf_read<8>(u, surv, coef, p, lane0, lanes, nobj, s)
                   : c.w == 16 ? launch_gf_read<16>(u, surv, coef, p, lane0, lanes, nobj, s)
                               : launch_gf_read<32>(u, surv, coef, p, lane0, lanes, nobj, s);
    if (rc) return rc;
  }
  return LEOEC_OK;
}

// One lost block of the packet classes over one chunk of objects.
int bit_read_segment(const RdArgs& u, const Code& c, const std::vector<int>& surv,
                     const std::vector<uint32_t>& cols, const upd::Seg& g, uint32_t nobj, hipStream_t s) {
  BitRdArgs a;
  a.u = u;
  a.w = (uint32_t)c.w;
  a.ps = u.bs / (uint32_t)c.w;
  const upd::Positions pos = upd::packet_positions(g.lo, g.hi, a.ps);
  a.pos0 = pos.first;
  a.npos = pos.count;
  a.pad = 0;
  a.u.tiles = (pos.count + kBitRdLanes - 1) / kBitRdLanes;
  const size_t lds = (size_t)c.w * kBitRdLanes * sizeof(rd_u32x4);  // <= 32 KiB
  const uint32_t per = (uint32_t)kBitRdWords / (a.w + 1u);          // >= 23
  const uint32_t parts = rd::part_count((uint32_t)c.k, per);
  for (uint32_t n = 0; n < parts; ++n) {
    const rd::Part p = rd::part((uint32_t)c.k, per, n);
    a.u.first = n == 0;
    a.nsurv = p.count;
    uint32_t at = 0;
    for (uint32_t i = 0; i < p.count; ++i) {
      a.words[at++] = (uint32_t)surv[p.first + i];
      for (uint32_t col = 0; col < a.w; ++col) a.words[at++] = cols[(size_t)(p.first + i) * a.w + col];
    }
    while (at < (uint32_t)kBitRdWords) a.words[at++] = 0u;
    const int rc = launch_kernel(bit_read, dim3(nobj * a.u.tiles), dim3(kBitRdLanes), lds, s, a);
    if (rc) return rc;
  }
  return LEOEC_OK;
}

}  // namespace detail

namespace {

using namespace detail;

// [p, p + n) meets [q, q + qn) (no sum that could wrap).
bool overlaps(const void* p, uint64_t n, const void* q, uint64_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a >= b ? a - b < qn : b - a < n;
}

// Bytes from the first row's first byte to the last row's last: false when
// that overflows.
bool extent(uint64_t nobj, uint64_t stride, uint64_t row, uint64_t* bytes) {
  uint64_t e;
  if (__builtin_mul_overflow(nobj - 1, stride, &e) || __builtin_add_overflow(e, row, &e)) return false;
  *bytes = e;
  return true;
}

int op_read_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride, uint64_t size,
                uint64_t nobj, const uint8_t* parity, uint64_t parity_stride, const int* erased,
                int nerased, uint64_t offset, uint64_t length, uint8_t* out, uint64_t out_stride,
                hipStream_t s) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  // the erased list, as op_decode_dev reads it
  if (nerased < 0 || (nerased && !erased)) return LEOEC_E_ARG;
  std::vector<char> gone((size_t)k + m, 0);
  for (int i = 0; i < nerased; ++i) {
    if (erased[i] < 0 || erased[i] >= k + m) return LEOEC_E_BAD_ID;
    gone[(size_t)erased[i]] = 1;
  }
  std::vector<int> surv;
  for (int id = 0; id < k + m && (int)surv.size() < k; ++id)
    if (!gone[(size_t)id]) surv.push_back(id);
  if ((int)surv.size() < k) return LEOEC_E_NOT_ENOUGH_BLOCKS;
  if (nobj == 0 || length == 0 || size == 0) return LEOEC_OK;
  uint64_t end;
  if (__builtin_add_overflow(offset, length, &end) || end > size) return LEOEC_E_BAD_SIZE;
  if ((rc = check_dev_batch(objs, obj_stride, size, parity, parity_stride, m, bs))) return rc;
  const uint64_t lead = offset % 16u;
  if (!out || ((uintptr_t)out & 15u) || (out_stride & 15u) || out_stride < lead + length)
    return LEOEC_E_ARG;
  uint64_t eo, ep, en;
  if (!extent(nobj, obj_stride, size, &eo) || !extent(nobj, parity_stride, (uint64_t)m * bs, &ep) ||
      !extent(nobj, out_stride, lead + length, &en))
    return LEOEC_E_ARG;
  if (overlaps(out, en, objs, eo) || overlaps(out, en, parity, ep)) return LEOEC_E_ARG;
  if ((rc = device_init())) return rc;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  std::vector<upd::Seg> segs((size_t)((end - 1) / bs - offset / bs + 1));
  const int nseg = upd::split_range(bs, offset, length, segs.data(), (int)segs.size());
  if (nseg < 0) return LEOEC_E_ARG;
  std::vector<rd::Group> groups((size_t)nseg);
  const int ngroup = rd::group_segments(segs.data(), nseg, gone.data(), groups.data(), nseg);
  if (ngroup < 0) return LEOEC_E_ARG;
  // the rows of every lost block the range meets, before anything is launched
  std::vector<std::shared_ptr<const std::vector<uint32_t>>> rows((size_t)ngroup);
  for (int g = 0; g < ngroup; ++g)
    if (groups[(size_t)g].lost &&
        (rc = read_rows(*c, surv, (int)segs[groups[(size_t)g].first].block, &rows[(size_t)g])))
      return rc;
  // objects of a launch: objects x tiles < 2^31; no group has more lanes than
  // the row (k bs bytes, bs < 2^32), 64 of them a tile at the least
  uint64_t max_obj = (uint64_t)0x7FFFFFFF / ((uint64_t)k * bs / (16u * kBitRdLanes) + 2u);
  if (kMeasureBuild && knobs().read_chunk > 0 && (uint64_t)knobs().read_chunk < max_obj)
    max_obj = (uint64_t)knobs().read_chunk;
  for (uint64_t o0 = 0; o0 < nobj; o0 += max_obj) {
    const uint32_t no = (uint32_t)(nobj - o0 < max_obj ? nobj - o0 : max_obj);
    RdArgs u;
    u.objs = objs + o0 * obj_stride;
    u.parity = parity + o0 * parity_stride;
    u.out = out + o0 * out_stride;
    u.obj_stride = obj_stride;
    u.parity_stride = parity_stride;
    u.out_stride = out_stride;
    u.size = size;
    u.bs = (uint32_t)bs;  // < 2^32 (check_dev_batch)
    u.k = (uint32_t)k;
    u.first = 1;
    for (int gi = 0; gi < ngroup; ++gi) {
      const rd::Group& grp = groups[(size_t)gi];
      const upd::Seg& g = segs[grp.first];
      if (!grp.lost) {
        const upd::Seg& last = segs[grp.first + grp.count - 1];
        CopyArgs a;
        a.u = u;
        a.p0 = (uint64_t)g.block * bs + g.lo;
        a.p1 = (uint64_t)last.block * bs + last.hi;
        // object byte p is out byte lead + p - offset
        a.u.out_shift = -(int64_t)(offset - lead);
        a.u.lo = a.u.hi = 0;
        const uint64_t tiles = (upd::lane_count(a.p0, a.p1) + kCopyLanes - 1) / kCopyLanes;
        a.u.tiles = (uint32_t)tiles;  // <= k bs / 4096 + 1
        if ((rc = launch_kernel(range_copy, dim3(no * a.u.tiles), dim3(kCopyLanes), 0, s, a))) return rc;
        continue;
      }
      // block byte x of block j is object byte j bs + x
      u.out_shift = (int64_t)((uint64_t)g.block * bs) - (int64_t)(offset - lead);
      u.lo = (uint32_t)g.lo;
      u.hi = (uint32_t)g.hi;  // <= bs < 2^32
      u.tiles = 0;
      rc = c->bitmatrix ? bit_read_segment(u, *c, surv, *rows[(size_t)gi], g, no, s)
                        : gf_read_segment(u, *c, surv, *rows[(size_t)gi], g, no, s);
      if (rc) return rc;
    }
  }
  return LEOEC_OK;
}

}  // namespace
}  // namespace leoec

extern "C" {

int leoec_read_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                   uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                   const int* erased, int nerased, uint64_t offset, uint64_t length, uint8_t* out,
                   uint64_t out_stride, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_read_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride,
                              erased, nerased, offset, length, out, out_stride, (hipStream_t)stream);
  });
}

}  // extern "C"
