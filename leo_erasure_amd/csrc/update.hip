// update.hip — leoec_update_dev: a byte range of every object of a stored
// batch overwritten in place, and the parity patched to match, without reading
// the rest of the object.
//
// Every code is linear: with D = old ^ new inside the range and zero
// elsewhere, parity(new) = parity(old) ^ encode(D) (update_core.hpp).  The
// range is split at data-block boundaries; per touched data block j, on the
// stream, nothing allocated, uploaded or waited for:
//   gf_update<W, R>  vandrs w = 8 / 16 / 32, isars: one lane per 16-byte lane
//                    of the segment; old from objs, new from the patch, the
//                    delta masked to the range bytewise, the new bytes stored,
//                    and parity_i ^= C[i][j] * delta for R coding blocks, whose
//                    products C[i][j] * alpha^b travel as kernel arguments.
//                    m > 4: ceil(m / 4) launches.
//   bit_update       cauchyrs, liberation: one lane per object and lane
//                    position y of a packet; the masked deltas of the touched
//                    data packets at y go to LDS (every lane its own slots: no
//                    barrier, no register array indexed by a runtime w), then
//                    per coding packet whose bit-row meets a touched packet one
//                    read-modify-write of its lane at y.  Column block j of
//                    the coding bitmatrix travels as kernel arguments, 64
//                    bit-rows a launch.
// When the rows of a data block take several launches, every launch reads old
// from objs again, so only the last one stores the new bytes (`store`).
// The kernels depend on w and the rows of a launch, never on k.  Head and tail
// lanes gather and scatter their bytes one by one: nothing outside the range
// is read from objs or the patch, or written to objs.
// A chunk of objects exists only to keep a launch's grid below 2^31.
// This unit is kept out of engine.cpp / capi.cpp for verify.hip's reason: the
// host sanitizer harness links those against stand-in kernels.
#include <vector>

#include "engine.hpp"
#include "knobs.hpp"
#include "update_core.hpp"

namespace leoec {
namespace detail {

typedef uint32_t upd_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kGfUpdLanes = 256;  // 4 KiB of the segment per workgroup
constexpr int kGfUpdRows = 4;     // coding blocks per launch
constexpr int kBitUpdLanes = 64;  // 1 KiB of every packet per workgroup
constexpr int kBitUpdRows = 64;   // coding packets (bit-rows) per launch

// One segment of one chunk of objects.
struct UpdArgs {
  uint8_t* objs;         // the chunk's first row + j bs: byte 0 of the data block
  uint8_t* parity;       // the chunk's first row
  const uint8_t* patch;  // the chunk's first row
  uint64_t obj_stride, parity_stride, patch_stride;
  int64_t patch_shift;   // block byte x is patch byte x + patch_shift (a multiple of 16)
  uint32_t lo, hi;       // the segment, block-local bytes
  uint32_t bs;
  uint32_t tiles;        // workgroups per object
  uint32_t store;        // the last launch of the segment: write the new bytes
  uint32_t pad;
};

template <int W, int R>
struct GfUpdArgs {
  UpdArgs u;
  uint32_t row0;      // first coding block of the launch
  uint32_t lane0;     // first 16-byte lane of the block, and how many
  uint32_t lanes;
  uint32_t t[R][W];   // spread(C[row0 + r][j] * alpha^b)
};

struct BitUpdArgs {
  UpdArgs u;
  uint32_t w, ps;
  uint32_t row0, nrows;  // coding packets row0 .. row0 + nrows - 1 (packet i w + r of the parity row)
  uint32_t pos0, npos;   // upd::Positions
  uint32_t rows[kBitUpdRows];  // bit c: data packet c of block j feeds the coding packet
};

// A whole lane in one access; a head or tail lane byte by byte
// (upd::gather16 / scatter16: zero outside the range, nothing else touched).
__device__ __forceinline__ upd_u32x4 upd_load(const uint8_t* p, uint32_t bytes) {
  if (bytes == 0xFFFFu) return *reinterpret_cast<const upd_u32x4*>(p);
  uint32_t d[4];
  upd::gather16(p, bytes, d);
  return upd_u32x4{d[0], d[1], d[2], d[3]};
}

__device__ __forceinline__ void upd_store(uint8_t* p, uint32_t bytes, upd_u32x4 v) {
  if (bytes == 0xFFFFu) {
    *reinterpret_cast<upd_u32x4*>(p) = v;
    return;
  }
  const uint32_t d[4] = {v[0], v[1], v[2], v[3]};
  upd::scatter16(p, bytes, d);
}

// grid: objects x tiles; a workgroup is 256 consecutive lanes of one object's
// segment.  Every lane of the segment holds a byte of the range.
template <int W, int R>
__global__ void __launch_bounds__(kGfUpdLanes) gf_update(const GfUpdArgs<W, R> a) {
  const uint32_t o = blockIdx.x / a.u.tiles;
  const uint32_t l = (blockIdx.x - o * a.u.tiles) * (uint32_t)kGfUpdLanes + threadIdx.x;
  if (l >= a.lanes) return;
  const uint32_t x = (a.lane0 + l) * 16u;  // < bs
  const uint32_t bytes = upd::lane_bytes(x, a.u.lo, a.u.hi);
  uint8_t* const op = a.u.objs + (uint64_t)o * a.u.obj_stride + x;
  const uint8_t* const np = a.u.patch + (uint64_t)o * a.u.patch_stride + ((int64_t)x + a.u.patch_shift);
  const upd_u32x4 old = upd_load(op, bytes);
  const upd_u32x4 nw = upd_load(np, bytes);  // gathered lanes: zero outside the range, as old
  const upd_u32x4 delta = old ^ nw;
  if (a.u.store) upd_store(op, bytes, nw);
  uint8_t* const pp = a.u.parity + (uint64_t)o * a.u.parity_stride + (uint64_t)a.row0 * a.u.bs + x;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    upd_u32x4* const p = reinterpret_cast<upd_u32x4*>(pp + (uint64_t)r * a.u.bs);
    upd_u32x4 v = *p;
#pragma unroll
    for (int d = 0; d < 4; ++d) v[d] ^= upd::mul_dword<W>(delta[d], a.t[r]);
    *p = v;
  }
}

// grid: objects x tiles; a workgroup is one wave, 64 lane positions of one
// object.  Dynamic LDS: [w][64] deltas.
__global__ void __launch_bounds__(kBitUpdLanes) bit_update(const BitUpdArgs a) {
  extern __shared__ upd_u32x4 bit_update_delta[];  // [w][kBitUpdLanes]
  upd_u32x4* const delta = bit_update_delta + threadIdx.x;
  const uint32_t o = blockIdx.x / a.u.tiles;
  const uint32_t t = (blockIdx.x - o * a.u.tiles) * (uint32_t)kBitUpdLanes + threadIdx.x;
  if (t >= a.npos) return;  // (no barrier below)
  const uint32_t per = a.ps / 16u;
  uint32_t pos = a.pos0 + t;  // < 2 per
  if (pos >= per) pos -= per;
  const uint32_t y = pos * 16u;
  uint8_t* const ob = a.u.objs + (uint64_t)o * a.u.obj_stride;
  const uint8_t* const nb = a.u.patch + (uint64_t)o * a.u.patch_stride + a.u.patch_shift;
  uint32_t touched = 0u;
  for (uint32_t c = 0; c < a.w; ++c) {
    const uint32_t at = c * a.ps + y;  // < bs
    const uint32_t bytes = upd::lane_bytes(at, a.u.lo, a.u.hi);
    if (!bytes) continue;
    touched |= 1u << c;
    delta[c * kBitUpdLanes] = upd_load(ob + at, bytes) ^ upd_load(nb + at, bytes);
  }
  uint8_t* const pb = a.u.parity + (uint64_t)o * a.u.parity_stride + y;
  for (uint32_t q = 0; q < a.nrows; ++q) {
    uint32_t hit = a.rows[q] & touched;
    if (!upd::row_meets(a.rows[q], touched)) continue;  // neither read nor written
    upd_u32x4 acc = {0u, 0u, 0u, 0u};
    for (; hit != 0u; hit &= hit - 1u) acc ^= delta[(uint32_t)__builtin_ctz(hit) * kBitUpdLanes];
    upd_u32x4* const p = reinterpret_cast<upd_u32x4*>(pb + (uint64_t)(a.row0 + q) * a.ps);
    *p = *p ^ acc;
  }
  if (!a.u.store) return;
  for (uint32_t rest = touched; rest != 0u; rest &= rest - 1u) {
    const uint32_t at = (uint32_t)__builtin_ctz(rest) * a.ps + y;
    const uint32_t bytes = upd::lane_bytes(at, a.u.lo, a.u.hi);
    upd_store(ob + at, bytes, upd_load(nb + at, bytes));
  }
}

template <int W, int R>
int launch_gf_update_wr(const UpdArgs& u, const Code& c, uint32_t j, uint32_t row0, uint32_t lane0,
                        uint32_t lanes, uint32_t nobj, hipStream_t s) {
  GfUpdArgs<W, R> a;
  a.u = u;
  a.row0 = row0;
  a.lane0 = lane0;
  a.lanes = lanes;
  const Field& f = field(W);
  for (int r = 0; r < R; ++r)
    for (int b = 0; b < W; ++b)
      a.t[r][b] = upd::spread<W>(f.mul(c.C.at((int)row0 + r, (int)j), 1u << b));
  return launch_kernel((gf_update<W, R>), dim3(nobj * u.tiles), dim3(kGfUpdLanes), 0, s, a);
}

template <int W>
int launch_gf_update_w(int rows, const UpdArgs& u, const Code& c, uint32_t j, uint32_t row0,
                       uint32_t lane0, uint32_t lanes, uint32_t nobj, hipStream_t s) {
  switch (rows) {
    case 1: return launch_gf_update_wr<W, 1>(u, c, j, row0, lane0, lanes, nobj, s);
    case 2: return launch_gf_update_wr<W, 2>(u, c, j, row0, lane0, lanes, nobj, s);
    case 3: return launch_gf_update_wr<W, 3>(u, c, j, row0, lane0, lanes, nobj, s);
    default: return launch_gf_update_wr<W, 4>(u, c, j, row0, lane0, lanes, nobj, s);
  }
}

// One segment of the word classes over one chunk of objects.
int gf_update_segment(UpdArgs u, const Code& c, const upd::Seg& g, uint32_t nobj, hipStream_t s) {
  const uint32_t lane0 = (uint32_t)upd::first_lane(g.lo);
  const uint32_t lanes = (uint32_t)upd::lane_count(g.lo, g.hi);
  u.tiles = (lanes + kGfUpdLanes - 1) / kGfUpdLanes;
  for (int row0 = 0; row0 < c.m; row0 += kGfUpdRows) {
    const int rows = c.m - row0 < kGfUpdRows ? c.m - row0 : kGfUpdRows;
    u.store = row0 + rows == c.m;
    const int rc = c.w == 8    ? launch_gf_update_w<8>(rows, u, c, g.block, row0, lane0, lanes, nobj, s)
                   : c.w == 16 ? launch_gf_update_w<16>(rows, u, c, g.block, row0, lane0, lanes, nobj, s)
                               : launch_gf_update_w<32>(rows, u, c, g.block, row0, lane0, lanes, nobj, s);
    if (rc) return rc;
  }
  return LEOEC_OK;
}

// One segment of the packet classes over one chunk of objects.
int bit_update_segment(const UpdArgs& u, const Code& c, const upd::Seg& g, uint32_t nobj, hipStream_t s) {
  BitUpdArgs a;
  a.u = u;
  a.w = (uint32_t)c.w;
  a.ps = u.bs / (uint32_t)c.w;
  const upd::Positions pos = upd::packet_positions(g.lo, g.hi, a.ps);
  a.pos0 = pos.first;
  a.npos = pos.count;
  a.u.tiles = (pos.count + kBitUpdLanes - 1) / kBitUpdLanes;
  const size_t lds = (size_t)c.w * kBitUpdLanes * sizeof(upd_u32x4);  // <= 32 KiB
  const int total = c.m * c.w;
  for (int row0 = 0; row0 < total; row0 += kBitUpdRows) {
    const int rows = total - row0 < kBitUpdRows ? total - row0 : kBitUpdRows;
    a.row0 = (uint32_t)row0;
    a.nrows = (uint32_t)rows;
    a.u.store = row0 + rows == total;
    for (int q = 0; q < kBitUpdRows; ++q) {
      uint32_t word = 0u;
      if (q < rows)
        for (int col = 0; col < c.w; ++col)
          word |= (uint32_t)c.B.get(row0 + q, (int)g.block * c.w + col) << col;
      a.rows[q] = word;
    }
    const int rc = launch_kernel(bit_update, dim3(nobj * a.u.tiles), dim3(kBitUpdLanes), lds, s, a);
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

int op_update_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride, uint64_t size,
                  uint64_t nobj, uint8_t* parity, uint64_t parity_stride, const uint8_t* patch,
                  uint64_t patch_stride, uint64_t offset, uint64_t length, hipStream_t s) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  if (nobj == 0 || length == 0 || size == 0) return LEOEC_OK;
  uint64_t end;
  if (__builtin_add_overflow(offset, length, &end) || end > size) return LEOEC_E_BAD_SIZE;
  if ((rc = check_dev_batch(objs, obj_stride, size, parity, parity_stride, m, bs))) return rc;
  const uint64_t lead = offset % 16u;
  if (!patch || ((uintptr_t)patch & 15u) || (patch_stride & 15u) || patch_stride < lead + length)
    return LEOEC_E_ARG;
  uint64_t eo, ep, en;
  if (!extent(nobj, obj_stride, size, &eo) || !extent(nobj, parity_stride, (uint64_t)m * bs, &ep) ||
      !extent(nobj, patch_stride, lead + length, &en))
    return LEOEC_E_ARG;
  if (overlaps(patch, en, objs, eo) || overlaps(patch, en, parity, ep)) return LEOEC_E_ARG;
  if ((rc = device_init())) return rc;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  std::vector<upd::Seg> segs((size_t)((end - 1) / bs - offset / bs + 1));
  const int nseg = upd::split_range(bs, offset, length, segs.data(), (int)segs.size());
  if (nseg < 0) return LEOEC_E_ARG;
  // objects of a launch: objects x tiles < 2^31; a segment has at most
  // bs / 16 lanes (bs < 2^32), 64 of them a tile at the least
  uint64_t max_obj = (uint64_t)0x7FFFFFFF / ((bs / 16u + kBitUpdLanes - 1) / kBitUpdLanes);
  if (kMeasureBuild && knobs().update_chunk > 0 && (uint64_t)knobs().update_chunk < max_obj)
    max_obj = (uint64_t)knobs().update_chunk;
  for (uint64_t o0 = 0; o0 < nobj; o0 += max_obj) {
    const uint32_t no = (uint32_t)(nobj - o0 < max_obj ? nobj - o0 : max_obj);
    for (int i = 0; i < nseg; ++i) {
      const upd::Seg& g = segs[(size_t)i];
      UpdArgs u;
      u.objs = objs + o0 * obj_stride + (uint64_t)g.block * bs;
      u.parity = parity + o0 * parity_stride;
      u.patch = patch + o0 * patch_stride;
      u.obj_stride = obj_stride;
      u.parity_stride = parity_stride;
      u.patch_stride = patch_stride;
      // object byte p is patch byte lead + p - offset; p = block bs + x
      u.patch_shift = (int64_t)((uint64_t)g.block * bs) - (int64_t)(offset - lead);
      u.lo = (uint32_t)g.lo;
      u.hi = (uint32_t)g.hi;  // <= bs < 2^32
      u.bs = (uint32_t)bs;
      u.tiles = 0;
      u.store = 0;
      u.pad = 0;
      rc = c->bitmatrix ? bit_update_segment(u, *c, g, no, s) : gf_update_segment(u, *c, g, no, s);
      if (rc) return rc;
    }
  }
  return LEOEC_OK;
}

}  // namespace
}  // namespace leoec

extern "C" {

int leoec_update_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                     const uint8_t* patch, uint64_t patch_stride, uint64_t offset, uint64_t length,
                     void* stream) {
  return leoec::guarded([&] {
    return leoec::op_update_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride,
                                patch, patch_stride, offset, length, (hipStream_t)stream);
  });
}

}  // extern "C"
