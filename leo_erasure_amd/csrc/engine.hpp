// engine.hpp — host side of the engine: code cache, survivor selection,
// decoding maps, device context and the operations behind the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <new>
#include <vector>

#include "../../include/leoec.h"
#include "codes.hpp"
#include "kernels.hpp"

namespace leoec {

// The coding class resolved for (coding, k, m, w): either a GF(2^w) coding
// matrix (vandrs, isars) or a GF(2) coding bitmatrix (cauchyrs, liberation).
struct Code {
  int coding = 0, k = 0, m = 0, w = 0;
  bool bitmatrix = false;
  GfMatrix C;   // m x k
  BitMatrix B;  // (m*w) x (k*w)
};

int check_params(int coding, int k, int m, int w);
int get_code(int coding, int k, int m, int w, const Code** out);  // cached

// Rows expressing the `want` block ids in terms of the k survivor ids `surv`
// (the reference's decoding matrices; see engine.cpp).
int gf_rows(const Code& c, const int* surv, const int* want, int nwant, std::vector<uint32_t>* rows);
int bit_rows(const Code& c, const int* surv, const int* want, int nwant, std::vector<uint8_t>* rows);

// The map "out blocks = f(survivor blocks)" of one (code, survivors,
// wanted ids), built on the host once: GF(2^w) coefficient rows (vandrs,
// isars, cauchyrs through the packet-bitsliced kernel), GF(2) bit rows (the
// generic bitmatrix kernel) or liberation's syndrome-decode masks.  All the
// host arithmetic of a call (the k x k / kw x kw inversions) happens here, so
// a plan that fails fails on the calling thread, before any device work.
struct Plan {
  enum Kind { kGf, kGfBit, kLibDec, kBit };
  Kind kind = kGf;
  const Code* code = nullptr;
  std::vector<int> surv, want;
  std::vector<uint32_t> coef;   // kGf, kGfBit: nwant x k
  std::vector<uint8_t> bits;    // kBit: (nwant w) x (k w)
  std::vector<int> lib_pos;     // kLibDec: id -> index of its shard in `in` (k + 2), -1 absent
  std::vector<uint32_t> mbits;  // kLibDec: nwant x 2w
};

// Cached by (code, survivors, wanted ids): repeated erasure patterns reuse
// their inverse.  The shared_ptr keeps a plan alive while a batch uses it.
int make_plan(const Code& c, const int* surv, const int* want, int nwant,
              std::shared_ptr<const Plan>* out);
// Host bytes a plan holds (its tables): the plan cache's size bound.
size_t plan_bytes(const Plan& p);
// Enqueue a plan over a batch.  in: k shards in survivor order; out: nwant.
int run_plan(const Plan& p, const std::vector<Shard>& in, const std::vector<Shard>& out,
             uint64_t block_size, uint64_t nobj, hipStream_t s);
// make_plan + run_plan.
int apply(const Code& c, const int* surv, const std::vector<Shard>& in, const int* want,
          const std::vector<Shard>& out, uint64_t block_size, uint64_t nobj, hipStream_t s);

// Opens the HIP runtime once and lists its gfx950 devices; LEOEC_E_NO_DEVICE
// if there is none.
int device_init();
// The gfx950 device ordinals the host-memory entry points spread their calls
// over (valid after device_init() returned LEOEC_OK).
const std::vector<int>& host_devices();
constexpr int kMaxDevices = 64;

// For a HIP call whose failure the engine recovers from or has nothing to do
// about (a buffer that cannot be had: the call takes another form; a free or
// a drain on a path that goes on): true when it succeeded.  A failure is
// also taken out of the calling thread's last-error slot, where the runtime
// left it and where the caller, or torch after its next launch, would find
// an error that is nobody's any more (include/leoec.h, Conventions).  What
// the clear drops is this call's own failure; an older error of the caller's
// pending in the slot goes with it, which only host-memory calls can cause:
// the *_dev entry points swallow no failure, with two exceptions on paths
// where a HIP call of their own has failed, which the contract leaves open —
// the process's first call of any kind runs device_init, which passes over a
// device whose property query fails, and heal's table upload frees its
// buffer when the copy into it fails (that call returns LEOEC_E_HIP).
inline bool hip_drop(hipError_t e) {
  if (e == hipSuccess) return true;
  (void)hipGetLastError();
  return false;
}

// Makes `dev` the calling thread's current HIP device for a scope and puts
// the previous one back (host-memory calls run on the device the dispatcher
// picked without changing the caller's own device).
class DeviceScope {
 public:
  explicit DeviceScope(int dev);
  ~DeviceScope();
  bool ok() const { return ok_; }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;

 private:
  int prev_ = -1;
  bool ok_ = true;
};

// No C++ exception crosses the C ABI: anything thrown below an entry point
// becomes a status code.
template <typename F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return LEOEC_E_NOMEM;
  } catch (...) {
    return LEOEC_E_ARG;
  }
}

// Bytes of [start, start + bs) that lie inside an object of `size` bytes.
uint64_t clamp_valid(uint64_t size, uint64_t start, uint64_t bs);
// Block `id` of every object of a device batch: a data id (< k) lies in the
// objs rows and is clipped to `size`, a coding id is whole, in the parity rows.
Shard block_shard(int id, int k, uint64_t bs, uint64_t size, const uint8_t* objs,
                  uint64_t obj_stride, const uint8_t* parity, uint64_t parity_stride);
// The encode direction of a device batch: the data blocks 0..k-1 in, the m
// coding blocks out (block_shard), and their ids as make_plan / apply take them.
struct EncodeShards {
  std::vector<Shard> in, par;
  std::vector<int> ids;  // 0..k+m-1
  const int* surv() const { return ids.data(); }
  const int* want() const { return ids.data() + in.size(); }
};
EncodeShards encode_shards(int k, int m, uint64_t bs, uint64_t size, const uint8_t* objs,
                           uint64_t obj_stride, const uint8_t* parity, uint64_t parity_stride);
// The batch checks of the verify / heal / locate entry points, in this order:
// null or not 16-byte aligned bases, strides not multiples of 16
// (LEOEC_E_ARG); bs >= 2^32 (LEOEC_E_BAD_SIZE); a stride shorter than its row
// (LEOEC_E_ARG).
int check_dev_batch(const uint8_t* objs, uint64_t obj_stride, uint64_t size, const uint8_t* parity,
                    uint64_t parity_stride, int m, uint64_t bs);

// Operations behind the C ABI (argument checking included).
int op_layout(int coding, int k, int m, int w, uint64_t size, uint64_t* bs, int* filled);
int op_encode(int coding, int k, int m, int w, const uint8_t* obj, uint64_t size, uint8_t* out,
              uint64_t out_size);
int op_decode(int coding, int k, int m, int w, const uint8_t* const* blocks, const int* ids, int n,
              uint64_t bs, uint64_t size, uint8_t* out);
int op_repair(int coding, int k, int m, int w, const uint8_t* const* blocks, const int* ids, int n,
              uint64_t bs, const int* rep, int nrep, uint8_t* out);
int op_encode_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                  uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                  hipStream_t s);
int op_decode_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                  uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                  const int* erased, int nerased, hipStream_t s);
int op_repair_dev(int coding, int k, int m, int w, const uint8_t* const* blocks,
                  uint64_t block_stride, uint64_t bs, uint64_t nobj, const int* rep, int nrep,
                  uint8_t* const* out, uint64_t out_stride, hipStream_t s);

// The runtime warm-up of one device (once per device; best effort, always
// LEOEC_OK): hardware queues, the pageable-copy staging, every kernel code
// object, the device's batching queue and its pools of per-thread streams
// and mapped buffers.  gf_init warms the caller's current device;
// leoec_host_spread warms every device of its set (warm_devices, one thread
// per device).
int warm_device(int dev);
int warm_current_device();
void warm_devices(const int* devs, int n);

// What the warm-up left on a device (tests): pooled streams and mapped
// buffers not yet taken by a thread, whether every lane of the device has
// its batching queue, and the process's count of built queues.
struct WarmState {
  int pool_streams = 0;
  int pool_mapped = 0;
  bool queue = false;
  int queues_built = 0;
};
WarmState warm_state(int dev);

// The per-thread staging of exited threads (engine.cpp Staging::hand_off,
// reclaim_drain): stagings handed off at thread exit, stagings freed by a
// live thread, and handed-off stagings found with work in flight (the
// invariant says none); and warm_devices' threads started / finished.
struct ReclaimState {
  long handed_off = 0;
  long drained = 0;
  long busy = 0;
  long warm_threads_started = 0;
  long warm_threads_done = 0;
};
ReclaimState reclaim_state();

}  // namespace leoec
