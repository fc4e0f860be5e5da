// scrub_steps.hpp — what scrub.hip (leoec_scrub_dev, leoec_scrub_ws_dev) takes
// from locate.hip and heal.hip: the locate calls with the caller's own steps
// in them, the heal call and heal's pattern table.  Internal to those three
// units.
#pragma once

#include "engine.hpp"

namespace leoec {

// The places of op_locate_dev where a caller that goes on from the words does
// its own share, each a status that ends the call when it is not LEOEC_OK.
struct LocateSteps {
  // After the parameters, the served test, the empty batch and `lost`'s own
  // check, before the batch's pointers and strides: the caller's buffers
  // (bs: the block size).
  virtual int check(uint64_t bs) = 0;
  // The device is open and nothing is enqueued yet.
  virtual int begin(const Code& c, hipStream_t s) = 0;
  // In place of locate_finish, after the memset and gf8_locate of objects
  // [o0, o0 + no): lost[o0 ..] holds the ANDed candidate masks.
  virtual int finish(uint64_t o0, uint64_t no, hipStream_t s) = 0;

 protected:
  ~LocateSteps() = default;
};

// locate.hip; steps == nullptr: leoec_locate_dev.
int op_locate_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                  uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                  uint32_t* lost, hipStream_t s, LocateSteps* steps);

// locate.hip: cauchyrs or liberation, the classes of leoec_locate_ws_dev's
// bitmatrix branch.
bool bit_class(int coding);

// locate.hip; steps == nullptr: leoec_locate_ws_dev.  The steps stand in the
// bitmatrix branch (cauchyrs, liberation) at the same three places: check
// after the served test, the empty batch and `lost`'s check, begin once the
// device is open, finish(o0, no, s) in locate_finish's place after the
// chunk's encode, memset and bit_locate.  `workspace` is the encode region:
// the chunk size comes from workspace_bytes.
int op_locate_ws_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                     uint32_t* lost, void* workspace, uint64_t workspace_bytes, hipStream_t s,
                     LocateSteps* steps);

// locate.hip: class (a) of leoec_locate_gfw_dev, what it forwards to
// leoec_locate_ws_dev (the bitmatrix configurations that call refuses among
// them).
bool gfw_forwarded(int coding, int k, int m, int w);

// locate.hip; steps == nullptr: leoec_locate_gfw_dev.  The steps stand in the
// word branch (class (c)) at the same three places as in op_locate_ws_dev:
// check after the served test, the empty batch and `lost`'s check, begin once
// the device is open, finish(o0, no, s) in locate_finish's place after the
// chunk's encode, memset and gfw_locate.  `workspace` is the encode region.
int op_locate_gfw_dev(int coding, int k, int m, int w, const uint8_t* objs, uint64_t obj_stride,
                      uint64_t size, uint64_t nobj, const uint8_t* parity, uint64_t parity_stride,
                      uint32_t* lost, void* workspace, uint64_t workspace_bytes, hipStream_t s,
                      LocateSteps* steps);

// heal.hip: leoec_heal_dev, and the code's pattern table on the current
// device: LEOEC_OK and *out = the device image, or *out = nullptr when the
// cache is full; a status when the build or the upload failed.
int op_heal_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride, uint64_t size,
                uint64_t nobj, uint8_t* parity, uint64_t parity_stride, const uint32_t* lost,
                uint32_t* unhealed, hipStream_t s);
int heal_table(const Code& c, const uint32_t** out);

}  // namespace leoec
