// dev_table.hpp — a cache of per-(code, device) tables on the devices (heal's
// pattern tables, scrub's block tables): each built and uploaded at the first
// call that needs it and kept for the process.  Never evicted (a queued launch
// may still be reading one), so bounded by count: past Cap the caller takes
// its path without a table.  The host image stays alive beside the device copy.
#pragma once

#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "engine.hpp"

namespace leoec {

template <class Key, size_t Cap>
class DevTableCache {
 public:
  // The table of `key` on the current device, from build(&host image) -> status
  // the first time.  LEOEC_OK and *out = the device image, or *out = nullptr
  // when the cache is full; a status when the build or the upload failed.
  template <class Build>
  int get(const Key& key, Build&& build, const uint32_t** out) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return LEOEC_E_HIP;
    std::lock_guard<std::mutex> lock(mu_);
    const auto it = map_.find({key, dev});
    if (it != map_.end()) {
      *out = it->second.dev;
      return LEOEC_OK;
    }
    *out = nullptr;
    if (map_.size() >= Cap) return LEOEC_OK;
    Entry t;
    const int rc = build(&t.host);
    if (rc) return rc;
    const size_t bytes = t.host.size() * sizeof(uint32_t);
    if (hipMalloc(&t.dev, bytes) != hipSuccess) return LEOEC_E_NOMEM;
    // a blocking copy: the image is on the device before any launch reads it
    if (hipMemcpy(t.dev, t.host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
      hip_drop(hipFree(t.dev));
      return LEOEC_E_HIP;
    }
    *out = t.dev;
    map_.emplace(std::make_pair(key, dev), std::move(t));
    return LEOEC_OK;
  }

 private:
  struct Entry {
    std::vector<uint32_t> host;
    uint32_t* dev = nullptr;
  };
  std::mutex mu_;
  std::map<std::pair<Key, int>, Entry> map_;
};

}  // namespace leoec
