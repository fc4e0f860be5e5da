// Group-wise completion of the batching queue (hostq.cpp,
// Knobs::hostq_done_groups) under the sanitizers, TEST INFRASTRUCTURE ONLY:
// built by tests/test_hostq_groups_sanitize.py with the fake HIP runtime of
// this directory and -DLEOEC_MEASURE, once with -fsanitize=address,undefined
// and once with -fsanitize=thread, as an executable of its own.
//
// 32 threads drive vandrs RS(10,4,8) encodes, decodes and repairs through the
// queue with G = 4 (every call batched; the 1 MiB bound on a grouped batch's
// output lowered with -DLEOEC_HOSTQ_GROUP_MIN_OUT so the CPU kernels stay
// quick), in each waiting form (polled events, blocking-sync events,
// broadcast wake-ups).  Every result equals the oracle's, batches did come
// back in several groups, and every slot returns to FREE.
//
// Then the output copy of group 1 of every grouped batch "fails"
// (LEOEC_HOSTQ_FAIL_GROUP): a call returns LEOEC_OK with bit-exact output (its
// group came before the failing one: that copy landed) or LEOEC_E_HIP (the
// failing group and every later one), both occur, no slot leaks, and with the
// injection off again every call succeeds.
//
//   hostq_groups [threads] [rounds]     exit 0 = all of the above held
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>  // the fake runtime of this directory

#include "../../include/leoec.h"
#include "../../leo_erasure_amd/csrc/hostq.hpp"
extern "C" {
#include "../../oracle/leoec_oracle.h"
}

extern "C" int leoec_measure_set_knob(const char* name, const char* value);
extern "C" void leoec_measure_reset_knobs(void);

namespace {

constexpr int kK = 10, kM = 4, kW = 8, kN = kK + kM;

struct Obj {
  uint64_t size = 0, bs = 0;
  int filled = 0;  // encode writes blocks filled .. k + m - 1
  std::vector<uint8_t> data, ref;  // ref: the oracle's (k + m) * bs blocks
  const uint8_t* block(int id) const { return ref.data() + (size_t)id * bs; }
};

std::mutex g_err_mu;
std::vector<std::string> g_errs;
void fail(const std::string& e) {
  std::lock_guard<std::mutex> l(g_err_mu);
  if (g_errs.size() < 20) g_errs.push_back(e);
}

void prepare(Obj* c, uint64_t size, uint32_t seed) {
  std::mt19937 rng(seed);
  c->size = size;
  c->data.resize(size);
  for (auto& x : c->data) x = (uint8_t)rng();
  c->bs = orc_block_size(kK, kW, size);
  c->ref.assign((size_t)kN * c->bs, 0);
  if (orc_encode(LEOEC_VANDRS, kK, kM, kW, c->data.data(), size, c->ref.data())) std::abort();
  uint64_t bs = 0;
  if (leoec_layout(LEOEC_VANDRS, kK, kM, kW, size, &bs, &c->filled) || bs != c->bs) std::abort();
}

// One call (what % 3: encode, decode of {0,1,2,3}, repair of {0,5,10,13})
// into a buffer filled with 0xA5.  Returns the status; *exact: the output
// equals the oracle's.
int call(const Obj& c, int what, bool* exact) {
  const uint64_t bs = c.bs;
  if (what % 3 == 0) {
    std::vector<uint8_t> out((size_t)(kN - c.filled) * bs, 0xA5);
    const int rc = leoec_encode(LEOEC_VANDRS, kK, kM, kW, c.data.data(), c.size, out.data(), out.size());
    *exact = !std::memcmp(out.data(), c.block(c.filled), out.size());
    return rc;
  }
  const bool dec = what % 3 == 1;
  const int gone[4] = {0, dec ? 1 : 5, dec ? 2 : 10, dec ? 3 : 13};
  std::vector<int> ids;
  std::vector<const uint8_t*> ptrs;
  for (int id = 0; id < kN; ++id)
    if (id != gone[0] && id != gone[1] && id != gone[2] && id != gone[3]) {
      ids.push_back(id);
      ptrs.push_back(c.block(id));
    }
  if (dec) {
    std::vector<uint8_t> out(c.size, 0xA5);
    const int rc = leoec_decode(LEOEC_VANDRS, kK, kM, kW, ptrs.data(), ids.data(), (int)ids.size(), bs,
                                c.size, out.data());
    *exact = !std::memcmp(out.data(), c.data.data(), c.size);
    return rc;
  }
  std::vector<uint8_t> out((size_t)4 * bs, 0xA5);
  const int rc = leoec_repair(LEOEC_VANDRS, kK, kM, kW, ptrs.data(), ids.data(), (int)ids.size(), bs,
                              gone, 4, out.data());
  *exact = true;
  for (int r = 0; r < 4; ++r) *exact &= !std::memcmp(out.data() + (size_t)r * bs, c.block(gone[r]), bs);
  return rc;
}

void set(const char* name, const char* value) {
  if (leoec_measure_set_knob(name, value)) std::abort();
}

}  // namespace

int main(int argc, char** argv) {
  const int threads = argc > 1 ? std::atoi(argv[1]) : 32;
  const int rounds = argc > 2 ? std::atoi(argv[2]) : 6;
  if (leoec_gf_init() != LEOEC_OK) {
    std::fprintf(stderr, "gf_init failed\n");
    return 2;
  }
  // every thread's own objects, one per size (another caller's output in a
  // buffer is then a mismatch)
  const uint64_t sizes[3] = {4096, 65537, 262144};
  std::vector<Obj> objs((size_t)threads * 3);
  for (int t = 0; t < threads; ++t)
    for (int s = 0; s < 3; ++s) prepare(&objs[(size_t)t * 3 + s], sizes[s], 1000u + (uint32_t)(t * 3 + s));

  std::atomic<long> n_ok{0}, n_hip{0};
  auto phase = [&](const char* what, bool injected) {
    n_ok = n_hip = 0;
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
      th.emplace_back([&, t] {
        for (int r = 0; r < rounds; ++r) {
          const Obj& c = objs[(size_t)t * 3 + (size_t)((t + r) % 3)];
          bool exact = false;
          const int rc = call(c, t + 2 * r, &exact);
          if (rc == LEOEC_OK && exact)
            ++n_ok;
          else if (rc == LEOEC_E_HIP && injected)
            ++n_hip;
          else
            fail(std::string(what) + ": thread " + std::to_string(t) + " round " + std::to_string(r) +
                 " size " + std::to_string(c.size) + " rc " + std::to_string(rc) +
                 (exact ? "" : ", output differs"));
        }
      });
    for (auto& x : th) x.join();
    const int busy = leoec::hostq_slots_busy();
    if (busy) fail(std::string(what) + ": " + std::to_string(busy) + " slots not FREE");
    std::printf("%s: %ld ok, %ld failed as injected, %ld grouped batches so far: %s\n", what,
                n_ok.load(), n_hip.load(), leoec::hostq_group_batches(),
                g_errs.empty() ? "ok" : "FAILED");
  };

  set("LEOEC_HOSTQ_DONE_GROUPS", "4");
  set("LEOEC_HOSTQ_DIRECT", "0");
  set("LEOEC_HOSTQ_DIRECT_MAP", "0");
  set("LEOEC_HOSTQ_SPLIT_KIB", "0");  // every batch on the copy streams
  phase("G = 4, polled events", false);
  set("LEOEC_HOSTQ_SYNC", "2");
  phase("G = 4, blocking-sync events", false);
  set("LEOEC_HOSTQ_SYNC", "0");
  set("LEOEC_HOSTQ_WAKE", "0");
  phase("G = 4, broadcast wake-ups", false);
  set("LEOEC_HOSTQ_SYNC", "1");
  set("LEOEC_HOSTQ_WAKE", "1");
  if (leoec::hostq_group_batches() == 0) fail("no batch came back in more than one group");

  set("LEOEC_HOSTQ_FAIL_GROUP", "1");
  const long before = leoec::hostq_group_batches();
  phase("G = 4, group 1's copy fails", true);
  if (leoec::hostq_group_batches() > before && (n_hip == 0 || n_ok == 0))
    fail("injected group failure: " + std::to_string(n_ok.load()) + " ok, " +
         std::to_string(n_hip.load()) + " failed");
  if (leoec::hostq_group_batches() == before) fail("no grouped batch under the injection");
  set("LEOEC_HOSTQ_FAIL_GROUP", "-1");
  phase("G = 4, injection off again", false);
  set("LEOEC_HOSTQ_DONE_GROUPS", "1");
  const long g1 = leoec::hostq_group_batches();
  phase("G = 1", false);
  if (leoec::hostq_group_batches() != g1) fail("G = 1 launched a grouped batch");
  leoec_measure_reset_knobs();

  for (const auto& e : g_errs) std::fprintf(stderr, "ERROR %s\n", e.c_str());
  std::printf("%s\n", g_errs.empty() ? "hostq_groups: all checks held" : "hostq_groups: FAILED");
  return g_errs.empty() ? 0 : 1;
}
