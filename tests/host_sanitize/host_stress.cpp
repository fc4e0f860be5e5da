// Host-side stress test of the engine's C ABI under the sanitizers, TEST
// INFRASTRUCTURE ONLY (tests/test_host_sanitize.py builds it with the fake
// HIP runtime of this directory, once with -fsanitize=address,undefined and
// once with -fsanitize=thread).
//
// What runs: the plan cache (engine.cpp make_plan), the per-thread staging
// (engine.cpp Staging, zero-copy / copy forms), the batching queue
// (hostq.cpp: slots, worker, completer, per-job status) and the dispatcher
// lanes (default: the caller's device; leoec_host_spread), driven by many
// concurrent callers as the reference's NIF is (basho_bench {concurrent, 4},
// test/basho_bench_leo_erasure_rs_10_4_8_1M_w_t4.config:24;
// c_src/leo_erasure_nif.cpp:346-351).  Every result is compared with the CPU
// oracle (oracle/leoec_oracle.c).  In the measurement build
// (-DLEOEC_MEASURE) one more thread flips staging / queue knobs through
// leoec_measure_set_knob while the callers run.
//
//   host_stress [threads] [rounds]     exit 0 = every result bit-exact
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>  // the fake runtime of this directory (hipSetDevice)

#include "../../include/leoec.h"
#include "../../leo_erasure_amd/csrc/engine.hpp"  // leoec::warm_state (the warm-up's effects)
extern "C" {
#include "../../oracle/leoec_oracle.h"
}

#ifdef LEOEC_MEASURE
extern "C" int leoec_measure_set_knob(const char* name, const char* value);
extern "C" void leoec_measure_reset_knobs(void);
#endif

namespace {

struct Case {
  int coding, k, m, w;
  uint64_t size;
  std::vector<uint8_t> data, ref;  // ref: the oracle's (k+m)*bs blocks
  uint64_t bs = 0;
  int filled = 0;
};

std::mutex g_err_mu;
std::vector<std::string> g_errs;
void fail(const std::string& e) {
  std::lock_guard<std::mutex> l(g_err_mu);
  if (g_errs.size() < 20) g_errs.push_back(e);
}

std::string name(const Case& c) {
  char b[96];
  std::snprintf(b, sizeof b, "coding %d (%d,%d,%d) size %llu", c.coding, c.k, c.m, c.w,
                (unsigned long long)c.size);
  return b;
}

void prepare(Case* c, uint32_t seed) {
  std::mt19937 rng(seed);
  c->data.resize(c->size);
  for (auto& x : c->data) x = (uint8_t)rng();
  c->bs = orc_block_size(c->k, c->w, c->size);
  c->ref.assign((size_t)(c->k + c->m) * c->bs, 0);
  if (orc_encode(c->coding, c->k, c->m, c->w, c->data.data(), c->size, c->ref.data()))
    std::abort();
  uint64_t bs = 0;
  if (leoec_layout(c->coding, c->k, c->m, c->w, c->size, &bs, &c->filled) || bs != c->bs)
    std::abort();
}

const uint8_t* block(const Case& c, int id) { return c.ref.data() + (size_t)id * c.bs; }

// include/leoec.h, Conventions: a call that returned LEOEC_OK on a thread whose
// HIP last-error slot was clean leaves it clean (the engine drops the HIP
// failures it recovers from).  Every phase's threads start clean and check
// after every call; a leftover is reported once and cleared.
void slot_clean(const char* op, const Case& c) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    fail(std::string(op) + " " + name(c) + " left HIP error " + std::to_string((int)e) +
         " in the thread's last-error slot");
}

int encode_case(const Case& c) {
  const int n = c.k + c.m;
  std::vector<uint8_t> out((size_t)(n - c.filled) * c.bs + 1);
  const int rc =
      leoec_encode(c.coding, c.k, c.m, c.w, c.data.data(), c.size, out.data(), out.size());
  if (rc || std::memcmp(out.data(), block(c, c.filled), (size_t)(n - c.filled) * c.bs))
    fail("encode " + name(c) + " rc " + std::to_string(rc));
  slot_clean("encode", c);
  return rc;
}

// decode from the blocks outside `lost`, each a separate buffer, listed in reverse
int decode_case(const Case& c, const std::vector<int>& lost) {
  std::vector<int> ids;
  std::vector<const uint8_t*> ptrs;
  for (int id = c.k + c.m - 1; id >= 0; --id) {
    bool gone = false;
    for (int x : lost) gone |= x == id;
    if (!gone) {
      ids.push_back(id);
      ptrs.push_back(block(c, id));
    }
  }
  std::vector<uint8_t> out(c.size + 1);
  const int rc = leoec_decode(c.coding, c.k, c.m, c.w, ptrs.data(), ids.data(), (int)ids.size(),
                              c.bs, c.size, out.data());
  if (rc || std::memcmp(out.data(), c.data.data(), c.size))
    fail("decode " + name(c) + " rc " + std::to_string(rc));
  slot_clean("decode", c);
  return rc;
}

// encode, decode (m blocks lost, survivors listed in reverse), repair of two
// blocks; t picks the erasure pattern
void roundtrip(const Case& c, int t, bool with_repair = true) {
  const int k = c.k, m = c.m, n = k + m;
  const uint64_t bs = c.bs;
  encode_case(c);
  std::vector<int> lost;
  for (int j = 0; j < m; ++j) {
    const int id = (t * 7 + j * 3) % n;
    bool dup = false;
    for (int x : lost) dup |= x == id;
    if (!dup) lost.push_back(id);
  }
  decode_case(c, lost);
  if (with_repair) {
    const int rep[2] = {t % n, (t + 5) % n};
    const int nrep = rep[0] == rep[1] ? 1 : 2;
    std::vector<int> avail;
    std::vector<const uint8_t*> ptrs;
    for (int id = 0; id < n; ++id)
      if (id != rep[0] && id != rep[1]) {
        avail.push_back(id);
        ptrs.push_back(block(c, id));
      }
    std::vector<uint8_t> out((size_t)nrep * bs + 1);
    const int rc = leoec_repair(c.coding, k, m, c.w, ptrs.data(), avail.data(), (int)avail.size(),
                                bs, rep, nrep, out.data());
    bool ok = rc == 0;
    for (int r = 0; ok && r < nrep; ++r)
      ok = !std::memcmp(out.data() + (size_t)r * bs, block(c, rep[r]), bs);
    if (!ok) fail("repair " + name(c) + " rc " + std::to_string(rc));
    slot_clean("repair", c);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int threads = argc > 1 ? std::atoi(argv[1]) : 16;
  const int rounds = argc > 2 ? std::atoi(argv[2]) : 6;
  if (leoec_gf_init() != LEOEC_OK) {
    std::fprintf(stderr, "gf_init failed\n");
    return 2;
  }
  // the engine's batching and staging thresholds: objects around kGatherMax
  // and kBatchMaxJobBytes (8 / 16 MiB) would make the CPU kernels slow, so
  // the shapes cover the code paths at small sizes plus one 9 MiB object
  std::vector<Case> cases = {
      {LEOEC_VANDRS, 10, 4, 8, 262144},   {LEOEC_VANDRS, 10, 4, 8, 100003},
      {LEOEC_CAUCHYRS, 10, 4, 8, 80077},  {LEOEC_ISARS, 10, 4, 8, 65543},
      {LEOEC_LIBERATION, 4, 2, 7, 77777}, {LEOEC_VANDRS, 4, 2, 16, 23457},
      {LEOEC_VANDRS, 6, 3, 32, 9999},     {LEOEC_CAUCHYRS, 4, 2, 3, 5000},
      {LEOEC_VANDRS, 20, 6, 8, 200003},   {LEOEC_CAUCHYRS, 5, 3, 17, 40000},
      {LEOEC_LIBERATION, 5, 2, 5, 3001},
  };
  Case big{LEOEC_VANDRS, 10, 4, 8, (9u << 20) + 5};  // per-thread path (> the batch cap)
  for (size_t i = 0; i < cases.size(); ++i) prepare(&cases[i], 100 + (uint32_t)i);
  prepare(&big, 99);

  // phase 0: what gf_init and leoec_host_spread warm.  gf_init warms the
  // caller's device only (its batching queue and pools of streams and mapped
  // buffers); a spread set warms each of its devices before returning, so
  // no data call afterwards builds a queue (round-4 verdict item 6)
  int queues_after_warm = -1;
  {
    const leoec::WarmState w0 = leoec::warm_state(0), w1 = leoec::warm_state(1);
    if (!w0.queue || w0.pool_streams < 1 || w0.pool_mapped < 1)
      fail("gf_init left its device without queue / pools");
    if (w1.queue || w1.pool_streams || w1.pool_mapped)
      fail("device 1 warmed before any spread set named it");
    int devs[2] = {0, 1};
    if (leoec_host_spread(devs, 2) != 2) fail("leoec_host_spread({0,1}) != 2 (phase 0)");
    const leoec::WarmState a = leoec::warm_state(0), b = leoec::warm_state(1);
    if (!a.queue || !b.queue || b.pool_streams < 1 || b.pool_mapped < 1)
      fail("leoec_host_spread({0,1}) left a device without queue / pools");
    queues_after_warm = b.queues_built;
    // both devices warmed by a thread of their own, which ended (its staging
    // handed off while alive: no HIP call at its exit, tls_teardown.cpp)
    const leoec::ReclaimState r = leoec::reclaim_state();
    if (r.warm_threads_started != 2 || r.warm_threads_done != 2)
      fail("warm threads started / done: " + std::to_string(r.warm_threads_started) + " / " +
           std::to_string(r.warm_threads_done));
    if (queues_after_warm != 2) fail("queues built after warming 2 devices: " +
                                     std::to_string(queues_after_warm));
    if (leoec_host_spread(nullptr, 0) != 0) fail("leoec_host_spread reset (phase 0)");
    std::printf("warm-up: device 0 %d streams / %d mapped, device 1 %d / %d, %d queues: %s\n",
                a.pool_streams, a.pool_mapped, b.pool_streams, b.pool_mapped, b.queues_built,
                g_errs.empty() ? "ok" : "FAILED");
  }

  // phase 1: concurrent callers on the default lane (the caller's device);
  // half the threads on device 1
  auto phase = [&](const char* what, bool spread_devices) {
    std::atomic<bool> stop{false};
#ifdef LEOEC_MEASURE
    std::thread flipper([&] {
      const char* staging[] = {"auto", "gather", "pageable", "pinned", "zerocopy"};
      const char* direct[] = {"0", "4"};
      unsigned i = 0;
      while (!stop.load()) {
        leoec_measure_set_knob("LEOEC_HOST_STAGING", staging[i % 5]);
        leoec_measure_set_knob("LEOEC_HOSTQ_DIRECT", direct[i % 2]);
        leoec_measure_set_knob("LEOEC_HOSTQ_DIRECT_MAP", direct[(i / 2) % 2]);
        leoec_measure_set_knob("LEOEC_STAGE_CHUNK_KIB", i % 3 ? "16" : "256");
        leoec_measure_set_knob("LEOEC_HOSTQ_NTCOPY", (i / 3) % 2 ? "1" : "0");
        leoec_measure_set_knob("LEOEC_HOSTQ_SURVIVORS", i % 3 == 0 ? "0" : i % 3 == 1 ? "1" : "2");
        leoec_measure_set_knob("LEOEC_ZC_CHUNKS", i % 4 == 0 ? "1" : i % 4 == 1 ? "2" : i % 4 == 2 ? "3" : "8");
        // targeted / broadcast wake-ups, flipped while callers wait in both forms
        leoec_measure_set_knob("LEOEC_HOSTQ_WAKE", (i / 5) % 2 ? "0" : "1");
        leoec_measure_set_knob("LEOEC_HOSTQ_STREAMS", (i / 7) % 2 ? "0" : "1");
        leoec_measure_set_knob("LEOEC_HOSTQ_SPLIT_KIB", i % 2 ? "0" : "1024");
        leoec_measure_set_knob("LEOEC_HOSTQ_EAGER", (i / 2) % 2 ? "1" : "0");
        leoec_measure_set_knob("LEOEC_HOSTQ_SLOT_KIB", i % 3 == 0 ? "16384" : i % 3 == 1 ? "4096" : "512");
        ++i;
        std::this_thread::sleep_for(std::chrono::milliseconds(3));
      }
      leoec_measure_reset_knobs();
    });
#endif
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
      th.emplace_back([&, t] {
        if (!spread_devices && (t & 1)) hipSetDevice(1);
        for (int r = 0; r < rounds; ++r) roundtrip(cases[(size_t)(t + r) % cases.size()], t + r);
        if (t == 0) roundtrip(big, 3);
      });
    for (auto& x : th) x.join();
    stop = true;
#ifdef LEOEC_MEASURE
    flipper.join();
#endif
    std::printf("%s: %s\n", what, g_errs.empty() ? "ok" : "FAILED");
  };
  phase("callers on their own devices", false);

  // phase 2: spread over both devices (opt-in), then back to the default
  {
    int devs[2] = {0, 1};
    if (leoec_host_spread(devs, 2) != 2) fail("leoec_host_spread({0,1}) != 2");
    int bad = 7;
    if (leoec_host_spread(&bad, 1) != LEOEC_E_NO_DEVICE) fail("spread to a missing device accepted");
    phase("spread over 2 devices", true);
    if (leoec_host_spread(nullptr, 0) != 0) fail("leoec_host_spread reset");
    const int q = leoec::warm_state(0).queues_built;
    if (q != queues_after_warm)
      fail("data calls built queues after the warm-up: " + std::to_string(q));
  }

  // phase 2b: a per-thread zero-copy call (packed: its object is not on a
  // 16-byte boundary) whose second column chunk cannot
  // get its event (the n-th hipEventCreateWithFlags of the thread fails):
  // the call reports LEOEC_E_HIP having drained chunk 0, which reads and
  // writes the thread's mapped buffer, so the thread's next call — which
  // repacks that buffer — is bit-exact (under TSan an undrained chunk is a
  // data race on the buffer)
  {
    Case c{LEOEC_VANDRS, 10, 4, 8, 262144};  // bs 26,240: two 16 KiB column chunks
    prepare(&c, 31);
    Case d{LEOEC_VANDRS, 10, 4, 8, 262144};
    prepare(&d, 32);
    std::thread t([&] {
      // (the object 8 bytes past a 16-byte boundary: packed column chunks)
      std::vector<uint8_t> shifted(c.size + 32);
      uint8_t* src = shifted.data() + ((24 - ((uintptr_t)shifted.data() & 15u)) & 15u);
      std::memcpy(src, c.data.data(), c.size);
      fakehip::fail_nth_event_create(2);
      std::vector<uint8_t> out((size_t)(c.k + c.m - c.filled) * c.bs);
      const int rc = leoec_encode(c.coding, c.k, c.m, c.w, src, c.size, out.data(),
                                  out.size());
      const int left = fakehip::fail_event_create_in();
      fakehip::fail_nth_event_create(0);
      if (rc != LEOEC_E_HIP || left != 0)
        fail("injected event failure at chunk 1: rc " + std::to_string(rc) + ", " +
             std::to_string(left) + " creations short of it");
      // the failure the call reported is its own: it may stay in the slot
      // (a caller that goes on clears it, as here)
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess && e != hipErrorOutOfMemory)
        fail("injected event failure: slot holds " + std::to_string((int)e));
      for (int r = 0; r < 3; ++r) roundtrip(r == 1 ? c : d, r, false);
    });
    t.join();
    std::printf("chunk-1 event failure: %s\n", g_errs.empty() ? "ok" : "FAILED");
  }

  // phase 2c: HIP failures the engine recovers from leave nothing behind.
  // One thread, three calls, each after an injected failure that makes the
  // staging fall back to a copy form; each must return LEOEC_OK, be bit-exact
  // and leave the thread's last-error slot clean (encode_case / decode_case
  // check all three).  fake_kernels.cpp's launchers report LEOEC_E_HIP when
  // the slot is not clean, as a launcher reading the sticky slot would.
  {
    Case small{LEOEC_VANDRS, 10, 4, 8, 65543};
    // span (k + m) bs = 2.24 MiB: above the 2 MiB mapped buffers of the pool,
    // so a thread holding one has to grow it (engine.cpp zc_ready)
    Case grow{LEOEC_VANDRS, 10, 4, 8, 1677721 + 3};
    Case over{LEOEC_VANDRS, 10, 4, 8, (16u << 20) + 5};  // above the zero-copy cap
    prepare(&small, 51);
    prepare(&grow, 52);
    prepare(&over, 53);
    std::thread t([&] {
      auto unused = [](const char* what, int left) {
        if (left != 0) fail(std::string(what) + ": the injected failure was not reached");
      };
      // Where each failure lands is pinned by the order of the thread's
      // allocations in a per-thread call (engine.cpp stage_for: zc_ready's
      // mapped buffer first; then, for separate input blocks, gather_buf's
      // pinned buffer) and by counting: between arming and the check the
      // thread makes exactly the hipHostMalloc calls listed at each step,
      // the failing ones first, so no other allocation site took a failure.
      auto mallocs = [](const char* what, long before, long want) {
        const long got = fakehip::host_malloc_calls() - before;
        if (got != want)
          fail(std::string(what) + ": " + std::to_string(got) + " hipHostMalloc calls, expected " +
               std::to_string(want));
      };
      // (a) zero-copy: the thread takes a pooled mapped buffer, then needs a
      // larger one, and its hipHostMalloc fails: pageable copies instead
      encode_case(small);
      long calls = fakehip::host_malloc_calls();
      fakehip::fail_nth_host_malloc(1);
      encode_case(grow);
      unused("zc_ready hipHostMalloc", fakehip::fail_host_malloc_in());
      mallocs("zc_ready hipHostMalloc", calls, 1);
      // (b) gather: a decode from k separate survivor buffers; the mapped
      // buffer cannot be had (first failure), nor the pinned gather buffer of
      // the survivors (second, engine.cpp gather_buf in stage_h2d_segs): one
      // pageable copy each.  The four rebuilt blocks then come back through
      // gather_buf again (stage_d2h_sync_impl), whose allocation succeeds:
      // the third and last hipHostMalloc of the call
      calls = fakehip::host_malloc_calls();
      fakehip::fail_nth_host_malloc(1, 2);
      decode_case(grow, {0, 3, 7, 9});
      unused("gather_buf hipHostMalloc", fakehip::fail_host_malloc_in());
      mallocs("zc_ready + gather_buf hipHostMalloc", calls, 3);
      // (c) a call above the cap after a small call whose mapped buffer got
      // no device address (zc_ready's hipHostGetDevicePointer, the only one a
      // data call makes; its one hipHostMalloc before it succeeds)
      calls = fakehip::host_malloc_calls();
      fakehip::fail_nth_host_get_device_pointer(1);
      encode_case(grow);
      unused("zc_ready hipHostGetDevicePointer", fakehip::fail_host_get_device_pointer_in());
      mallocs("zc_ready hipHostGetDevicePointer", calls, 1);
      decode_case(over, {2});
      fakehip::fail_nth_host_malloc(0);
      fakehip::fail_nth_host_get_device_pointer(0);
    });
    t.join();
    std::printf("recovered HIP failures: %s\n", g_errs.empty() ? "ok" : "FAILED");
  }

  // phase 3: plan-cache churn: every 4-erasure pattern of vandrs(10,4,8)
  // from 4 threads, and bitmatrix plans (cauchyrs w = 17) large enough to
  // cross the cache's byte bound
  {
    Case c{LEOEC_VANDRS, 10, 4, 8, 4096};
    prepare(&c, 7);
    Case cb{LEOEC_CAUCHYRS, 24, 8, 20, 24 * 20 * 16 * 2};
    prepare(&cb, 8);
    std::vector<std::thread> th;
    for (int t = 0; t < 4; ++t)
      th.emplace_back([&, t] {
        int idx = 0;
        for (int a = 0; a < 14; ++a)
          for (int b = a + 1; b < 14; ++b)
            for (int d = b + 1; d < 14; ++d)
              for (int e = d + 1; e < 14; ++e, ++idx) {
                if (idx % 4 != t) continue;
                std::vector<int> ids;
                std::vector<const uint8_t*> ptrs;
                for (int id = 0; id < 14; ++id)
                  if (id != a && id != b && id != d && id != e) {
                    ids.push_back(id);
                    ptrs.push_back(block(c, id));
                  }
                std::vector<uint8_t> out(c.size);
                const int rc = leoec_decode(c.coding, 10, 4, 8, ptrs.data(), ids.data(), 10, c.bs,
                                            c.size, out.data());
                if (rc || std::memcmp(out.data(), c.data.data(), c.size))
                  fail("pattern decode rc " + std::to_string(rc));
                slot_clean("pattern decode", c);
              }
        for (int r = 0; r < 40; ++r) {
          // distinct lost pairs of the 32-block cauchyrs code: distinct plans
          const int x = (t * 40 + r) % 32, y = (t * 40 + r * 7 + 1) % 32;
          if (x == y) continue;
          std::vector<int> avail;
          std::vector<const uint8_t*> ptrs;
          for (int id = 0; id < 32; ++id)
            if (id != x && id != y) {
              avail.push_back(id);
              ptrs.push_back(block(cb, id));
            }
          const int rep[2] = {x, y};
          std::vector<uint8_t> out(2 * cb.bs);
          const int rc = leoec_repair(cb.coding, 24, 8, 20, ptrs.data(), avail.data(),
                                      (int)avail.size(), cb.bs, rep, 2, out.data());
          if (rc || std::memcmp(out.data(), block(cb, x), cb.bs) ||
              std::memcmp(out.data() + cb.bs, block(cb, y), cb.bs))
            fail("bitmatrix repair rc " + std::to_string(rc));
          slot_clean("bitmatrix repair", cb);
        }
      });
    for (auto& x : th) x.join();
    std::printf("plan cache churn: %s\n", g_errs.empty() ? "ok" : "FAILED");
  }

  // phase 4: objects whose span is above the zero-copy cap (16 MiB): the
  // per-thread copy path (pageable copies, or the gather buffer for the
  // survivors), 3 threads on the SAME object and blocks
  {
    Case large{LEOEC_VANDRS, 10, 4, 8, (17u << 20) + 5};
    prepare(&large, 12);
    std::vector<std::thread> th;
    // (repair is left out: its span of k + 2 blocks stays under the cap)
    for (int t = 0; t < 3; ++t) th.emplace_back([&, t] { roundtrip(large, t, false); });
    for (auto& x : th) x.join();
    std::printf("large objects: %s\n", g_errs.empty() ? "ok" : "FAILED");
  }

  // phase 5: threads that come and go.  Each exiting caller thread hands its
  // staging off with no HIP call (the fake runtime aborts on one from a
  // thread_local destructor); a live thread's next call frees it.  Nothing a
  // thread hands off may still be in flight (engine.cpp Reclaim invariant).
  {
    Case c{LEOEC_VANDRS, 10, 4, 8, 262144};
    prepare(&c, 41);
    const long before = leoec::reclaim_state().handed_off;
    for (int wave = 0; wave < 4; ++wave) {
      std::vector<std::thread> th;
      for (int t = 0; t < 6; ++t)
        th.emplace_back([&, t] {
          if (t & 1) hipSetDevice(1);
          roundtrip(c, wave + t, false);
        });
      for (auto& x : th) x.join();
    }
    roundtrip(c, 1, false);  // a live thread's call drains the list
    const leoec::ReclaimState r = leoec::reclaim_state();
    std::printf("thread exits: %ld stagings handed off (%ld this phase), %ld freed, %ld busy\n",
                r.handed_off, r.handed_off - before, r.drained, r.busy);
    if (r.handed_off - before < 24) fail("exited threads handed off fewer stagings than threads");
    if (r.drained != r.handed_off) fail("handed-off stagings left undrained by a live call");
    if (r.busy != 0) fail("a thread exited with work in flight or pins held");
    std::printf("thread exits: %s\n", g_errs.empty() ? "ok" : "FAILED");
  }

  for (const auto& e : g_errs) std::fprintf(stderr, "ERROR %s\n", e.c_str());
  std::printf("%s\n", g_errs.empty() ? "host_stress: all results bit-exact" : "host_stress: FAILED");
  return g_errs.empty() ? 0 : 1;
}
