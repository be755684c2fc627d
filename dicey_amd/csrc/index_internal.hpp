// The object behind the opaque dg_index handle.
#pragma once
#include <mutex>
#include <string>
#include <atomic>
#include "common.hpp"
#include "devfm.hpp"
#include "experiments.hpp"
#include "hunt_hints.hpp"

namespace dg {
// dg_index::ws: the grow-only batch workspaces (hunt.hip / seam.hip / search.hip)
enum WsSlot { WS_QB = 0, WS_QOFF, WS_FW, WS_RV, WS_QSEQ, WS_QMETA, WS_LEAF, WS_LEAFG, WS_SEL, WS_GRP, WS_MISC, WS_SEEDS, WS_HITS, WS_ALN, WS_CUM, WS_SCR, WS_JOBS, WS_DP, WS_PRIM, WS_GINFO, WS_XS, WS_OPS, WS_PACK, WS_CAP, WS_WALK, WS_SELKEY, WS_COUNT };
// dg_index::ev: the events run_batch records on the lane's stream, in stream order except EV_FLAT_END (behind the flat search kernel)
enum BatchEvent : int { EV_BEGIN = 0, EV_PREPARED, EV_SEARCHED, EV_GROUPS_SCANNED, EV_SELECTED, EV_HITS_SCANNED, EV_LOCATED, EV_END, EV_FLAT_END, EV_COUNT };
}  // namespace dg

// Test / development switches of the hunt pipeline (environment variables).  Read ONCE per batch, on the thread that calls the
// library (the submitting thread for dg_hunt_submit batches) — never on the lanes' helper threads, where getenv would race with a
// host process that writes its environment — and carried to run_batch in the handle.
struct dg_switches {
  bool host_timing = false, no_band = false, cap_host = false, no_fuse = false, no_fuse2 = false, no_prep_fusion = false, no_pre5_d2 = false;
  bool debug_caps = false, no_flat_ham2 = false, no_nwin = false, no_long2 = false, no_direct_ctx = false;
  uint32_t fused_lcap = 0;       // DICEY_FUSED_LCAP (0 = unset)
  int verify_ch = 0;             // DICEY_VERIFY_CH
  uint64_t cap_budget_mb = 0;    // DICEY_CAP_BUDGET_MB (0 = unset)
  unsigned host_threads = 0;     // DICEY_HOST_THREADS (0 = unset)
  uint32_t exp_bits = 0;         // DICEY_EXP: measurement aid, phases of k_search1s switched off (results are then wrong)
  std::string dump_jobs, debug_caps_s;
  static dg_switches read();     // hunt.hip
};

struct dg_index {
  int device = 0;
  hipStream_t stream = nullptr;
  dg::FmView view;
  std::vector<void*> owned;  // device allocations that live as long as the index
  uint32_t sigma = 0;
  uint32_t code_len[256] = {0};
  uint64_t file_bytes = 0, hbm_bytes = 0;
  double load_seconds = 0, derive_seconds = 0;
  // The one place where a device block becomes the index's: released by ~dg_index on `stream`, counted in hbm_bytes.
  void adopt(void* p, size_t bytes) {  // a block a stage made complete before it handed it over (index.hip: a prefix level)
    owned.push_back(p);
    hbm_bytes += bytes;
  }
  int own(void** p, size_t bytes) {
    DG_HIP(dg::big_alloc(p, bytes, stream));
    adopt(*p, bytes);
    return DG_OK;
  }
  bool try_own(void** p, size_t bytes) {  // the optional blocks: false, *p null and HIP's sticky error cleared when there is no room
    if (dg::big_alloc(p, bytes, stream) == hipSuccess) {
      adopt(*p, bytes);
      return true;
    }
    (void)hipGetLastError();
    *p = nullptr;
    return false;
  }
  // grow-only batch workspaces (see hunt.hip / seam.hip for the slot meaning)
  dg::DevBuf ws[dg::WS_COUNT];
  hipEvent_t ev[dg::EV_COUNT] = {nullptr};
  dg::Hints hints;  // what the handle learnt from its earlier hunt batches (hunt_hints.hpp; hunt.hip run_batch)
  // dg_hunt_device: the (offsets pointer, count, bytes) of the previous call and the longest query it held; a repeated
  // call skips reading the offsets back, and k_prepare reports any query longer than this bound (hunt.hip)
  // (r04: a small table, not one entry — a caller that cycles through a ring of resident batches finds each of them again)
  struct QoffSeen {
    const void* qoff = nullptr;
    uint64_t nq = 0, total = 0;
    uint32_t maxlen = 0;
  };
  static constexpr int NSEEN = 32;
  QoffSeen seen[NSEEN];
  uint32_t seen_next = 0;
  void* pinned = nullptr;             // 4 KB of pinned host memory for the end-of-batch summary
  // the batch counters are left zeroed by the last kernel of a batch (hunt.hip batch_finish): the next batch skips its memset
  // when they still sit where that kernel cleaned them
  std::atomic<bool> busy{false};      // a dg_hunt_submit batch is in flight on this handle (lane)
  dg_switches sw;                     // the switches of the batch this handle (lane) runs; set by the entry point on the caller's thread
  std::mutex lanes_mu;                // guards the lazy creation of lanes[] / shared_hints / a lane's worker (concurrent submitters)
  // ABI 5: dg_hunt_submit keeps several batches in flight on one handle; a submission that finds the handle busy runs on an internal
  // lane (a shared handle: own stream, workspaces, helper thread; created at the first need, closed with the handle)
#ifndef DG_NEXTRA
#define DG_NEXTRA 2
#endif
  static constexpr int NEXTRA = DG_NEXTRA;    // internal lanes beside the handle itself: 1 + NEXTRA batches in flight.  r05, same box (tools/r05_call13.sh): 3 in flight
                                              // 0.178-0.184 ms per step at distance 1, 4: 0.193-0.195, 5: 0.186, 6: 0.181; distance 2: 6.14-6.61 / 6.34-6.68 / - / 6.05-6.31
  dg_index* lanes[NEXTRA] = {};
  // The lanes learn together (r04): capacities and kernel-family hints live per lane (each lane's batches read and write its own
  // without locks), and a lane merges the pair's common record in when a batch starts and writes its own back when it ends — a
  // lane that runs its first batch does not repeat it for a capacity another lane has already learnt.
  struct SharedHints {
    std::mutex mu;
    dg::Hints h;         // Hints::publish writes it, Hints::merge reads it ...
    bool valid = false;  // ... once a lane has published
    // the lanes' common timeline (dg_hunt_result::t_search_*): two base events used in turn, a new one every few seconds
    hipEvent_t ev_base[2] = {nullptr, nullptr};
    uint32_t base_gen = 0;
    double base_host_us = 0;
  };
  // owned by the handle that owns the internal lanes, which point at the same record; atomic: created by the submitting thread while the first
  // lane's helper thread may be finishing a batch
  std::atomic<SharedHints*> shared_hints{nullptr};
  struct Worker;                      // the helper thread that drives dg_hunt_submit batches (hunt.hip)
  Worker* worker = nullptr;
  void stop_worker();
  bool any_lane_busy() {              // a dg_hunt_submit batch is in flight on the handle or one of its lanes
    if (busy.load()) return true;
    std::lock_guard<std::mutex> lk(lanes_mu);
    for (dg_index* l : lanes)
      if (l && l->busy.load()) return true;
    return false;
  }
  const void* ctr_clean = nullptr;
  unsigned long long ctr_clean_gen = 0;
  std::vector<uint64_t> cum_cache;    // cumulative sequence starts currently resident in WS_CUM
  ~dg_index();
};

namespace dg {
// build.hip: sa = inverse permutation of isa by a radix sort of (isa[p], p); isa is clobbered
int derive_sa_by_sort(hipStream_t st, u32* isa, u64 n, u32* sa);
}
