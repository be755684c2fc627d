// The data of run_batch (hunt.hip, the only includer): what is fixed for a batch and how its workspaces are carved up (what one
// attempt decides and what survives a repeat: Attempt, hunt_hints.hpp).  The functions that use them are in hunt.hip, in the order a batch runs them.
#pragma once
#include <type_traits>

#include "hunt_internal.hpp"
#include "hunt_search.hpp"
#include "hunt_select.hpp"

namespace dg {

// f(std::bool_constant<on>{}) / f(std::integral_constant<u32, v>{}): the kernels are templates on what the host decides per batch, and
// a generic lambda names the launch once.  with_value: the LAST of the listed values serves every value not listed.
template <class F>
static inline void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
template <u32 V0, u32... Vs, class F>
static inline void with_value(u32 v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<u32, V0>{});
  else if (v == V0) f(std::integral_constant<u32, V0>{});
  else with_value<Vs...>(v, f);
}

// What is fixed for the whole batch (make_plan): the call and what follows from it alone.
struct BatchPlan {
  const dg_hunt_params* p;
  u32 nseq;
  const void* d_qbytes;
  const void* d_qoff;
  size_t nq;
  u64 total;
  u32 maxlen;
  // the caller's host copy of the offsets (nullptr on the dg_hunt_device path).  The cap stage's read-back serves cap_scan only and must
  // not outlive it: queue_fetch and the result's qoff distinguish "the caller has the offsets" from "pack them on the device" by this.
  const uint64_t* caller_qoff;
  // the mode: search sites (sx), count per group (group_counts), or hits (neither: `hunt`); fetch: hits to the host as well
  SearchExtra* sx;
  uint64_t* group_counts;
  int fetch;
  bool hunt;  // !sx && !group_counts
  bool indel;
  u32 dmax_eff;
  u64 ngrp;
  bool packed;  // every neighbourhood string fits 128 bits
  // Alignment rows.  The banded verify writes a row front to back, and a row it keeps has the query's characters plus at most d
  // gap columns inside the query (leading and trailing query-gap columns are stripped, hunter.h:391-401, and an optimal path has
  // score >= -d): maxlen + d bytes, rounded up to the 64-bit words it stores.  The other verify kernels build the row from the
  // end of a buffer twice as long.  (r02: 56 -> 24 bytes per row for 20-mers — what travels to the host and over xGMI.)
  bool band_verify;
  u32 stride;       // scratch rows of the full-matrix kernels (built from the end of a buffer twice the row length); the banded kernel needs none
  u32 ops_per_hit;  // compact alignment description: at most |score| <= d columns are not a match
  // ABI 5: results as compact records (position, meta, ops) + one word per query, in ONE device block [qhits | qinfo | records]
  // that a single copy brings to the host — no pack kernel, 12 instead of 24 bytes per hit at distance 1
  bool compact;
  u32 chit_words;
  // HIP events between the stages (ms_select / ms_locate / ms_verify of the result) only on request: every record is a marker packet
  // the next kernel waits behind; the batch's total and the flat search kernel's time are always measured (four events)
  bool phase_events;
  u64 scan_tmp;
};

// WS_XS: [qmode | explicit patterns' codes | their offsets | their groups], for nbytes codes in nstrings patterns
struct XsLayout {
  u64 o_bytes, o_off, o_gid, bytes;
  XsLayout(u64 nq, u64 nbytes, u64 nstrings)
      : o_bytes((nq + 63) & ~63ull), o_off(o_bytes + ((nbytes + 63) & ~63ull)), o_gid(o_off + (nstrings + 1) * 8), bytes(o_gid + nstrings * 4 + 64) {}
};

// WS_CAP (k_cap_enum): [two hash tables per workgroup | two event arrays per workgroup | job list | allocator word and status]
struct CapLayout {
  u32 tcap_log2, evcap;
  u64 o_tab, o_ev, o_jobs, o_alloc, bytes;
  // table slots: twice the number of DISTINCT strings a strand can hold (neighbourhood_bound; 15 705 for a 25-mer at distance 2
  // against 20 201 leaves) — 512 KB per strand instead of 1 MB for 25-mers
  CapLayout(u32 nwg, u32 njobs, u64 leaves, u64 distinct) {
    tcap_log2 = 8;
    while ((1ull << tcap_log2) < 2 * distinct) ++tcap_log2;
    evcap = (u32)((leaves + 2 + 63) & ~63ull);
    o_tab = 0;
    o_ev = o_tab + (u64)nwg * 2 * (16ull << tcap_log2);
    o_jobs = o_ev + (u64)nwg * 2 * evcap * 4;
    o_alloc = (o_jobs + (u64)njobs * 4 + 63) & ~63ull;
    bytes = o_alloc + 64;
  }
};
struct CapAlloc {  // the word k_cap_enum allocates patterns from (strings << 36 | bytes) and its status
  unsigned long long alloc;
  u32 status, pad;
};

// What the cap stage leaves: the explicit patterns on the device (nullptr: no query of the batch was looked at) and its report
struct CapResult {
  u8* d_qmode = nullptr;
  u8* d_xs_bytes = nullptr;
  u64* d_xs_off = nullptr;
  u32* d_xs_gid = nullptr;
  u64 nxs = 0;
  u64 dev_queries = 0;  // enumerated by k_cap_enum
  u64 looked_at = 0;    // enumerated on the host
  double ms_cap = 0.0;
};

// WS_GRP: [grp_off | hit_off | scan_buf | (to 64 bytes) Counters | grp_cnt | nsel | selbase | qhits].  Counters, group counts and
// selection counts sit next to each other: one memset (zero_from, zero_bytes) clears them.  Offsets, not pointers: the base is a
// hipMalloc block, aligned far beyond the 64 bytes the counters ask for.
struct GrpLayout {
  u64 o_grp_off, o_hit_off, o_scan, o_ctr, o_grp_cnt, o_nsel, o_selbase, o_qhits, o_end;
  GrpLayout(u64 nq, u64 ngrp, u64 scan_tmp) {
    o_grp_off = 0;
    o_hit_off = o_grp_off + (ngrp + 1) * 8;
    o_scan = o_hit_off + (nq + 1) * 8;
    o_ctr = (o_scan + scan_tmp * 8 + 63) & ~63ull;
    o_grp_cnt = o_ctr + ((sizeof(Counters) + 63) & ~(u64)63);
    o_nsel = o_grp_cnt + ngrp * 4;
    o_selbase = o_nsel + ngrp * 4;  // first Sel slot of the groups k_search1s serves (set by k_prepare / k_search1s)
    o_qhits = o_selbase + ngrp * 4;  // (compact results: qhits is re-pointed into the compact block, per attempt)
    o_end = o_qhits + nq * 4;
  }
  u64 bytes() const { return o_end + sizeof(Summary) + 512; }
  u64 zero_bytes() const { return o_selbase - o_ctr; }
  template <class T>
  static T* at(void* base, u64 off) {
    return (T*)((u8*)base + off);
  }
  u64* grp_off(void* base) const { return at<u64>(base, o_grp_off); }
  u64* hit_off(void* base) const { return at<u64>(base, o_hit_off); }
  u64* scan_buf(void* base) const { return at<u64>(base, o_scan); }
  u8* zero_from(void* base) const { return at<u8>(base, o_ctr); }
  Counters* ctr(void* base) const { return at<Counters>(base, o_ctr); }
  u32* grp_cnt(void* base) const { return at<u32>(base, o_grp_cnt); }
  u32* nsel(void* base) const { return at<u32>(base, o_nsel); }
  u32* selbase(void* base) const { return at<u32>(base, o_selbase); }
  u32* qhits(void* base) const { return at<u32>(base, o_qhits); }
};

// Fetched results: one pinned block from the pool (pageable copies run at a fraction of the link's speed, and a fresh
// hipHostMalloc per batch costs more than the copies), laid out for `capn` hits:
// [hit_off | qoff | qdistance qflags qnondna | qseq | hits | ops].  When the previous fetched batch on this handle tells how many
// hits to expect, the copies are queued BEHIND the batch's kernels, before its one synchronisation (no second round trip);
// a batch with more hits than expected copies again after the synchronisation.
struct FetchLayout {
  u64 o_hit_off, o_qoff, o_meta, o_qseq, o_hits, o_ops, bytes;
  FetchLayout(const BatchPlan& plan, u64 capn) {
    const u64 nq = plan.nq;
    o_hit_off = 0;
    o_qoff = o_hit_off + (nq + 1) * 8;
    if (plan.compact) {  // [hit_off (filled on the host) | qhits | qinfo | records]; o_qoff = qhits, o_meta = qinfo, o_hits = records
      o_meta = o_qoff + nq * 4;
      o_qseq = o_meta + nq * 4;
      o_hits = o_qseq;
      o_ops = o_hits + capn * (u64)plan.chit_words * 4;
      bytes = o_ops + 64;
      return;
    }
    o_meta = o_qoff + (nq + 1) * 8;
    o_qseq = o_meta + 3 * nq * 4;
    o_hits = (o_qseq + plan.total + 15) & ~15ull;
    o_ops = (o_hits + capn * sizeof(dg_hit) + 15) & ~15ull;
    bytes = o_ops + capn * (u64)plan.ops_per_hit * 4 + 64;
  }
};

// The batch's device pointers: the fixed ones (init_batch), and the ones an attempt's capacities move (reserve_attempt)
struct BatchBufs {
  Batch b;
  u64 nxs = 0;
  BatchFacts facts;  // what the rules of hunt_hints.hpp read of the batch (init_batch)
  u64 *grp_off, *hit_off, *scan_buf;
  Counters* ctr;
  u32 *grp_cnt, *nsel, *selbase;
  Summary* hsum;  // the pinned host record k_summary_block writes
  // per attempt
  u64 leaf_slots = 0, flat_slots = 0;
  Sel* sel_all = nullptr;
  Sel* sel_gen = nullptr;  // the generic path's slots: grp_off based, behind the flat region
  u32 job_shard_cap = 0;
  u32* qhits = nullptr;
  u32* d_chits = nullptr;
  WalkList kl{nullptr, nullptr, 0u};  // the strands of k_nkeep (k_walk_list), set by launch_search
};

}  // namespace dg
