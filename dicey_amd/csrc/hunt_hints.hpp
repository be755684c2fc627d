// What a handle learnt from its earlier hunt batches, and the rules that read and write it: plain values and pure functions, no HIP.
// run_batch (hunt.hip) gathers a batch's facts, calls a rule and launches what it decided; a host harness (tests/host) runs the same
// rules on scripted and random streams of batches without a GPU.  A wrong hint costs a repeated batch, never a hit.
#pragma once
#include <algorithm>
#include <cstdint>

namespace dg {

using u32 = uint32_t;
using u64 = uint64_t;

// Shards of the leaf buffer and slices of the flat Sel region (Counters, hunt_internal.hpp): shard_cap and flat_cap below are per shard
static constexpr u32 NSHARD = 1024;

// A kernel family that a batch needed stays on for the next STICKY_BATCHES batches of the handle, so that a stream that alternates
// (chunks with and without N-containing queries, with and without repeat-rich strings) does not pay a repeated batch at every
// change (r03 advice; r04 repeats genome: 4 of 14 rotating steps ran twice).
static constexpr u32 STICKY_BATCHES = 8;
struct Sticky {
  u32 left = 0;  // batches the family stays on
  void seen(bool needed) {
    if (needed) left = STICKY_BATCHES;
    else if (left) --left;
  }
  void next_batch_at_least() { left = std::max(left, 1u); }  // an attempt found the family missing: on for the repeat and the next batch
  bool on() const { return left > 0; }
};

// Everything a handle (lane) learnt from earlier batches.  Beside each field: what merge() takes from the lanes' common record when a
// batch starts / what publish() writes to it when the batch ends.
struct Hints {
  // capacities that were enough so far: they only grow
  u32 shard_cap = 0;  // max / max            leaf slots per shard
  u32 flat_cap = 0;   // max / max            slice capacity of the flat Sel region (k_search1s, k_search2p)
  u64 hit_cap = 0;    // max / max
  // kernel families, sticky
  Sticky generic{1};  // max / latest         the kernels outside the flat search kernels (distance 2: the walker) had work
  Sticky jobs{1};     // max / latest         strings were queued for the locate job kernels
  Sticky nwin;        // per lane             the walker keeps its root split beside the flat distance-1 kernel (N-bearing strands in window mode)
  Sticky short2;      // per lane             distance 2: k_search2p's r04 body, after a batch that held queries too short for LONG2
  // sizes of the previous batch
  u32 walk = 0;          // per lane             groups listed for the walker (k_walk_list)
  u64 jobs_big = 0;      // latest / latest      repeat-rich strings (workgroup locate jobs)
  u64 fused_leaves = 0;  // latest / latest      occurring strings of a distance-1 batch in k_search1s' LDS lists (+ generic leaves)
  u64 fetch_hits = 0;    // latest if non-zero / latest   hits of the previous fetched batch (+3 %): copied to the host before the batch's synchronisation

  // what the handle's other lanes have learnt since this lane's previous batch (`shared` has been published to)
  void merge(const Hints& shared) {
    shard_cap = std::max(shard_cap, shared.shard_cap);
    flat_cap = std::max(flat_cap, shared.flat_cap);
    hit_cap = std::max(hit_cap, shared.hit_cap);
    generic.left = std::max(generic.left, shared.generic.left);
    jobs.left = std::max(jobs.left, shared.jobs.left);
    jobs_big = shared.jobs_big;
    fused_leaves = shared.fused_leaves;
    if (shared.fetch_hits) fetch_hits = shared.fetch_hits;
  }
  // for the other lanes' next batches
  void publish(Hints& shared) const {
    shared.shard_cap = std::max(shared.shard_cap, shard_cap);
    shared.flat_cap = std::max(shared.flat_cap, flat_cap);
    shared.hit_cap = std::max(shared.hit_cap, hit_cap);
    shared.generic = generic;
    shared.jobs = jobs;
    shared.jobs_big = jobs_big;
    shared.fused_leaves = fused_leaves;
    shared.fetch_hits = fetch_hits;
  }
  // What dg_index_share gives a new handle: the capacities, whether the two shared families are on, the LDS list and fetch sizes;
  // everything else starts at its default.  A family that is on is carried as one batch, one that has decayed as off — so a lane
  // created from a handle whose hint has decayed starts with the hint off whatever the lanes' common record holds at its first
  // merge (a counter of 1 in its place let max(1, 0) switch the hint back on when the record's counter was 0, and whether it was
  // depended on which thread got there first).  Results do not depend on it; the flat kernel form of that lane's first batch does.
  Hints inherited() const {
    Hints h;
    h.shard_cap = shard_cap;
    h.flat_cap = flat_cap;
    h.hit_cap = hit_cap;
    h.generic.left = generic.on() ? 1u : 0u;
    h.jobs.left = jobs.on() ? 1u : 0u;
    h.fused_leaves = fused_leaves;
    h.fetch_hits = fetch_hits;
    return h;
  }
};

// What the rules need to know of a batch (run_batch: batch_facts)
struct BatchFacts {
  bool fast1 = false, fast2 = false;  // Batch::fastK / fast2K non-zero: the batch qualifies for the flat distance-1 / distance-2 kernel
  bool packed = false;                // every neighbourhood string fits 128 bits
  bool count_mode = false;            // group counts: no locate, no verify
  bool hunt = false;                  // hits (neither sites nor counts)
  bool band_verify = false;
  bool sax = false;                   // FmView::sax: the context records are resident
  bool long_ok = false;               // the long filter is usable (its word offsets inside a copy stay below 2^32) ...
  u32 long_k = 0;                     // ... and its order
  bool indel = false;
  u64 nq = 0, ngrp = 0, nxs = 0;
  // switches (dg_switches; development builds only)
  bool no_fuse = false, no_fuse2 = false, no_long2 = false, no_prep_fusion = false, debug_caps = false;
  u32 debug_caps_value = 0;           // DICEY_DEBUG_CAPS, at least 1
};

// The state that survives a repeat of the batch, what one attempt decided, and the forms reported in the result.
struct Attempt {
  // survives a repeat (start_caps; raised by review_attempt)
  u32 shard_cap = 0;
  u64 hit_cap = 0;
  u32 flat_req = 0;  // slices of the flat Sel region asked for
  u64 walk_cap = 0;  // room of the walker's group list (k_walk_list)
  bool force_generic = false, force_jobs = false, force_short2 = false;
  // decided per attempt: by decide_attempt at its top, unless a stage is named
  bool fused = false;          // the flat search kernel settles the select stage as well
  u32 flat_cap = 0;
  bool generic_on = false;     // the generic search / select kernels run
  bool walker_on = true;       // ... k_search among them (edit distance 2 leaves it out when the handle's batches have no group for it)
  bool long2 = false;          // k_search2p's LONG2 body
  bool prep_in = false;        // k_search1s settles the `take` values too (TAKE form)
  bool with_ctx_hits = false;  // hits of the job kernels leave with their context characters
  bool keys_on = false;        // launch_search, after the WS_SELKEY reserve: this attempt's k_search1s wrote the kept strings' keys (FlatSel::key)
  bool jobs_on = false;        // launch_locate: the job kernels run (stays false in count mode, which has no locate stage)
  u32 direct_ctx = 0;          // launch_locate (needs keys_on): k_locate hands a single occurrence's context on itself
  // reported in the result, of the last attempt
  u32 flat_form = 0;    // which flat search kernel was launched: dg_hunt_result::flat_kernel_form
  u32 verify_form = 0;  // ... and which k_verify_memo instantiation: dg_hunt_result::verify_kernel_form
  u64 nleaf = 0, nhits = 0;
};

// What the host needs at the end of a batch, in 160 bytes instead of the 36 KB of sharded counters: batch_finish (hunt_select.hpp) writes
// it to pinned host memory, the host reads it after the batch's one synchronisation.  Plain data; the kernel depends on the layout.
struct Summary {
  unsigned long long nleaf, worst_shard, steps, lookups, sa_reads, win_bytes, nhits, overflow, refused, too_long, probes, worst_surv;
  unsigned long long jobs_big, jobs_small;  // repeat-rich strings queued by k_locate (workgroup / wavefront jobs)
  unsigned long long worst_sel;             // fullest slice of the flat Sel region (k_search1s)
  unsigned long long fused_leaves;          // occurring strings k_search1s kept in LDS (they never became Leaf records)
  unsigned long long n_generic;             // groups searched outside the flat distance-1 kernel (k_prepare)
  unsigned long long n_nwin;                // flag: N-bearing strands that walk in window mode (k_prepare)
  unsigned long long n_short2;              // distance 2: queries k_search2p<., true> left to the walker for their length (k_prepare)
  unsigned long long n_walk;                // groups listed for the walker (k_walk_list)
#ifdef DG_TOPK_PROFILE
  unsigned long long prof[24];
#endif
};

// The capacities the first attempt starts from: what was enough for the handle's previous batch, or an estimate from the batch's size
inline void start_caps(const Hints& h, const BatchFacts& f, Attempt& at) {
  at.shard_cap = std::max<u32>(h.shard_cap, (u32)std::max<u64>(64, (16 * f.nq + f.nxs / 8) / NSHARD));
  at.hit_cap = std::max<u64>(h.hit_cap, 4 * f.nq + 1024);
  // slices of the flat Sel region (k_search1s): what the previous batch's fullest slice needed plus a quarter — kept strings are a
  // third of the leaf estimate above, and k_locate walks every slot of the region
  at.flat_req = h.flat_cap ? h.flat_cap : at.shard_cap;
  if (f.debug_caps) {  // tests: start from tiny capacities to exercise the retry path
    at.shard_cap = f.debug_caps_value;
    at.hit_cap = f.debug_caps_value;
    at.flat_req = at.shard_cap;
  }
}

// What an attempt decides before its first launch (Attempt names the fields a stage sets later)
inline void decide_attempt(const Hints& h, const BatchFacts& f, Attempt& at) {
  // Distance 1, every string in 128 bits: k_search1s settles the select stage inside the search kernel (flat Sel region of
  // NSHARD slices).  The generic kernels (k_search for N-containing / long queries, k_explicit, scan, pack, alive, rank) run
  // when the previous batch of this handle had work for them; a batch that turns out to need them after all is repeated.
  // DICEY_NO_FUSED_SELECT: the search without the select stage (k_search1p + the generic select kernels) — what batches with
  // strings above 42 characters take anyway; the GPU tests run every distance-1 case both ways
  // r04: the same at edit distance 2 (k_search2p<true, .>: one workgroup per group or per query); DICEY_NO_FUSED_SELECT2 keeps the
  // generic select kernels for that distance only
  at.fused = (f.fast1 || (f.fast2 && !f.no_fuse2)) && f.packed && !f.no_fuse;
  at.flat_cap = at.fused ? at.flat_req : 0u;
  at.generic_on = !at.fused || h.generic.on() || f.nxs > 0 || at.force_generic;
  // edit distance 2: the walker (k_search) only serves the groups k_search2p does not take (N in the query, above 30 nt); it is
  // launched when the previous batch of the handle had such groups — 0.17 ms of the 13 ms step on batches that have none — and
  // a batch that has some after all is repeated with it, like the generic kernels at distance 1
  at.walker_on = !(f.fast2 && !h.generic.on() && !at.force_generic && f.nxs == 0);
  // distance 2: the LONG2 body of k_search2p takes queries whose shortest string still asks the long filter; the handle falls back to
  // the r04 body while its batches hold shorter ones (Hints::short2), and a batch that turns out to hold some is repeated with it
  at.long2 = f.fast2 && f.long_ok && !h.short2.on() && !at.force_short2 && !f.no_long2;
  // the whole batch on the flat distance-1 path: k_search1s settles the `take` values of its own queries (TAKE form);
  // DICEY_NO_PREP_FUSION keeps k_take a launch of its own (the GPU suite runs both)
  at.prep_in = at.fused && f.fast1 && !at.generic_on && !f.count_mode && !f.no_prep_fusion;
  at.flat_form = f.fast1 ? (at.fused ? (at.prep_in ? 3u : 2u) : 1u) : f.fast2 ? (at.fused ? 5u : 4u) + (at.long2 ? 2u : 0u) : 0u;
  // hits of the job kernels leave with their context characters (FmView::sax) when the kernel that reads the seeds is
  // k_verify_memo — the only reader that knows the encoding (HitSeed::len, devfm.hpp)
  at.with_ctx_hits = f.hunt && f.band_verify && f.sax;
  at.keys_on = at.jobs_on = false;
  at.direct_ctx = 0;
}
// Batch::fast2_minlen of the attempt: the shortest query k_search2p's LONG2 body takes
inline u32 fast2_minlen(const BatchFacts& f, const Attempt& at) { return at.long2 ? f.long_k + (f.indel ? 2u : 0u) : 0u; }

// launch_walker beside a flat kernel: room of the walker's group list — what the previous batch listed plus a quarter (a list that
// overflows repeats the batch); without a flat kernel the list simply holds every group
inline u64 walk_list_room(const Hints& h, const BatchFacts& f, const Attempt& at) {
  return std::max<u64>(at.walk_cap, (f.fast1 || f.fast2) ? std::min<u64>(f.ngrp, (u64)h.walk + h.walk / 4 + 4096) : f.ngrp);
}
// launch_locate: the job kernels run (beyond_topk: hunt -m above what k_locate_topk serves)
inline bool jobs_wanted(const Hints& h, const Attempt& at, bool beyond_topk) { return h.jobs.on() || at.force_jobs || beyond_topk; }

// Everything an attempt found wanting is put right before the batch is repeated (one repeat usually serves several causes).
// Returns whether the batch runs again.
inline bool review_attempt(const Summary& hsum, const BatchFacts& f, Attempt& at, Hints& h) {
  at.nleaf = hsum.nleaf;
  at.nhits = hsum.nhits;
  bool again = false;
  // the generic kernels were left out, and the batch had work for them after all (queries with N, longer than 31 nt, a workgroup
  // of k_search1s whose strings did not fit its LDS list): once more, with them
  if (at.fused && !at.generic_on && (hsum.nleaf > 0 || hsum.n_generic > 0)) {
    h.generic.next_batch_at_least();
    at.force_generic = true;
    again = true;
  }
  if (!at.walker_on && hsum.n_generic > 0) {  // edit distance 2: groups for the walker after all
    h.generic.seen(true);
    at.force_generic = true;
    again = true;
  }
  if (at.long2 && hsum.n_short2 > 0) {  // queries too short for the LONG2 body went to the walker (or to nobody): once more with the r04 body
    h.short2.seen(true);
    at.force_short2 = true;
    again = true;
  }
  if (!at.jobs_on && !f.count_mode && (hsum.jobs_small > 0 || hsum.jobs_big > 0)) {  // strings were queued and nobody served them
    h.jobs.next_batch_at_least();
    at.force_jobs = true;
    again = true;
  }
  const u32 worst = (u32)hsum.worst_shard;
  if (worst > at.shard_cap) {
    at.shard_cap = worst + worst / 4 + 64;
    again = true;
  }
  if (at.fused && hsum.worst_sel > at.flat_cap) {
    at.flat_req = (u32)(hsum.worst_sel + hsum.worst_sel / 4 + 64);
    again = true;
  }
  if (!(hsum.overflow & 1) && at.nhits > at.hit_cap) {  // (after a buffer overflow the hit count is not this batch's)
    at.hit_cap = at.nhits + at.nhits / 4 + 1024;
    again = true;
  }
  if (hsum.overflow & 8u) {  // the walker's group list was too short
    at.walk_cap = std::min<u64>(f.ngrp, hsum.n_walk + hsum.n_walk / 4 + 4096);
    again = true;
  }
  h.walk = (u32)std::min<u64>(hsum.n_walk, 0xFFFFFFFFull);
  return again;
}

// What the handle's next batch starts from, after the attempt that stood.
inline void settle_hints(const Summary& hsum, const BatchFacts& f, const Attempt& at, Hints& h) {
  // (a distance-2 batch without the fused select has no leaf census of its own: every leaf is the generic select kernels')
  if (at.fused || f.fast2) h.generic.seen((at.fused && hsum.nleaf > 0) || hsum.n_generic > 0 || f.nxs > 0);
  h.nwin.seen(hsum.n_nwin > 0);
  if (f.fast2 && !at.long2 && !at.force_short2) h.short2.seen(false);  // (eight batches on the r04 body, then LONG2 is tried again)
  if (!f.count_mode) h.jobs.seen(hsum.jobs_small > 0 || hsum.jobs_big > 0);
  h.shard_cap = at.shard_cap;
  if ((f.fast1 || f.fast2) && hsum.worst_sel) h.flat_cap = (u32)std::max<unsigned long long>(h.flat_cap, hsum.worst_sel + hsum.worst_sel / 4 + 64);
  h.jobs_big = hsum.jobs_big;
  if (f.fast1) h.fused_leaves = hsum.fused_leaves + at.nleaf;
  h.hit_cap = std::max<u64>(h.hit_cap, at.nhits + at.nhits / 4 + 1024);
}

}  // namespace dg
