// Test harness (not part of the product): the rules that steer a hunt batch by the handle's history (dicey_amd/csrc/hunt_hints.hpp)
// behind a C interface, so that `pytest -m "not gpu"` can run streams of fake batches through them.  Records cross the interface as
// arrays of 64-bit words in the order of the enums below (tests/test_hunt_hints_host.py names them in the same order).
#include "../../dicey_amd/csrc/hunt_hints.hpp"

using namespace dg;
typedef unsigned long long W;

enum { H_SHARD_CAP, H_FLAT_CAP, H_HIT_CAP, H_GENERIC, H_JOBS, H_NWIN, H_SHORT2, H_WALK, H_JOBS_BIG, H_FUSED_LEAVES, H_FETCH_HITS, H_COUNT };
enum { F_FAST1, F_FAST2, F_PACKED, F_COUNT_MODE, F_HUNT, F_BAND_VERIFY, F_SAX, F_LONG_OK, F_LONG_K, F_INDEL, F_NQ, F_NGRP, F_NXS, F_NO_FUSE, F_NO_FUSE2,
       F_NO_LONG2, F_NO_PREP_FUSION, F_DEBUG_CAPS, F_DEBUG_CAPS_VALUE, F_COUNT };
enum { A_SHARD_CAP, A_HIT_CAP, A_FLAT_REQ, A_WALK_CAP, A_FORCE_GENERIC, A_FORCE_JOBS, A_FORCE_SHORT2, A_FUSED, A_FLAT_CAP, A_GENERIC_ON, A_WALKER_ON,
       A_LONG2, A_PREP_IN, A_WITH_CTX_HITS, A_KEYS_ON, A_JOBS_ON, A_DIRECT_CTX, A_FLAT_FORM, A_VERIFY_FORM, A_NLEAF, A_NHITS, A_COUNT };
enum { S_NLEAF, S_WORST_SHARD, S_NHITS, S_OVERFLOW, S_JOBS_BIG, S_JOBS_SMALL, S_WORST_SEL, S_FUSED_LEAVES, S_N_GENERIC, S_N_NWIN, S_N_SHORT2, S_N_WALK,
       S_COUNT };

// Every field of Hints, by name: a field added to the struct does not compile here until it has a word, and with the word a row in
// the test's table of merge / publish / inherited rules.
static void get(const Hints& h, W* w) {
  const auto& [shard_cap, flat_cap, hit_cap, generic, jobs, nwin, short2, walk, jobs_big, fused_leaves, fetch_hits] = h;
  const W v[H_COUNT] = {shard_cap, flat_cap, hit_cap, generic.left, jobs.left, nwin.left, short2.left, walk, jobs_big, fused_leaves, fetch_hits};
  for (int i = 0; i < H_COUNT; ++i) w[i] = v[i];
}
static Hints hints_of(const W* w) {
  Hints h;
  h.shard_cap = (u32)w[H_SHARD_CAP];
  h.flat_cap = (u32)w[H_FLAT_CAP];
  h.hit_cap = w[H_HIT_CAP];
  h.generic.left = (u32)w[H_GENERIC];
  h.jobs.left = (u32)w[H_JOBS];
  h.nwin.left = (u32)w[H_NWIN];
  h.short2.left = (u32)w[H_SHORT2];
  h.walk = (u32)w[H_WALK];
  h.jobs_big = w[H_JOBS_BIG];
  h.fused_leaves = w[H_FUSED_LEAVES];
  h.fetch_hits = w[H_FETCH_HITS];
  return h;
}
static BatchFacts facts_of(const W* w) {
  BatchFacts f;
  f.fast1 = w[F_FAST1];
  f.fast2 = w[F_FAST2];
  f.packed = w[F_PACKED];
  f.count_mode = w[F_COUNT_MODE];
  f.hunt = w[F_HUNT];
  f.band_verify = w[F_BAND_VERIFY];
  f.sax = w[F_SAX];
  f.long_ok = w[F_LONG_OK];
  f.long_k = (u32)w[F_LONG_K];
  f.indel = w[F_INDEL];
  f.nq = w[F_NQ];
  f.ngrp = w[F_NGRP];
  f.nxs = w[F_NXS];
  f.no_fuse = w[F_NO_FUSE];
  f.no_fuse2 = w[F_NO_FUSE2];
  f.no_long2 = w[F_NO_LONG2];
  f.no_prep_fusion = w[F_NO_PREP_FUSION];
  f.debug_caps = w[F_DEBUG_CAPS];
  f.debug_caps_value = (u32)w[F_DEBUG_CAPS_VALUE];
  return f;
}
static Attempt attempt_of(const W* w) {
  Attempt a;
  a.shard_cap = (u32)w[A_SHARD_CAP];
  a.hit_cap = w[A_HIT_CAP];
  a.flat_req = (u32)w[A_FLAT_REQ];
  a.walk_cap = w[A_WALK_CAP];
  a.force_generic = w[A_FORCE_GENERIC];
  a.force_jobs = w[A_FORCE_JOBS];
  a.force_short2 = w[A_FORCE_SHORT2];
  a.fused = w[A_FUSED];
  a.flat_cap = (u32)w[A_FLAT_CAP];
  a.generic_on = w[A_GENERIC_ON];
  a.walker_on = w[A_WALKER_ON];
  a.long2 = w[A_LONG2];
  a.prep_in = w[A_PREP_IN];
  a.with_ctx_hits = w[A_WITH_CTX_HITS];
  a.keys_on = w[A_KEYS_ON];
  a.jobs_on = w[A_JOBS_ON];
  a.direct_ctx = (u32)w[A_DIRECT_CTX];
  a.flat_form = (u32)w[A_FLAT_FORM];
  a.verify_form = (u32)w[A_VERIFY_FORM];
  a.nleaf = w[A_NLEAF];
  a.nhits = w[A_NHITS];
  return a;
}
static void put(const Attempt& a, W* w) {
  const W v[A_COUNT] = {a.shard_cap, a.hit_cap, a.flat_req, a.walk_cap, a.force_generic, a.force_jobs, a.force_short2, a.fused, a.flat_cap, a.generic_on,
                        a.walker_on, a.long2, a.prep_in, a.with_ctx_hits, a.keys_on, a.jobs_on, a.direct_ctx, a.flat_form, a.verify_form, a.nleaf, a.nhits};
  for (int i = 0; i < A_COUNT; ++i) w[i] = v[i];
}
static Summary summary_of(const W* w) {
  Summary s = {};
  s.nleaf = w[S_NLEAF];
  s.worst_shard = w[S_WORST_SHARD];
  s.nhits = w[S_NHITS];
  s.overflow = w[S_OVERFLOW];
  s.jobs_big = w[S_JOBS_BIG];
  s.jobs_small = w[S_JOBS_SMALL];
  s.worst_sel = w[S_WORST_SEL];
  s.fused_leaves = w[S_FUSED_LEAVES];
  s.n_generic = w[S_N_GENERIC];
  s.n_nwin = w[S_N_NWIN];
  s.n_short2 = w[S_N_SHORT2];
  s.n_walk = w[S_N_WALK];
  return s;
}

extern "C" {

int hh_counts(int which) {  // words of a Hints, BatchFacts, Attempt, Summary record
  const int n[4] = {H_COUNT, F_COUNT, A_COUNT, S_COUNT};
  return n[which & 3];
}
unsigned hh_sticky_batches() { return STICKY_BATCHES; }
void hh_fresh_hints(W* h) { get(Hints(), h); }
void hh_fresh_attempt(W* a) { put(Attempt(), a); }

void hh_merge(W* h, const W* shared) {
  Hints x = hints_of(h);
  x.merge(hints_of(shared));
  get(x, h);
}
void hh_publish(const W* h, W* shared) {
  Hints s = hints_of(shared);
  hints_of(h).publish(s);
  get(s, shared);
}
void hh_inherited(const W* h, W* out) { get(hints_of(h).inherited(), out); }

void hh_start_caps(const W* h, const W* f, W* a) {
  Attempt at = attempt_of(a);
  start_caps(hints_of(h), facts_of(f), at);
  put(at, a);
}
// decide_attempt, then what the launch stages decide from the hints before the batch's synchronisation: the walker's list (when the
// walker runs beside a flat kernel) and the locate job kernels (not in count mode).  Returns Batch::fast2_minlen.
unsigned hh_decide(const W* h, const W* f, W* a) {
  const Hints x = hints_of(h);
  const BatchFacts bf = facts_of(f);
  Attempt at = attempt_of(a);
  decide_attempt(x, bf, at);
  if (at.generic_on && at.walker_on && (bf.fast1 || bf.fast2)) at.walk_cap = walk_list_room(x, bf, at);
  if (!bf.count_mode) at.jobs_on = jobs_wanted(x, at, false);
  put(at, a);
  return fast2_minlen(bf, at);
}
int hh_review(const W* s, const W* f, W* a, W* h) {
  Attempt at = attempt_of(a);
  Hints x = hints_of(h);
  const bool again = review_attempt(summary_of(s), facts_of(f), at, x);
  put(at, a);
  get(x, h);
  return again ? 1 : 0;
}
void hh_settle(const W* s, const W* f, const W* a, W* h) {
  Hints x = hints_of(h);
  settle_hints(summary_of(s), facts_of(f), attempt_of(a), x);
  get(x, h);
}

}  // extern "C"
