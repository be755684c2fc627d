"""The rules that steer a hunt batch by what its handle ran before (dicey_amd/csrc/hunt_hints.hpp), on the host: the header's own
functions behind tests/host/libhintshost.so, driven by fake batches.

A batch kind fixes what the kernels would report: the groups for the generic kernels, the leaves those kernels write, the short
strings, the N windows, the small and big locate jobs, the fullest shard and slice, the hits and the walker's groups.  The Summary
of an attempt follows from the kind and the attempt's flags (summary_of): leaves and shard counts only when the generic kernels
ran, n_short2 only under LONG2, the slice only under the fused select, overflow bit 1 when a shard exceeds shard_cap, bit 8 when
the walker's list is too short.

Held against: the schedules of test_gpu_handle_history.py (exact here: forms and repeats), the capacity formulas of every retry
cause, a model of the rules as they stood before Hints existed (bools beside the sticky counters, the fields listed by hand in pull,
push and share: class Before) on seeded random streams of batches on one handle and on two and three lanes, and a table of what
merge, publish and inherited do with every field."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

H = ["shard_cap", "flat_cap", "hit_cap", "generic", "jobs", "nwin", "short2", "walk", "jobs_big", "fused_leaves", "fetch_hits"]
F = ["fast1", "fast2", "packed", "count_mode", "hunt", "band_verify", "sax", "long_ok", "long_k", "indel", "nq", "ngrp", "nxs", "no_fuse", "no_fuse2",
     "no_long2", "no_prep_fusion", "debug_caps", "debug_caps_value"]
A = ["shard_cap", "hit_cap", "flat_req", "walk_cap", "force_generic", "force_jobs", "force_short2", "fused", "flat_cap", "generic_on", "walker_on",
     "long2", "prep_in", "with_ctx_hits", "keys_on", "jobs_on", "direct_ctx", "flat_form", "verify_form", "nleaf", "nhits"]
S = ["nleaf", "worst_shard", "nhits", "overflow", "jobs_big", "jobs_small", "worst_sel", "fused_leaves", "n_generic", "n_nwin", "n_short2", "n_walk"]
NSHARD = 1024
STICKY = 8
LONG_K = 10
W = C.c_ulonglong


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host")])
    L = C.CDLL(os.path.join(HERE, "host", "libhintshost.so"))
    assert [L.hh_counts(i) for i in range(4)] == [len(H), len(F), len(A), len(S)]
    assert L.hh_sticky_batches() == STICKY
    return L


def words(names, d):
    return (W * len(names))(*[int(d[k]) for k in names])


def record(names, w):
    return dict(zip(names, w))


# ------------------------------------------------------------------------------------------------------------------- fake batches

def kind(dist=1, nq=300, count=False, packed=True, nxs=0, n_generic=0, leaves=0, n_short=0, n_nwin=0, jobs_small=0, jobs_big=0, worst_shard=0,
         worst_sel=20, nhits=400, n_walk=0, fused_leaves=500, fetch=False, **switches):
    return dict(dist=dist, nq=nq, count=count, packed=packed, nxs=nxs, n_generic=n_generic, leaves=leaves, n_short=n_short, n_nwin=n_nwin,
                jobs_small=jobs_small, jobs_big=jobs_big, worst_shard=worst_shard, worst_sel=worst_sel, nhits=nhits, n_walk=n_walk,
                fused_leaves=fused_leaves, fetch=fetch, switches=switches)


def facts_of(k, long_ok):
    f = dict.fromkeys(F, 0)
    f.update(fast1=k["dist"] == 1, fast2=k["dist"] == 2, packed=k["packed"], count_mode=k["count"], hunt=not k["count"], band_verify=1, sax=1,
             long_ok=long_ok, long_k=LONG_K, indel=1, nq=k["nq"], ngrp=2 * k["nq"], nxs=k["nxs"])
    f.update(k["switches"])
    return f


def summary_of(k, f, at):
    """what the kernels of an attempt with these flags report for a batch of this kind"""
    s = dict.fromkeys(S, 0)
    gen = at["generic_on"]
    s["n_generic"] = k["n_generic"]
    s["n_nwin"] = k["n_nwin"]
    s["nleaf"] = k["leaves"] if gen else 0
    s["worst_shard"] = k["worst_shard"] if gen else 0
    s["n_short2"] = k["n_short"] if at["long2"] else 0
    s["worst_sel"] = k["worst_sel"] if at["fused"] else 0
    s["fused_leaves"] = k["fused_leaves"] if at["fused"] and f["fast1"] else 0
    if not k["count"]:
        s["jobs_small"], s["jobs_big"], s["nhits"] = k["jobs_small"], k["jobs_big"], k["nhits"]
    if s["worst_shard"] > at["shard_cap"]:
        s["overflow"] |= 1
    if gen and at["walker_on"] and (f["fast1"] or f["fast2"]):  # the walker beside a flat kernel: its groups go through the list
        s["n_walk"] = k["n_walk"]
        if s["n_walk"] > at["walk_cap"]:
            s["overflow"] |= 8
    return s


# ---------------------------------------------------------------------------------------------------------- the header's rules

class Rules:
    """one handle (lane) on the header's rules"""

    def __init__(self, L, long_ok=True, hints=None):
        self.L, self.long_ok = L, long_ok
        self.h = (W * len(H))()
        if hints is None:
            L.hh_fresh_hints(self.h)
        else:
            self.h[:] = hints

    def hints(self):
        return record(H, self.h)

    def begin(self, k):
        self.f = facts_of(k, self.long_ok)
        self.fw = words(F, self.f)
        self.a = (W * len(A))()
        self.L.hh_fresh_attempt(self.a)
        self.L.hh_start_caps(self.h, self.fw, self.a)

    def decide(self):
        self.minlen = self.L.hh_decide(self.h, self.fw, self.a)
        return record(A, self.a)

    def review(self, s):
        self.sw = words(S, s)
        return bool(self.L.hh_review(self.sw, self.fw, self.a, self.h)), record(A, self.a)

    def settle(self, k):
        self.L.hh_settle(self.sw, self.fw, self.a, self.h)
        if k["fetch"] and not k["count"]:  # fill_result_host
            n = self.a[A.index("nhits")]
            self.h[H.index("fetch_hits")] = n + n // 32 + 1024

    def share(self):
        out = (W * len(H))()
        self.L.hh_inherited(self.h, out)
        return Rules(self.L, self.long_ok, out)

    def merge(self, shared):
        if shared["valid"]:
            self.L.hh_merge(self.h, shared["new"])

    def publish(self, shared):
        self.L.hh_publish(self.h, shared["new"])


# -------------------------------------------------------------------------------------- the rules before Hints, bools included

class Before:
    """start_caps, decide_attempt (with the walker's list and the job kernels' switch of the launch stages), review_attempt,
    settle_hints, pull_shared_hints, push_shared_hints and dg_index_share as they stood on fourteen loose fields of the handle"""

    def __init__(self, long_ok=True):
        self.long_ok = long_ok
        self.flat_cap_hint = self.shard_cap_hint = self.hit_cap_hint = 0
        self.generic_hint = self.jobs_hint = True
        self.walk_hint = self.nwin_sticky = self.short2_sticky = 0
        self.generic_sticky = self.jobs_sticky = 1
        self.jobs_big_hint = self.fused_leaves_hint = self.fetch_hits_hint = 0

    def hints(self):
        return dict(shard_cap=self.shard_cap_hint, flat_cap=self.flat_cap_hint, hit_cap=self.hit_cap_hint, generic=self.generic_sticky,
                    jobs=self.jobs_sticky, nwin=self.nwin_sticky, short2=self.short2_sticky, walk=self.walk_hint, jobs_big=self.jobs_big_hint,
                    fused_leaves=self.fused_leaves_hint, fetch_hits=self.fetch_hits_hint)

    def begin(self, k):
        f = self.f = facts_of(k, self.long_ok)
        at = self.at = dict.fromkeys(A, 0)
        at["walker_on"] = 1
        at["shard_cap"] = max(self.shard_cap_hint, max(64, (16 * f["nq"] + f["nxs"] // 8) // NSHARD))
        at["hit_cap"] = max(self.hit_cap_hint, 4 * f["nq"] + 1024)
        at["flat_req"] = self.flat_cap_hint if self.flat_cap_hint else at["shard_cap"]
        if f["debug_caps"]:
            at["shard_cap"] = at["hit_cap"] = at["flat_req"] = f["debug_caps_value"]

    def decide(self):
        f, at = self.f, self.at
        at["fused"] = (f["fast1"] or (f["fast2"] and not f["no_fuse2"])) and f["packed"] and not f["no_fuse"]
        at["flat_cap"] = at["flat_req"] if at["fused"] else 0
        at["generic_on"] = not at["fused"] or self.generic_hint or f["nxs"] > 0 or at["force_generic"]
        at["walker_on"] = not (f["fast2"] and not self.generic_hint and not at["force_generic"] and f["nxs"] == 0)
        at["long2"] = f["fast2"] and f["long_ok"] and not self.short2_sticky and not at["force_short2"] and not f["no_long2"]
        self.minlen = f["long_k"] + (2 if f["indel"] else 0) if at["long2"] else 0
        at["prep_in"] = at["fused"] and f["fast1"] and not at["generic_on"] and not f["count_mode"] and not f["no_prep_fusion"]
        if f["fast1"]:
            at["flat_form"] = (3 if at["prep_in"] else 2) if at["fused"] else 1
        elif f["fast2"]:
            at["flat_form"] = (5 if at["fused"] else 4) + (2 if at["long2"] else 0)
        else:
            at["flat_form"] = 0
        at["with_ctx_hits"] = f["hunt"] and f["band_verify"] and f["sax"]
        at["keys_on"] = at["jobs_on"] = at["direct_ctx"] = 0
        if at["generic_on"] and at["walker_on"] and (f["fast1"] or f["fast2"]):  # launch_walker
            at["walk_cap"] = max(at["walk_cap"], min(f["ngrp"], self.walk_hint + self.walk_hint // 4 + 4096))
        if not f["count_mode"]:  # launch_locate
            at["jobs_on"] = self.jobs_hint or at["force_jobs"]
        return {k: int(v) for k, v in at.items()}

    def review(self, s):
        f, at = self.f, self.at
        self.s = s
        at["nleaf"], at["nhits"] = s["nleaf"], s["nhits"]
        again = False
        if at["fused"] and not at["generic_on"] and (s["nleaf"] > 0 or s["n_generic"] > 0):
            self.generic_hint = True
            at["force_generic"] = again = True
        if not at["walker_on"] and s["n_generic"] > 0:
            self.generic_hint = True
            self.generic_sticky = 8
            at["force_generic"] = again = True
        if at["long2"] and s["n_short2"] > 0:
            self.short2_sticky = 8
            at["force_short2"] = again = True
        if not at["jobs_on"] and not f["count_mode"] and (s["jobs_small"] > 0 or s["jobs_big"] > 0):
            self.jobs_hint = True
            at["force_jobs"] = again = True
        worst = s["worst_shard"]
        if worst > at["shard_cap"]:
            at["shard_cap"] = worst + worst // 4 + 64
            again = True
        if at["fused"] and s["worst_sel"] > at["flat_cap"]:
            at["flat_req"] = s["worst_sel"] + s["worst_sel"] // 4 + 64
            again = True
        if not (s["overflow"] & 1) and at["nhits"] > at["hit_cap"]:
            at["hit_cap"] = at["nhits"] + at["nhits"] // 4 + 1024
            again = True
        if s["overflow"] & 8:
            at["walk_cap"] = min(f["ngrp"], s["n_walk"] + s["n_walk"] // 4 + 4096)
            again = True
        self.walk_hint = min(s["n_walk"], 0xFFFFFFFF)
        return again, {k: int(v) for k, v in at.items()}

    def settle(self, k):
        f, at, s = self.f, self.at, self.s
        if f["fast2"] and not at["fused"]:
            if s["n_generic"] > 0 or f["nxs"] > 0:
                self.generic_sticky = 8
            elif self.generic_sticky:
                self.generic_sticky -= 1
            self.generic_hint = self.generic_sticky > 0
        if at["fused"]:
            if s["nleaf"] > 0 or s["n_generic"] > 0 or f["nxs"] > 0:
                self.generic_sticky = 8
            elif self.generic_sticky:
                self.generic_sticky -= 1
            self.generic_hint = self.generic_sticky > 0
        if s["n_nwin"]:
            self.nwin_sticky = 8
        elif self.nwin_sticky:
            self.nwin_sticky -= 1
        if f["fast2"] and not at["long2"] and self.short2_sticky and not at["force_short2"]:
            self.short2_sticky -= 1
        if not f["count_mode"]:
            if s["jobs_small"] > 0 or s["jobs_big"] > 0:
                self.jobs_sticky = 8
            elif self.jobs_sticky:
                self.jobs_sticky -= 1
            self.jobs_hint = self.jobs_sticky > 0
        self.shard_cap_hint = at["shard_cap"]
        if (f["fast1"] or f["fast2"]) and s["worst_sel"]:
            self.flat_cap_hint = max(self.flat_cap_hint, s["worst_sel"] + s["worst_sel"] // 4 + 64)
        self.jobs_big_hint = s["jobs_big"]
        if f["fast1"]:
            self.fused_leaves_hint = s["fused_leaves"] + at["nleaf"]
        self.hit_cap_hint = max(self.hit_cap_hint, at["nhits"] + at["nhits"] // 4 + 1024)
        if k["fetch"] and not k["count"]:
            self.fetch_hits_hint = at["nhits"] + at["nhits"] // 32 + 1024

    def share(self):
        ix = Before(self.long_ok)
        ix.shard_cap_hint, ix.hit_cap_hint, ix.flat_cap_hint = self.shard_cap_hint, self.hit_cap_hint, self.flat_cap_hint
        ix.generic_hint, ix.jobs_hint = self.generic_hint, self.jobs_hint
        ix.fetch_hits_hint, ix.fused_leaves_hint = self.fetch_hits_hint, self.fused_leaves_hint
        return ix

    def merge(self, shared):
        sh = shared["old"]
        if not shared["valid"]:
            return
        self.shard_cap_hint = max(self.shard_cap_hint, sh["shard_cap"])
        self.flat_cap_hint = max(self.flat_cap_hint, sh["flat_cap"])
        self.hit_cap_hint = max(self.hit_cap_hint, sh["hit_cap"])
        if sh["fetch_hits"]:
            self.fetch_hits_hint = sh["fetch_hits"]
        self.generic_sticky = max(self.generic_sticky, sh["generic_sticky"])
        self.jobs_sticky = max(self.jobs_sticky, sh["jobs_sticky"])
        self.generic_hint = self.generic_sticky > 0
        self.jobs_hint = self.jobs_sticky > 0
        self.jobs_big_hint = sh["jobs_big"]
        self.fused_leaves_hint = sh["fused_leaves"]

    def publish(self, shared):
        sh = shared["old"]
        sh["shard_cap"] = max(sh["shard_cap"], self.shard_cap_hint)
        sh["flat_cap"] = max(sh["flat_cap"], self.flat_cap_hint)
        sh["hit_cap"] = max(sh["hit_cap"], self.hit_cap_hint)
        sh["fetch_hits"] = self.fetch_hits_hint
        sh["generic_sticky"], sh["jobs_sticky"] = self.generic_sticky, self.jobs_sticky
        sh["jobs_big"], sh["fused_leaves"] = self.jobs_big_hint, self.fused_leaves_hint


def shared_record(L):
    new = (W * len(H))()
    L.hh_fresh_hints(new)
    return {"valid": False, "new": new,
            "old": dict(flat_cap=0, shard_cap=0, generic_sticky=0, jobs_sticky=0, hit_cap=0, jobs_big=0, fused_leaves=0, fetch_hits=0)}


# ----------------------------------------------------------------------------------------------------------------- one batch

def run_batch(k, new, old=None):
    """the attempt loop of run_batch on the header's rules, beside the rules before Hints when `old` is given: after every attempt
    the flags, capacities, flat_form, fast2_minlen and `again` are equal.  Returns the attempts (flags as decided, Summary)."""
    new.begin(k)
    if old:
        old.begin(k)
    attempts = []
    while True:
        assert len(attempts) <= 8
        at = new.decide()
        if old:
            assert at == old.decide(), (k, len(attempts))
            assert new.minlen == old.minlen
        s = summary_of(k, new.f, at)
        again, after = new.review(s)
        if old:
            assert (again, after) == old.review(s), (k, len(attempts))
        attempts.append((at, s, after))
        if not again:
            break
    new.settle(k)
    if old:
        old.settle(k)
        same_state(new, old, k)
    return attempts


PROBES = [kind(dist=1), kind(dist=2), kind(dist=1, count=True)]


def same_state(new, old, tag):
    """after a batch: the same hints (a bool of `old` is its counter > 0), and the next batch of either distance decides the same"""
    assert new.hints() == old.hints(), tag
    assert old.generic_hint == (old.generic_sticky > 0) and old.jobs_hint == (old.jobs_sticky > 0), tag
    for p in PROBES:
        new.begin(p)
        old.begin(p)
        assert new.decide() == old.decide(), (tag, p)


def forms(attempts_per_batch):
    return [a[-1][0]["flat_form"] for a in attempts_per_batch]


def repeats(attempts_per_batch):
    return [len(a) - 1 for a in attempts_per_batch]


CLEAN = kind(dist=1)
WITH_N = kind(dist=1, n_generic=30, leaves=700, n_nwin=1, n_walk=30)
D2 = kind(dist=2, nq=120, nhits=900)
D2_SHORT = kind(dist=2, nq=40, n_short=8)
D2_N = kind(dist=2, nq=40, n_generic=20, leaves=9000, worst_shard=30, n_walk=20)
RICH = kind(dist=1, nq=40, jobs_small=60, jobs_big=5, nhits=900)


# ----------------------------------------------------------------------------------------------------------- scripted schedules

def test_generic_hint_rearms_and_decays(lib):
    """test_gpu_handle_history.py's schedule: a fresh handle's first clean batch runs the generic kernels (form 2), the next one not (3);
    an N-bearing batch after the hint decayed is repeated with them, the hint stays for STICKY clean batches, then form 3 again"""
    ix = Rules(lib)
    got = [run_batch(k, ix, None) for k in [CLEAN, CLEAN, WITH_N] + [CLEAN] * (STICKY + 1)]
    assert forms(got) == [2, 3, 2] + [2] * STICKY + [3]
    assert repeats(got) == [0, 0, 1] + [0] * (STICKY + 1)
    first, second = got[2][0][0], got[2][1][0]
    assert (first["flat_form"], first["generic_on"], second["generic_on"], second["force_generic"]) == (3, 0, 1, 1)


def test_short_strings_leave_long2_for_sticky_batches(lib):
    ix = Rules(lib, long_ok=True)
    got = [run_batch(k, ix, None) for k in [D2, D2, D2_SHORT] + [D2] * (STICKY + 1)]
    assert forms(got) == [7, 7, 5] + [5] * STICKY + [7]
    assert repeats(got) == [0, 0, 1] + [0] * (STICKY + 1)
    assert ix.minlen == LONG_K + 2 and got[3][0][0]["long2"] == 0
    # without the long filter every distance-2 batch runs the r04 body, and short strings are no reason to repeat
    ix = Rules(lib, long_ok=False)
    got = [run_batch(k, ix, None) for k in [D2, D2_SHORT, D2]]
    assert forms(got) == [5, 5, 5] and repeats(got) == [0, 0, 0] and ix.minlen == 0


def test_locate_job_hint_decays_then_rearms(lib):
    ix = Rules(lib)
    got = [run_batch(k, ix, None) for k in [CLEAN] * (STICKY + 1) + [RICH] + [CLEAN] * (STICKY + 1)]
    assert repeats(got) == [0] * (STICKY + 1) + [1] + [0] * (STICKY + 1)
    assert [a[-1][0]["jobs_on"] for a in got] == [1] + [0] * STICKY + [1] + [1] * STICKY + [0]
    first, second = got[STICKY + 1][0][0], got[STICKY + 1][1][0]
    assert (first["jobs_on"], second["jobs_on"], second["force_jobs"]) == (0, 1, 1)


def test_walker_rearms_after_clean_distance2_batches(lib):
    ix = Rules(lib)
    got = [run_batch(k, ix, None) for k in [D2] * 3 + [D2_N] + [D2] * (STICKY + 1) + [D2_N]]
    assert [a[-1][0]["walker_on"] for a in got] == [1, 0, 0, 1] + [1] * STICKY + [0] + [1]
    assert repeats(got) == [0, 0, 0, 1] + [0] * (STICKY + 1) + [1]
    assert got[3][0][0]["walker_on"] == 0 and got[3][1][0]["generic_on"] == 1
    # nothing packs (a 42-nt query): no fused select, so only the walker branch can ask for the repeat
    ix = Rules(lib)
    got = [run_batch(k, ix, None) for k in [D2] * 3 + [dict(D2_N, packed=False)]]
    assert repeats(got) == [0, 0, 0, 1] and forms(got)[3] == 6 and got[3][1][0]["walker_on"] == 1


# ---------------------------------------------------------------------------------------------------------------- retry causes

BIG = dict(nq=10000, n_generic=7000, leaves=40000, n_nwin=1)  # 20 000 groups: first capacities 156 per shard, 41 024 hits, 4 096 listed groups
CAUSES = {"shard": dict(worst_shard=1000), "slice": dict(worst_sel=3000), "hits": dict(nhits=100000), "walk": dict(n_walk=6000)}


@pytest.mark.parametrize("which", list(CAUSES) + ["slice+hits+walk", "all"])
def test_every_retry_cause(lib, which):
    """shard, flat slice, hit capacity and walker list, each alone and together: one repeat serves them, and the capacities it runs
    with are the formulas' values.  The one exception is the rule's own: after a leaf overflow (bit 1) the hit count is not the
    batch's, so with a shard among the causes the hit capacity is raised by the review of the repeat, one attempt later."""
    causes = list(CAUSES) if which == "all" else which.split("+")
    over = dict(BIG)
    for c in causes:
        over.update(CAUSES[c])
    k = kind(dist=1, **over)
    ix = Rules(lib)  # fresh: generic kernels on, so leaf shards and walker groups are seen in the first attempt
    attempts = run_batch(k, ix, None)
    first, s, _ = attempts[0]
    assert (first["shard_cap"], first["flat_cap"], first["hit_cap"], first["walk_cap"]) == (156, 156, 41024, 4096)
    assert bool(s["overflow"] & 1) == ("shard" in causes) and bool(s["overflow"] & 8) == ("walk" in causes)
    want = dict(shard_cap=1000 + 1000 // 4 + 64 if "shard" in causes else 156,
                flat_cap=3000 + 3000 // 4 + 64 if "slice" in causes else 156,
                hit_cap=100000 + 100000 // 4 + 1024 if "hits" in causes else 41024,
                walk_cap=min(20000, 6000 + 6000 // 4 + 4096) if "walk" in causes else 4096)
    masked = "shard" in causes and "hits" in causes
    assert len(attempts) == (3 if masked else 2)
    second = attempts[1][0]
    assert {c: second[c] for c in want} == (dict(want, hit_cap=41024) if masked else want)
    last = attempts[-1][0]
    assert {c: last[c] for c in want} == want
    h = ix.hints()
    assert (h["shard_cap"], h["walk"]) == (want["shard_cap"], k["n_walk"])
    assert h["flat_cap"] == k["worst_sel"] + k["worst_sel"] // 4 + 64
    assert h["hit_cap"] == k["nhits"] + k["nhits"] // 4 + 1024
    assert len(run_batch(k, ix, None)) == 1  # the same batch again: nothing left to learn


# ---------------------------------------------------------------------------------------------------------------- differential

def random_kind(rng):
    dist = rng.choice([1, 1, 1, 2, 2, 3])
    nq = rng.choice([1, 40, 300, 3000, 20000])
    n_generic = rng.choice([0, 0, 0, 1, rng.randrange(1, 2 * nq + 1)])
    sw = {}
    if rng.random() < 0.1:
        sw[rng.choice(["no_fuse", "no_fuse2", "no_long2", "no_prep_fusion"])] = 1
    if rng.random() < 0.04:
        sw.update(debug_caps=1, debug_caps_value=rng.choice([1, 7, 100]))
    est = max(64, 16 * nq // NSHARD)
    return kind(dist=dist, nq=nq, count=rng.random() < 0.15, packed=rng.random() < 0.9, nxs=rng.choice([0] * 8 + [5, 90000]), n_generic=n_generic,
                leaves=rng.choice([0, 0, 3, 50 * nq]), n_short=rng.choice([0, 0, 0, 2]) if dist == 2 else 0, n_nwin=rng.choice([0, 0, 1]),
                jobs_small=rng.choice([0, 0, 0, 30]), jobs_big=rng.choice([0, 0, 0, 1, 4000]), worst_shard=rng.choice([0, est // 2, est, 3 * est, 40 * est]),
                worst_sel=rng.choice([0, 1, est // 3, est + 1, 10 * est]), nhits=rng.choice([0, nq, 5 * nq + 1024, 400 * nq]),
                n_walk=rng.choice([0, n_generic, n_generic // 2]), fused_leaves=rng.choice([0, 40 * nq, 100 * nq]), fetch=rng.random() < 0.5, **sw)


def test_same_decisions_as_the_rules_before_hints(lib):
    """2 000 seeded random streams of 40 batches on one handle: mixed distances, kinds, count mode, switches.  Every attempt decides
    the same, every batch leaves the same state"""
    rng = random.Random(20261020)
    nrep = 0
    for stream in range(2000):
        long_ok = rng.random() < 0.7
        new, old = Rules(lib, long_ok), Before(long_ok)
        pool = [random_kind(rng) for _ in range(6)] + [CLEAN, D2]
        for b in range(40):
            nrep += len(run_batch(rng.choice(pool), new, old)) - 1
    assert 2000 < nrep < 40000, nrep  # the streams repeat batches, and not every batch


@pytest.mark.parametrize("nlanes", [2, 3])
def test_lanes_merge_and_publish_like_pull_and_push(lib, nlanes):
    """the handle and its internal lanes: each runs merge, batch, publish; the lanes' steps interleave at random.  A lane is created
    (dg_index_share of the owner) while the owner's two shared hints are on: fresh, or right behind a batch that needed them"""
    rng = random.Random(77 + nlanes)
    for stream in range(300):
        shared = shared_record(lib)
        owner = (Rules(lib), Before())
        if rng.random() < 0.5:
            run_batch(dict(WITH_N, jobs_small=3, fetch=True), *owner)
            owner[0].publish(shared)
            owner[1].publish(shared)
            shared["valid"] = True
        assert owner[0].hints()["generic"] and owner[0].hints()["jobs"]
        lanes = [owner] + [(owner[0].share(), owner[1].share()) for _ in range(nlanes - 1)]
        pool = [random_kind(rng) for _ in range(4)] + [CLEAN, D2, WITH_N, RICH]
        todo = [[(step, rng.choice(pool)) for _ in range(12) for step in ("merge", "batch", "publish")] for _ in lanes]
        while any(todo):
            i = rng.choice([j for j, t in enumerate(todo) if t])
            (step, k), (new, old) = todo[i].pop(0), lanes[i]
            if step == "merge":
                new.merge(shared)
                old.merge(shared)
            elif step == "batch":
                run_batch(k, new, old)
            else:
                new.publish(shared)
                old.publish(shared)
                shared["valid"] = True
                sh = record(H, shared["new"])
                assert {c: sh[c] for c in ("flat_cap", "shard_cap", "hit_cap", "jobs_big", "fused_leaves", "fetch_hits")} == \
                    {c: shared["old"][c] for c in ("flat_cap", "shard_cap", "hit_cap", "jobs_big", "fused_leaves", "fetch_hits")}
                assert (sh["generic"], sh["jobs"]) == (shared["old"]["generic_sticky"], shared["old"]["jobs_sticky"])
            if step != "batch":
                same_state(new, old, (stream, i, step))


def test_lane_of_a_decayed_handle_starts_with_the_hint_off(lib):
    """the one deliberate difference (hunt_hints.hpp, inherited()): a lane created from a handle whose generic hint has decayed, the
    lanes' record valid with a counter of 0.  The copied bool asked for "off"; the counter of 1 beside it let the first merge switch
    the hint back on (max(1, 0)) — when the owner's publish came first.  inherited() carries 0: off either way, form 3"""
    shared = shared_record(lib)
    new, old = Rules(lib), Before()
    for _ in range(STICKY + 1):
        run_batch(CLEAN, new, old)
    assert new.hints()["generic"] == 0 and not old.generic_hint
    for order in ("share first", "publish first"):
        if order == "publish first":
            new.publish(shared)
            old.publish(shared)
            shared["valid"] = True
        ln, lo = new.share(), old.share()
        assert (ln.hints()["generic"], ln.hints()["jobs"]) == (0, 0) and (lo.generic_hint, lo.generic_sticky) == (False, 1)
        ln.merge(shared)
        lo.merge(shared)
        assert ln.hints()["generic"] == 0
        assert lo.generic_hint == (order == "publish first")
        assert forms([run_batch(CLEAN, ln, None)]) == [3]
        assert forms([run_batch(CLEAN, lo_as_rules(lib, lo), None)]) == [2 if order == "publish first" else 3]


def lo_as_rules(L, old):
    """the header's rules started from a state of the rules before Hints (a bool that is on is a counter of at least 1)"""
    h = old.hints()
    h["generic"] = max(h["generic"], 1) if old.generic_hint else 0
    h["jobs"] = max(h["jobs"], 1) if old.jobs_hint else 0
    return Rules(L, old.long_ok, [h[c] for c in H])


# ------------------------------------------------------------------------------------------------------------- field coverage

#             field: (merge,          publish,  inherited)
FIELD_RULES = {"shard_cap": ("max", "max", "copy"),
               "flat_cap": ("max", "max", "copy"),
               "hit_cap": ("max", "max", "copy"),
               "generic": ("max", "latest", "on"),
               "jobs": ("max", "latest", "on"),
               "nwin": ("lane", "lane", "default"),
               "short2": ("lane", "lane", "default"),
               "walk": ("lane", "lane", "default"),
               "jobs_big": ("latest", "latest", "default"),
               "fused_leaves": ("latest", "latest", "copy"),
               "fetch_hits": ("latest if non-zero", "latest", "copy")}


def test_every_field_has_its_rule(lib):
    """every Hints field set to a distinct non-default value on a lane and in the record: merge, publish and inherited() field by
    field against the table (the harness names the struct's fields one by one: a field without a word there does not compile)"""
    assert list(FIELD_RULES) == H
    fresh = (W * len(H))()
    lib.hh_fresh_hints(fresh)
    fresh = record(H, fresh)
    for lane_big in (False, True):
        lane = {c: 10 + 2 * i + (100 if lane_big else 0) for i, c in enumerate(H)}
        rec = {c: 60 + 2 * i for i, c in enumerate(H)}
        assert all(lane[c] != fresh[c] and rec[c] != fresh[c] and lane[c] != rec[c] for c in H)
        for zero_fetch in (False, True):
            if zero_fetch:
                rec["fetch_hits"] = 0
            a, b = words(H, lane), words(H, rec)
            lib.hh_merge(a, b)
            assert list(b) == [rec[c] for c in H]
            for c, got in record(H, a).items():
                rule = FIELD_RULES[c][0]
                want = {"max": max(lane[c], rec[c]), "latest": rec[c], "lane": lane[c], "latest if non-zero": rec[c] or lane[c]}[rule]
                assert got == want, ("merge", c, rule)
            a, b = words(H, lane), words(H, rec)
            lib.hh_publish(a, b)
            assert list(a) == [lane[c] for c in H]
            for c, got in record(H, b).items():
                rule = FIELD_RULES[c][1]
                want = {"max": max(lane[c], rec[c]), "latest": lane[c], "lane": rec[c]}[rule]
                assert got == want, ("publish", c, rule)
        for off in (False, True):
            src = dict(lane, generic=0, jobs=0) if off else lane
            out = (W * len(H))()
            lib.hh_inherited(words(H, src), out)
            for c, got in record(H, out).items():
                rule = FIELD_RULES[c][2]
                want = {"copy": src[c], "on": 0 if off else 1, "default": fresh[c]}[rule]
                assert got == want, ("inherited", c, rule)
