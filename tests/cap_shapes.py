"""Inputs for the cap stage of `dicey hunt` — which strings are searched at all once neighbors() reaches maxNeighborhood (reference
src/neighbors.h:50, hunter.h:342-345; dicey_amd/csrc/hunt_cap.hpp: k_cap_enum, hunt.hip: cap_scan, hunt_search.hpp: k_explicit, and the
explicit-leaf paths of hunt_select.hpp) — from the reference side only: nothing here touches a GPU or the library under test.

The mechanism is the SATURATED text of tests/select_shapes.py turned on the capped set.  On a random text almost none of the strings of a
capped neighbourhood occur, so a set with missing or extra strings, taken at the wrong rank or for the wrong strand answers the same hits.
Here, for every saturated (query, strand) and every (distance, mode, max_neighborhood) a case runs it with, the text holds between 14-nt
spacers

  members  every string of the reference's capped set (oracle_lib.neighbors at distance 1, neighbors_fast at distance 2), and
  decoys   strings of the uncapped language outside that set: strings that were members at an earlier rank and were removed by a later
           substring (the set at a smaller cap, minus the set), strings born after the cap rank (the uncapped set, minus the set), and
           strings of the language that never were members.  Where the language is small (FULL_MAX) all of it is planted.

No census is kept: the oracle is evaluated on the finished text, whatever the spacers complete by accident.

Which queries the stage looks at, restated (dicey_amd/csrc/hunt.hip, cap_scan):

    if (m < 10 && !count_mode) continue;                                                                       // hunt.hip:223
    if (d >= m) d = (u32)m - 1;                                                                                // hunt.hip:225
    if (neighbourhood_bound((u32)m, d, indel, bad) < p->max_neighborhood) continue;                            // hunt.hip:231
    if (dev_jobs && indel && d >= 1 && d <= 2 && bad == 0 && m >= 10 && m + d <= cap::MAX_KEY_LEN && ...)      // hunt.hip:232: k_cap_enum
    const u32 nwg = std::min<u32>(njobs, 1024u);                                                               // hunt.hip:506

cap::MAX_KEY_LEN = 31; `bad` counts the characters outside A/C/G/T after upper-casing; every other query looked at is enumerated on the
host.  A query fires when either strand's set holds max_neighborhood strings (hunter.h:342); both strands of a fired query travel as
explicit strings (cap_patterns), a query looked at that does not fire is left to the search kernels."""
import hashlib
import json
import os
import random
import tempfile

import oracle_lib as O
import select_shapes as S
from conftest import revcomp
from select_shapes import substrings  # noqa: F401  (tests/test_cap_shapes_host.py counts with it)

K, K2 = S.K, S.K2
MAX_KEY_LEN, PERSISTENT_WG, FULL_MAX, UNCAPPED = 31, 1024, 4000, 1 << 30
DEFAULT_CAP = 10000
_memo = {}


# ---- the rule restated ---------------------------------------------------------------------------------------------------------------------

def binom(n, k):
    r = 1
    for i in range(1, k + 1):
        r = r * (n - k + i) // i
    return r


def neighbourhood_bound(m, d, indel, nN=0):
    """hunt_search.hpp:54-97: the largest number of distinct strings neighbors() can hold; None where the library has no proof"""
    nN = min(nN, m)
    if not indel:
        t = 0
        for i in range(min(d, m) + 1):
            for j in range(min(i, nN) + 1):
                if i - j <= m - nN:
                    t += binom(nN, j) * binom(m - nN, i - j) * 4 ** j * 3 ** (i - j)
        return t
    extra = 0
    if nN:
        if d > 2:
            return None
        extra = nN if d == 1 else nN * (9 * m + 5) if d == 2 else 0
    if d == 0:
        return 1
    if d == 1:
        return 7 * m + 5 + extra
    if d == 2:
        M = m - 1
        len_m2 = binom(m, 2)
        len_m1 = m + 3 * m * (m - 1)
        len_0 = 1 + 3 * m + 9 * binom(m, 2) + m * (3 * (m - 1) + 4) - (3 * m + 1)
        len_p1 = (3 * M + 4) * (1 + 3 * M) - 6 * M - 3 * M + 3 * (3 * M + 4)
        len_p2 = 1 + 3 * (m + 1) + 9 * binom(m + 1, 2)
        return len_m2 + len_m1 + len_0 + len_p1 + len_p2 + extra
    return None


def norm(q):
    """hunter.h:306-307: upper case, everything outside A/C/G/T an N"""
    return "".join(c if c in "ACGT" else "N" for c in q.upper())


def strands(q, forward_only=False):
    s = norm(q)
    return (s,) if forward_only else (s, revcomp(s))


def capped(s, d, hamming, cap):
    """the reference's set of strand s at max_neighborhood = cap"""
    key = ("set", s, d, hamming, cap)
    if key not in _memo:
        _memo[key] = frozenset((O.neighbors if d < 2 else O.neighbors_fast)(s, d, not hamming, cap))
    return _memo[key]


def universe(s, d, hamming):
    """every string the reference's walk spells for s, and s itself (neighbors.h:90 inserts it first)"""
    return S.language(s, d, hamming) | {s}


def expect(run, host_only=False):
    """{"device", "host": queries the stage looks at on either side, "patterns": explicit strings it emits, "fired": per query} from the
    rule above and the oracle's sets.  host_only: DICEY_CAP_HOST, nothing qualifies for the device."""
    kw = run["kw"]
    cap, ham, fwd = kw["max_neighborhood"], kw.get("hamming", False), kw.get("forward_only", False)
    out = {"device": 0, "host": 0, "patterns": 0, "fired": []}
    for q in run["qs"]:
        m = len(q)
        if m < 10:
            out["fired"].append(False)
            continue
        d = min(kw["distance"], m - 1)
        bad = sum(c not in "ACGT" for c in q.upper())
        sets = [capped(s, d, ham, cap) for s in strands(q, fwd)]
        fired = any(len(x) >= cap for x in sets)
        out["fired"].append(fired)
        bound = neighbourhood_bound(m, d, not ham, bad)
        if bound is not None and bound < cap:
            assert not fired
            continue
        if not host_only and not ham and 1 <= d <= 2 and bad == 0 and m + d <= MAX_KEY_LEN:
            out["device"] += 1
        else:
            out["host"] += 1
        if fired:
            out["patterns"] += sum(len(x) for x in sets)
    return out


def device_jobs(run):
    """the (strand, distance, cap) k_cap_enum enumerates for this run"""
    kw = run["kw"]
    if kw.get("hamming", False):
        return []
    out = []
    for q in run["qs"]:
        m, d = len(q), min(kw["distance"], len(q) - 1)
        if m >= 10 and 1 <= d <= 2 and all(c in "ACGT" for c in q.upper()) and m + d <= MAX_KEY_LEN and \
                neighbourhood_bound(m, d, True, 0) >= kw["max_neighborhood"]:
            out += [(s, d, kw["max_neighborhood"]) for s in strands(q, kw.get("forward_only", False))]
    return out


# ---- planting ------------------------------------------------------------------------------------------------------------------------------

def _rand(rng, m):
    return "".join(rng.choices("ACGT", k=m))


LOW = "GGGGACACACTTTTTCAGAGAGAAAAACGT"    # runs and 2-nt repeats in every prefix from 10 nt on


def decoys(s, d, hamming, cap, n=48):
    """up to n strings of the uncapped language outside the set at `cap`: (earlier members, born later, never members)"""
    mem, rng = capped(s, d, hamming, cap), random.Random("decoy/%s/%d/%d/%d" % (s, d, hamming, cap))
    earlier = sorted(capped(s, d, hamming, max(1, cap // 2)) - mem)
    earlier = rng.sample(earlier, min(n // 2, len(earlier)))
    later = sorted(capped(s, d, hamming, UNCAPPED) - mem)
    later = rng.sample(later, min(n - len(earlier), len(later)))
    rest = sorted(universe(s, d, hamming) - mem - set(earlier) - set(later))
    never = rng.sample(rest, min(n - len(earlier) - len(later) + 8, len(rest)))
    return earlier, later, never


class _Plan:
    """what a case plants: `which`, and per saturated (strand, distance, mode, cap) a group record for the host test"""

    def __init__(self):
        self.which, self.groups = [], []

    def saturate(self, q, d, hamming, caps, whole=True):
        """whole: all of a language of at most FULL_MAX strings; members and chosen decoys otherwise"""
        for s in strands(q):
            full = whole and len(universe(s, d, hamming)) <= FULL_MAX
            if full:
                self.which += sorted(universe(s, d, hamming))
            for cap in caps:
                self.groups.append({"s": s, "d": d, "hamming": hamming, "cap": cap})
                self.which += sorted(capped(s, d, hamming, cap))
                if not full:
                    for kind in decoys(s, d, hamming, cap):
                        self.which += kind

    def text(self, name, seed):
        which = list(dict.fromkeys(self.which))
        random.Random(seed).shuffle(which)
        return S.saturated("cap/" + name, 0, 0, which, seed=seed)


def _run(label, qs, sat, d, cap, hamming=False, forward_only=False, limits=None, count=True):
    kw = {"distance": d, "max_neighborhood": cap}
    if hamming:
        kw["hamming"] = True
    if forward_only:
        kw["forward_only"] = True
    return {"label": label, "qs": list(qs), "sat": list(sat), "kw": kw, "limits": limits, "count": count and not forward_only}


def full_size(q, d):
    """F: the size of the forward strand's uncapped set"""
    return len(capped(norm(q), d, False, UNCAPPED))


def _one_strand_only(seed, m, d, strand):
    """a (query, cap) whose cap fires on `strand` alone: seeded search over two-letter sequences (runs make the two strands' sets differ)"""
    rng = random.Random(seed)
    for _ in range(300):
        q = "".join(rng.choices("AC", k=m - 4)) + _rand(rng, 4)
        size = [len(capped(s, d, False, UNCAPPED)) for s in strands(q)]
        for cap in sorted({size[0], size[1], size[0] + 1, size[1] + 1}):
            if [len(capped(s, d, False, cap)) >= cap for s in strands(q)] == [strand == 0, strand == 1]:
                return q, cap
    return None


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------

SEEDS = {"c1": 5100, "c2_small": 5200, "c2_m29": 5229, "c2_m21": 5221, "c3": 5300, "c4": 5400, "c5": 5500, "c6": 5600, "c7": 5700}


def _c1(seed):
    """device, distance 1: a random and a low-complexity query of 10, 20 and 30 nt, each at max_neighborhood 1, 2, 17, F - 1, F, F + 1.  (A cap
    that fires on one strand only does not exist at distance 1 among 300 sequences tried per strand and length — the two strands' sets
    grow alike — so those two queries stand in case 2.)"""
    rng, plan, runs = random.Random(seed), _Plan(), []
    for m in (10, 20, 30):
        for kind, q in (("random", _rand(rng, m)), ("low", LOW[:m])):
            F = full_size(q, 1)
            caps = [1, 2, 17, F - 1, F, F + 1]
            plan.saturate(q, 1, False, caps)
            runs += [_run("%s%d/x%d" % (kind, m, cap), [q], [0], 1, cap) for cap in caps]
    return plan, runs


def _c2_small(seed):
    """device, distance 2: a 10-mer and a 12-mer at max_neighborhood 2, 50, F // 2, F - 1, F, F + 1; a 10-mer whose cap fires on the
    forward strand only and one on the reverse strand only (seeded search: seed + 1, seed + 2) — the silent strand travels too"""
    rng, plan, runs = random.Random(seed), _Plan(), []
    for m in (10, 12):
        q = _rand(rng, m)
        F = full_size(q, 2)
        caps = [2, 50, F // 2, F - 1, F, F + 1]
        plan.saturate(q, 2, False, caps)
        runs += [_run("m%d/x%d" % (m, cap), [q], [0], 2, cap) for cap in caps]
    for strand, name in ((0, "forward"), (1, "reverse")):
        q, cap = _one_strand_only(seed + 1 + strand, 10, 2, strand)
        plan.saturate(q, 2, False, [cap])
        runs.append(_run("%s_only" % name, [q], [0], 2, cap))
    return plan, runs


def _c2_m29(seed):
    """device, distance 2, 29 nt — the longest key, the largest table and event array — at 64 and at the default 10 000"""
    q, plan = _rand(random.Random(seed), 29), _Plan()
    plan.saturate(q, 2, False, [64, DEFAULT_CAP])
    return plan, [_run("m29/x64", [q], [0], 2, 64), _run("m29/x10000", [q], [0], 2, DEFAULT_CAP, limits="top")]


def _c2_m21(seed):
    """device, distance 2, 21 nt at the default 10 000: the shortest length the stage looks at there (bound 10 787; 9 784 for 20 nt).  A
    21-mer's working set stays far below 10 000 (about 6 500 strings at the end), so the query is enumerated and left silent: its whole
    uncapped set is planted, the search kernels have to find it."""
    q, plan = _rand(random.Random(seed), 21), _Plan()
    for s in strands(q):
        plan.groups.append({"s": s, "d": 2, "hamming": False, "cap": DEFAULT_CAP})
        plan.which += sorted(capped(s, 2, False, DEFAULT_CAP))
    return plan, [_run("m21/x10000", [q], [0], 2, DEFAULT_CAP, limits="top")]


def _c3(seed):
    """the qualification edge m + d <= 31: 30 / 31 nt at distance 1 and 29 / 30 nt at distance 2 in one batch each, small caps, so that one
    query of the pair fires on the device and one on the host; the first batch again on the forward strand only; one 20-mer in upper and
    in lower case (both on the device)"""
    rng, plan = random.Random(seed), _Plan()
    q30, q31, q29, q30b, q20 = _rand(rng, 30), _rand(rng, 31), _rand(rng, 29), _rand(rng, 30), _rand(rng, 20)
    for q in (q30, q31, q20):
        plan.saturate(q, 1, False, [17])
    for q in (q29, q30b):
        plan.saturate(q, 2, False, [50])
    return plan, [_run("d1/30+31", [q30, q31], [0, 1], 1, 17), _run("d2/29+30", [q29, q30b], [0, 1], 2, 50),
                  # (no count mode: padlock.h:392-421 counts an arm as it stands, only hunter.h:306 upper-cases)
                  _run("case/20", [q20, q20.lower()], [0, 1], 1, 17, count=False), _run("d1/30+31/forward", [q30, q31], [0, 1], 1, 17, forward_only=True)]


C4_N, C4_CAP = 1100, 24


def c4_length(i):
    """30-mers first, 10-mers last: job i and job i + 1024 of the persistent loop differ as much as they can"""
    return 30 if i < 76 else 10 if i >= 1024 else 29 - (i - 76) * 19 // (1024 - 76)


def _c4(seed):
    """persistence: 1 100 device queries at distance 1, max_neighborhood 24 (every length from 10 nt up is looked at: bound 75), so that 76
    workgroups of k_cap_enum take a second job; queries 0-75 and 1024-1099 saturated, the rest random.  Then twelve 12-mers at distance 2,
    max_neighborhood 50, for the same handle: the tables are sized per batch."""
    rng, plan = random.Random(seed), _Plan()
    qs = [_rand(rng, c4_length(i)) for i in range(C4_N)]
    sat = list(range(76)) + list(range(1024, C4_N))
    for i in sat:
        plan.saturate(qs[i], 1, False, [C4_CAP], whole=False)      # (members and decoys only: 152 whole languages are 1.7 MB)
    q12 = [_rand(rng, 12) for _ in range(12)]
    for q in q12:
        plan.saturate(q, 2, False, [50], whole=False)
    return plan, [_run("d1/1100", qs, sat, 1, C4_CAP), _run("d2/12", q12, range(12), 2, 50)]


def _c5(seed):
    """many occurring explicit leaves: one 12-mer at distance 2 with max_neighborhood 1 024 and 1 025 (SELCAP of hunt_select.hpp either
    side) and F where F is above them, every string of its language planted; alone in the batch and as query 40 of 64"""
    rng, plan, runs = random.Random(seed), _Plan(), []
    q = _rand(rng, 12)
    F = full_size(q, 2)
    caps = [S.SELCAP, S.SELCAP + 1] + ([F] if F > S.SELCAP + 1 else [])
    plan.saturate(q, 2, False, caps)
    pads = [_rand(rng, 12) for _ in range(64)]
    for cap in caps:
        runs.append(_run("alone/x%d" % cap, [q], [0], 2, cap))
        runs.append(_run("at40/x%d" % cap, pads[:40] + [q] + pads[40:], [40], 2, cap))
    return plan, runs


def _c6(seed):
    """host-path explicit strings: a 20-mer with two N at distance 2 (strings with code 4; max_neighborhood 100, so that it fires),
    Hamming distance 2 on a 20-mer at 100, and 41, 42 and 43 nt at distance 1 at 100 (strings of 40 to 44 characters, either side of
    PACK_MAX_LEN)"""
    rng, plan = random.Random(seed), _Plan()
    base = _rand(rng, 20)
    qn = base[:5] + "N" + base[6:12] + "N" + base[13:]
    qh = _rand(rng, 20)
    longs = [_rand(rng, m) for m in (41, 42, 43)]
    plan.saturate(qn, 2, False, [100])
    plan.saturate(qh, 2, True, [100])
    for q in longs:
        plan.saturate(q, 1, False, [100])
    return plan, [_run("two_n", [qn], [0], 2, 100), _run("hamming2", [qh], [0], 2, 100, hamming=True)] + \
        [_run("m%d" % len(q), [q], [0], 1, 100) for q in longs] + [_run("m41-43", longs, [0, 1, 2], 1, 100)]


C7_CAP = 3000


def _c7(seed):
    """one batch at distance 2, max_neighborhood 3 000: a 20-mer that fires on the device, a 30-mer that fires on the host, a 12-mer the
    device looks at (bound 3 524) and leaves silent — its uncapped set is planted, the search kernels enumerate it —, a 10-mer never
    looked at (bound 2 449) and a 9-mer, which is not searched; random 14-mers (looked at, silent) in between"""
    rng, plan = random.Random(seed), _Plan()
    q20, q30, q12, q10, q9 = (_rand(rng, m) for m in (20, 30, 12, 10, 9))
    pads = [_rand(rng, 14) for _ in range(4)]
    for q in (q20, q30, q12, q10):
        plan.saturate(q, 2, False, [C7_CAP])
    qs = [pads[0], q20, q12, pads[1], q30, q9, q10, pads[2], pads[3]]
    return plan, [_run("mixed", qs, [1, 2, 4, 6], 2, C7_CAP)]


CASES = {"c1": _c1, "c2_small": _c2_small, "c2_m29": _c2_m29, "c2_m21": _c2_m21, "c3": _c3, "c4": _c4, "c5": _c5, "c6": _c6, "c7": _c7}
DEVICE_CASES = ("c1", "c2_small", "c2_m29", "c2_m21", "c3", "c4", "c5", "c7")      # cases 1 to 5 and 7: both cap paths


def case(name):
    """{"name", "text", "seqlen", "names", "runs": [{"label", "qs", "sat": indices of the saturated queries, "kw": distance, mode and
    max_neighborhood, "limits", "count"}], "groups": [{"s", "d", "hamming", "cap"}]}, built once per process"""
    key = ("case", name)
    if key not in _memo:
        plan, runs = CASES[name](SEEDS[name])
        text, seqlen = plan.text(name, SEEDS[name])
        _memo[key] = {"name": name, "text": text, "seqlen": seqlen, "names": ["%s_%d" % (name, i + 1) for i in range(len(seqlen))],
                      "runs": runs, "groups": plan.groups}
    return _memo[key]


def run_of(name, label):
    (r,) = [r for r in case(name)["runs"] if r["label"] == label]
    return r


def digest(name):
    """the text and the batches of a case in one number"""
    c = case(name)
    h = hashlib.sha1(c["text"])
    h.update(json.dumps([c["seqlen"], [(r["label"], r["qs"], r["sat"], sorted(r["kw"].items())) for r in c["runs"]]]).encode())
    return h.hexdigest()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------------------

class Reference:
    """the oracle on one case's text behind the interface tests/test_gpu_locate_topk.py's _compare asks for; every query is answered
    once per parameter set (hits in push order and message titles); sums(): what count mode reports, per query and strand"""

    def __init__(self, name):
        self.c = case(name)
        self.dir = tempfile.mkdtemp(prefix="cap_shapes_")
        self.path = os.path.join(self.dir, name + ".fm9")
        O.build_fm9(self.c["text"], self.path)
        self.orc = O.Index(self.path)
        self.memo = {}

    def _answers(self, qs, kw):
        memo = self.memo.setdefault(tuple(sorted(kw.items())), {})
        todo = [q for q in dict.fromkeys(qs) if q not in memo]
        if todo:
            O.fast_neighbors(kw.get("distance", 1) >= 2)
            try:
                lines, per = self.orc.hunt_parallel(self.c["seqlen"], self.c["names"], todo, workers=min(16, os.cpu_count() or 1), **kw)
            finally:
                O.fast_neighbors(False)
            for i, q in enumerate(todo):
                memo[q] = (per.get(i, []), [e["title"] for e in json.loads(lines[i])["errors"]])
        return [memo[q] for q in qs]

    def hunt(self, seqlen, names, qs, want_hits=True, **kw):
        assert list(seqlen) == self.c["seqlen"] and list(names) == self.c["names"]
        return None, [(qi,) + h for qi, (hits, _) in enumerate(self._answers(qs, kw)) for h in hits]

    def titles(self, qs, **kw):
        return [t for _, t in self._answers(qs, kw)]

    def sums(self, qs, d, hamming, cap):
        memo = self.memo.setdefault(("sums", d, hamming, cap), {})
        for q in qs:
            if q not in memo:
                memo[q] = tuple(sum(self.orc.count(w.encode()) for w in capped(s, min(d, len(q) - 1), hamming, cap)) for s in strands(q))
        return [memo[q] for q in qs]


def reference(name):
    key = ("ref", name)
    if key not in _memo:
        _memo[key] = Reference(name)
    return _memo[key]


def limits(ref, run):
    """max_locations above every query's total, and inside the forward and inside the reverse strand's strings of the run's first
    saturated query ("top": the first only)"""
    kw = run["kw"]
    sums = ref.sums(run["qs"], kw["distance"], kw.get("hamming", False), kw["max_neighborhood"])
    if kw.get("forward_only", False):
        sums = [(a, 0) for a, _ in sums]
    fw, rv = sums[run["sat"][0]]
    out = [max(a + b for a, b in sums) + 7]
    if run["limits"] != "top":
        if fw > 1:
            out.append(fw // 2)
        if rv > 1:
            out.append(fw + rv // 2)
    return out
