"""tests/locate_shapes.py has the properties its cases exist for — shown on the reference side alone (a scan of the text with bytes.find,
the stage's arithmetic restated in Python, and the oracle's own locate / sort / truncate); no GPU, no library under test."""
import types

import pytest

import locate_shapes as S
from conftest import revcomp
from test_gpu_locate_topk import _compare

COUNTS = {"run_600": 600, "huge_16400": 16400, "skew_flat": 200, "topk_skew": 3000, "plv_run": 12000, "plv_next": 12000, "plv_dense": 12000, "plv_exact": 20000, "fam300": 300}
COUNTS.update({"skew_%d" % c: 200 for c in S.SKEW_C})


def _intended(name):
    if name.startswith("crowd_"):
        return S.CROWD_COPIES
    return COUNTS[name] if name in COUNTS else int("".join(ch for ch in name.rsplit("_", 1)[-1] if ch.isdigit()))


@pytest.fixture(scope="module")
def g():
    return S.genome()


def test_text_has_four_prefix_levels(g):
    assert len(g["seqs"]) == 4 and g["n"] == len(g["text"]) + 1 > S.LEVELS[3]
    assert g["n"] <= 4 * S.LEVELS[3]                        # no fifth level
    assert g["text"].count(b"\n") == 4 and g["text"].endswith(b"\n")
    assert set(g["text"]) == set(b"ACGT\n")


def test_every_family_has_its_exact_count_and_occurs_nowhere_else(g):
    names = set(g["fam"])
    assert {"n%d" % c for c in S.N_COUNTS} | {"small_%d" % c for c in S.SMALL_COUNTS} | {"skew_%d" % c for c in S.SKEW_C} <= names
    for name, f in g["fam"].items():
        u = f["unit"].encode()
        found = S.scan(g["text"], u)                        # brute force: bytes.find in a loop
        assert found == f["pos"], name
        assert len(found) == _intended(name), (name, len(found))
        assert g["text"].find(revcomp(f["unit"]).encode()) < 0, name
        assert 16 <= len(u) <= 20 or name.startswith("long40_"), name
        assert name in ("skew_flat", "run_600") or len(set(u)) > 1, name
    for s in (g["star"]["q"], revcomp(g["star"]["q"])):
        assert g["text"].find(s.encode()) < 0


def test_few_copy_families_sit_at_the_ends_of_the_text_and_of_sequences(g):
    cum, end = g["cum"], len(g["text"]) - 1
    at_start, at_end = set(), set()
    for c in S.N_COUNTS:
        f = g["fam"]["n%d" % c]
        for p in f["pos"]:
            if p in cum[:-1]:
                at_start.add(p)
            if p + len(f["unit"]) + 1 in cum[1:]:
                at_end.add(p + len(f["unit"]) + 1)
        assert S.route(f["pos"], c, g["n"], S.MID_MAX) is None or c == 17     # <= 16 occurrences: the lane serves them
    assert at_start == set(cum[:-1]) and at_end == set(cum[1:])              # the text's first position .. the last before the final separator
    assert S.route(g["fam"]["n17"]["pos"], 17, g["n"])["list"] == 0


def test_small_families_cover_every_padded_size_of_the_wavefront_sort(g):
    n2s = set()
    for c in S.SMALL_COUNTS:
        pos = g["fam"]["small_%d" % c]["pos"]
        assert pos[-1] - pos[0] >= 1_000_000
        n2 = 32
        while n2 < c:
            n2 <<= 1
        n2s.add((n2, n2 == c))
        r = S.route(pos, c, g["n"], S.MID_MAX)
        assert r["list"] == (0 if c <= 256 else 1) and S.route(pos, c, g["n"], 0)["list"] == (0 if c <= 256 else 2)
        if c <= 256:
            span, sh, per = S.bucket_lanes(pos, 64)
            assert max(per) <= S.BUCKET_SKEW, (c, max(per))  # spread positions: sorted by buckets
    assert n2s == {(32, False), (32, True), (64, False), (64, True), (128, False), (128, True), (256, False), (256, True), (512, False)}


def test_tandem_families_land_on_their_side_of_the_bucket_skew(g):
    for c in S.SKEW_C:
        pos = g["fam"]["skew_%d" % c]["pos"]
        a, cc = g["fam"]["skew_%d" % c]["array"]
        assert cc == c and pos[:c] == [a + 20 * i for i in range(c)]
        assert pos[c] - pos[c - 1] > 65536 and pos[-1] - pos[c] >= 1_000_000
        span, sh, per = S.bucket_lanes(pos, 64)
        assert span >= 256 and per[0] == c, (c, sh, per[0])           # lane 0 holds the array and nothing else
        assert max(per[1:]) <= S.BUCKET_SKEW
        assert (max(per) <= S.BUCKET_SKEW) == (c <= 32), (c, per[0])  # 31, 32: buckets; 33, 34, 64: the network
    pos = g["fam"]["skew_flat"]["pos"]
    span, sh, per = S.bucket_lanes(pos, 64)
    assert len(pos) == 200 and span == 199 < 256 and sh == 0 and max(per) == 4


def test_topk_skew_sends_the_workgroup_sort_to_the_network(g):
    pos = g["fam"]["topk_skew"]["pos"]
    a, c = g["fam"]["topk_skew"]["array"]
    assert c == 500 and pos[:500] == [a + 20 * i for i in range(500)] and pos[500] - pos[499] > 1_000_000
    for surv in S.topk_survivors(pos, 501):                  # 501 .. 597 survivors: the array and 1 .. 97 outliers
        span, sh, per = S.bucket_lanes(surv, 256)
        assert per[0] > S.BUCKET_SKEW and sum(per[:2]) == 500, (len(surv), sh, per[:3])
    spread = g["fam"]["mid_4608"]["pos"]
    for surv in S.topk_survivors(spread, 928):
        assert max(S.bucket_lanes(surv, 256)[2]) <= S.BUCKET_SKEW     # the counterpart: spread survivors sort by buckets


def test_radix_select_of_the_topk_kernel_ends_at_every_byte(g):
    """topk_threshold returns after the byte at which the k-th value's bin fits k + 96: spread positions end it early, 600 consecutive
    positions (156 in the first 256-wide bin, 256 in the second) take it to the last byte, where exactly k values survive"""
    exits = set()
    for name, k in (("mid_4608", 928), ("mid_4608", 4), ("lvl_9216", 577), ("topk_skew", 501), ("topk_skew", 100), ("run_600", 300),
                    ("run_600", 257)):
        pos = g["fam"][name]["pos"]
        shift, kept = S.threshold_exit(pos, k, min(k + 96, S.TOPK_KMAX))
        assert k <= kept <= min(k + 96, S.TOPK_KMAX)
        exits.add(shift)
        if name == "run_600":
            assert pos[0] % 256 == 100 and pos == list(range(pos[0], pos[0] + 600)) and (shift, kept) == (0, k)
    assert exits >= {0, 8, 16}, exits
    # k_locate_big's loop has the same exit, behind limit >= 1 024 values in one bin of 256 positions: no text reaches it


def test_workgroup_thresholds(g):
    n = g["n"]
    for c in (4607, 4608, 4609):
        pos = g["fam"]["mid_%d" % c]["pos"]
        assert S.route(pos, 1000, n, S.MID_MAX)["list"] == (1 if c <= 4608 else 2)
        assert S.route(pos, 1025, n, S.MID_MAX)["list"] == 2              # take above 1 024: k_locate_big's list
        assert S.route(pos, 1000, n, 0) == {"list": 2, "level": None, "occs": c, "take": 1000}
    for c in (9215, 9216, 9217):
        pos = g["fam"]["lvl_%d" % c]["pos"]
        for m in (1, 577, 1024):
            r = S.route(pos, m, n, 0)
            assert (r["level"] is not None) == (c == 9217), (c, m, r)     # only 9 217 asks the prefix levels ...
            if c == 9217:
                assert r["occs"] == sum(1 for p in pos if p < S.LEVELS[r["level"]]) and m <= r["occs"] <= S.WALK_MAX
        assert S.route(pos, 1025, n, 0)["level"] is None                  # ... and only for take <= 1 024


def test_prefix_level_outcomes(g):
    n, fam = g["n"], g["fam"]

    def below(name, x):
        return sum(1 for p in fam[name]["pos"] if p < x)          # from the scanned positions

    def asked(name, take):
        occs = len(fam[name]["pos"])
        return next(i for i, x in enumerate(S.LEVELS) if occs * x >= 2 * take * n)
    # 1: the level asked first holds the run
    lv = asked("plv_run", 1000)
    assert lv == 2 and 1000 <= below("plv_run", S.LEVELS[lv]) <= S.WALK_MAX
    assert S.route(fam["plv_run"]["pos"], 1000, n) == {"list": 2, "level": 2, "occs": below("plv_run", 1 << 20), "take": 1000}
    # 2: the run of the asked level is shorter than take, the next level serves
    lv = asked("plv_next", 700)
    assert lv == 2 and below("plv_next", 1 << 20) == 10 < 700 <= below("plv_next", 1 << 22) == 5010 <= S.WALK_MAX
    assert S.route(fam["plv_next"]["pos"], 700, n) == {"list": 2, "level": 3, "occs": 5010, "take": 700}
    # 3: more than 9 216 copies below the asked X: refused, the walk serves the whole interval
    lv = asked("plv_dense", 1000)
    assert lv == 2 and below("plv_dense", 1 << 20) == 9500 > S.WALK_MAX
    assert S.route(fam["plv_dense"]["pos"], 1000, n) == {"list": 2, "level": None, "occs": 12000, "take": 1000}
    # 4: exactly c copies below 2^18: taken at take == c, one record short at c + 1
    c = below("plv_exact", 1 << 18)
    assert c == 400 and asked("plv_exact", c) == asked("plv_exact", c + 1) == 1
    assert S.route(fam["plv_exact"]["pos"], c, n) == {"list": 2, "level": 1, "occs": c, "take": c}
    assert S.route(fam["plv_exact"]["pos"], c + 1, n) == {"list": 2, "level": 2, "occs": below("plv_exact", 1 << 20), "take": c + 1}
    assert (c, c) in [(S.route(fam[k]["pos"], m, n)["occs"], m) for k, m in S.plv_cases()]
    # the decisions above do not hang on whether n counts the sentinel
    for k, m in S.plv_cases():
        assert S.route(fam[k]["pos"], m, n - 1) == S.route(fam[k]["pos"], m, n) == S.route(fam[k]["pos"], m, n + 1)


def _per_query(hits, nq):
    per = [[] for _ in range(nq)]
    for h in hits:
        per[h[0]].append(h[1:])
    return per


def test_star_has_ten_kept_strings_in_set_order(g):
    q, R = g["star"]["q"], S.Reference()
    want = S.star_strings()
    assert sorted(c for _, c in want) == sorted(S.STAR_FWD + S.STAR_REV) and len(want) == 10
    total = sum(c for _, c in want)
    for hamming in (False, True):
        _, hits = R.hunt(g["seqlen"], g["names"], [q], distance=1, hamming=hamming, max_locations=total + 100)
        assert len(hits) == total
        # every hit lies where the scan found a copy of that string's family
        k = 0
        for (name, c) in want:
            pos = g["fam"][name]["pos"]
            cum = g["cum"]
            assert [cum[h[2]] + h[3] - 1 for h in hits[k:k + c]] == pos, name
            assert {h[4] for h in hits[k:k + c]} == {"+" if name in g["star"]["fwd"] else "-"}, name
            assert {h[1] for h in hits[k:k + c]} == {-1}, name      # one substitution each
            k += c
        full = [h[1:] for h in hits]
        for m in S.star_marks():                              # truncation: inside a string, at its end, and nothing for the strings behind
            _, cut = R.hunt(g["seqlen"], g["names"], [q], distance=1, hamming=hamming, max_locations=m)
            assert [h[1:] for h in cut] == full[:m], (hamming, m)
    acc, sums = 0, []
    for _, c in want:
        acc += c
        sums.append(acc)
    assert set(sums) <= set(S.star_marks()) and {s - 1 for s in sums if s > 1} <= set(S.star_marks())


@pytest.mark.parametrize("batches", ["exact", "big", "long", "walk"])
def test_oracle_equals_the_scan_on_every_exact_batch(g, batches):
    """two references that owe nothing to the library: the oracle's locate + sort + truncate, and the first m scanned positions"""
    R = S.Reference()
    table = {"exact": S.exact_batches, "big": S.big_batches, "long": S.long_batches, "walk": S.walk_batches}[batches]()
    nhits = 0
    for m, names in table.items():
        _, hits = R.hunt(g["seqlen"], g["names"], S.units(names), max_locations=m, **S.D0)
        per = _per_query(hits, len(names))
        want = S.scan_expectation(names, m)
        assert per == want, (m, names[S.first_difference(per, want)[0]], S.first_difference(per, want))
        nhits += len(hits)
    print("%s: %d batches, %d hits" % (batches, len(table), nhits))


def test_exact_batches_ask_every_family_at_its_own_count_and_at_the_marks(g):
    b = S.exact_batches()
    for name in S.exact_families():
        occs = len(g["fam"][name]["pos"])
        asked = {m for m, names in b.items() if name in names}
        own = {m for m in (1, occs - 1, occs, occs + 1) if m >= 1 and min(m, occs) <= 16384}
        assert own >= {occs, occs + 1} or name in ("huge_16400", "plv_exact"), name
        assert own | {m for m in S.MARKS if m < occs} == asked, name
    assert set(S.MARKS) >= {4, 5, 16, 17, 256, 257, 576, 577, 927, 928, 929, 1024, 1025}
    big = S.big_batches()
    assert set(big) == {1025, 2560, 4608, 4609, 8192, 8193, 16384}
    assert "lvl_9216" in big[4608] and {"lvl_9217", "lvl_9215"} <= set(big[4609])
    assert all({"lvl_9217", "plv_exact"} <= set(v) for v in big.values()) and len(g["fam"]["plv_exact"]["pos"]) == 20000
    # nothing in any batch asks one lane for more than 16 384 positions
    for table in (b, big, S.long_batches(), S.walk_batches()):
        for m, names in table.items():
            assert all(S.route(g["fam"][k]["pos"], min(m, len(g["fam"][k]["pos"])), g["n"]) != {"list": 3, "level": None, "occs": len(g["fam"][k]["pos"]), "take": min(m, len(g["fam"][k]["pos"]))} for k in names), m


def test_tails_have_the_interval_and_the_mask_they_were_built_for(g):
    """per query: occurrences of the table window (the last 16 characters: the interval k_search1s filters) against those of the whole
    string (the bits of its mask)"""
    text, seen = g["text"], set()
    for q, gi in S.tails_queries():
        t = g["tails"][gi]
        w, b = len(S.scan(text, q[-S.TAIL_K:].encode())), len(S.scan(text, q.encode()))
        if q == t["head"] + t["tail"]:
            assert (w, b) == (t["w"], t["b"]), (q, w, b)
            assert 1 <= len(q) - S.TAIL_K <= 5                       # the characters in front of the window: FmView::pre5 holds five
            seen.add((w, b))
        elif q.endswith(t["tail"]) and len(q) < 20:
            assert w == t["w"] and b >= t["b"], (q, w, b)            # fewer characters in front: the mask can only gain bits
        assert text.find(revcomp(q).encode()) < 0
    assert seen == set(S.TAILS)
    assert {b for _, b in seen} == {1, 2, 4, 5, 15, 16} and {w for w, _ in seen} >= {2, 3, 4, 16}
    assert any(w <= 4 for w, _ in seen) and any(4 < w <= 16 for w, _ in seen)     # locate_in_registers<4> and <16>
    for t in g["tails"]:
        heads = [h for _, h in t["pos"]]
        assert heads.count(t["head"]) == t["b"] and len(heads) == t["w"]
        others = [h for h in heads if h != t["head"]]
        assert all(sum(x != y for x, y in zip(h, t["head"])) == 1 for h in others)
        if len(others) >= 2:                                          # a head that differs next to the window, one that differs four in front
            assert {next(i for i in range(4) if h[i] != t["head"][i]) for h in others} == {0, 3}


def test_crowd_batch_queues_more_wavefront_jobs_than_the_regions_hold(g):
    """a batch of up to 4 096 queries on the flat path has shard_cap = 64 (hunt.hip: max(64, 16 nq / 1024)), so leaf_slots = 1 024 * 64 and
    job_shard_cap = 65 536 / 64 * 3 / 2 + 32 = 1 568 jobs in each of the 64 regions of a list: whatever region a wavefront of k_locate
    writes to, 64 * 1 568 = 100 352 jobs is all a list holds"""
    q, names = g["crowd"]["q"], g["crowd"]["names"]
    qs = S.crowd_batch()
    assert len(names) == S.CROWD and len(qs) <= 4096 and max(64, 16 * len(qs) // 1024) == 64
    cap = min(1024 * 64, 1 << 20) // 64 * 3 // 2 + 32
    assert cap == 1568 and len(qs) * S.CROWD > 64 * cap
    for k in names:
        u = g["fam"][k]["unit"]
        assert sum(x != y for x, y in zip(u, q)) == 1 and len(g["fam"][k]["pos"]) == S.CROWD_COPIES
        assert S.route(g["fam"][k]["pos"], S.CROWD_COPIES, g["n"])["list"] == 0
    per = S.per_query([q], distance=1, hamming=True, forward_only=True, max_locations=1000)[0]
    assert len(per) == S.CROWD * S.CROWD_COPIES                      # every kept string reports all its copies: 30 jobs per query


# ---- the comparator fails where it must ---------------------------------------------------------------------------------------------------------

class _FakeIndex:
    """answers like dicey_amd.FmIndex.hunt, from per-query hit tuples"""

    def __init__(self, per):
        self.per = per

    def hunt(self, qs, seqlen, **kw):
        mk = lambda h: types.SimpleNamespace(score=h[0], chr=h[1], start=h[2], strand=h[3], refalign=h[4], queryalign=h[5])
        return types.SimpleNamespace(queries=[types.SimpleNamespace(hits=[mk(h) for h in hs]) for hs in self.per])


@pytest.mark.parametrize("mutation", ["kth_replaced_by_next", "neighbours_swapped", "one_dropped"])
def test_comparator_names_the_query_and_the_hit_of_a_wrong_answer(g, mutation):
    names = ["n5", "small_64", "mid_4608", "n17"]
    qs, m, victim = S.units(names), 40, 1
    want = S.scan_expectation(names, m)
    full = S.scan_expectation(names, m + 1)
    _compare(_FakeIndex(want), S.Canned(want), g, qs, max_locations=m, **S.D0)        # equal lists pass
    bad = [list(h) for h in want]
    if mutation == "kth_replaced_by_next":
        at = m - 1
        bad[victim][at] = full[victim][m]                     # the (k+1)-th smallest position in the k-th place
    elif mutation == "neighbours_swapped":
        at = 17
        bad[victim][at], bad[victim][at + 1] = bad[victim][at + 1], bad[victim][at]
    else:
        at = 23
        del bad[victim][at]                                   # the list closes up: every later hit moves one place
    assert S.first_difference(bad, want) == (victim, at)
    with pytest.raises(AssertionError) as err:
        _compare(_FakeIndex(bad), S.Canned(want), g, qs, max_locations=m, **S.D0)
    assert "(%d, %r" % (victim, qs[victim]) in str(err.value)
