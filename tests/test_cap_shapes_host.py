"""tests/cap_shapes.py reaches what each of its cases was built for — shown on the reference side alone: every member of every
saturated capped set occurs in the case's text, every firing group has occurring decoys, the numbers the GPU test expects of the cap
stage come from the restated rule and the oracle's sets, the shared header's formulation (tests/host/libcapenum.so, as in
tests/test_cap_enum.py) gives the oracle's set for every (strand, distance, cap) the device will enumerate, and one string more or
less in any case's set changes the hits the reference model expects.  No GPU, no library under test."""
import os
import subprocess
import sys

import pytest

import cap_shapes as C
from test_cap_enum import ce, run as ce_run  # noqa: F401  (the fixture builds and binds libcapenum.so)

ALL = sorted(C.CASES)


def occurs(ref, w):
    return ref.orc.count(w.encode()) > 0


def groups(name):
    """(group, members, language outside the set) of every saturated group"""
    for g in C.case(name)["groups"]:
        mem = C.capped(g["s"], g["d"], g["hamming"], g["cap"])
        yield g, mem, C.universe(g["s"], g["d"], g["hamming"]) - mem


@pytest.mark.parametrize("name", ALL)
def test_texts_are_small_and_hold_every_member_and_decoys(name):
    c, ref = C.case(name), C.reference(name)
    assert len(c["text"]) <= 1_000_000 and set(c["text"]) <= set(b"ACGTN\n") and c["text"].endswith(b"\n")
    assert sum(c["seqlen"]) == len(c["text"]) and len(c["seqlen"]) == c["text"].count(b"\n") == 2
    fired = 0
    for g, mem, outside in groups(name):
        missing = [w for w in mem if not occurs(ref, w)]
        assert not missing, (name, g, len(missing))                          # share left out: 0
        if len(mem) >= g["cap"]:
            fired += 1
            have = sum(1 for w in outside if occurs(ref, w))
            assert have >= min(32, len(outside)), (name, g, have)
        w = min(mem)
        assert (w.encode() in c["text"]) and ref.orc.count(w.encode()) == S_scan(c["text"], w)
    assert fired or name == "c2_m21"


def S_scan(text, w):
    return C.S.scan(text, w.encode())


def test_texts_and_batches_are_the_same_on_every_build():
    """another interpreter with another string hash seed builds the same texts and batches"""
    names = ["c1", "c2_small", "c3", "c5", "c6"]
    code = "import sys; sys.path[:0] = %r; import cap_shapes as C; print(' '.join(C.digest(n) for n in %r))" % (
        [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))], names)
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, PYTHONHASHSEED="12345")).decode().split()
    assert out == [C.digest(n) for n in names]


def test_the_cases_are_what_they_say():
    e = {(n, r["label"]): C.expect(r) for n in ALL for r in C.case(n)["runs"]}
    # case 1 and 2: one device query each; the caps below F fire, F + 1 may not
    for n in ("c1", "c2_small", "c2_m29", "c2_m21"):
        for r in C.case(n)["runs"]:
            x = e[n, r["label"]]
            assert (x["device"], x["host"]) == (1, 0), (n, r["label"])
            cap = r["kw"]["max_neighborhood"]
            sizes = [len(C.capped(s, r["kw"]["distance"], False, cap)) for s in C.strands(r["qs"][0])]
            assert x["patterns"] == (sum(sizes) if max(sizes) >= cap else 0)
    assert {len(r["qs"][0]) for r in C.case("c1")["runs"]} == {10, 20, 30} and len(C.case("c1")["runs"]) == 36
    for lab, want in (("forward_only", [True, False]), ("reverse_only", [False, True])):
        r = C.run_of("c2_small", lab)
        cap = r["kw"]["max_neighborhood"]
        assert [len(C.capped(s, 2, False, cap)) >= cap for s in C.strands(r["qs"][0])] == want and e["c2_small", lab]["fired"] == [True]
    assert e["c2_m29", "m29/x10000"]["patterns"] == 20000 and e["c2_m21", "m21/x10000"]["fired"] == [False]
    assert C.neighbourhood_bound(21, 2, True) == 10787 >= C.DEFAULT_CAP > C.neighbourhood_bound(20, 2, True) == 9784
    # case 3: one of each pair on either side, both fire
    for lab in ("d1/30+31", "d2/29+30", "d1/30+31/forward"):
        assert (e["c3", lab]["device"], e["c3", lab]["host"], e["c3", lab]["fired"]) == (1, 1, [True, True])
    assert e["c3", "d1/30+31/forward"]["patterns"] * 2 == e["c3", "d1/30+31"]["patterns"]
    r = C.run_of("c3", "case/20")
    assert r["qs"][1] == r["qs"][0].lower() != r["qs"][0] and e["c3", "case/20"]["device"] == 2
    # case 4: every length from 10 nt up is looked at; the persistent loop's second pass has 76 jobs, 30 nt before and 10 nt behind
    assert C.neighbourhood_bound(10, 1, True) == 75 >= C.C4_CAP
    r = C.run_of("c4", "d1/1100")
    assert [len(q) for q in r["qs"]] == [C.c4_length(i) for i in range(1100)] and len(C.device_jobs(r)) == 2200
    assert e["c4", "d1/1100"]["device"] == 1100 > C.PERSISTENT_WG and e["c4", "d1/1100"]["host"] == 0
    assert all(len(r["qs"][i]) == 30 and len(r["qs"][i + 1024]) == 10 for i in range(76)) and r["sat"] == list(range(76)) + list(range(1024, 1100))
    assert sorted({len(q) for q in r["qs"]}) == list(range(10, 31))
    assert e["c4", "d2/12"]["device"] == 12 and e["c4", "d2/12"]["patterns"] == 12 * 2 * 50
    # case 5: a group of SELCAP and of SELCAP + 1 occurring explicit strings
    for cap in (C.S.SELCAP, C.S.SELCAP + 1):
        assert e["c5", "alone/x%d" % cap]["patterns"] == 2 * cap and e["c5", "at40/x%d" % cap]["device"] == 65
        assert C.run_of("c5", "at40/x%d" % cap)["qs"][40] == C.run_of("c5", "alone/x%d" % cap)["qs"][0]
    # case 6: all on the host, whatever the switch says
    for r in C.case("c6")["runs"]:
        x = e["c6", r["label"]]
        assert x == C.expect(r, host_only=True) and x["device"] == 0 and x["host"] == len(r["qs"]) and all(x["fired"])
    mem = C.capped(C.strands(C.run_of("c6", "two_n")["qs"][0])[0], 2, False, 100)
    assert any("N" in w for w in mem)
    assert sorted({len(w) for r in C.case("c6")["runs"][2:5] for s in C.strands(r["qs"][0]) for w in C.capped(s, 1, False, 100)}) == [40, 41, 42, 43, 44]
    # case 7: a fired query on either side, silent ones, one never looked at, one not searched
    r = C.run_of("c7", "mixed")
    x = e["c7", "mixed"]
    assert [len(q) for q in r["qs"]] == [14, 20, 12, 14, 30, 9, 10, 14, 14] and x["fired"] == [False, True, False, False, True, False, False, False, False]
    assert (x["device"], x["host"], x["patterns"]) == (6, 1, 4 * C.C7_CAP)
    assert C.neighbourhood_bound(10, 2, True) == 2449 < C.C7_CAP <= C.neighbourhood_bound(12, 2, True) == 3524
    assert C.expect(r, host_only=True)["host"] == 7


@pytest.mark.parametrize("name", C.DEVICE_CASES)
def test_the_shared_header_gives_the_oracles_set(ce, name):  # noqa: F811
    """every (strand, distance, cap) k_cap_enum will see, through cap_enum.hpp on the host first"""
    seen = set()
    for r in C.case(name)["runs"]:
        for job in C.device_jobs(r):
            if job in seen:
                continue
            seen.add(job)
            s, d, cap = job
            want = C.capped(s, d, False, cap)
            got, fired = ce_run(ce, s, d, cap)
            assert got == sorted(want) and fired == (len(want) >= cap), (name, r["label"], s, cap, len(got), len(want))
    assert seen


def model_hits(ref, strings):
    """the hits the reference pushes for one strand's set: the strings in std::set order, each with its sorted places"""
    return [(w, p) for w in sorted(strings) for p in sorted(ref.orc.locate(w.encode()))]


@pytest.mark.parametrize("name", ALL)
def test_one_string_more_or_less_changes_the_expected_hits(name):
    """on the reference model: a member removed from, or a decoy added to, a group's set — the text can see a one-string error"""
    ref = C.reference(name)
    firing = [(g, mem, out) for g, mem, out in groups(name) if len(mem) >= g["cap"]] or list(groups(name))
    g, mem, outside = firing[0]
    base = model_hits(ref, mem)
    assert len(base) >= len(mem)
    assert model_hits(ref, mem - {max(mem)}) != base
    extra = [w for w in sorted(outside) if occurs(ref, w)]
    if len(mem) >= g["cap"]:
        assert extra
    if extra:
        assert model_hits(ref, mem | {extra[len(extra) // 2]}) != base
