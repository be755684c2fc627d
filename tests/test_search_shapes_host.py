"""tests/search_shapes.py without a GPU: the oracle runs every case, and each case must still have the property it was built for,
counted on the reference side alone (the oracle's hit list and push list, windows rebuilt from the text, a plain restatement of
symmetry_thermo).  A generator that quietly stopped producing its shape fails here, not in the GPU module."""
import math

import pytest

import oracle_lib as O
import search_shapes as S


def test_the_reference_builds_are_present():
    assert O.ref_libs() is not None, "oracle/_ref is missing: __graft_entry__.build() compiles it (oracle/Makefile)"


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_every_case_runs_and_its_push_list_is_its_json(name):
    """the push list the GPU module compares in order holds exactly the sites of the JSON (which is sorted by Tm)"""
    import json
    e = S.expected(name)
    doc = json.loads(e["json"])
    g = S.genome()
    ref_of = {n: i for i, n in enumerate(g["names"])}
    a = sorted((ref_of[p["Chrom"]], p["Pos"] - 1, int(p["Name"][1:]), p["Ori"] == "forward", p["Tm"], p["MatchTm"], p["Genome"])
               for p in doc["data"]["primers"])
    assert a == sorted(e["pushed"]) and len(a) >= 3
    kept = sum(1 for h in e["located"] if h[5] > S.cases()[name]["cutTemp"])
    print("%s: %d primers, %d located hits, %d over the cut, %d sites" % (name, len(e["primers"]), len(e["located"]), kept, len(a)))
    assert kept >= len(a)


def _kept(name):
    cut = S.cases()[name]["cutTemp"]
    return [x for x in S.hit_windows(name) if x[0][5] > cut]


@pytest.mark.parametrize("name", ["len31_57", "len31_57_k30"])
def test_long_primers_fill_the_second_trace_word(name):
    kept = [x for x in _kept(name) if len(x[1]) >= 33]
    fw, rv = sum(1 for x in kept if x[0][1] == 0), sum(1 for x in kept if x[0][1] == 1)
    sites = [p for p in S.expected(name)["pushed"] if len(p[6]) >= 33]
    print("%s: %d kept hits with a window of 33 nt or more (%d forward, %d reverse), %d sites with Genome >= 33 nt" %
          (name, len(kept), fw, rv, len(sites)))
    assert len(sites) >= 100 and any(p[3] for p in sites) and any(not p[3] for p in sites)
    assert len(kept) >= 100 and fw >= 20 and rv >= 20


def test_k_of_primer_length_minus_one():
    c = S.cases()["k_plen_minus_1"]
    assert all(len(p) == c["kmer"] + 1 for p in c["primers"]) and len(S.expected("k_plen_minus_1")["pushed"]) >= 8


def _flags(name):
    e = S.expected(name)
    return [(x, S.self_complementary(e["primers"][x[0][0]]), S.self_complementary(x[1])) for x in _kept(name)]


def test_palindromes_and_their_near_misses():
    c = S.cases()["palindromes"]
    fl = _flags("palindromes")
    e = S.expected("palindromes")
    lo, rng_of = 0, {}
    for kind, n in c["kinds"].items():
        rng_of[kind] = range(lo, lo + n)
        lo += n
    per = {k: [(p, w) for x, p, w in fl if x[0][0] in r] for k, r in rng_of.items()}
    both = sum(1 for x, p, w in fl if p and w)
    print("palindromes: %d kept sites, %d with both symmetry flags; per kind %s" % (len(fl), both, {k: len(v) for k, v in per.items()}))
    assert both >= 26 and all(p and w for p, w in per["both"]) and len(per["both"]) >= 26
    assert len(per["odd"]) >= 10 and not any(p or w for p, w in per["odd"])
    assert len(per["central"]) >= 10 and not any(p or w for p, w in per["central"])
    assert sum(1 for p, w in per["window_only"] if w and not p) >= 10
    with_n = [(x, p, w) for x, p, w in fl if x[0][0] in rng_of["with_n"]]
    assert sum(1 for x, p, w in with_n if p and w) >= 10 and sum(1 for x, p, w in with_n if "N" in x[1] and p and w) >= 5
    assert all("N" in e["primers"][q] for q in rng_of["with_n"])
    fl1 = _flags("palindromes_edit1")    # the flanks of edit distance 1 break the window's symmetry
    only_p = sum(1 for x, p, w in fl1 if p and not w)
    print("palindromes_edit1: %d kept sites, %d with a palindromic primer in a window that is none" % (len(fl1), only_p))
    assert only_p >= 10


@pytest.mark.parametrize("name", ["sequential_58_60_d0", "sequential_58_60_d1", "sequential_mixed"])
def test_primers_of_58_to_60_nt(name):
    c, e = S.cases()[name], S.expected(name)
    assert 58 <= max(len(p) for p in c["primers"]) <= 60
    long_sites = sum(1 for p in e["pushed"] if len(e["primers"][p[2]]) >= 58)
    print("%s: %d sites, %d of primers with 58 nt or more" % (name, len(e["pushed"]), long_sites))
    if name == "sequential_mixed":
        assert long_sites >= 1 and len(e["pushed"]) - long_sites >= 10 and min(len(p) for p in c["primers"]) == 20
    else:
        assert long_sites >= 12 and {len(e["primers"][p[2]]) for p in e["pushed"]} == {58, 59, 60}


@pytest.mark.parametrize("name", ["handback_k10", "handback_k11", "handback_k12", "handback_k13"])
def test_the_wave_kernel_keeps_every_window_of_a_57_nt_primer(name):
    """The wave kernel hands a hit back when its raw window has more than 64 letters or pre + mlen >= 64.  With the longest primer the
    wave path admits (plen + 3 * distance + 2 <= 62) neither can happen: pre + mlen <= (plen - k + d) + (k + d) = plen + 2d <= 59 and
    the raw window has at most plen + 3d <= 60 letters.  So this counts 0, for any input; what the case does produce is the longest
    windows that kernel computes itself, on both strands.  (Hand-back as such is exercised through DICEY_DEBUG_THAL_REDO and by the
    ambiguous pairs of the thal corpus.)"""
    hw = S.hit_windows(name)
    worst = max(x[2] + x[0][3] for x in hw)
    raw = max(x[2] + x[0][3] + x[3] for x in hw)
    handed = sum(1 for x in hw if x[2] + x[0][3] >= 64 or x[2] + x[0][3] + x[3] > 64)
    longw = [x for x in _kept(name) if len(x[1]) >= 57]
    print("%s: %d located hits, largest pre + mlen %d, largest raw window %d, handed back %d, kept hits with a window >= 57 nt: %d" %
          (name, len(hw), worst, raw, handed, len(longw)))
    assert handed == 0 and 57 <= worst <= 59 and 58 <= raw <= 60
    assert len(hw) >= 20 and {x[0][1] for x in longw} == {0, 1}


@pytest.mark.parametrize("name", ["distance2_edit_k13", "distance2_hamming_k13", "distance2_edit_k15", "distance2_hamming_k15"])
def test_distance_two_finds_the_planted_copies(name):
    c, e = S.cases()[name], S.expected(name)
    k = c["kmer"]
    other = sum(1 for h in e["located"] if h[3] != k)
    per = {}
    for p in e["pushed"]:
        per[p[2]] = per.get(p[2], 0) + 1
    print("%s: %d sites for %d primers, %d located hits of another length than k" % (name, len(e["pushed"]), len(c["primers"]), other))
    assert all(18 <= len(p) <= 30 for p in c["primers"])
    assert all(per.get(q, 0) >= 2 for q in range(len(c["primers"])))     # the piece itself and at least one edited copy
    assert (other == 0) if c["hamming"] else (other >= 4)


def test_many_hits_span_two_launches_and_mostly_fail_the_cut():
    """more located hits than one k_site launch takes with a 57-nt primer in the batch (S.chunk_of restates launch_site_stage), under
    5 % of them over the cut, and the 57-mer's own site behind the first launch's share"""
    c, e = S.cases()["many_hits_57"], S.expected("many_hits_57")
    chunk, wave = S.chunk_of(c)
    kept = sum(1 for h in e["located"] if h[5] > c["cutTemp"])
    last = [i for i, h in enumerate(e["located"]) if h[0] == len(c["primers"]) - 1]
    print("many_hits_57: %d located hits, %d per launch (%d launches), %d over the cut (%.2f %%), %d sites; the 57-mer's hit is number %d" %
          (len(e["located"]), chunk, -(-len(e["located"]) // chunk), kept, 100.0 * kept / len(e["located"]), len(e["pushed"]), last[0]))
    assert wave and chunk == 19954 and len(e["located"]) > chunk
    assert kept * 20 < len(e["located"]) and kept >= 100
    assert last and last[0] >= chunk and any(p[2] == len(c["primers"]) - 1 for p in e["pushed"])


@pytest.mark.parametrize("name", ["len_equals_k_d0", "len_equals_k_d1"])
def test_primers_of_exactly_k_letters(name):
    c, e = S.cases()[name], S.expected(name)
    assert all(len(p) == c["kmer"] for p in c["primers"]) and len(e["pushed"]) >= len(c["primers"])
    assert all(len(x[1]) <= c["kmer"] + 3 * c["distance"] for x in S.hit_windows(name))
    assert sum(1 for x in S.hit_windows(name) if x[5] == 0) >= 1       # one at the very start of a sequence


def test_long_palindromes_for_the_sequential_kernel():
    fl = _flags("palindromes_58_60")
    assert len(fl) >= 12 and all(p and w and len(x[1]) >= 58 for x, p, w in fl)
    assert not S.chunk_of(S.cases()["palindromes_58_60"])[1]      # not on the wave path


def test_distance_two_capped_neighbourhood_warns():
    e = S.expected("distance2_capped")
    assert e["nbhd_warnings"] == len(e["primers"]) >= 1


def test_trace2600_needs_the_wide_traceback():
    c, e = S.cases()["trace2600"], S.expected("trace2600")
    maxp = max(len(p) for p in c["primers"])
    assert (maxp + 3 * c["distance"] + 3) * (c["kmer"] + 1) > 4096
    assert len(e["pushed"]) >= 3 and {p[2] for p in e["pushed"]} == {0, 1, 2} and e["nbhd_warnings"] == 0


def test_refused_primers_are_refused_by_the_reference():
    g = S.genome()
    base = S.cases()["refused_base"]["primers"]
    for key, p in S.refused_primers().items():
        js, rc = S.oracle_index().search(g["seqlen"], g["names"], g["text"], S.fasta(base[:1] + [p] + base[1:]))
        assert rc == 1 and "Error: Thermodynamical calculation failed!" in js and '"data"' not in js, (key, js[:200])


def test_dirty_windows_are_dirty():
    hw = S.hit_windows("dirty_windows")
    kept = _kept("dirty_windows")
    left = sum(1 for x in kept if x[4] < x[2])
    right = sum(1 for x in kept if len(x[1]) - x[4] - x[0][3] < x[3])
    with_n = sum(1 for x in kept if "N" in x[1])
    iupac = sum(1 for x in kept if set(x[1]) & set("RY"))
    eq = sum(1 for x in kept if x[4] == x[5])
    at0 = sum(1 for x in kept if x[0][2] - x[4] == 0)
    last = sum(1 for x in kept if x[0][2] + x[0][3] + (len(x[1]) - x[4] - x[0][3]) == len(S.genome()["text"]) - 1)
    n_in_kmer = sum(1 for p in S.expected("dirty_windows")["primers"] if "N" in p[-15:])
    print("dirty_windows: %d hits, %d kept; cut on the left %d, on the right %d, holding N %d, holding R/Y %d, pre_eff == chrpos %d, "
          "starting at text offset 0: %d, ending with the last sequence: %d" % (len(hw), len(kept), left, right, with_n, iupac, eq, at0, last))
    assert left >= 20 and right >= 20 and with_n >= 6 and iupac >= 6 and eq >= 20 and at0 >= 3 and last >= 3 and n_in_kmer >= 4


def cut_values():
    e = S.expected("cut_edge")
    temps = sorted({p[4] for p in e["pushed"]})
    return [c for t in temps[:12] for c in (math.nextafter(t, -math.inf), t, math.nextafter(t, math.inf))]


def test_cut_edge_moves_one_site_at_a_time():
    e = S.expected("cut_edge")
    cuts = cut_values()
    assert len(cuts) == 36
    for i in range(0, 36, 3):
        below, at, above = (len(S.expected("cut_edge", cutTemp=c)["pushed"]) for c in cuts[i:i + 3])
        assert below == at + 1 == above + 1, (cuts[i + 1], below, at, above)     # `> cut` is strict
