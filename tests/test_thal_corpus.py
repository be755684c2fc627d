"""The thal corpus (thal_corpus.py) on the CPU: the conditions the corpus must meet, and the product's sequential formulation
(thal.hpp's end1_tm with the product's table loader and environment arithmetic, built for the host in tests/host) against
the reference's own thal() on every pair, bit for bit.  test_gpu_thal_wave.py compares the wave kernel with the sequential
kernel; this is the link from the sequential formulation to the reference."""
import json
import os

import pytest

import thal_corpus as TC
import thal_expect as TE

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_ref = pytest.mark.skipif(not TE.have_ref(), reason="oracle/_ref (the reference's thal.h built in place) is not available")


def test_corpus_is_deterministic_and_holds_every_group():
    g = TC.groups()
    TC._cache.clear()
    assert TC.groups() == g
    want = ["geometry_%dx%d" % s for s in TC.GEOMETRIES] + ["cap_%dx%d" % s for s in TC.CAP_SIZES] + \
        ["structure", "alphabet", "long_49_64", "both_over_60", "long_x_short"]
    assert [k for k in g if not k.startswith(("regression_", "entropy_cutoff"))] == want
    assert all(a and b for pairs in g.values() for a, b in pairs)          # no empty oligo (see thal_corpus)
    assert sum(len(v) for v in g.values()) + len(TC.ENVS) * len(TC.env_pairs()) >= 18000


def test_geometry_groups_set_the_batch_maxima_and_share_their_pairs():
    g = TC.groups()
    s8, s20 = TC.shared_pairs()
    assert len(s8) == len(s20) == TC.N_SHARED
    assert all(len(a) <= 8 and len(b) <= 8 for a, b in s8) and all(len(a) <= 20 and len(b) <= 20 for a, b in s20)
    for L1, L2 in TC.GEOMETRIES:
        pairs = g["geometry_%dx%d" % (L1, L2)]
        assert 1900 <= len(pairs) <= 2100
        assert max(len(a) for a, _ in pairs) == L1 and max(len(b) for _, b in pairs) == L2
        assert any(len(a) == L1 and len(b) == L2 for a, b in pairs)
        assert min(len(a) for a, _ in pairs) == 1 and min(len(b) for _, b in pairs) == 1
        have = set(pairs)
        assert all(p in have for p in s8)
        if L1 >= 20 and L2 >= 20:   # the 9-20 nt pairs would break the maxima of (8, 8)
            assert all(p in have for p in s20)
    assert sum(1 for s in TC.GEOMETRIES if s[0] >= 20 and s[1] >= 20) == len(TC.GEOMETRIES) - 1


@pytest.mark.parametrize("size", TC.CAP_SIZES, ids=lambda s: "%dx%d" % s)
def test_cap_boundary_groups_sit_on_the_wave_kernels_capacity(size):
    """wave_cell_cap is restated once, in thal_corpus.wave_cell_cap (dicey_amd/csrc/thal_wave.hpp:55); the hand-back test is
    `rowbase + popcount > cap` (thal_wave.hpp:248).  If the capacity changes, this fails first: regenerate the group around the
    new value."""
    import re
    src = open(os.path.join(TE.ROOT, "dicey_amd", "csrc", "thal_wave.hpp")).read()
    m = re.search(r"wave_cell_cap\(unsigned len1, unsigned stride\) \{ return ([^;]+); \}", src)
    assert m and m.group(1) == "(len1 * stride * 7u) / 16u + stride + 16u", "wave_cell_cap changed: restate it in thal_corpus.py"
    assert "if (rowbase + (unsigned)__popcll(imask) > m.cap) {" in src, "the hand-back test changed: revisit the cap groups"
    L1, L2 = size
    cap, area = TC.wave_cell_cap(L1, L2), L1 * L2
    assert cap == {(20, 20): 211, (32, 48): 736, (48, 48): 1072}[size]
    pairs, exact = TC.cap_groups()[size]
    assert pairs == TC.groups()["cap_%dx%d" % size]
    assert all(len(a) == L1 and len(b) == L2 for a, b in pairs)
    n = [TC.pairing_cells(a, b) for a, b in pairs]
    # the count in Python equals the definition: cells (i, j) with a[i] + b_rev[j] == 3, both < 4
    a, b = pairs[0]
    assert n[0] == sum(1 for x in a for y in b[::-1] if TC.code(x) < 4 and TC.code(y) < 4 and TC.code(x) + TC.code(y) == 3)
    band = 0.03 * area
    assert sum(1 for x in n if cap - band <= x <= cap) >= 30
    assert sum(1 for x in n if cap < x <= cap + band) >= 30
    assert sum(1 for t in range(cap - 2, cap + 3) if t in exact and TC.pairing_cells(*exact[t]) == t and exact[t] in pairs) >= 3
    # perfect duplexes from position 1 on, a few cells either side of the capacity: an overrun of the cell array lands on the
    # traceback records of the first rows, which only such a duplex reads back
    back = [(a, b) for (a, b), x in zip(pairs, n) if cap - 8 <= x <= cap + 8 and b[:L1] == TC.revcomp(a)[:L2]]
    assert len(back) >= 10 and any(TC.pairing_cells(a, b) > cap for a, b in back) and any(TC.pairing_cells(a, b) <= cap for a, b in back)


def test_structure_and_alphabet_groups_hold_what_they_are_for():
    g = TC.groups()
    st = set(g["structure"])
    for n in range(1, TC.WAVE_LEN_CAP + 1):
        assert ("A" * n, "T" * n) in st and ("G" * n, "C" * n) in st
    sym = [(a, b) for a, b in g["structure"] if all(len(s) % 2 == 0 and s == TC.revcomp(s) and "N" not in s for s in (a, b))]
    assert len(sym) >= 150
    assert any(a.startswith("N") for a, _ in st) and any(a.endswith("N") for a, _ in st) and any(set(a) == {"N"} == set(b) for a, b in st)
    al = g["alphabet"]
    assert any(a.islower() for a, _ in al) and any("U" in a for a, _ in al) and any("u" in b for _, b in al)
    assert sum(1 for a, b in al if set((a + b).upper()) - set("ACGTNU")) >= 100
    ls = g["long_x_short"]
    assert len(ls) == 200 and all(max(len(a), len(b)) > 60 and min(len(a), len(b)) <= 60 for a, b in ls)
    assert sum(1 for a, b in ls if len(a) > 60) == sum(1 for a, b in ls if len(b) > 60) == 100
    assert {len(a) for a, b in g["long_49_64"] if len(a) > 48} >= set(range(49, 65))
    assert all(len(a) > 60 and len(b) > 60 for a, b in g["both_over_60"])


@needs_ref
def test_the_reference_answers_every_pair_but_the_refused_group():
    total = 0
    for name, pairs in TC.groups().items():
        want = TE.expected(name)
        assert len(want) == len(pairs)
        total += len(want)
        refused = [p for p, w in zip(pairs, want) if not w[3]]
        if name in TC.REFUSED_GROUPS:
            assert len(refused) == len(pairs) and all(w[0] == TE.hexd(-999999.0) for w in want)   # THAL_ERROR_SCORE
        else:
            assert not refused, (name, refused[:3])
    for env in TC.ENVS:
        want = TE.expected("env", env)
        assert len(want) == len(TC.env_pairs()) == TC.N_ENV and all(w[3] for w in want)
        total += len(want)
    assert total == sum(len(v) for v in TC.groups().values()) + len(TC.ENVS) * TC.N_ENV


@needs_ref
def test_the_environments_change_the_known_answer_as_the_reference_says():
    """the SURVEY.md known-answer primer against its complement; the four added settings as the reference answered them when the
    corpus was designed (two decimals), so that an environment that never reaches thal() cannot pass as two equal mistakes"""
    assert TC.env_pairs()[0][0] == "GCCCCATAGGTTTTGAACTCA"
    import struct
    t = {env: struct.unpack(">d", bytes.fromhex(TE.expected("env", env)[0][0]))[0] for env in TC.ENVS}
    assert repr(t["default"]) == "58.12604603130177"
    assert ["%.2f" % t[e] for e in ("no_divalent", "dntp_above_dv", "low", "high")] == ["52.23", "52.23", "29.67", "73.69"]


@needs_ref
def test_host_build_of_the_sequential_formulation_equals_the_reference_on_the_corpus():
    compared, cutoff = 0, []
    for name, pairs in TC.groups().items():
        got = TE.host_values(pairs, TC.ENVS["default"], cutoff)
        bad = TE.mismatches(got, TE.expected(name))
        assert not bad, (name, [(pairs[i], got[i], TE.expected(name)[i]) for i in bad[:3]])
        compared += len(got)
    for env in TC.ENVS:
        got = TE.host_values(TC.env_pairs(), TC.ENVS[env], cutoff)
        bad = TE.mismatches(got, TE.expected("env", env))
        assert not bad, (env, [(TC.env_pairs()[i], got[i], TE.expected("env", env)[i]) for i in bad[:3]])
        compared += len(got)
    assert compared == len(cutoff) == sum(len(v) for v in TC.groups().values()) + len(TC.ENVS) * TC.N_ENV
    # candidates below the entropy cut-off that win (thal.h:1322-1330; thal_wave.hpp hands such pairs back): the corpus holds
    # exactly the pairs of CUTOFF_PAIRS that do this (thal section)
    assert sum(1 for c in cutoff if c) == len(TC.CUTOFF_PAIRS)


@pytest.mark.parametrize("name", ["thal_vectors.json", "thal_vectors_long.json"])
def test_host_build_of_the_sequential_formulation_equals_the_golden_vectors(name):
    g = json.load(open(os.path.join(GOLD, name)))
    p = g["params"]
    assert p["temp_c"] == 37.0
    got = TE.host_values([(v[0], v[1]) for v in g["vectors"]], p)
    want = [(v[2], v[3], v[4], bool(v[5])) for v in g["vectors"]]
    bad = TE.mismatches(got, want)
    assert not bad, [(g["vectors"][i], got[i]) for i in bad[:3]]
