"""Conditions on the INPUTS of tests/test_gpu_query_iupac.py, shown on the brute-force model of tests/query_iupac_ref.py alone (no GPU): the
record set on the session genome makes a degenerate letter matter in every way the kernel can get wrong, and the model's own arithmetic
(complement table, degeneracy) is pinned by hand.

Measured on this record set (3142 positions; k = 12 / 16 / 20; e = 0..2; max_degeneracy 4096): valid positions 2895 / 2850 / 2809;
non-zero values >= 1796 everywhere; both strands non-zero >= 15; differs from `first` >= 99 at every (k, e), from `wild` >= 18; `dbl` >= 666
at every k for e >= 1; anchor 5 lowers the value at >= 267 positions at every k for e >= 1; valid at max_degeneracy 64: 2892 / 2847 / 2808."""
import numpy as np
import pytest

import query_iupac_ref as I
from conftest import genome_text, make_genome

KS, ES = I.KS, I.ES


@pytest.fixture(scope="module")
def model():
    """the session genome of conftest.small_genome (the same generator call; no index is needed here), the model and its two wrong variants"""
    seqs = make_genome(101, 3, 30000, iupac=True)
    text = genome_text(seqs)
    s = I.session(seqs, text)
    only0 = {k: [0] for k in KS}
    out = dict(s)
    out["first"], _ = I.parts(text, s["qbuf"], KS, ES, only0, variant="first")
    out["wild"], _ = I.parts(text, s["qbuf"], KS, ES, only0, variant="wild")
    return out


def _tot(p, key):
    return p[key][0] + p[key][1]


def test_the_record_set():
    seqs = make_genome(101, 3, 30000, iupac=True)
    recs = I.record_set(seqs)
    assert [len(r) for r in recs[:6]] == [600, 600, 400, 600, 400, 25] and [len(r) for r in recs[6:11]] == [12, 16, 20, 9, 0] and len(recs[-1]) == 300
    assert set(recs[-1]) <= set(b"ACGT") and recs[11].islower() and b"U" in recs[12] and recs[5] == I.TOO_DEGENERATE.encode()
    codes = lambda r: sum(int(I.POP[I.SETS[chr(c)]] > 1) for c in r)
    every = lambda n, step: len(range(step // 2, n, step))
    assert [codes(recs[i]) for i in range(5)] == [every(600, 23), every(600, 11), every(400, 29), every(600, 23), every(400, 7)] == [26, 55, 14, 26, 57]
    assert recs[2].count(b"N") == 14 and codes(recs[6]) == codes(recs[7]) == 1 and codes(recs[8]) == 0
    # a miss code excludes the base it replaces, a hit code holds it
    s2 = seqs[1]
    b = I._clean(s2, 5000, 600)
    assert all(x == ord(y) or not (I.SETS[chr(x)] & I.SETS[y]) for x, y in zip(recs[0], s2[b:b + 600]))
    assert sum(x != ord(y) for x, y in zip(recs[0], s2[b:b + 600])) == 26


def test_inputs_exercise_the_feature(model):
    right, first, wild, dbl = model["parts"], model["first"], model["wild"], model["dbl"]
    for k, nvalid, n64 in zip(KS, (2895, 2850, 2809), (2892, 2847, 2808)):
        letters, deg = I.degeneracy(model["qbuf"], k)
        valid = right[k, 0, 0][2]
        assert valid.sum() == nvalid and (letters & (deg <= 64)).sum() == n64 and (letters & ~valid).sum() == 5
        for e in ES:
            f, r, _ = right[k, e, 0]
            tot = f + r
            n = {"nonzero": int((tot > 0)[valid].sum()), "both": int(((f > 0) & (r > 0))[valid].sum()),
                 "first": int((tot != _tot(first, (k, e, 0)))[valid].sum()), "wild": int((tot != _tot(wild, (k, e, 0)))[valid].sum()),
                 "dbl": int(dbl[k, e].sum()), "anchor": int((_tot(right, (k, e, 5)) < tot)[valid].sum())}
            print(k, e, n)
            assert n["nonzero"] >= 1700 and n["both"] >= 15 and n["first"] >= 40 and n["wild"] >= 15, (k, e, n)
            if e >= 1:
                assert n["dbl"] >= 40 and n["anchor"] >= 40, (k, e, n)
            else:
                assert n["dbl"] == 0 and n["anchor"] == 0, (k, e, n)  # at e = 0 every letter is inside its set: nothing to count twice or to anchor
            assert (_tot(right, (k, e, k)) == _tot(right, (k, 0, 0))).all()  # anchor k: the e = 0 values
            assert (_tot(right, (k, e, 1)) <= tot).all() and (_tot(right, (k, e, 5)) <= _tot(right, (k, e, 1))).all()


def test_too_degenerate_record(model):
    """INVALID exactly where a window covers more than six of the record's seven N's"""
    recs = model["recs"]
    off = sum(len(r) + 1 for r in recs[:5])
    for k in KS:
        valid = model["parts"][k, 0, 0][2]
        for p in range(len(I.TOO_DEGENERATE)):
            w = I.TOO_DEGENERATE[p:p + k]
            assert bool(valid[off + p]) == (len(w) == k and w.count("N") <= 6), (k, p)
        assert sum(I.TOO_DEGENERATE[p:p + k].count("N") == 7 for p in range(len(I.TOO_DEGENERATE) - k + 1)) == 5


def test_edge_records(model):
    recs = model["recs"]
    for k in KS:
        per = [model["parts"][k, 0, 0][2][o:o + len(r)] for o, r in zip(np.cumsum([0] + [len(r) + 1 for r in recs[:-1]]), recs)]
        assert [int(per[6 + i].sum()) for i in range(3)] == [int(kk >= k) * (kk - k + 1) for kk in (12, 16, 20)]  # records of exactly 12, 16, 20
        assert per[9].sum() == 0 and len(per[10]) == 0 and per[11].sum() == 0  # shorter than k, empty, lower case
        assert per[12].sum() == max(0, 30 - k + 1) + max(0, 29 - k + 1) and not per[12][30]  # U ends a k-mer like any other byte
        assert per[0][0] and per[-1][300 - k] and not per[-1][300 - k + 1:].any()


def test_complement_table():
    pairs = {"A": "T", "C": "G", "R": "Y", "K": "M", "B": "V", "D": "H", "S": "S", "W": "W", "N": "N"}
    for a, b in pairs.items():
        assert I.complement(a) == b and I.complement(b) == a
    assert sorted(I.SETS) == sorted("ACGTRYSWKMBDHVN") and len(set(I.SETS.values())) == 15
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for c in I.SETS:
        members = {b for b in "ACGT" if I.SETS[b] & I.SETS[c]}
        assert {b for b in "ACGT" if I.SETS[b] & I.SETS[I.complement(c)]} == {comp[b] for b in members}
        assert int(I.COMP_MASK[I.COMP_MASK[I.SETS[c]]]) == I.SETS[c]
    assert I.revcomp("ACRYKMBDHVSWN") == "NWSBDHVKMRYGT"
    assert [sorted(b for b in "ACGT" if I.SETS[b] & I.SETS[c]) for c in "RYSWKM"] == [list(x) for x in ("AG", "CT", "CG", "AT", "GT", "AC")]
    assert ["".join(b for b in "ACGT" if I.SETS[b] & I.SETS[c]) for c in "BDHV"] == ["CGT", "AGT", "ACT", "ACG"]


def test_degeneracy_arithmetic():
    assert I.deg("ACGT") == 1 and I.deg("ACRT") == 2 and I.deg("NNB") == 48 and I.deg("ACGU") == 0 and I.deg("acgt") == 0
    assert I.deg(I.TOO_DEGENERATE) == 16384 and I.deg("N" * 6) == 4096
    assert I.expansions("ARC") == ["AAC", "AGC"] and len(I.expansions("NBR")) == 24 == len(set(I.expansions("NBR")))
    buf = b"ACRTNNB\nHHVDBACGTAC\n"
    for k in (2, 3, 5):
        letters, d = I.degeneracy(buf, k)
        for p in range(len(buf)):
            w = buf[p:p + k].decode()
            exp = I.deg(w) if len(w) == k and "\n" not in w else 0
            assert int(d[p]) == exp and bool(letters[p]) == (exp > 0), (k, p)
    # nine three-letter codes: 3^9 = 19683, exact in the log-sum
    assert int(I.degeneracy(b"BDHVBDHVB", 9)[1][0]) == 19683
    first = I.query_sets(b"ACGTRYSWKMBDHVN", "first")
    assert [int(x) for x in first] == [1, 2, 4, 8, 1, 2, 2, 1, 4, 1, 2, 1, 1, 1, 1]
    assert [int(x) for x in I.query_sets(b"ACGTRBN", "wild")] == [1, 2, 4, 8, 15, 15, 15]
