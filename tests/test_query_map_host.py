"""The two references of tests/query_map_ref.py against each other and against the genome track's reference (CPU only): what the GPU tests
of dg_query_map compare with is itself checked here."""
import random

import numpy as np
import pytest

import mappability_mm_ref as M
import mappability_ref as R
import query_map_ref as Q
from conftest import genome_text, make_genome, revcomp


def _subst(s, every, rng):
    s = list(s)
    for i in range(every // 2, len(s), every):
        if s[i] in "ACGT":
            s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
    return "".join(s)


def _clean(seq, start, m):
    """the first position >= start from which m characters are all A/C/G/T"""
    return next(a for a in range(start, len(seq) - m) if set(seq[a:a + m]) <= set("ACGT"))


@pytest.fixture(scope="module")
def case():
    """a 6 kb text of two sequences (N runs, IUPAC letters, copied segments) and 2 kb of query records"""
    rng = random.Random(7)
    seqs = make_genome(31, 2, 3000, nrate=0.004, iupac=True)
    text = genome_text(seqs)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    s0, s1 = seqs
    # a 600-nt cut with clean ends and an N inside
    a = next(a for a in range(200, 2000) if "N" in s0[a:a + 600] and set(s0[a:a + 40] + s0[a + 560:a + 600]) <= set("ACGT"))
    b, c = _clean(s1, 200, 400), _clean(s1, 1000, 400)
    j0, j1 = _clean(s0, 100, 60), _clean(s1, 2000, 60)
    recs = [s0[a:a + 600], revcomp(s1[b:b + 400]), _subst(s1[c:c + 400], 13, rng), s0[j0:j0 + 60] + s1[j1:j1 + 60], rnd(300), "", rnd(11),
            s0[2000:2100].lower(), "ACGTNNACGTRYACGTACGTACGTACGTACGTACGTACGTACGT"]
    assert 1900 <= sum(map(len, recs)) <= 2100
    return {"text": text, "seqs": seqs, "recs": [r.encode() for r in recs], "cut": (a, a + 600)}


@pytest.mark.parametrize("k", [12, 20, 32])
def test_the_two_references_agree(case, k):
    qbuf, _ = Q.buffer_of(case["recs"])
    diag = Q.parts_diagonal(case["text"], qbuf, k, (0, 1, 2))
    seen = 0
    for e in (0, 1, 2):
        fb, rb, vb = Q.parts_ball(case["text"], qbuf, k, e)
        fd, rd, vd = diag[e]
        assert (vb == vd).all()
        assert (fb == fd).all() and (rb == rd).all(), (k, e)
        seen += int((fb + rb)[vb].sum())
        for fo in (False, True):
            a = Q.values(case["text"], case["recs"], k, e, forward_only=fo, max_count=3)
            b = Q.split(Q.finish(fd, rd, vd, fo, 3), case["recs"])
            assert [len(x) for x in a] == [len(r) for r in case["recs"]]
            assert all((x == y).all() for x, y in zip(a, b))
    assert seen > 1000
    # the lower-case record and the one shorter than k are invalid everywhere, the empty one has no position
    vals = Q.values(case["text"], case["recs"], k, 1)
    assert (vals[7] == Q.INVALID).all() and (vals[6] == Q.INVALID).all() and len(vals[5]) == 0
    assert (vals[0][-(k - 1):] == Q.INVALID).all() and vals[0][len(vals[0]) - k] != Q.INVALID


@pytest.mark.parametrize("k", [12, 20, 32])
def test_a_cut_of_the_text_has_the_genome_track_values(case, k):
    a, b = case["cut"]
    for e in (0, 1, 2):
        track = M.values(case["text"], k, e)
        for method in ("ball", "diagonal"):
            got = Q.values(case["text"], case["recs"][:1], k, e, method=method)[0]
            inside = np.arange(0, b - a - k + 1)
            ok = got[inside] != Q.INVALID
            assert ok.sum() >= 200 and (~ok).sum() >= k and (ok == R.valid_positions(case["text"], k)[a + inside]).all()
            assert (got[inside][ok] == track[a + inside][ok]).all(), (k, e, method)
            assert (track[a + inside][ok] >= 1).all()


def test_a_junction_is_absent_from_the_genome(case):
    k = 20
    v0 = Q.values(case["text"], case["recs"], k, 0)[3]
    span = np.arange(60 - k + 1, 60)  # windows that hold characters of both 60-mers
    assert len(span) == k - 1 and (v0[span] == 0).all()
    assert (v0[:60 - k + 1] >= 1).all() and (v0[60:120 - k + 1] >= 1).all() and (v0[120 - k + 1:] == Q.INVALID).all()
    assert (Q.values(case["text"], case["recs"], k, 0, method="diagonal")[3] == v0).all()


def test_bedgraph_keeps_zero_runs_and_drops_invalid_ones():
    I = Q.INVALID
    vals = [np.array([0, 0, 1, 1, I, I, 0, 2], dtype=np.uint32), np.zeros(0, np.uint32), np.array([I, I], dtype=np.uint32), np.array([5], dtype=np.uint32)]
    assert Q.bedgraph(vals, ["a", "b", "c", "d"]) == b"a\t0\t2\t0\na\t2\t4\t1\na\t6\t7\t0\na\t7\t8\t2\nd\t0\t1\t5\n"
