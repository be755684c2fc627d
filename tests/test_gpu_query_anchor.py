"""dg_query_map_anchored / FmIndex.query_mappability(anchor=) against the brute-force references of tests/query_anchor_ref.py, which know
nothing of the FM-index: every record shape on the session genome across the K-mer table order and every anchor at which the search takes
another path (inside, at and behind the table's order, k-1 and k), with the K-mer table reads counted; a = 0 and a = k against the
unanchored call; max_count; long k-mers around every 8-byte edge of the narrow finish's byte mask; the edges of the text; the open flags
and development-build switches; the argument checks; and the orientation pinned by hand."""
import ctypes as C
import random

import numpy as np
import pytest

import conftest
import dicey_amd
import query_anchor_ref as A
import query_map_ref as Q
import mappability_ref as R
from conftest import genome_text, revcomp
from dicey_amd import _capi

pytestmark = pytest.mark.gpu
INV = Q.INVALID
KS, ES, TABLE_K = (12, 16, 20), (0, 1, 2), 16


def _anchors(k):
    return sorted({a for a in (0, 1, 5, 9, 15, 16, 17, k - 1, k) if a <= k})


def _same(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for i, (g, x) in enumerate(zip(got, exp)):
        assert g.dtype == np.uint32 and len(g) == len(x), (what, i)
        bad = np.nonzero(g != x)[0]
        assert len(bad) == 0, (what, i, len(bad), bad[:10], g[bad[:10]], x[bad[:10]])


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def small_k16(small_genome, monkeypatch_module):
    """the session genome opened with a K-mer table of order 16: k = 12 lies below the table's order, 16 at it, 20 above"""
    monkeypatch_module.setenv("DICEY_KMER_K", "16")
    ix = dicey_amd.FmIndex(small_genome["fm9"])
    monkeypatch_module.delenv("DICEY_KMER_K")
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def shapes(small_genome):
    """the records and, computed once, the ball reference's parts per (k, e, a): all anchors of a (k, e) in one pass over the masks"""
    recs = A.record_set(small_genome["seqs"])
    qbuf, _ = Q.buffer_of(recs)
    parts = {}
    for k in KS:
        for e in ES:
            for a, p in A.parts_ball(small_genome["text"], qbuf, k, e, _anchors(k)).items():
                parts[k, e, a] = p
    return {"recs": recs, "parts": parts}


def _exp(shapes, k, e, a, fo=False, cap=0):
    return Q.split(Q.finish(*shapes["parts"][k, e, a], fo, cap), shapes["recs"])


# ---- session genome --------------------------------------------------------------------------------------------------------------

def test_inputs_exercise_the_feature(shapes):
    """conditions on the INPUTS, shown on the reference alone: at every (k, e, a) the anchor removes places on each strand and leaves
    places that e = 0 does not have"""
    recs = shapes["recs"]
    assert len(recs[0]) == 3000 and b"N" in recs[0] and len(recs[12]) == 0 and recs[13].islower() and len(recs[11]) == 9
    for k in KS:
        f0, r0, valid = shapes["parts"][k, 0, 0]
        for e in (1, 2):
            fu, ru, _ = shapes["parts"][k, e, 0]
            for a in (1, 5, 9, k - 1):
                f, r, _ = shapes["parts"][k, e, a]
                n = ((f < fu)[valid].sum(), (r < ru)[valid].sum(), ((f + r) > (f0 + r0))[valid].sum())
                assert min(n) >= 40, (k, e, a, n)
        per = _exp(shapes, k, 1, 1)
        assert per[0][0] != INV and per[-1][len(per[-1]) - k] != INV and (per[-1][len(per[-1]) - k + 1:] == INV).all()
        assert (per[11] == INV).all() and (per[13] == INV).all() and (per[8 + KS.index(k)] != INV).sum() == 1


@pytest.mark.parametrize("k", KS)
def test_session_genome_every_anchor(shapes, small_k16, k):
    npos = sum(len(r) for r in shapes["recs"])
    for e in ES:
        for a in _anchors(k):
            for fo in (False, True):
                st = {}
                got = small_k16.query_mappability(shapes["recs"], k=k, mismatches=e, forward_only=fo, anchor=a, stats=st)
                _same(got, _exp(shapes, k, e, a, fo), (k, e, a, fo))
                nvalid = int(shapes["parts"][k, e, a][2].sum())
                assert st["positions"] == npos and st["valid"] == nvalid and st["launches"] >= 1 and st["early_exits"] == 0
                assert st["ms_total"] == pytest.approx(st["ms_valid"] + st["ms_search"], rel=1e-9)
                assert st["table_reads"] == nvalid * A.table_reads(k, e, a, TABLE_K, fo), (k, e, a, fo)


def test_anchor_0_and_anchor_k(shapes, small_k16):
    recs = shapes["recs"]
    for k in KS:
        exact = {fo: small_k16.query_mappability(recs, k=k, forward_only=fo) for fo in (False, True)}
        for e in ES:
            for fo in (False, True):
                _same(small_k16.query_mappability(recs, k=k, mismatches=e, forward_only=fo, anchor=0),
                      small_k16.query_mappability(recs, k=k, mismatches=e, forward_only=fo), (k, e, fo, "a = 0"))
                _same(small_k16.query_mappability(recs, k=k, mismatches=e, forward_only=fo, anchor=k), exact[fo], (k, e, fo, "a = k"))


def test_max_count(shapes, small_k16):
    recs, k = shapes["recs"], 16
    for e in ES:
        for a in (5, 15):
            full = _exp(shapes, k, e, a)
            for cap in (1, 2):
                st = {}
                got = small_k16.query_mappability(recs, k=k, mismatches=e, max_count=cap, anchor=a, stats=st)
                _same(got, _exp(shapes, k, e, a, False, cap), (e, a, cap))
                _same(got, [np.where(x == INV, INV, np.minimum(x, cap)).astype(np.uint32) for x in full], (e, a, cap, "min"))
                assert st["early_exits"] == sum(int(((x != INV) & (x >= cap)).sum()) for x in full) > 0


# ---- long k ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [64, 100])
def test_long_kmers(small_genome, k, tmp_path):
    """k above 32 against the diagonal reference on the 12 kb cut-and-twin genome of test_gpu_query_map.test_long_kmers: the twin's
    substitution at offset 150 makes windows whose only mismatch sits on either side of every 8-byte edge of the byte mask"""
    t = small_genome["text"][:12000].replace(b"\n", b"N").decode()
    a0 = next(a for a in range(1000, 6000) if set(t[a:a + 400]) <= set("ACGT"))
    src = t[a0:a0 + 400]
    twin = src[:150] + ("A" if src[150] != "A" else "C") + src[151:]
    text = genome_text([t[:7000] + twin + t[7000:], t[8000:9000] + revcomp(twin) + "ACGTTGCAAC"])
    path = str(tmp_path / "cut.fm9")
    dicey_amd.build_index(text, path)
    recs = [src.encode(), twin.encode(), (src[:230] + twin[100:]).encode()]
    qbuf, _ = Q.buffer_of(recs)
    anchors = [0] + sorted({1, 7, 8, 9, 16, 17, 33, k - 1})
    parts = A.parts_diagonal(text, qbuf, k, (0, 1), anchors)
    v0 = parts[0, 0][0] + parts[0, 0][1]
    for a in anchors[1:]:
        va, vu = parts[1, a][0] + parts[1, a][1], parts[1, 0][0] + parts[1, 0][1]
        assert (va < vu).sum() >= a and (va > v0).sum() >= k - a, (k, a)  # the anchor rejects windows and keeps others
    with dicey_amd.FmIndex(path) as ix:
        for e in (0, 1):
            for a in anchors[1:]:
                for fo in (False, True):
                    _same(ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo, anchor=a), Q.split(Q.finish(*parts[e, a], fo), recs), (k, e, a, fo))


# ---- the edges of the text ---------------------------------------------------------------------------------------------------------

def test_edges_of_the_text(tmp_path):
    rng = random.Random(77)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    x10 = rnd(10)
    c1 = rnd(1500) + "N" + rnd(800) + x10 + revcomp(x10) + rnd(700)
    c2 = rnd(2000)
    text, k = genome_text([c1, c2]), 20
    fm9 = str(tmp_path / "edge.fm9")
    dicey_amd.build_index(text, fm9)
    recs = [c1[-10:] + c2[:10],                  # across the '\n' between two sequences
            c1[1490:1500] + "A" + c1[1501:1511],  # around the genome's N, the N replaced
            rnd(5) + c1[:15],                     # the window would start five characters before position 0
            revcomp(rnd(5) + c1[:15]),
            c1[:20], c2[-20:]]                   # and the first and last windows themselves
    assert text[1500:1501] == b"N" and text[len(c1):len(c1) + 1] == b"\n"
    recs = [r.encode() for r in recs]
    qbuf, _ = Q.buffer_of(recs)
    with dicey_amd.FmIndex(fm9) as ix:
        for e in ES:
            parts = A.parts_ball(text, qbuf, k, e, [1, 10])
            for a in (1, 10):
                exp = Q.split(Q.finish(*parts[a]), recs)
                assert [int(x[0]) for x in exp] == [0, 0, 0, 0, 1, 1], (e, a)  # the reference alone: none of the first four is counted
                for fo in (False, True):
                    _same(ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo, anchor=a), Q.split(Q.finish(*parts[a], fo), recs), (e, a, fo))


# ---- paths -----------------------------------------------------------------------------------------------------------------------

def test_open_flags_give_identical_arrays(shapes, small_genome):
    for kw in ({"kmer_table": False}, {"compact": True}, {"compact": True, "pre5": False}):
        with dicey_amd.FmIndex(small_genome["fm9"], **kw) as ix:
            for e in ES:
                _same(ix.query_mappability(shapes["recs"], k=20, mismatches=e, anchor=5), _exp(shapes, 20, e, 5), (kw, e))


def test_switches_of_the_development_build(shapes, small_genome, monkeypatch):
    """DICEY_QMAP_CHUNK (positions per launch) and DICEY_MAP_NARROW (W) change how the search runs, never what it returns"""
    recs, k, a = shapes["recs"], 20, 5
    npos = sum(len(r) + 1 for r in recs)
    ix = dicey_amd.FmIndex(small_genome["fm9"], _lib=conftest.exp_lib())
    try:
        seen = {}
        for name, env in (("default", {}), ("chunk", {"DICEY_QMAP_CHUNK": "64"}), ("never", {"DICEY_MAP_NARROW": "0"}),
                          ("always", {"DICEY_MAP_NARROW": "1000000000"})):
            for kk, vv in env.items():
                monkeypatch.setenv(kk, vv)
            for e in ES:
                st = {}
                _same(ix.query_mappability(recs, k=k, mismatches=e, anchor=a, stats=st), _exp(shapes, k, e, a), (name, e))
                seen[name, e] = st
            _same(ix.query_mappability(recs, k=k, mismatches=1, max_count=2, forward_only=True, anchor=a), _exp(shapes, k, 1, a, True, 2), (name, "cap"))
            for kk in env:
                monkeypatch.delenv(kk)
        for e in ES:
            assert seen["default", e]["launches"] == 1 and seen["default", e]["verified_rows"] > 0
            assert seen["chunk", e]["launches"] == -(-npos // 64) and seen["never", e]["launches"] == 1 and seen["always", e]["launches"] == 1
            assert seen["never", e]["verified_rows"] == 0 and seen["never", e]["steps"] > 0
            assert seen["always", e]["steps"] == 0 and seen["always", e]["verified_rows"] > 0
            assert len({s["valid"] for (_, ee), s in seen.items() if ee == e}) == 1
    finally:
        ix.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_argument_checks(small_genome):
    L = _capi.load()
    EINVAL, ELIMIT = -1, -7
    seq = small_genome["seqs"][0][:40].encode()
    off = (C.c_uint64 * 2)(0, 40)
    vals = (C.c_uint32 * 40)(*([0xABCD1234] * 40))

    def prm(k=20, e=0, a=5, flags=0, res=(0, 0)):
        return _capi.QmapAnchorParams(k, e, a, 0, 0, flags, (C.c_uint32 * 2)(*res))

    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        h = ix.handle

        def call(p, handle=h, s=seq, o=off, n=1, v=vals, st=None):
            rc = L.dg_query_map_anchored(handle, C.byref(p) if p is not None else None, s, o, n, v, st)
            if rc:
                assert L.dg_last_error() and b"dg_query_map_anchored" in L.dg_last_error()
            return rc

        assert call(None) == EINVAL
        assert call(prm(flags=1)) == EINVAL
        for r in ((1, 0), (0, 1)):
            assert call(prm(res=r)) == EINVAL
        assert call(prm(k=9)) == ELIMIT and call(prm(k=1001)) == ELIMIT and call(prm(e=3)) == ELIMIT
        assert call(prm(a=21)) == ELIMIT and call(prm(k=10, a=11)) == ELIMIT  # anchor = k + 1
        big = (C.c_uint64 * 2)(0, 1 << 31)
        assert call(prm(), o=big) == ELIMIT
        assert call(prm(), o=(C.c_uint64 * 2)(0, (1 << 31) - 1)) == ELIMIT  # with its separator
        assert call(prm(), handle=None) == EINVAL
        assert call(prm(), s=None) == EINVAL and call(prm(), o=None) == EINVAL and call(prm(), v=None) == EINVAL
        assert call(prm(), o=(C.c_uint64 * 3)(0, 30, 20), n=2) == EINVAL
        # the order: parameter block, limits, then the handle
        assert call(prm(k=9, flags=1)) == EINVAL and call(prm(a=21), handle=None) == ELIMIT and call(prm(), o=big, handle=None) == ELIMIT
        assert list(vals) == [0xABCD1234] * 40
        # nothing to do is not an error, and writes nothing
        st = _capi.QmapStats()
        assert call(prm(), n=0, st=C.byref(st)) == 0 and call(prm(), s=None, o=None, n=0, v=None) == 0
        assert call(prm(), o=(C.c_uint64 * 3)(0, 0, 0), n=2, st=C.byref(st)) == 0 and st.positions == 0 and st.launches == 0
        assert list(vals) == [0xABCD1234] * 40
        assert call(prm(a=20), st=C.byref(st)) == 0 and st.positions == 40 and st.valid == R.valid_positions(seq, 20).sum() and st.launches == 1
        assert list(vals) == [int(x) for x in Q.values(small_genome["text"], [seq], 20, 0)[0]] and list(vals[21:]) == [INV] * 19
        with pytest.raises(dicey_amd.DgError) as err:
            ix.query_mappability([seq], k=20, anchor=21)
        assert err.value.code == ELIMIT and "dg_query_map_anchored" in str(err.value)


# ---- orientation -----------------------------------------------------------------------------------------------------------------

def test_orientation_pinned_by_hand(tmp_path):
    """the anchored bases are the LAST a of the oligo; on the other strand the text shows them as the first a of the window"""
    rng = random.Random(12)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    text = genome_text([rnd(1000) + "GATTACAGGCTTCAAGTCCA" + rnd(1000)])
    table = [(b"GATTACAGGCTTCAAGTCCC", 0),   # X with its last base changed
             (b"CATTACAGGCTTCAAGTCCA", 1),   # X with its first base changed
             (b"TGGACTTGAAGCCTGTAATG", 0),   # revcomp(X) with its last base changed
             (b"AGGACTTGAAGCCTGTAATC", 1)]   # revcomp(X) with its first base changed
    recs = [w for w, _ in table]
    assert [int(v[0]) for v in Q.values(text, recs, 20, 1)] == [1, 1, 1, 1]  # X once, nothing else near it
    path = str(tmp_path / "x.fm9")
    dicey_amd.build_index(text, path)
    with dicey_amd.FmIndex(path) as ix:
        got = ix.query_mappability(recs, k=20, mismatches=1, anchor=1)
        assert [int(g[0]) for g in got] == [v for _, v in table]
        assert [int(g[0]) for g in ix.query_mappability(recs, k=20, mismatches=1, anchor=1, forward_only=True)] == [0, 1, 0, 0]
        assert [int(g[0]) for g in ix.query_mappability(recs, k=20, mismatches=1, anchor=0)] == [1, 1, 1, 1]
