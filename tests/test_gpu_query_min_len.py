"""dg_query_min_len / FmIndex.query_min_length against the linear-scan reference of tests/query_min_len_ref.py, which knows nothing of the
FM-index and does not assume that values fall with k: every record shape on the session genome across the K-mer table order, e, t, the
strand setting and two (min_k, max_k) pairs (the expected values shown, on the reference alone, to hold every class of answer); long
k-mers against the dict route; a scan of dg_query_map on the device on a genome of a few Mb; dg_min_unique for cuts of the genome; the
switches of the development build, the argument checks and the stats."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import conftest
import dicey_amd
import query_map_ref as Q
import query_min_len_ref as ML
from conftest import revcomp
from dicey_amd import _capi

pytestmark = pytest.mark.gpu
INV = ML.INVALID
ES, TS = (0, 1, 2), (0, 1, 2)
RANGES = ((10, 24), (12, 16))


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
def indices(small_genome, monkeypatch_module):
    """the session genome with the default K-mer table and with one of order 16: with min_k = 10 and max_k = 24 one lane's probes lie
    below the table's order, at it and above it"""
    dflt = dicey_amd.FmIndex(small_genome["fm9"])
    monkeypatch_module.setenv("DICEY_KMER_K", "16")
    k16 = dicey_amd.FmIndex(small_genome["fm9"])
    monkeypatch_module.delenv("DICEY_KMER_K")
    yield {"default": dflt, "K16": k16}
    dflt.close()
    k16.close()


@pytest.fixture(scope="module")
def shapes(small_genome):
    """the record set and, computed once and left unchanged, the brute-force parts per (k, e) that every expectation is scanned from"""
    text = small_genome["text"]
    recs = ML.record_set(small_genome["seqs"], text, 10, 24)
    qbuf, offs = Q.buffer_of(recs)
    parts = {e: ML.parts_by_k(text, qbuf, range(10, 25), e) for e in ES}
    return {"recs": recs, "qbuf": qbuf, "offs": offs, "parts": parts, "run": ML.run_lengths(qbuf)}


def _exp_buf(shapes, e, t, fo=False, rng=(10, 24)):
    return ML.min_len(shapes["parts"][e], shapes["qbuf"], rng[0], rng[1], t, fo)


def _exp(shapes, e, t, fo=False, rng=(10, 24)):
    return ML.split(_exp_buf(shapes, e, t, fo, rng), shapes["recs"])


# ---- session genome --------------------------------------------------------------------------------------------------------------

def test_expected_values_hold_every_class(shapes):
    """a condition on the INPUTS, shown on the reference alone: no test below can pass on a degenerate expectation"""
    lo, hi = 10, 24
    limit = np.minimum(shapes["run"], hi)
    recs = shapes["recs"]
    assert shapes["offs"][0] == 0 and len(recs[0]) == 3000 and b"N" in recs[0] and b"" in recs
    for e in ES:
        assert ML.violations(shapes["parts"][e], lo, hi) == 0
        for t in (0, 1):
            v = _exp_buf(shapes, e, t)
            assert (v == INV).sum() >= 100 and (v == 0).sum() >= 100, (e, t)
            assert ((v > lo) & (v < hi)).sum() >= 100, (e, t)
            assert (e, t) == (2, 0) or (v == hi).sum() >= 1, (e, t)
            assert e == 2 or (v == lo).sum() >= 1, (e, t)
            # an answer at the end of a run that a record end or an N cut short
            assert ((v == limit) & (limit < hi) & (v != 0) & (v != INV)).sum() >= 1, (e, t)
    per = _exp(shapes, 0, 1)
    assert (per[9] == INV).all() and (per[11] == INV).all() and len(per[10]) == 0      # 9 nt, lower case, empty
    assert (per[5] != INV).sum() == 1 and (per[6] != INV).sum() == 24 - 10 + 1          # exactly min_k, exactly max_k
    assert per[-1][len(per[-1]) - 10] != INV and (per[-1][len(per[-1]) - 9:] == INV).all()


@pytest.mark.parametrize("e", ES)
def test_session_genome_every_shape(shapes, indices, e):
    npos = sum(len(r) for r in shapes["recs"])
    for rng in RANGES:
        for t in TS:
            for fo in (False, True):
                exp = _exp(shapes, e, t, fo, rng)
                for name, ix in indices.items():
                    st = {}
                    got = ix.query_min_length(shapes["recs"], max_k=rng[1], min_k=rng[0], at_most=t, mismatches=e, forward_only=fo, stats=st)
                    _same(got, exp, (name, e, t, fo, rng))
                    valid = sum(int((x != INV).sum()) for x in exp)
                    found = sum(int(((x != INV) & (x != 0)).sum()) for x in exp)
                    assert st["positions"] == npos and st["valid"] == valid and st["found"] == found and st["launches"] == 1
                    assert valid <= st["probes"] <= valid * 8 and found <= valid
                    assert st["ms_total"] == pytest.approx(st["ms_valid"] + st["ms_search"], rel=1e-9)


def test_long_kmers(shapes, small_genome, indices):
    """max_k = 120 at e = 0 against the dict route: probes far above the table's order, limits cut by record ends well below max_k, and
    the genome's repeats with 120 nt of what follows them, where the answer is the distance to the repeat's end"""
    text = small_genome["text"]
    t = text.decode()
    recs = list(shapes["recs"])
    for r in shapes["recs"][12:18]:
        at = t.find(r.decode())
        ext = t[at:at + len(r) + 120]
        recs.append(ext[:(ext + "\n").index("\n")].encode())
    qbuf, _ = Q.buffer_of(recs)
    exp_buf = ML.min_len_dict(text, qbuf, 10, 120, 1)  # (t = 1: a cut of the genome is never absent from it)
    assert ((exp_buf != INV) & (exp_buf > 32)).sum() >= 100 and (exp_buf == 0).sum() >= 100 and (exp_buf == 10).sum() >= 100
    n0 = len(shapes["qbuf"])
    short = (exp_buf[:n0] <= 24) & (exp_buf[:n0] > 0)  # an answer of at most 24 is the answer of the (10, 24) scan
    assert (exp_buf[:n0][short] == _exp_buf(shapes, 0, 1)[short]).all()
    exp = ML.split(exp_buf, recs)
    for name, ix in indices.items():
        _same(ix.query_min_length(recs, max_k=120, at_most=1), exp, name)


def test_agrees_with_min_unique_for_cuts_of_the_genome(shapes, small_genome, indices):
    """e = 0, t = 1: for a cut of the genome every k-mer has a value >= 1, so "at most one place" is "unique" and the answer is the genome
    track's minimum unique length where the record is long enough for it"""
    ix = indices["K16"]
    text, lo, hi = small_genome["text"], 10, 24
    for fo in (False, True):
        mul = ix.min_unique(max_k=hi, forward_only=fo)
        got = ix.query_min_length(shapes["recs"], max_k=hi, min_k=lo, at_most=1, forward_only=fo)
        checked = 0
        for rec in (0, len(shapes["recs"]) - 1):
            at = text.find(shapes["recs"][rec])
            assert at >= 0
            g = got[rec]
            limit = np.minimum(shapes["run"][shapes["offs"][rec]:shapes["offs"][rec] + len(g)], hi)
            m = mul[at:at + len(g)].astype(np.int64)
            want = np.maximum(m, lo)
            has = (m != 0) & (want <= limit) & (limit >= lo)
            assert has.sum() >= 200 and (g[has] == want[has]).all(), (fo, rec)
            assert (g[limit < lo] == INV).all() and (g[(limit >= lo) & ~has] == 0).all()
            checked += int(has.sum())
        assert checked >= 2000


def test_a_large_at_most_gives_min_k_everywhere(shapes, indices):
    for e in ES:
        got = indices["default"].query_min_length(shapes["recs"], max_k=24, min_k=10, at_most=0xFFFFFFFD, mismatches=e)
        exp = ML.split(np.where(shapes["run"] >= 10, 10, INV).astype(np.uint32), shapes["recs"])
        _same(got, exp, e)
    low = shapes["recs"][-1].decode().lower()  # str records are upper-cased, bytes go through as given
    _same(indices["default"].query_min_length([low], max_k=24), [_exp(shapes, 0, 0)[-1]], "str")
    assert (indices["default"].query_min_length([low.encode()], max_k=24)[0] == INV).all()
    assert indices["default"].query_min_length([], max_k=24) == []


# ---- paths -----------------------------------------------------------------------------------------------------------------------

def test_switches_of_the_development_build(shapes, small_genome, monkeypatch):
    """DICEY_QMINLEN_CHUNK (positions per launch) and DICEY_MAP_NARROW (W) change how the search runs, never what it returns"""
    recs = shapes["recs"]
    npos = len(shapes["qbuf"])
    ix = dicey_amd.FmIndex(small_genome["fm9"], _lib=conftest.exp_lib())
    try:
        seen = {}
        for name, env in (("default", {}), ("chunk", {"DICEY_QMINLEN_CHUNK": "64"}), ("never", {"DICEY_MAP_NARROW": "0"}),
                          ("both", {"DICEY_QMINLEN_CHUNK": "777", "DICEY_MAP_NARROW": "1000000000"})):
            for kk, vv in env.items():
                monkeypatch.setenv(kk, vv)
            for e in ES:
                st = {}
                _same(ix.query_min_length(recs, max_k=24, at_most=1, mismatches=e, stats=st), _exp(shapes, e, 1), (name, e))
                seen[name, e] = st
            _same(ix.query_min_length(recs, max_k=16, min_k=12, mismatches=1, forward_only=True), _exp(shapes, 1, 0, True, (12, 16)), (name, "fo"))
            for kk in env:
                monkeypatch.delenv(kk)
        for e in ES:
            assert seen["default", e]["launches"] == 1 and seen["default", e]["verified_rows"] > 0
            assert seen["chunk", e]["launches"] == -(-npos // 64) and seen["both", e]["launches"] == -(-npos // 777)
            assert seen["never", e]["verified_rows"] == 0 and seen["never", e]["steps"] > 0
            assert seen["both", e]["steps"] == 0 and seen["both", e]["verified_rows"] > 0
            assert len({(s["valid"], s["found"], s["probes"]) for (_, ee), s in seen.items() if ee == e}) == 1
    finally:
        ix.close()


def test_open_flags_give_identical_arrays(shapes, small_genome):
    for kw in ({"kmer_table": False}, {"compact": True, "pre5": False}):
        with dicey_amd.FmIndex(small_genome["fm9"], **kw) as ix:
            for e in ES:
                _same(ix.query_min_length(shapes["recs"], max_k=24, mismatches=e), _exp(shapes, e, 0), (kw, e))


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_argument_checks(small_genome, shapes):
    L = _capi.load()
    EINVAL, ELIMIT = -1, -7
    seq = small_genome["seqs"][0][:40].encode()
    off = (C.c_uint64 * 2)(0, 40)
    vals = (C.c_uint32 * 40)(*([0xABCD1234] * 40))

    def prm(min_k=10, max_k=24, e=0, t=0, flags=0, res=(0, 0)):
        return _capi.QminlenParams(min_k, max_k, e, 0, t, flags, (C.c_uint32 * 2)(*res))

    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        h = ix.handle

        def call(p, handle=h, s=seq, o=off, n=1, v=vals, st=None):
            rc = L.dg_query_min_len(handle, C.byref(p) if p is not None else None, s, o, n, v, st)
            if rc:
                assert L.dg_last_error() and b"dg_query_min_len" in L.dg_last_error()
            return rc

        assert call(None) == EINVAL and call(prm(flags=1)) == EINVAL and call(prm(res=(1, 0))) == EINVAL and call(prm(res=(0, 1))) == EINVAL
        for p in (prm(min_k=9), prm(max_k=1001), prm(min_k=9, max_k=9), prm(min_k=1001, max_k=1001), prm(min_k=25), prm(e=3), prm(t=0xFFFFFFFE),
                  prm(t=0xFFFFFFFF)):
            assert call(p) == ELIMIT
        big = (C.c_uint64 * 2)(0, 1 << 31)
        assert call(prm(), o=big) == ELIMIT and call(prm(), o=(C.c_uint64 * 2)(0, (1 << 31) - 1)) == ELIMIT  # with its separator
        assert call(prm(), handle=None) == EINVAL
        assert call(prm(), s=None) == EINVAL and call(prm(), o=None) == EINVAL and call(prm(), v=None) == EINVAL
        assert call(prm(), o=(C.c_uint64 * 3)(0, 30, 20), n=2) == EINVAL
        # the order: the block's form, its values, the size limit, then the handle
        assert call(prm(min_k=9, flags=1)) == EINVAL and call(prm(min_k=9), handle=None) == ELIMIT and call(prm(), o=big, handle=None) == ELIMIT
        assert call(prm(e=3), o=big) == ELIMIT and b"mismatches" in L.dg_last_error()
        assert list(vals) == [0xABCD1234] * 40
        # nothing to do is not an error, and writes nothing
        st = _capi.QminlenStats()
        assert call(prm(), n=0, st=C.byref(st)) == 0 and call(prm(), s=None, o=None, n=0, v=None) == 0
        assert call(prm(), o=(C.c_uint64 * 3)(0, 0, 0), n=2, st=C.byref(st)) == 0 and st.positions == 0 and st.launches == 0
        assert list(vals) == [0xABCD1234] * 40
        text = small_genome["text"]
        assert call(prm(t=1), st=C.byref(st)) == 0 and st.positions == 40 and st.launches == 1 and st.found <= st.valid <= st.probes
        qbuf, _ = Q.buffer_of([seq])
        exp = ML.min_len(ML.parts_by_k(text, qbuf, range(10, 25), 0), qbuf, 10, 24, 1)[:40]
        assert list(vals) == [int(x) for x in exp] and st.valid == (exp != INV).sum() and st.found == ((exp != INV) & (exp != 0)).sum()
        # offsets that do not start at 0: records are seqs[off[i] .. off[i+1]) and values[off[i] ..]
        v2 = (C.c_uint32 * 40)(*([7] * 40))
        assert call(prm(t=1), o=(C.c_uint64 * 3)(10, 25, 40), n=2, v=v2) == 0
        two = [seq[10:25], seq[25:40]]
        qb2, _ = Q.buffer_of(two)
        e2 = ML.split(ML.min_len(ML.parts_by_k(text, qb2, range(10, 25), 0), qb2, 10, 24, 1), two)
        assert list(v2) == [7] * 10 + [int(x) for x in e2[0]] + [int(x) for x in e2[1]]


def test_refused_while_a_hunt_batch_is_in_flight(small_genome, shapes):
    g = small_genome
    rng = random.Random(9)
    t = g["text"].decode()
    qs = []
    while len(qs) < 300:
        p = rng.randrange(len(t) - 20)
        if "\n" not in t[p:p + 20]:
            qs.append(t[p:p + 20])
    recs = shapes["recs"]
    with dicey_amd.FmIndex(g["fm9"]) as ix:
        tk = ix.hunt_submit(qs, g["seqlen"], distance=1)
        try:
            with pytest.raises(dicey_amd.DgError) as e:
                ix.query_min_length(recs, max_k=24, mismatches=1)
            assert e.value.code == -1 and "in flight" in str(e.value) and "dg_query_min_len" in str(e.value)
        finally:
            ix.hunt_wait(tk)
        _same(ix.query_min_length(recs, max_k=24, mismatches=1), _exp(shapes, 1, 0), "after the batch")


# ---- a genome too large for brute force: the new code against a scan of dg_query_map, which it shares no kernel with -----------------

def _scan(ix, recs, lo, hi, e, t, fo):
    """what a caller without dg_query_min_len does: one query_mappability per k, the first k with a value <= t (a linear scan)"""
    out = None
    for k in range(lo, hi + 1):
        vals = ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo)
        if out is None:
            out = [np.where(v == INV, INV, 0).astype(np.uint32) for v in vals]  # invalid at min_k: no k-mer of the smallest length
        for o, v in zip(out, vals):
            hit = (o == 0) & (v != INV) & (v <= t)
            o[hit] = k
    return out


def test_same_answer_as_a_scan_of_query_map_on_a_few_mb(tmp_path):
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = []
    for length in (2_000_000, 1_000_000):
        s = acgt[rng.integers(0, 4, length)].copy()
        for _ in range(200):
            a, m, d = int(rng.integers(0, length - 5000)), int(rng.integers(50, 3000)), int(rng.integers(0, length - 5000))
            piece = s[a:a + m].copy()
            if rng.random() < 0.5:
                piece = np.frombuffer(revcomp(piece.tobytes().decode()).encode(), dtype=np.uint8).copy()
            hits = rng.integers(0, m, max(1, m // 40))
            piece[hits] = acgt[rng.integers(0, 4, len(hits))]
            s[d:d + m] = piece
        for _ in range(20):
            a = int(rng.integers(0, length - 2000))
            s[a:a + int(rng.integers(1, 1500))] = ord("N")
        for _ in range(20):
            a = int(rng.integers(0, length - 500))
            s[a:a + int(rng.integers(10, 400))] = ord("ACGT"[int(rng.integers(0, 4))])
        seqs.append(s.tobytes())
    text = b"\n".join(seqs) + b"\n"
    path = str(tmp_path / "mid.fm9")
    dicey_amd.build_index(text, path)
    recs = []
    for _ in range(6):
        a = int(rng.integers(0, len(seqs[0]) - 2500))
        piece = np.frombuffer(seqs[0][a:a + 2500], dtype=np.uint8).copy()
        hits = rng.integers(0, 2500, 25)
        piece[hits] = acgt[rng.integers(0, 4, 25)]
        recs.append(piece.tobytes())
    recs += [acgt[rng.integers(0, 4, 4800)].tobytes(), b"A" * 200]
    assert sum(map(len, recs)) == 20000
    between = zero = 0
    with dicey_amd.FmIndex(path, compact=True, pre5=False) as ix:
        for e, lo, hi in ((0, 14, 40), (1, 14, 40), (2, 16, 24)):
            for t, fo in ((0, False), (1, False), (1, True)):
                st = {}
                got = ix.query_min_length(recs, max_k=hi, min_k=lo, at_most=t, mismatches=e, forward_only=fo, stats=st)
                exp = _scan(ix, recs, lo, hi, e, t, fo)
                _same(got, exp, (e, t, fo))
                allv = np.concatenate(exp)
                assert (allv == INV).sum() >= lo and (allv == lo).sum() >= 100 and st["found"] == ((allv != 0) & (allv != INV)).sum()
                between += int(((allv > lo) & (allv < hi)).sum())
                zero += int((allv == 0).sum())
                # a search, not a scan: the probe at the limit, the one at min_k, a gallop and a bisection of at most log2 steps each
                assert st["valid"] <= st["probes"] <= st["valid"] * (2 + 2 * math.log2(hi - lo + 1)) < st["valid"] * (hi - lo + 1)
    assert between >= 5000 and zero >= 5000
