"""dg_query_min_len_end / FmIndex.query_min_length_end against the linear-scan reference of tests/query_min_len_end_ref.py, which knows
nothing of the FM-index and does not assume that values fall with k: every record shape on the session genome across the K-mer table
order, e, the anchor, t, the strand setting and two (min_k, max_k) pairs, on the product and the development library (the expected values
shown, on the reference alone, to hold every class of answer); long k-mers, whose backward limit walks three bitmap words, against the
diagonal route; the device's own dg_query_map_anchored at min_k = max_k and around every answer; the switches of the development build,
the open flags, the argument checks and the refusal while a hunt batch is in flight."""
import ctypes as C
import random

import numpy as np
import pytest

import conftest
import dicey_amd
import query_anchor_ref as A
import query_map_ref as Q
import query_min_len_end_ref as ME
from dicey_amd import _capi

pytestmark = pytest.mark.gpu
INV = ME.INVALID
ES, TS = (0, 1, 2), (0, 1)
RANGES = ((10, 24), (12, 16))
LONG = (126, 132)


def _anchors(rng):
    return (0, 1, 5, rng[0])


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
    """the session genome on the product library with the default K-mer table and with one of order 16 (with min_k = 10 and max_k = 24
    one lane's probes lie below the table's order, at it and above it), and on the development library"""
    dflt = conftest.open_index(small_genome["fm9"])
    monkeypatch_module.setenv("DICEY_KMER_K", "16")
    k16 = conftest.open_index(small_genome["fm9"])
    monkeypatch_module.delenv("DICEY_KMER_K")
    dev = dicey_amd.FmIndex(small_genome["fm9"], _lib=conftest.exp_lib())
    yield {"default": dflt, "K16": k16, "dev": dev}
    for ix in (dflt, k16, dev):
        ix.close()


@pytest.fixture(scope="module")
def shapes(small_genome):
    """the record set and, computed once and left unchanged, the brute-force parts per (k, e, a) that every expectation is scanned from"""
    text = small_genome["text"]
    recs = ME.record_set(small_genome["seqs"], 10, 24)
    qbuf, offs = Q.buffer_of(recs)
    parts = {e: ME.parts_by_k(text, qbuf, range(10, 25), e, (0, 1, 5, 10, 12)) for e in ES}
    return {"recs": recs, "qbuf": qbuf, "offs": offs, "parts": parts, "brun": ME.brun_lengths(qbuf)}


def _exp_buf(shapes, e, a, t, fo=False, rng=(10, 24)):
    return ME.min_len_end(shapes["parts"][e], shapes["qbuf"], rng[0], rng[1], a, t, fo)


def _exp(shapes, e, a, t, fo=False, rng=(10, 24)):
    return ME.split(_exp_buf(shapes, e, a, t, fo, rng), shapes["recs"])


# ---- session genome --------------------------------------------------------------------------------------------------------------

def test_expected_values_hold_every_class(shapes):
    """a condition on the INPUTS, shown on the reference alone: no test below can pass on a degenerate expectation"""
    recs, offs, brun = shapes["recs"], shapes["offs"], shapes["brun"]
    assert offs[0] == 0 and len(recs[0]) == 3000 and b"N" in recs[0] and b"" in recs and len(recs[-4]) == 10
    cut_short = differ = 0
    for rng in RANGES:
        lo, hi = rng
        limit = np.minimum(brun, hi)
        for e in ES:
            for a in _anchors(rng):
                for fo in (False, True):
                    assert ME.violations_by_end(shapes["parts"][e], lo, hi, a, fo) == 0
                    for t in TS:
                        v = _exp_buf(shapes, e, a, t, fo, rng)
                        what = (rng, e, a, t, fo)
                        assert (v == INV).sum() >= 100 and (v == 0).sum() >= 100, what
                        assert ((v > lo) & (v < hi)).sum() >= 5, what
                        assert ((v == limit) & (v != 0) & (v != INV)).sum() >= 1, what
                        # (a 10-mer free to differ in two places, none of them or few of them anchored, has places in 90 kb wherever it lies)
                        assert (rng == (10, 24) and e == 2 and a < lo) or (v == lo).sum() >= 1, what
                        # an answer at the start of a run that a record start or an N cut short
                        cut_short += int(((v == limit) & (limit < hi) & (v > lo) & (v != INV)).sum())
                        differ += int(a > 0 and e > 0 and (v != _exp_buf(shapes, e, 0, t, fo, rng)).sum())
    assert cut_short >= 100 and differ >= 10000  # and the anchor changes answers
    per = _exp(shapes, 0, 0, 1)
    assert (per[11] == INV).all() and (per[13] == INV).all() and len(per[12]) == 0       # 9 nt, lower case, empty
    assert (per[-4] != INV).sum() == 1 and per[-4][9] != INV                              # exactly min_k: its last base alone
    assert (per[0][:9] == INV).all() and per[0][9] != INV                                 # the first record: runs end at the buffer's start
    assert per[-1][len(per[-1]) - 1] != INV
    # the value sits at the oligo's LAST base: by start position the same records are invalid at their end, not at their start
    assert (per[-1][:9] == INV).all()


@pytest.mark.parametrize("e", ES)
def test_session_genome_every_shape(shapes, indices, e):
    npos = sum(len(r) for r in shapes["recs"])
    for rng in RANGES:
        for a in _anchors(rng):
            for t in TS:
                for fo in (False, True):
                    exp = _exp(shapes, e, a, t, fo, rng)
                    valid = sum(int((x != INV).sum()) for x in exp)
                    found = sum(int(((x != INV) & (x != 0)).sum()) for x in exp)
                    for name, ix in indices.items():
                        st = {}
                        got = ix.query_min_length_end(shapes["recs"], max_k=rng[1], min_k=rng[0], at_most=t, mismatches=e, anchor=a,
                                                      forward_only=fo, stats=st)
                        _same(got, exp, (name, e, a, t, fo, rng))
                        assert st["positions"] == npos and st["valid"] == valid and st["found"] == found and st["launches"] == 1
                        assert valid <= st["probes"] <= valid * 8 and found <= valid
                        assert st["ms_total"] == pytest.approx(st["ms_valid"] + st["ms_search"], rel=1e-9)


def test_str_records_and_the_empty_call(shapes, indices):
    ix = indices["default"]
    low = shapes["recs"][-1].decode().lower()  # str records are upper-cased, bytes go through as given
    _same(ix.query_min_length_end([low], max_k=24, mismatches=1, anchor=5), [_exp(shapes, 1, 5, 0)[-1]], "str")
    assert (ix.query_min_length_end([low.encode()], max_k=24)[0] == INV).all()
    assert ix.query_min_length_end([], max_k=24) == []
    for e in ES:  # a large at_most: min_k wherever a run of min_k ends
        got = ix.query_min_length_end(shapes["recs"], max_k=24, min_k=10, at_most=0xFFFFFFFD, mismatches=e, anchor=5)
        _same(got, ME.split(np.where(shapes["brun"] >= 10, 10, INV).astype(np.uint32), shapes["recs"]), e)


# ---- long k-mers: the backward limit walks three bitmap words --------------------------------------------------------------------

def _tiny_case():
    """a text of 2.4 kb (the diagonal route costs |Q| * |T| per k) and cuts of it with three substitutions 6 nt apart near their start:
    an oligo that ends at p loses its place in the text once it reaches back over e + 1 of them, at lengths around p - 60"""
    rng = random.Random(77)
    seqs = ["".join(rng.choice("ACGT") for _ in range(1200)) for _ in range(2)]
    text = conftest.genome_text(seqs)

    def cut(s, at, m, where=(58, 64, 70)):
        s = list(s[at:at + m])
        for i in where:
            s[i] = "ACGT"[("ACGT".index(s[i]) + 1) % 4]
        return "".join(s)

    recs = [cut(seqs[0], 300, 210),                       # at buffer offset 0: the walk stops at word 0
            A._revcomp(cut(seqs[1], 500, 210)),           # the other strand (its substitutions near its END)
            "N" * 17 + cut(seqs[1], 100, 205),            # a run that starts inside a word, behind an N
            cut(seqs[0], 700, 128, (0,)),                 # 128 nt, the first one substituted: every limit is cut short of max_k, and at
            "ACGTTGCAAC"]                                 # e = 0 the full run alone has no place; and a record of 10
    recs = [r.encode() for r in recs]
    qbuf, _ = Q.buffer_of(recs)
    parts = {e: ME.parts_by_k(text, qbuf, range(LONG[0], LONG[1] + 1), e, (0, 5), "diagonal") for e in ES}
    return {"text": text, "recs": recs, "qbuf": qbuf, "parts": parts}


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    case = _tiny_case()
    case["fm9"] = str(tmp_path_factory.mktemp("tiny") / "tiny.fm9")
    dicey_amd.build_index(case["text"], case["fm9"])
    return case


def test_long_kmers_against_the_diagonal_route(tiny):
    lo, hi = LONG
    brun = ME.brun_lengths(tiny["qbuf"])
    assert brun.max() == 210 and (brun == 210).sum() == 2 and (brun == 205).sum() == 3
    limit = np.minimum(brun, hi)
    classes = set()
    with conftest.open_index(tiny["fm9"]) as ix:
        for e in ES:
            for a in (0, 5):
                for fo in (False, True):
                    buf = ME.min_len_end(tiny["parts"][e], tiny["qbuf"], lo, hi, a, 0, fo)
                    v = buf[buf != INV]
                    assert (buf == INV).sum() >= 400 and (v == 0).sum() >= 5 and (v == lo).sum() >= 5 and ((v > lo) & (v < hi)).sum() >= 3, (e, a, fo)
                    classes |= set(np.unique(buf[(buf == limit) & (limit < hi) & (buf >= lo)]).tolist())
                    got = ix.query_min_length_end(tiny["recs"], max_k=hi, min_k=lo, mismatches=e, anchor=a, forward_only=fo)
                    _same(got, ME.split(buf, tiny["recs"]), (e, a, fo))
    assert classes  # an answer equal to a limit that the record's start cut short of max_k


# ---- against the device's own dg_query_map_anchored -------------------------------------------------------------------------------

def _by_end(vals, k):
    out = []
    for v in vals:
        o = np.full(len(v), INV, dtype=np.uint32)
        if len(v) >= k:
            o[k - 1:] = v[:len(v) - k + 1]
        out.append(o)
    return out


def test_one_length_is_the_shifted_anchored_count(shapes, indices):
    """min_k = max_k = k: the answer is k where dg_query_map_anchored's value of the k-mer that ends there is at most t, else 0"""
    ix, recs = indices["K16"], shapes["recs"]
    for k, e, a, t, fo in ((10, 1, 5, 0, False), (16, 2, 16, 0, False), (17, 2, 1, 0, True), (24, 1, 0, 0, False), (24, 2, 9, 2, False)):
        cnt = _by_end(ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo, anchor=a), k)
        exp = [np.where(c == INV, INV, np.where(c <= t, k, 0)).astype(np.uint32) for c in cnt]
        allv = np.concatenate(exp)
        # (t = 0: the cuts of the genome have a place, the windows over enough substitutions have none)
        assert t or ((allv == k).sum() >= 100 and (allv == 0).sum() >= 100 and (allv == INV).sum() >= 100), (k, e, a, t)
        _same(ix.query_min_length_end(recs, max_k=k, min_k=k, at_most=t, mismatches=e, anchor=a, forward_only=fo), exp, (k, e, a, t, fo))


def test_a_full_anchor_is_the_exact_search(shapes, indices):
    """a = min_k = max_k: every base is anchored, so e = 2 answers what e = 0 answers"""
    ix, recs = indices["K16"], shapes["recs"]
    for k in (12, 16, 20):
        for fo in (False, True):
            exact = ix.query_min_length_end(recs, max_k=k, min_k=k, at_most=0, mismatches=0, anchor=k, forward_only=fo)
            assert sum(int((x == k).sum()) for x in exact) >= 100 and sum(int((x == 0).sum()) for x in exact) >= 100
            _same(ix.query_min_length_end(recs, max_k=k, min_k=k, at_most=0, mismatches=2, anchor=k, forward_only=fo), exact, (k, fo))


def test_every_answer_is_the_first_length_that_passes(shapes, indices):
    """for every len L > 0 the device's own anchored count of the L-mer that ends there is <= t, and that of the (L-1)-mer is > t"""
    ix, recs = indices["default"], shapes["recs"]
    lo, hi = 10, 24
    for e, a, t in ((1, 5, 0), (2, 1, 1)):
        got = np.concatenate(ix.query_min_length_end(recs, max_k=hi, min_k=lo, at_most=t, mismatches=e, anchor=a))
        cnt = {k: np.concatenate(_by_end(ix.query_mappability(recs, k=k, mismatches=e, anchor=a), k)) for k in range(lo, hi + 1)}
        checked = 0
        for L in range(lo, hi + 1):
            at = got == L
            assert (cnt[L][at] <= t).all(), (e, a, t, L)
            if L > lo:
                assert (cnt[L - 1][at] != INV).all() and (cnt[L - 1][at] > t).all(), (e, a, t, L)
            checked += int(at.sum())
        zero = got == 0
        assert all(((cnt[k][zero] == INV) | (cnt[k][zero] > t)).all() for k in cnt) and checked >= 1000 and zero.sum() >= 100


# ---- paths -----------------------------------------------------------------------------------------------------------------------

def test_switches_of_the_development_build(shapes, indices, monkeypatch):
    """DICEY_QMINLEN_CHUNK (positions per launch) and DICEY_MAP_NARROW (W) change how the search runs, never what it returns"""
    recs, ix = shapes["recs"], indices["dev"]
    npos = len(shapes["qbuf"])
    seen = {}
    for name, env in (("default", {}), ("chunk", {"DICEY_QMINLEN_CHUNK": "64"}), ("never", {"DICEY_MAP_NARROW": "0"}),
                      ("both", {"DICEY_QMINLEN_CHUNK": "777", "DICEY_MAP_NARROW": "1000000000"})):
        for kk, vv in env.items():
            monkeypatch.setenv(kk, vv)
        for e in ES:
            st = {}
            _same(ix.query_min_length_end(recs, max_k=24, at_most=1, mismatches=e, anchor=5, stats=st), _exp(shapes, e, 5, 1), (name, e))
            seen[name, e] = st
        _same(ix.query_min_length_end(recs, max_k=16, min_k=12, mismatches=1, anchor=12, forward_only=True), _exp(shapes, 1, 12, 0, True, (12, 16)),
              (name, "fo"))
        for kk in env:
            monkeypatch.delenv(kk)
    for e in ES:
        assert seen["default", e]["launches"] == 1 and seen["default", e]["verified_rows"] > 0
        assert seen["chunk", e]["launches"] == -(-npos // 64) and seen["both", e]["launches"] == -(-npos // 777)
        assert seen["never", e]["verified_rows"] == 0 and seen["never", e]["steps"] > 0
        assert seen["both", e]["steps"] == 0 and seen["both", e]["verified_rows"] > 0
        assert len({(s["valid"], s["found"], s["probes"]) for (_, ee), s in seen.items() if ee == e}) == 1
    # the product library does not read the switches
    monkeypatch.setenv("DICEY_QMINLEN_CHUNK", "64")
    st = {}
    _same(indices["default"].query_min_length_end(recs, max_k=24, at_most=1, mismatches=1, anchor=5, stats=st), _exp(shapes, 1, 5, 1), "product")
    assert st["launches"] == 1


def test_open_flags_give_identical_arrays(shapes, small_genome):
    for kw in ({"kmer_table": False}, {"compact": True, "pre5": False}):
        with conftest.open_index(small_genome["fm9"], **kw) as ix:
            for e in ES:
                _same(ix.query_min_length_end(shapes["recs"], max_k=24, mismatches=e, anchor=5), _exp(shapes, e, 5, 0), (kw, e))


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_argument_checks(small_genome, shapes):
    L = _capi.load()
    EINVAL, ELIMIT = -1, -7
    seq = small_genome["seqs"][0][:40].encode()
    off = (C.c_uint64 * 2)(0, 40)
    vals = (C.c_uint32 * 40)(*([0xABCD1234] * 40))

    def prm(min_k=10, max_k=24, e=0, a=5, t=0, flags=0, res=(0, 0)):
        return _capi.QminlenEndParams(min_k, max_k, e, a, 0, t, flags, (C.c_uint32 * 2)(*res))

    with conftest.open_index(small_genome["fm9"]) as ix:
        h = ix.handle

        def call(p, handle=h, s=seq, o=off, n=1, v=vals, st=None):
            rc = L.dg_query_min_len_end(handle, C.byref(p) if p is not None else None, s, o, n, v, st)
            if rc:
                assert L.dg_last_error() and b"dg_query_min_len_end" in L.dg_last_error()
            return rc

        assert call(None) == EINVAL and call(prm(flags=1)) == EINVAL and call(prm(res=(1, 0))) == EINVAL and call(prm(res=(0, 1))) == EINVAL
        for p in (prm(min_k=9), prm(max_k=1001), prm(min_k=9, max_k=9), prm(min_k=1001, max_k=1001), prm(min_k=25), prm(e=3), prm(t=0xFFFFFFFE),
                  prm(t=0xFFFFFFFF), prm(a=11), prm(a=24), prm(min_k=12, max_k=16, a=13), prm(a=0xFFFFFFFF)):
            assert call(p) == ELIMIT
        big = (C.c_uint64 * 2)(0, 1 << 31)
        assert call(prm(), o=big) == ELIMIT and call(prm(), o=(C.c_uint64 * 2)(0, (1 << 31) - 1)) == ELIMIT  # with its separator
        assert call(prm(), handle=None) == EINVAL
        assert call(prm(), s=None) == EINVAL and call(prm(), o=None) == EINVAL and call(prm(), v=None) == EINVAL
        assert call(prm(), o=(C.c_uint64 * 3)(0, 30, 20), n=2) == EINVAL
        # the order: the block's form, its values, the size limit, then the handle
        assert call(prm(a=11, flags=1)) == EINVAL and call(prm(a=11), handle=None) == ELIMIT and call(prm(), o=big, handle=None) == ELIMIT
        assert call(prm(a=11), o=big) == ELIMIT and b"anchor" in L.dg_last_error()
        assert list(vals) == [0xABCD1234] * 40
        # nothing to do is not an error, and writes nothing
        st = _capi.QminlenStats()
        assert call(prm(), n=0, st=C.byref(st)) == 0 and call(prm(), s=None, o=None, n=0, v=None) == 0
        assert call(prm(), o=(C.c_uint64 * 3)(0, 0, 0), n=2, st=C.byref(st)) == 0 and st.positions == 0 and st.launches == 0
        assert list(vals) == [0xABCD1234] * 40
        text = small_genome["text"]
        assert call(prm(e=1, t=1), st=C.byref(st)) == 0 and st.positions == 40 and st.launches == 1 and st.found <= st.valid <= st.probes
        qbuf, _ = Q.buffer_of([seq])
        exp = ME.min_len_end(ME.parts_by_k(text, qbuf, range(10, 25), 1, (5,)), qbuf, 10, 24, 5, 1)[:40]
        assert list(vals) == [int(x) for x in exp] and st.valid == (exp != INV).sum() and st.found == ((exp != INV) & (exp != 0)).sum()
        # offsets that do not start at 0: records are seqs[off[i] .. off[i+1]) and values[off[i] ..]
        v2 = (C.c_uint32 * 40)(*([7] * 40))
        assert call(prm(e=1, t=1), o=(C.c_uint64 * 3)(10, 25, 40), n=2, v=v2) == 0
        two = [seq[10:25], seq[25:40]]
        qb2, _ = Q.buffer_of(two)
        e2 = ME.split(ME.min_len_end(ME.parts_by_k(text, qb2, range(10, 25), 1, (5,)), qb2, 10, 24, 5, 1), two)
        assert list(v2) == [7] * 10 + [int(x) for x in e2[0]] + [int(x) for x in e2[1]]
    with pytest.raises(dicey_amd.DgError) as err:
        with conftest.open_index(small_genome["fm9"]) as ix:
            ix.query_min_length_end([seq], max_k=24, min_k=12, anchor=13)
    assert err.value.code == ELIMIT and "dg_query_min_len_end" in str(err.value)


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
    with conftest.open_index(g["fm9"]) as ix:
        tk = ix.hunt_submit(qs, g["seqlen"], distance=1)
        try:
            with pytest.raises(dicey_amd.DgError) as e:
                ix.query_min_length_end(recs, max_k=24, mismatches=1, anchor=5)
            assert e.value.code == -1 and "in flight" in str(e.value) and "dg_query_min_len_end" in str(e.value)
        finally:
            ix.hunt_wait(tk)
        _same(ix.query_min_length_end(recs, max_k=24, mismatches=1, anchor=5), _exp(shapes, 1, 5, 0), "after the batch")
