"""dg_min_unique_mm / FmIndex.min_unique(mismatches=e) against models that know nothing of the FM-index (tests/min_unique_mm_ref.py):
every position of a crafted 5 kb genome held to the pairwise model at e = 1 and 2, both strand modes, across the K-mer table order and
the open flags; on the 90 kb session genome the identities with FmIndex.mappability(mismatches=e), across e, with
FmIndex.query_min_length on the genome's own sequences and with FmIndex.min_unique; every genome shape of at most 8 000 bytes; launch
chunks and the narrow-interval finish on the development build; the run form, the counters and the argument checks."""
import ctypes as C
import random

import numpy as np
import pytest

try:  # torch bundles its own HIP runtime: it only finds the GPU if it initialises before libdiceygpu's (system) runtime does
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import conftest
import dicey_amd
import genome_shapes as S
import mappability_ref as R
import min_unique_mm_ref as W
import min_unique_ref as U
from conftest import genome_text

pytestmark = pytest.mark.gpu
MAX_KS = (10, 16, 17, 40, 64)
INV = 0xFFFFFFFF


def _same(got, exp, what):
    assert got.dtype == np.uint32 and len(got) == len(exp), what
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])


# ---- the crafted genome ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    text = genome_text(W.crafted_seqs()["seqs"])
    # the reference alone first (tests/test_min_unique_mm_host.py has the exact figures): no case is tested on an empty set
    for e in (1, 2):
        c = W.coverage(text, 64, e)
        assert c["raised"] >= 1000 and c["became_zero"] >= 50 and c["reverse_raises"] >= 500 and c["reverse_zeroes"] >= 1, (e, c)
    path = str(tmp_path_factory.mktemp("mumm") / "crafted.fm9")
    dicey_amd.build_index(text, path)
    return {"text": text, "fm9": path}


@pytest.mark.parametrize("how", ["as-is", "K16", "no-table", "compact-no-pre5"])
def test_crafted_genome_every_position(crafted, how):
    """max_k below, at and above the K-mer table's order, with and without a table"""
    text = crafted["text"]
    mp = pytest.MonkeyPatch()
    try:
        if how == "K16":
            mp.setenv("DICEY_KMER_K", "16")
        kw = {"no-table": {"kmer_table": False}, "compact-no-pre5": {"compact": True, "pre5": False}}.get(how, {})
        ix = dicey_amd.FmIndex(crafted["fm9"], **kw)
    finally:
        mp.undo()
    with ix:
        for max_k in MAX_KS:
            for e in (1, 2):
                for fo in (False, True):
                    _same(ix.min_unique(max_k=max_k, forward_only=fo, mismatches=e), W.pairwise(text, max_k, e, fo), (how, max_k, e, fo))


# ---- the session genome ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def session_values(small_genome):
    """(mismatches, forward_only) -> the product library's lengths at max_k = 64, computed once"""
    out = {}
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        for e in (0, 1, 2):
            for fo in (False, True):
                st = {}
                out[e, fo] = ix.min_unique(max_k=64, forward_only=fo, mismatches=e, stats=st)
                out[e, fo, "stats"] = st
        out["exact"] = ix.min_unique(max_k=64)
    return out


def test_zero_mismatches_is_min_unique(small_genome, session_values):
    _same(session_values[0, False], session_values["exact"], "e = 0")
    _same(session_values[0, False], U.by_values(small_genome["text"], 64), "e = 0 against the definition")
    assert "candidates" not in session_values[0, False, "stats"]


@pytest.mark.parametrize("forward_only", [False, True])
@pytest.mark.parametrize("e", [1, 2])
def test_identity_with_mappability(small_genome, session_values, e, forward_only):
    """(mul_e != 0 and mul_e <= k)  <=>  mappability(k, e) == 1, on the positions whose k-mer is valid"""
    text = small_genome["text"]
    mul = session_values[e, forward_only]
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        for k in (10, 20, 64):
            one = ix.mappability(k=k, mismatches=e, forward_only=forward_only) == 1
            ok = R.valid_positions(text, k)
            # both classes are there; at k = 10 the 31 (e = 1) or 436 (e = 2) strings around a 10-mer meet 180 000 windows among 4^10
            # strings, so next to nothing of 90 kb is unique and only the other class is asked for
            assert ok.sum() > 50000 and (~one[ok]).sum() > 500 and (k == 10 or one[ok].sum() > 10000)
            got = (mul != 0) & (mul <= k)
            bad = np.nonzero(got[ok] != one[ok])[0]
            assert len(bad) == 0, (k, len(bad), np.nonzero(ok)[0][bad[:10]])


@pytest.mark.parametrize("forward_only", [False, True])
def test_lengths_grow_with_the_mismatches(session_values, forward_only):
    for e in (1, 2):
        hi, lo = session_values[e, forward_only], session_values[e - 1, forward_only]
        assert ((hi == 0) | (hi >= lo)).all() and not hi[lo == 0].any()
        assert (hi > lo).sum() > 10000 and ((hi == 0) & (lo != 0)).sum() > 100


@pytest.mark.parametrize("e", [1, 2])
def test_query_min_length_of_the_genomes_own_sequences(small_genome, session_values, e):
    """a record equal to a whole sequence, at_most = 1: INVALID where limit(p) < min_k, 0 where mul_e(p) == 0, else max(mul_e(p), min_k)"""
    text, seqs = small_genome["text"], small_genome["seqs"]
    limit = np.minimum(U.run_lengths(text), 64)
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        for fo in (False, True):
            mul = session_values[e, fo]
            for min_k in (10, 17):
                got = ix.query_min_length(seqs, max_k=64, min_k=min_k, at_most=1, mismatches=e, forward_only=fo)
                exp = np.where(limit < min_k, INV, np.where(mul == 0, 0, np.maximum(mul, min_k))).astype(np.uint32)
                off = 0
                for s, g in zip(seqs, got):
                    _same(g, exp[off:off + len(s)], (e, fo, min_k, off))
                    off += len(s) + 1
                # every class of the rule is there (most lengths of a 90 kb genome lie below 17, next to none at or below 10)
                assert (exp == INV).sum() > 100 and (exp == 0).sum() > 1000 and ((exp > min_k) & (exp != INV)).sum() > 1000
                assert min_k == 10 or (exp == min_k).sum() > 1000


# ---- genome shapes --------------------------------------------------------------------------------------------------------------------

# every shape of tests/genome_shapes.py the pairwise model can serve (the cuts tests/mappability_shapes.py adds are all larger)
SMALL_SHAPES = [n for n, g in sorted(S.all_shapes().items()) if len(g["text"]) <= 8000]


def test_there_are_small_shapes():
    assert len(SMALL_SHAPES) >= 17 and "tiny_1" in SMALL_SHAPES and "tiny_4097" in SMALL_SHAPES


@pytest.mark.parametrize("name", SMALL_SHAPES)
def test_genome_shapes(tmp_path, name):
    text = S.all_shapes()[name]["text"]
    fm9 = str(tmp_path / "shape.fm9")
    dicey_amd.build_index(text, fm9)
    with dicey_amd.FmIndex(fm9) as ix:
        for max_k in (24, 100):
            for fo in (False, True):
                _same(ix.min_unique(max_k=max_k, forward_only=fo, mismatches=1), W.pairwise(text, max_k, 1, fo), (name, max_k, fo))


# ---- the development build ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [{"DICEY_MAP_HEAD_CHUNK": "4099"}, {"DICEY_MAP_NARROW": "0"}, {"DICEY_MAP_NARROW": "1000000000"},
                                 {"DICEY_MU_MM_RANK_ORDER": "1", "DICEY_MAP_HEAD_CHUNK": "4099"}])
def test_chunks_and_narrow_finish_on_the_development_build(small_genome, session_values, monkeypatch, env):
    """positions go through the search in chunks, one launch each, intervals of at most W rows are finished on the text, and the lanes
    may take their positions in suffix-array order: the development build takes all three from the environment, and the lengths are the
    product library's"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ix = dicey_amd.FmIndex(small_genome["fm9"], _lib=conftest.exp_lib())
    try:
        for e, fo in ((1, False), (2, False), (1, True)):
            st = {}
            _same(ix.min_unique(max_k=64, forward_only=fo, mismatches=e, stats=st), session_values[e, fo], (env, e, fo))
            ref = session_values[e, fo, "stats"]
            assert st["candidates"] == ref["candidates"] and st["probes"] == ref["probes"], (env, st, ref)
            if "DICEY_MAP_HEAD_CHUNK" in env:
                assert st["launches"] == -(-(len(small_genome["text"]) + 1) // 4099) and st["launches"] > 20, st
            if "DICEY_MAP_NARROW" not in env:
                continue
            if env["DICEY_MAP_NARROW"] == "0":
                assert st["verified_rows"] == 0 and st["steps"] > 0, st
            else:
                assert st["steps"] == 0 and st["verified_rows"] > 0, st
    finally:
        ix.close()


# ---- runs, counters, argument checks --------------------------------------------------------------------------------------------------

def _probes_of(lo, hi, answer):
    """the probes dicey_amd/csrc/probe_schedule.hpp spends on a position: first hi, then the gallop from lo and the bisection"""
    if answer == 0:
        return 1
    n, step = 1, 1
    while hi - lo > 1:
        k = lo + step if lo + step < hi else lo + (hi - lo) // 2
        n += 1
        if k >= answer:
            hi = k
        else:
            lo, step = k, step * 2
    return n


def test_runs_stats_and_argument_checks(small_genome, session_values):
    text = small_genome["text"]
    n1 = len(text)
    L = dicey_amd._capi.load()
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        vals = session_values[1, False]  # (held to mappability, to the other e and to query_min_length above)
        s0, l0, _ = R.runs(vals, 0, n1)
        long_runs = np.nonzero(l0 >= 5)[0]
        assert len(long_runs) >= 4
        a = int(s0[long_runs[1]] + 2)
        b = int(s0[long_runs[-2]] + 3)
        for lo, hi in ((0, n1), (a, b), (a, a + 1), (a, a), (n1 - 7, n1)):  # ranges that start and end inside runs
            got = ix.min_unique_runs(max_k=64, lo=lo, hi=hi, mismatches=1)
            for x, y in zip(got, R.runs(vals, lo, hi)):
                assert x.dtype == y.dtype and len(x) == len(y) and (x == y).all(), (lo, hi)
        got = ix.min_unique_runs(max_k=64, forward_only=True, mismatches=2)
        for x, y in zip(got, R.runs(session_values[2, True], 0, n1)):
            assert len(x) == len(y) and (x == y).all()
        # counters: a candidate is a position the exact pass left a length for; it is probed once at its limit and, where that passes and
        # lengths below the limit are open, along the schedule until the bracket closes: the number of probes follows from (mul_0, limit,
        # mul_e) alone, so the total is held exactly
        limit = np.minimum(U.run_lengths(text), 64)
        for e, fo in ((1, False), (2, False), (2, True)):
            st, mul0, mul = session_values[e, fo, "stats"], session_values[0, fo], session_values[e, fo]
            cand = np.nonzero(mul0)[0]
            assert st["candidates"] == len(cand) > 50000 and st["launches"] == 1
            exp = sum(_probes_of(int(mul0[p]) - 1, int(limit[p]), int(mul[p])) for p in cand.tolist())
            assert st["probes"] == exp and st["candidates"] <= st["probes"] <= 16 * st["candidates"], (e, fo, st, exp)
            assert st["table_reads"] > 0 and st["steps"] + st["verified_rows"] > 0
            assert st["k"] == 64 and st["n"] == n1 + 1 and st["ms_scatter"] == 0 and st["ms_valid"] == 0 and st["ms_search"] > 0
            assert st["ms_total"] == pytest.approx(st["ms_forward"] + st["ms_reverse"] + st["ms_search"], rel=1e-9)
            assert st["transient_bytes"] >= 2 * n1
        for kw in ({"max_k": 9}, {"max_k": 1001}, {"mismatches": 3}):
            for call in (ix.min_unique, ix.min_unique_runs):
                with pytest.raises(dicey_amd.DgError) as err:
                    call(**{"max_k": 40, "mismatches": 1, **kw})
                assert err.value.code == -7 and "dg_min_unique_mm" in str(err.value)
        # the result is an ordinary map: dg_map_mm_stats stays zero, the new getter is zero for maps made by other calls
        m = C.c_void_p()
        prm = dicey_amd._capi.MinUniqueMmParams(40, 1, 0, 0, 0)
        assert L.dg_min_unique_mm(ix.handle, C.byref(prm), C.byref(m)) == 0
        try:
            mm, mu = dicey_amd._capi.MapMmStats(), dicey_amd._capi.MuMmStats()
            assert L.dg_map_mm_stats(m, C.byref(mm)) == 0 and L.dg_map_mu_mm_stats(m, C.byref(mu)) == 0
            assert not any(getattr(mm, f) for f, _ in dicey_amd._capi.MapMmStats._fields_)
            assert mu.candidates > 50000 and mu.probes >= mu.candidates and mu.launches == 1
            assert L.dg_map_device_values(m)
            buf = (C.c_uint32 * 4)()
            assert L.dg_map_values(m, n1 - 2, n1 + 2, buf) == -1
            assert L.dg_map_values(m, n1 - 4, n1, buf) == 0
        finally:
            L.dg_map_free(m)
        for prm, other in ((dicey_amd._capi.MinUniqueMmParams(40, 0, 0, 0, 0), L.dg_min_unique_mm),
                           (dicey_amd._capi.MinUniqueParams(40, 0, 0, 0), L.dg_min_unique),
                           (dicey_amd._capi.MapMmParams(20, 1, 0, 0, 0, 0), L.dg_mappability_mm)):
            assert other(ix.handle, C.byref(prm), C.byref(m)) == 0
            try:
                mu = dicey_amd._capi.MuMmStats()
                assert L.dg_map_mu_mm_stats(m, C.byref(mu)) == 0
                assert not any(getattr(mu, f) for f, _ in dicey_amd._capi.MuMmStats._fields_)
            finally:
                L.dg_map_free(m)
        prm = dicey_amd._capi.MinUniqueMmParams(40, 1, 0, 1, 0)
        assert L.dg_min_unique_mm(ix.handle, C.byref(prm), C.byref(m)) == -1 and not m.value


def test_refused_while_a_hunt_batch_is_in_flight(small_genome, session_values):
    g = small_genome
    rng = random.Random(9)
    t = g["text"].decode()
    qs = []
    while len(qs) < 300:
        p = rng.randrange(len(t) - 20)
        if "\n" not in t[p:p + 20]:
            qs.append(t[p:p + 20])
    flat = lambda res: [[(h.score, h.chr, h.start, h.strand, h.refalign, h.queryalign) for h in q.hits] for q in res.queries]
    with dicey_amd.FmIndex(g["fm9"]) as ix:
        before = flat(ix.hunt(qs, g["seqlen"], distance=1))
        assert sum(len(x) for x in before) >= 300
        tk = ix.hunt_submit(qs, g["seqlen"], distance=1)
        try:
            with pytest.raises(dicey_amd.DgError) as e:
                ix.min_unique(max_k=64, mismatches=1)
            assert e.value.code == -1 and "in flight" in str(e.value) and "dg_min_unique_mm" in str(e.value)
        finally:
            waited = flat(ix.hunt_wait(tk))
        assert waited == before
        _same(ix.min_unique(max_k=64, mismatches=1), session_values[1, False], "after the batch")
        assert flat(ix.hunt(qs, g["seqlen"], distance=1)) == before
