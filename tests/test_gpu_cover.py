"""dg_map_cover / dg_map_min_cover and their Python mirror against tests/cover_ref.py: the cover count of every position of the 90 kb
session genome across k, mismatches, strands, thresholds and clamps, fed with the library's own start-position values (which other
tests pin); a crafted genome and tiny genomes against the definition alone; the minimum covering length against the formula, on the
product build and across tile sizes on the development build; the identity between the two tracks on a 4 Mb genome, library against
library; the argument checks in their order."""
import ctypes as C

import numpy as np
import pytest

try:  # torch bundles its own HIP runtime: it only finds the GPU if it initialises before libdiceygpu's (system) runtime does
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import conftest
import cover_ref as V
import dicey_amd
import genome_shapes as S
import mappability_ref as R
import min_unique_mm_ref as W
import min_unique_ref as U
from conftest import genome_text
from dicey_amd import _capi

pytestmark = pytest.mark.gpu
EINVAL, ENODEV, ENOMEM, ELIMIT = -1, -4, -6, -7
TOP = 0xFFFFFFFD


def _same(got, exp, what):
    assert got.dtype == np.uint32 and len(got) == len(exp), what
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])


class Maps:
    """the C calls on one index handle, maps as raw pointers"""

    def __init__(self, ix):
        self.ix, self.L = ix, ix._L

    def count_map(self, k, e=0, fo=False, max_count=0):
        return self.ix._map(k, fo, max_count, e)

    def length_map(self, max_k, e=0, fo=False):
        return self.ix._min_unique(max_k, fo, e)

    def cover(self, src, at_most=1, max_count=0, flags=0, reserved=0, handle=True, prm=True, out=True):
        m = C.c_void_p(0xDEAD)  # cleared on every failure
        p = _capi.CoverParams(at_most, max_count, flags, reserved)
        rc = self.L.dg_map_cover(self.ix.handle if handle else None, src, C.byref(p) if prm else None, C.byref(m) if out else None)
        return rc, m

    def min_cover(self, src, flags=0, reserved=0, handle=True, prm=True, out=True):
        m = C.c_void_p(0xDEAD)
        p = _capi.MinCoverParams(flags, reserved)
        rc = self.L.dg_map_min_cover(self.ix.handle if handle else None, src, C.byref(p) if prm else None, C.byref(m) if out else None)
        return rc, m

    def values(self, m):
        st = _capi.MapStats()
        assert self.L.dg_map_stats(m, C.byref(st)) == 0
        out = np.zeros(st.n - 1, dtype=np.uint32)
        assert self.L.dg_map_values(m, 0, st.n - 1, out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
        return out

    def cover_stats(self, m):
        cs = _capi.CoverStats()
        assert self.L.dg_map_cover_stats(m, C.byref(cs)) == 0
        return {f: getattr(cs, f) for f, _ in _capi.CoverStats._fields_}

    def map_stats(self, m):
        st = _capi.MapStats()
        assert self.L.dg_map_stats(m, C.byref(st)) == 0
        return {f: getattr(st, f) for f, _ in _capi.MapStats._fields_}

    def free(self, m):
        self.L.dg_map_free(m)

    def error(self):
        return (self.L.dg_last_error() or b"").decode()


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    text = genome_text(V.crafted_seqs())
    path = str(tmp_path_factory.mktemp("cover") / "crafted.fm9")
    dicey_amd.build_index(text, path)
    return {"text": text, "fm9": path}


# ---- the cover count ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 63, 64, 65, 127, 129, 1000])
def test_cover_on_the_session_genome(small_genome, k):
    """every position, for both mismatch settings and strands, every threshold and clamp: one count map each, sixteen transforms of it"""
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        M = Maps(ix)
        for e in (0, 1):
            for fo in (False, True):
                src = M.count_map(k, e, fo)
                try:
                    base = M.values(src)
                    for at_most in (1, 2, 5, TOP):
                        for max_count in (0, 1, 3, k):
                            rc, m = M.cover(src, at_most, max_count)
                            assert rc == 0, M.error()
                            try:
                                exp = V.cover(base, k, at_most, max_count)
                                _same(M.values(m), exp, (k, e, fo, at_most, max_count))
                                cs = M.cover_stats(m)
                                assert cs["specific"] == int(((base >= 1) & (base <= at_most)).sum()) and cs["covered"] == int((exp != 0).sum()), cs
                                assert cs["kind"] == _capi.DG_MAP_KIND_COVER and cs["k"] == k and cs["at_most"] == at_most and cs["max_count"] == max_count
                            finally:
                                M.free(m)
                    _same(M.values(src), base, "the source map after its transforms")
                finally:
                    M.free(src)


def test_session_genome_has_every_cover_class(small_genome):
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        c = ix.cover(k=64)
        assert (c == 64).sum() > 10000 and ((c > 0) & (c < 64)).sum() > 1000 and (c == 0).sum() > 500
        c2 = ix.cover(k=64, at_most=2)
        assert (c2 >= c).all() and (c2 > c).sum() > 100


@pytest.mark.parametrize("fo", [False, True])
@pytest.mark.parametrize("e", [0, 1])
def test_cover_on_the_crafted_genome_against_the_definition(crafted, e, fo):
    """no library value involved: FmIndex.cover against the windows of the brute-force models"""
    text = crafted["text"]
    with dicey_amd.FmIndex(crafted["fm9"]) as ix:
        for k in (10, 20, 40):
            for at_most, max_count in ((1, 0), (2, 0), (5, 3), (1, 1)):
                st = {}
                got = ix.cover(k=k, at_most=at_most, forward_only=fo, max_count=max_count, mismatches=e, stats=st)
                exp = V.cover_by_windows(text, k, at_most, max_count, e, fo)
                _same(got, exp, (k, e, fo, at_most, max_count))
                assert st["covered"] == int((exp != 0).sum()) and st["n"] == len(text) + 1 and st["k"] == k
        assert (V.cover_by_windows(text, 40, 1, 0, e, fo) != 0).sum() > 500


TINY_LENGTHS = (9, 10, 63, 64, 65, 128, 129)


@pytest.mark.parametrize("length", TINY_LENGTHS)
def test_tiny_genomes_of_one_sequence(tmp_path, length):
    """word edges, a window clipped at position 0, a text shorter than k: one random sequence, the text `length` bytes with its newline"""
    rng = np.random.default_rng(length)
    text = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), length - 1).tolist()) + b"\n"
    _tiny(tmp_path, text, length)


@pytest.mark.parametrize("name", S.TINY_NAMES)
def test_tiny_shapes(tmp_path, name):
    _tiny(tmp_path, S.all_shapes()[name]["text"], name)


def _tiny(tmp_path, text, what):
    fm9 = str(tmp_path / "tiny.fm9")
    dicey_amd.build_index(text, fm9)
    with dicey_amd.FmIndex(fm9) as ix:
        for k in (10, 24):
            _same(ix.cover(k=k), V.cover(R.values(text, k), k), (what, "cover", k))
            _same(ix.cover(k=k, at_most=2, max_count=1), V.cover(R.values(text, k), k, 2, 1), (what, "cover", k, 2, 1))
            _same(ix.min_cover(max_k=k), V.min_cover(text, U.by_values(text, k), k), (what, "min cover", k))
        if len(text) <= 600:
            _same(ix.cover(k=10), V.cover_by_windows(text, 10), (what, "by windows"))
            _same(ix.min_cover(max_k=24), V.min_cover_by_windows(text, 24), (what, "min cover by windows"))


# ---- the minimum covering length ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fo", [False, True])
@pytest.mark.parametrize("e", [0, 1])
def test_min_cover_on_the_crafted_genome(crafted, e, fo):
    text = crafted["text"]
    with dicey_amd.FmIndex(crafted["fm9"]) as ix:
        for max_k in (10, 16, 40, 64, 100):
            mul = U.by_values(text, max_k, fo) if e == 0 else W.pairwise(text, max_k, e, fo)
            exp = V.min_cover(text, mul, max_k)
            st = {}
            _same(ix.min_cover(max_k=max_k, forward_only=fo, mismatches=e, stats=st), exp, (max_k, e, fo))
            assert st["kind"] == _capi.DG_MAP_KIND_MIN_COVER and st["k"] == max_k and st["at_most"] == 0
            assert st["specific"] == int((mul != 0).sum()) and st["covered"] == int((exp != 0).sum()) > 500, st


@pytest.fixture(scope="module")
def session_min_cover(small_genome):
    """max_k -> (the product library's min_unique values, its min_cover values)"""
    out = {}
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        for max_k in (64, 1000):
            out[max_k] = (ix.min_unique(max_k=max_k), ix.min_cover(max_k=max_k))
    return out


@pytest.mark.parametrize("max_k", [64, 1000])
def test_min_cover_on_the_session_genome(small_genome, session_min_cover, max_k):
    mul, got = session_min_cover[max_k]
    exp = V.min_cover(small_genome["text"], mul, max_k)
    _same(got, exp, max_k)
    acgt = U.run_lengths(small_genome["text"]) > 0
    # both classes are there: most bases of a 90 kb genome have a unique window of at most 64 over them, those of its copies have none
    assert (exp != 0).sum() > len(exp) // 2 and (acgt & (exp == 0)).sum() > 50 and not exp[~acgt].any()


@pytest.mark.parametrize("tile", [64, 192, 2048])
def test_tiles_on_the_development_build(small_genome, session_min_cover, monkeypatch, tile):
    """max_k = 1000: the 999 positions in front of a tile span several tiles of 64 or 192; the lengths are the product library's"""
    monkeypatch.setenv("DICEY_COVER_TILE", str(tile))
    ix = dicey_amd.FmIndex(small_genome["fm9"], _lib=conftest.exp_lib())
    try:
        for max_k in (1000, 64):
            _same(ix.min_cover(max_k=max_k), session_min_cover[max_k][1], (tile, max_k))
    finally:
        ix.close()


# ---- the identity, library against library ---------------------------------------------------------------------------------------------

def _genome_4mb():
    """two sequences, 4 Mb: random bases, copies on both strands, N runs that leave A/C/G/T runs shorter than k behind, a poly-A"""
    rng = np.random.default_rng(4)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = acgt[rng.integers(0, 4, 4_000_000)].copy()
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    for _ in range(200):
        a, b, m = int(rng.integers(0, 3_990_000)), int(rng.integers(0, 3_990_000)), int(rng.integers(30, 3000))
        piece = t[a:a + m].copy()
        t[b:b + len(piece)] = comp[piece][::-1] if rng.random() < 0.5 else piece
    for _ in range(300):
        a = int(rng.integers(0, 3_999_000))
        t[a:a + int(rng.integers(1, 200))] = ord("N")
        b = a + 250 + int(rng.integers(5, 120))  # a second N run close behind: a short A/C/G/T run between them
        t[b:b + int(rng.integers(1, 50))] = ord("N")
    t[1_000_000:1_002_000] = ord("A")
    t[2_500_000] = ord("\n")
    return t.tobytes()[:3_999_999] + b"\n"


def test_identity_on_a_4mb_genome(tmp_path):
    text = _genome_4mb()
    fm9 = str(tmp_path / "g4.fm9")
    dicey_amd.build_index(text, fm9)
    with dicey_amd.FmIndex(fm9) as ix:
        mcl = ix.min_cover(max_k=100)
        for k in (24, 100):
            cov = ix.cover(k=k)
            _same(cov, V.cover(ix.mappability(k=k), k), ("sliding sum", k))
            ok = V.coverable(text, k)
            short = (mcl != 0) & (mcl <= k)
            bad = np.nonzero((cov[ok] >= 1) != short[ok])[0]
            assert len(bad) == 0, (k, len(bad), np.nonzero(ok)[0][bad[:10]])
            # both classes, and the restriction bites: short runs between N runs hold bases with a unique shorter window
            assert (cov[ok] >= 1).sum() > 2_500_000 and (cov[ok] == 0).sum() > 1000 and not cov[~ok].any()
            assert k == 24 or short[~ok].sum() > 100


# ---- the contract ---------------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order(small_genome, crafted):
    k = 20
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix, dicey_amd.FmIndex(crafted["fm9"]) as other:
        M, O = Maps(ix), Maps(other)
        cnt, ln, clamped = M.count_map(k), M.length_map(40), M.count_map(k, max_count=2)
        rc, cov = M.cover(cnt)
        assert rc == 0
        try:
            def refused(res, code, word):
                rc, m = res
                assert rc == code and word in M.error(), (rc, M.error())
                assert not m.value or m.value == 0xDEAD  # 0xDEAD: no out pointer was given
                return True

            # 1. null parameter block, out or src, before anything else (the other arguments bad as well)
            assert refused(M.cover(cnt, prm=False, handle=False), EINVAL, "null argument")
            rc, m = M.cover(cnt, out=False, flags=1)
            assert rc == EINVAL and "null argument" in M.error()
            assert refused(M.cover(None, flags=1, at_most=0), EINVAL, "null argument")
            assert refused(M.min_cover(None, flags=1), EINVAL, "null argument")
            assert refused(M.min_cover(ln, prm=False), EINVAL, "null argument")
            # 2. flags and reserved, before the threshold
            assert refused(M.cover(cnt, flags=1, at_most=0), EINVAL, "flags and reserved")
            assert refused(M.cover(cnt, reserved=1, at_most=0, handle=False), EINVAL, "flags and reserved")
            assert refused(M.min_cover(ln, reserved=7, handle=False), EINVAL, "flags and reserved")
            # 3. the threshold, before the handle
            for t in (0, 0xFFFFFFFE, 0xFFFFFFFF):
                assert refused(M.cover(cnt, at_most=t, handle=False), ELIMIT, "at_most")
            # 4. the handle, before the map's kind
            assert refused(M.cover(ln, handle=False), EINVAL, "null argument")
            assert refused(M.min_cover(cnt, handle=False), EINVAL, "null argument")
            # 5. the kind, before the index (`other` has another n)
            assert refused(O.cover(ln), EINVAL, "holds lengths")
            assert refused(O.cover(cov), EINVAL, "holds per-base values")
            assert refused(O.min_cover(cnt), EINVAL, "holds counts")
            assert refused(M.min_cover(cov), EINVAL, "holds per-base values")
            # 6. the index, before the clamp
            assert refused(O.cover(clamped, at_most=2), EINVAL, "of an index of")
            assert refused(O.min_cover(ln), EINVAL, "of an index of")
            # 7. a source whose clamp hides the answer
            assert refused(M.cover(clamped, at_most=2), EINVAL, "max_count = 2")
            assert refused(M.cover(clamped, at_most=TOP), EINVAL, "max_count = 2")
            rc, m = M.cover(clamped, at_most=1)
            assert rc == 0, M.error()
            try:
                _same(M.values(m), M.values(cov), "a source clamped at 2 answers at_most = 1")
            finally:
                M.free(m)
        finally:
            for m in (cnt, ln, clamped, cov):
                M.free(m)


def test_result_is_an_ordinary_map(small_genome):
    text = small_genome["text"]
    n1 = len(text)
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        M = Maps(ix)
        src = M.count_map(30)
        before = M.values(src)
        src_stats = M.cover_stats(src)
        assert not any(src_stats.values())  # all zero for a map of another kind
        rc, m = M.cover(src, 1, 0)
        assert rc == 0, M.error()
        M.free(src)  # the source goes first: the result owns what it needs
        try:
            vals = M.values(m)
            _same(vals, V.cover(before, 30), "cover")
            st = M.map_stats(m)
            assert st["n"] == n1 + 1 and st["k"] == 30 and st["ms_total"] > 0
            assert not any(st[f] for f in ("ms_valid", "ms_forward", "ms_reverse", "ms_scatter", "rev_steps", "transient_bytes"))
            cs = M.cover_stats(m)
            assert cs["ms_bits"] > 0 and cs["ms_cover"] > 0 and cs["transient_bytes"] >= n1 // 8 + n1 // 16
            assert st["ms_total"] == pytest.approx(cs["ms_bits"] + cs["ms_cover"], rel=1e-9)
            assert M.L.dg_map_device_values(m)
            mm, mu = _capi.MapMmStats(), _capi.MuMmStats()
            assert M.L.dg_map_mm_stats(m, C.byref(mm)) == 0 and M.L.dg_map_mu_mm_stats(m, C.byref(mu)) == 0
            assert not any(getattr(mm, f) for f, _ in _capi.MapMmStats._fields_) and not any(getattr(mu, f) for f, _ in _capi.MuMmStats._fields_)
            s0, l0, _ = R.runs(vals, 0, n1)
            long_runs = np.nonzero(l0 >= 5)[0]
            a, b = int(s0[long_runs[1]] + 2), int(s0[long_runs[-2]] + 3)
            for lo, hi in ((0, n1), (a, b), (a, a + 1), (a, a), (n1 - 7, n1)):
                got = ix._map_runs(m, lo, hi)
                for x, y in zip(got, R.runs(vals, lo, hi)):
                    assert x.dtype == y.dtype and len(x) == len(y) and (x == y).all(), (lo, hi)
        finally:
            M.free(m)
        for x, y in zip(ix.cover_runs(k=30, lo=a, hi=b), R.runs(vals, a, b)):
            assert len(x) == len(y) and (x == y).all()
        mc = ix.min_cover(max_k=64)
        for x, y in zip(ix.min_cover_runs(max_k=64), R.runs(mc, 0, n1)):
            assert len(x) == len(y) and (x == y).all()
        # existing maps keep their stats: nothing of the per-base record shows in dg_map_stats
        stc = {}
        ix.mappability(k=30, stats=stc)
        assert stc["k"] == 30 and stc["ms_total"] > 0 and stc["transient_bytes"] > 0 and "specific" not in stc


def test_runs_while_a_hunt_batch_is_in_flight(small_genome):
    """the transform reads the map and the text alone: a batch in flight on the handle does not refuse it (making the source map would)"""
    g = small_genome
    t = g["text"].decode()
    qs = [t[p:p + 20] for p in range(100, 30000, 97) if "\n" not in t[p:p + 20]][:300]
    with dicey_amd.FmIndex(g["fm9"]) as ix:
        M = Maps(ix)
        src = M.count_map(24)
        try:
            exp = V.cover(M.values(src), 24)
            tk = ix.hunt_submit(qs, g["seqlen"], distance=1)
            try:
                rc, m = M.cover(src)
                assert rc == 0, M.error()
            finally:
                ix.hunt_wait(tk)
            try:
                _same(M.values(m), exp, "beside a batch")
            finally:
                M.free(m)
        finally:
            M.free(src)
