"""The mappability family on the genome shapes of tests/genome_shapes.py (inputs and grids: tests/mappability_shapes.py, shown to exercise
what they claim by tests/test_mappability_shapes_host.py): dg_mappability_mm, dg_min_unique, dg_query_map, dg_query_map_anchored,
dg_query_map_iupac, dg_query_min_len and dg_query_min_len_end on thousands of short and empty records, N as the most frequent symbol, a
base missing from the alphabet, A/T tandem repeats, every IUPAC letter and texts of 1 to 4 097 symbols, against the brute-force references
that know nothing of the FM-index.  Every comparison is exact equality of uint32 arrays.  Each shape is built once and kept open; each
reference is computed once per module."""
import gzip
import os
import subprocess

import numpy as np
import pytest

try:  # torch bundles its own HIP runtime: it only finds the GPU if it initialises before libdiceygpu's (system) runtime does
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import conftest
import dicey_amd
import mappability_mm_ref as M
import mappability_ref as R
import mappability_shapes as P
import min_unique_ref as U
import query_anchor_ref as A
import query_iupac_ref as I
import query_map_ref as Q
import query_min_len_end_ref as QE
import query_min_len_ref as QL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")
INV = Q.INVALID
OPEN_FLAGS = [{}, {"compact": True, "pre5": False}, {"kmer_table": False}]
_memo = {}


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


# ---- the references, once per module ------------------------------------------------------------------------------------------------

def _text(name):
    return P.get(name)["text"]


def _recs(name, kind="plain"):
    """(records as handed to the library, the same as the bytes it sees, the model's buffer)"""
    def make():
        recs = P.records(name, P.get(name))[kind]
        b = P.as_bytes(recs)
        return recs, b, Q.buffer_of(b)[0]
    return _once(("recs", name, kind), make)


def _track(name, k, e):
    return _once(("track", name, k, e), lambda: M.parts_ball(_text(name), k, e))


def _plain(name, k, e):
    return _once(("plain", name, k, e), lambda: Q.parts_ball(_text(name), _recs(name)[2], k, e))


def _anchored(name, k, e):
    return _once(("anch", name, k, e), lambda: A.parts_ball(_text(name), _recs(name)[2], k, e, P.anchors_of(k)))


def _iupac_shape(name):
    """the shape whose index the IUPAC call runs against: a cut where the model's cost asks for one"""
    return P.IUPAC_TEXT.get(name, name)


def _iupac(name):
    ks = sorted({k for k, _ in P.count_cells(name)})
    return _once(("iupac", name), lambda: I.parts(_text(_iupac_shape(name)), _recs(name, "iupac")[2], ks, (0, 1, 2),
                                                  {k: P.anchors_of(k) for k in ks}, max_degeneracy=P.MAX_DEGENERACY)[0])


def _minlen(name, e):
    return _once(("minlen", name, e), lambda: QL.parts_by_k(_text(name), _recs(name)[2], range(P.MIN_K, P.MAX_K + 1), e))


def _minlen_end(name, e):
    return _once(("minlen_end", name, e),
                 lambda: QE.parts_by_k(_text(name), _recs(name)[2], range(P.MIN_K, P.MAX_K + 1), e, P.END_ANCHORS))


def _capped(full, cap):
    return [np.where(x == INV, INV, np.minimum(x, cap)).astype(np.uint32) if cap else x for x in full]


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------

def _same(got, exp, what):
    assert got.dtype == np.uint32 and len(got) == len(exp), (what, len(got), len(exp))
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])


def _same_recs(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for i, (g, x) in enumerate(zip(got, exp)):
        assert g.dtype == np.uint32 and len(g) == len(x), (what, i)
        bad = np.nonzero(g != x)[0]
        assert len(bad) == 0, (what, i, len(bad), bad[:10], g[bad[:10]], x[bad[:10]])


# ---- the indices ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> path of the shape's index, written by dicey_amd.build_index once"""
    d = tmp_path_factory.mktemp("mapshapes")
    made = {}

    def get(name):
        if name not in made:
            made[name] = str(d / (name + ".fm9"))
            dicey_amd.build_index(_text(name), made[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def opened(built):
    """name -> FmIndex with the default flags, kept open for the module"""
    ixs = {}

    def get(name):
        if name not in ixs:
            ixs[name] = dicey_amd.FmIndex(built(name))
        return ixs[name]
    yield get
    for ix in ixs.values():
        ix.close()


def _big_cell(name):
    """the e = 2 cell of the matrices: k = 20 where the grid has it"""
    return (20, 2) if (20, 2) in P.count_cells(name) else (12, 2)


# ---- the genome track -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.SHAPES)
def test_mappability_with_mismatches(opened, name):
    ix = opened(name)
    counted = 0
    for k, e in P.count_cells(name):
        fwd, rev = _track(name, k, e)
        for fo in P.STRANDS:
            full = M._finish(fwd, rev, fo, 0)
            for cap in P.MAX_COUNTS:
                st = {}
                got = ix.mappability(k=k, mismatches=e, forward_only=fo, max_count=cap, stats=st)
                _same(got, M._finish(fwd, rev, fo, cap), (name, k, e, fo, cap))
                if e and cap:   # a head whose count reaches the cap stops there; a tiny text may hold no such head
                    assert (st["early_exits"] > 0) == bool((full >= cap).any()), (name, k, e, fo, cap, st)
                    assert st["early_exits"] > 0 or name in P.TINY
        counted += int((fwd + rev > 0).sum())
    assert counted > 0 or len(_text(name)) < 20


@pytest.mark.parametrize("name", P.SHAPES + P.MU_ONLY)
def test_min_unique(opened, name):
    ix = opened(name)
    text = _text(name)
    for max_k in P.mu_max_ks(name):
        for fo in P.STRANDS:
            exp = _once(("mu", name, max_k, fo), lambda: U.by_values(text, max_k, fo))
            _same(ix.min_unique(max_k=max_k, forward_only=fo), exp, (name, max_k, fo))
    vals = _once(("mu", name, 24, False), lambda: U.by_values(text, 24, False))
    starts = [0]
    if name == "many_short_800":   # inside the adjacent pair of empty records
        starts += [i for i in range(1, len(text)) if text[i] == 10 and text[i - 1] == 10]
        assert len(starts) >= 3
    for lo in starts:
        for hi in (lo + 1, lo + 700, len(text)):
            hi = min(hi, len(text))
            got = ix.min_unique_runs(max_k=24, lo=lo, hi=hi)
            for x, y in zip(got, R.runs(vals, lo, hi)):
                assert x.dtype == y.dtype and len(x) == len(y) and (x == y).all(), (name, lo, hi)


# ---- the query calls ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.SHAPES)
def test_query_mappability_plain_and_anchored(opened, name):
    ix = opened(name)
    recs, b, qbuf = _recs(name)
    npos = sum(len(r) for r in b)
    for k, e in P.count_cells(name):
        for fo in P.STRANDS:
            for cap in P.MAX_COUNTS:
                fwd, rev, valid = _plain(name, k, e)
                st = {}
                got = ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo, max_count=cap, stats=st)
                full = Q.split(Q.finish(fwd, rev, valid, fo, 0), b)
                _same_recs(got, Q.split(Q.finish(fwd, rev, valid, fo, cap), b), (name, k, e, fo, cap))
                assert st["positions"] == npos and st["valid"] == valid.sum(), (name, k, e, fo, cap, st)
                if cap:
                    assert st["early_exits"] == sum(int(((x != INV) & (x >= cap)).sum()) for x in full), (name, k, e, fo, cap, st)
                for a, (fa, ra, va) in _anchored(name, k, e).items():
                    st = {}
                    got = ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo, max_count=cap, anchor=a, stats=st)
                    _same_recs(got, Q.split(Q.finish(fa, ra, va, fo, cap), b), (name, k, e, fo, cap, "anchor", a))
                    assert st["positions"] == npos and st["valid"] == va.sum(), (name, k, e, fo, cap, a, st)


@pytest.mark.parametrize("name", P.SHAPES)
def test_query_mappability_iupac(opened, name):
    ix = opened(_iupac_shape(name))
    recs, b, qbuf = _recs(name, "iupac")
    npos = sum(len(r) for r in b)
    parts = _iupac(name)
    for k, e in P.count_cells(name):
        letters, deg = I.degeneracy(qbuf, k)
        for a in P.anchors_of(k):
            f, r, valid = parts[k, e, a]
            for fo in P.STRANDS:
                for cap in P.MAX_COUNTS:
                    st = {}
                    got = ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo, max_count=cap, anchor=a, iupac=True,
                                               max_degeneracy=P.MAX_DEGENERACY, stats=st)
                    _same_recs(got, Q.split(I.finish(f, r, valid, fo, cap), b), (name, k, e, a, fo, cap))
                    assert st["positions"] == npos and st["valid"] == valid.sum(), (name, k, e, a, fo, cap, st)
                    assert st["too_degenerate"] == (letters & ~valid).sum() and st["degenerate"] == (deg[valid] > 1).sum(), (name, k, e, a, fo, cap, st)
                    if not cap:
                        assert st["expansions"] == deg[valid].sum() * (1 if fo else 2), (name, k, e, a, fo, st)
    if name in P.BIG:   # the coded records are not vacuous: degenerate 12-mers that occur (hit codes) and that do not (miss codes)
        f, r, valid = parts[12, 0, 0]
        d = I.degeneracy(qbuf, 12)[1]
        assert ((d > 1) & valid & (f + r > 0)).sum() >= 50 and ((d > 1) & valid & (f + r == 0)).sum() >= 50


@pytest.mark.parametrize("name", P.SHAPES)
def test_query_min_length(opened, name):
    ix = opened(name)
    recs, b, qbuf = _recs(name)
    for e in P.MINLEN_ES:
        parts = _minlen(name, e)
        for t in P.AT_MOST:
            for fo in P.STRANDS:
                got = ix.query_min_length(recs, max_k=P.MAX_K, min_k=P.MIN_K, at_most=t, mismatches=e, forward_only=fo)
                _same_recs(got, QL.split(QL.min_len(parts, qbuf, P.MIN_K, P.MAX_K, t, fo), b), (name, e, t, fo))


@pytest.mark.parametrize("name", P.SHAPES)
def test_query_min_length_end(opened, name):
    ix = opened(name)
    recs, b, qbuf = _recs(name)
    for e in P.MINLEN_ES:
        parts = _minlen_end(name, e)
        for a in P.END_ANCHORS:
            for t in P.AT_MOST:
                for fo in P.STRANDS:
                    got = ix.query_min_length_end(recs, max_k=P.MAX_K, min_k=P.MIN_K, at_most=t, mismatches=e, anchor=a, forward_only=fo)
                    _same_recs(got, QE.split(QE.min_len_end(parts, qbuf, P.MIN_K, P.MAX_K, a, t, fo), b), (name, e, a, t, fo))


def _by_end(per_record, k):
    """values indexed by the k-mer's first base -> by its last base, record by record"""
    out = []
    for v in per_record:
        w = np.full(len(v), INV, dtype=np.uint32)
        if len(v) >= k:
            w[k - 1:] = v[:len(v) - k + 1]
        out.append(w)
    return out


def test_every_answer_is_the_first_length_that_passes(opened):
    """on the tandem text, where nothing is rare: for every length L > 0 the device's own count of the L-mer there is <= t and that of the
    (L-1)-mer is > t, by start and by end position; where the answer is 0 no length passes"""
    ix = opened("at_tandem")
    recs = _recs("at_tandem")[0]
    lo, hi = P.MIN_K, P.MAX_K
    for by_end, e, a, t in ((False, 1, 0, 50), (False, 0, 0, 1), (True, 1, 5, 50), (True, 0, 10, 0)):
        if by_end:
            got = np.concatenate(ix.query_min_length_end(recs, max_k=hi, min_k=lo, at_most=t, mismatches=e, anchor=a))
            cnt = {k: np.concatenate(_by_end(ix.query_mappability(recs, k=k, mismatches=e, anchor=a), k)) for k in range(lo, hi + 1)}
        else:
            got = np.concatenate(ix.query_min_length(recs, max_k=hi, min_k=lo, at_most=t, mismatches=e))
            cnt = {k: np.concatenate(ix.query_mappability(recs, k=k, mismatches=e)) for k in range(lo, hi + 1)}
        checked = 0
        for L in range(lo, hi + 1):
            at = got == L
            assert (cnt[L][at] <= t).all(), (by_end, e, a, t, L)
            if L > lo:
                assert (cnt[L - 1][at] != INV).all() and (cnt[L - 1][at] > t).all(), (by_end, e, a, t, L)
            checked += int(at.sum())
        zero = got == 0
        assert all(((cnt[k][zero] == INV) | (cnt[k][zero] > t)).all() for k in cnt), (by_end, e, a, t)
        assert checked >= 100 and zero.sum() >= 100, (by_end, e, a, t, checked, int(zero.sum()))


# ---- the same index on other paths ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.FOUR)
def test_open_flags_give_identical_arrays(built, name):
    recs, b, _ = _recs(name)
    for kw in OPEN_FLAGS:
        with dicey_amd.FmIndex(built(name), **kw) as ix:
            for k, e in ((20, 1), _big_cell(name)):
                fwd, rev = _track(name, k, e)
                _same(ix.mappability(k=k, mismatches=e), M._finish(fwd, rev, False, 0), (name, kw, k, e))
                _same_recs(ix.query_mappability(recs, k=k, mismatches=e), Q.split(Q.finish(*_plain(name, k, e)), b), (name, kw, k, e, "query"))


@pytest.mark.parametrize("name", ["bisulfite", "at_tandem", "tiny_513"])
def test_table_order_twelve(built, name):
    """DICEY_KMER_K (a product tuning knob) = 12: k = 10 lies below the table's order, k = 12 at it"""
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("DICEY_KMER_K", "12")
        ix = dicey_amd.FmIndex(built(name))
    finally:
        mp.undo()
    recs, b, qbuf = _recs(name)
    try:
        for k in (10, 12):
            for e in (1, 2):
                fwd, rev = _track(name, k, e)
                st = {}
                _same(ix.mappability(k=k, mismatches=e, stats=st), M._finish(fwd, rev, False, 0), (name, k, e))
                assert (st["table_reads"] > 0) == (k >= 12 and st["heads"] > 0), (name, k, e, st)
                _same_recs(ix.query_mappability(recs, k=k, mismatches=e), Q.split(Q.finish(*_plain(name, k, e)), b), (name, k, e, "query"))
    finally:
        ix.close()


@pytest.mark.parametrize("narrow", ["0", "1000000000"])
@pytest.mark.parametrize("name", P.FOUR)
def test_narrow_finish_forbidden_and_forced(built, monkeypatch, name, narrow):
    """the development build with DICEY_MAP_NARROW = 0 (every interval goes through the levels) and = 10^9 (every interval is finished
    on the text): the same arrays"""
    recs, b, _ = _recs(name)
    irecs, ib, _ = _recs(name, "iupac")
    monkeypatch.setenv("DICEY_MAP_NARROW", narrow)
    ix = dicey_amd.FmIndex(built(name), _lib=conftest.exp_lib())
    iix = ix if _iupac_shape(name) == name else dicey_amd.FmIndex(built(_iupac_shape(name)), _lib=conftest.exp_lib())
    try:
        for k, e in ((20, 1), _big_cell(name)):
            # (on the tandem text with every interval finished row by row a lane walks intervals of up to 30 000 rows once per table
            # entry and, in the IUPAC call, per expansion: that one case takes 11 s on the device, every other one a second or less)
            fwd, rev = _track(name, k, e)
            sts = [{}, {}, {}]
            _same(ix.mappability(k=k, mismatches=e, stats=sts[0]), M._finish(fwd, rev, False, 0), (name, narrow, k, e))
            _same_recs(ix.query_mappability(recs, k=k, mismatches=e, stats=sts[1]), Q.split(Q.finish(*_plain(name, k, e)), b),
                       (name, narrow, k, e, "query"))
            got = iix.query_mappability(irecs, k=k, mismatches=e, iupac=True, max_degeneracy=P.MAX_DEGENERACY, stats=sts[2])
            _same_recs(got, Q.split(I.finish(*_iupac(name)[k, e, 0]), ib), (name, narrow, k, e, "iupac"))
            for st in sts:
                if narrow == "0":
                    assert st["verified_rows"] == 0 and st["steps"] > 0, (name, k, e, st)
                else:
                    assert st["steps"] == 0 and st["verified_rows"] > 0, (name, k, e, st)
    finally:
        if iix is not ix:
            iix.close()
        ix.close()


@pytest.mark.parametrize("name", ["tiny_129", "tiny_4097"])
def test_more_launches_than_wavefronts_of_work(built, monkeypatch, name):
    """the development build with DICEY_MAP_HEAD_CHUNK = 64: one launch per 64 ranks"""
    text = _text(name)
    monkeypatch.setenv("DICEY_MAP_HEAD_CHUNK", "64")
    ix = dicey_amd.FmIndex(built(name), _lib=conftest.exp_lib())
    try:
        for fo in P.STRANDS:
            for max_k in (24, 100):
                _same(ix.min_unique(max_k=max_k, forward_only=fo), _once(("mu", name, max_k, fo), lambda: U.by_values(text, max_k, fo)),
                      (name, max_k, fo))
            for k in (12, 20):
                fwd, rev = _track(name, k, 1)
                st = {}
                _same(ix.mappability(k=k, mismatches=1, forward_only=fo, stats=st), M._finish(fwd, rev, fo, 0), (name, k, fo))
                assert st["launches"] >= 2, (name, k, st)
    finally:
        ix.close()


# ---- the binary -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many_short_fasta(tmp_path_factory):
    """the 3 000-record FASTA with its empty records (a header line alone), indexed by `dicey index`, and two query files"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("mapshapes_cli")
    g = dict(P.S.all_shapes()["many_short"])
    fa = d / "contigs.fa.gz"
    with gzip.open(fa, "wt", compresslevel=1) as f:
        for i, (n, s) in enumerate(zip(g["names"], g["seqs"])):
            f.write(">%s%s\n" % (n, " len=%d" % len(s) if i % 3 == 0 else ""))
            for a in range(0, len(s), 60):
                f.write(s[a:a + 60] + "\n")
    r = subprocess.run([DICEY, "index", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g.update(fa=str(fa), dir=d)
    for kind in ("plain", "iupac"):   # the records of the cut, which the full text holds as well
        recs = [x for x in P.as_bytes(P.records("many_short_800", P.get("many_short_800"))[kind]) if x]
        path = d / ("recs_%s.fa" % kind)
        with open(path, "w") as f:
            for i, s in enumerate(recs):
                f.write(">r%d\n" % i)
                for a in range(0, len(s), 60):
                    f.write(s[a:a + 60].decode() + "\n")
        g[kind] = (str(path), recs, ["r%d" % i for i in range(len(recs))])
    return g


def test_binary_on_three_thousand_records(many_short_fasta):
    g = many_short_fasta
    text, names = g["text"], g["names"]
    base = [DICEY, "mappability", "-g", g["fa"]]

    def run(args):
        r = subprocess.run(base + args, capture_output=True)
        assert r.returncode == 0, (args, r.stderr[-1500:])
        return r.stdout

    fwd, rev = M.parts_ball(text, 20, 1)
    exp = M.bedgraph(M._finish(fwd, rev, False, 0), text, names)
    assert len(exp.splitlines()) >= 2000 and run(["-e", "1", "-k", "20"]) == exp
    exp = U.bedgraph(text, names, 24)
    assert len(exp.splitlines()) >= 2000 and run(["-u", "-k", "24"]) == exp
    path, recs, qnames = g["plain"]
    exp = Q.bedgraph(Q.values(text, recs, 20, 1), qnames)
    assert len(exp.splitlines()) >= 20 and run(["-q", path, "-k", "20", "-e", "1"]) == exp
    path, recs, qnames = g["iupac"]
    qbuf, _ = Q.buffer_of(recs)
    # at e = 0 no window is near two expansions and the anchor excludes nothing: the value is the plain count summed over the explicit
    # expansions of the k-mer (the shift-by-shift model takes 14 s against 400 kb)
    letters, deg = I.degeneracy(qbuf, 20)
    valid = letters & (deg <= 256)
    where = np.nonzero(valid)[0].tolist()
    xs = [[x.encode() for x in I.expansions(qbuf[p:p + 20].decode())] for p in where]
    flat = Q.ball_at(text, [x for per in xs for x in per], 20, 0)
    tot = np.zeros(len(qbuf), dtype=np.int64)
    tot[where] = np.add.reduceat(flat, np.cumsum([0] + [len(per) for per in xs[:-1]]))
    assert (deg[valid] > 1).sum() >= 100 and (tot[valid & (deg > 1)] > 0).sum() >= 50
    exp = Q.bedgraph(Q.split(I.finish(tot, np.zeros_like(tot), valid), recs), qnames)
    assert len(exp.splitlines()) >= 10 and run(["-q", path, "-I", "-k", "20", "-a", "5"]) == exp
