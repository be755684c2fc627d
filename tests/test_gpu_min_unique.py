"""dg_min_unique / FmIndex.min_unique against the definition read aloud (tests/min_unique_ref.py by_values: the first k at which the
brute-force mappability is 1), which knows nothing of the FM-index: every position, both strands and forward only, across the K-mer
table order and the open flags, on a crafted genome of inverted and tandem copies, palindromes and run ends; the identity with
FmIndex.mappability; launch chunks; a generated 4 Mb genome held to FmIndex.count; the run form and the argument checks."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import conftest
import dicey_amd
import mappability_ref as R
import min_unique_ref as U
from conftest import genome_text, revcomp

pytestmark = pytest.mark.gpu
MAX_KS = (10, 16, 17, 40, 64)


def _same(got, exp, what):
    assert got.dtype == np.uint32 and len(got) == len(exp), what
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])


@pytest.mark.parametrize("how", ["as-is", "K16", "no-table", "compact-no-pre5"])
def test_session_genome_every_position(small_genome, how):
    """max_k below, at and above the K-mer table's order, with and without a table"""
    text = small_genome["text"]
    # the reference alone first: at max_k = 64 no pass is tested on an empty set (tests/test_min_unique_host.py has the exact figures)
    c = U.coverage(text, 64)
    assert c["zeros"] >= 1000 and c["raised"] >= 10000 and c["kept_zero"] >= 20 and c["smallest"] < 10, c
    mp = pytest.MonkeyPatch()
    try:
        if how == "K16":
            mp.setenv("DICEY_KMER_K", "16")
        kw = {"no-table": {"kmer_table": False}, "compact-no-pre5": {"compact": True, "pre5": False}}.get(how, {})
        ix = dicey_amd.FmIndex(small_genome["fm9"], **kw)
    finally:
        mp.undo()
    with ix:
        for max_k in MAX_KS:
            for fo in (False, True):
                _same(ix.min_unique(max_k=max_k, forward_only=fo), U.by_values(text, max_k, fo), (how, max_k, fo))


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    rng = random.Random(17)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    inv, tri = rnd(2000), rnd(2000)
    pal20 = [(lambda x: x + revcomp(x))(rnd(10)) for _ in range(3)]
    pal32 = [(lambda x: x + revcomp(x))(rnd(16)) for _ in range(3)]
    # sequence 1: `inv` once forward and once reverse-complemented.  The forward copy is followed by A and the other copy preceded by
    # A (read on the other strand: T), so the two strands part exactly at the copy's end.
    s1 = rnd(300) + inv + "A" + rnd(299) + "A" + revcomp(inv) + rnd(300)
    # sequence 2: `tri` three times on one strand, followed by A, C and G
    s2 = rnd(200) + tri + "A" + rnd(150) + tri + "C" + rnd(150) + tri + "G" + rnd(200)
    # sequence 3: palindromes, a 2 kb poly-A, an N run, IUPAC letters
    s3 = "".join(rnd(rng.randrange(40, 120)) + p for p in pal20 + pal32) + rnd(100) + "A" * 2000 + rnd(100) + "N" * 57 + rnd(200) + "R" + rnd(60) + "Y" + rnd(5)
    # sequences shorter than 10, and a last one that ends in the middle of `inv`
    seqs = [s1, s2, s3, "ACGTAC", rnd(9), "AAAAAAAAA", rnd(3), rnd(250) + inv[500:1200]]
    text = genome_text(seqs)
    path = str(tmp_path_factory.mktemp("mu") / "crafted.fm9")
    dicey_amd.build_index(text, path)
    return {"text": text, "fm9": path, "inv": inv, "tri": tri, "pal20": pal20, "pal32": pal32}


def test_crafted_genome(crafted):
    text, max_k = crafted["text"], 100
    with dicey_amd.FmIndex(crafted["fm9"]) as ix:
        both = ix.min_unique(max_k=max_k)
        fwd = ix.min_unique(max_k=max_k, forward_only=True)
    _same(both, U.by_values(text, max_k), "both")
    _same(fwd, U.by_values(text, max_k, True), "forward")
    # the inverted copy: a k-mer inside the forward copy has its reverse complement in the other one, so the first unique length is
    # the one that leaves the copy: the distance to the copy's end plus one
    a = text.find(crafted["inv"].encode())
    d = a + 2000 - np.arange(a, a + 2000)  # distance to the end
    v = both[a:a + 2000].astype(np.int64)
    far, near = d + 1 > max_k, (d + 1 <= max_k) & (d + 1 >= 20)
    assert far.sum() > 1800 and not v[far].any()
    assert near.sum() > 70 and (v[near] == d[near] + 1).all()
    # (inv[500:1200] is also the tail of the last sequence: forward only, positions outside that stretch stay small)
    out = np.r_[0:480, 1210:1980]
    assert (fwd[a + out] > 0).all() and (fwd[a + out] < 20).all()
    # three copies on one strand: repeated until the k-mer leaves the copy
    t0 = text.find(crafted["tri"].encode())
    t1 = text.find(crafted["tri"].encode(), t0 + 1)
    t2 = text.find(crafted["tri"].encode(), t1 + 1)
    assert t0 >= 0 and t1 > t0 and t2 > t1
    for t in (t0, t1, t2):
        for arr in (both, fwd):
            v = arr[t:t + 2000].astype(np.int64)
            d = 2000 - np.arange(2000)
            assert not v[d >= max_k].any()
            near = (d + 1 <= max_k) & (d + 1 >= 20)
            assert (v[near] == d[near] + 1).all()
    # a reverse-complement palindrome has every prefix's reverse complement inside itself and counts twice at its own length
    for m in (20, 32):
        for pal in crafted["pal%d" % m]:
            p = text.find(pal.encode())
            assert p >= 0 and both[p] != m and (both[p] == 0 or both[p] > m), (pal, both[p])
            assert 0 < fwd[p] <= m
    # poly-A: nothing is unique until the run's end comes within max_k
    pa = text.find(b"A" * 2000)
    assert not both[pa:pa + 2000 - max_k].any() and not fwd[pa:pa + 2000 - max_k].any()
    # N run, IUPAC letters, separators, short sequences
    acgt = U.run_lengths(text) > 0
    assert not both[~acgt].any() and (~acgt).sum() > 60
    ps = text.find(b"\nACGTAC\n") + 1
    assert (both[ps:ps + 6] <= 6).all()
    # the last sequence ends in the middle of a repeat: its tail is repeated up to the sequence end
    assert not both[len(text) - 1 - 600:len(text) - 1].any()


@pytest.mark.parametrize("forward_only", [False, True])
def test_identity_with_mappability(small_genome, forward_only):
    """(mul != 0 and mul <= k)  <=>  mappability(k) == 1, on the positions whose k-mer is valid"""
    text = small_genome["text"]
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        mul = ix.min_unique(max_k=64, forward_only=forward_only)
        for k in (10, 20, 64):
            one = ix.mappability(k=k, forward_only=forward_only) == 1
            ok = R.valid_positions(text, k)
            assert ok.sum() > 50000 and one[ok].sum() > 10000 and (~one[ok]).sum() > 500
            got = (mul != 0) & (mul <= k)
            bad = np.nonzero(got[ok] != one[ok])[0]
            assert len(bad) == 0, (k, len(bad), np.nonzero(ok)[0][bad[:10]])


def test_launch_chunks_on_the_development_build(small_genome, monkeypatch, capfd):
    """ranks go through the two passes in chunks, one launch each; the development build takes the chunk from DICEY_MAP_HEAD_CHUNK"""
    text = small_genome["text"]
    monkeypatch.setenv("DICEY_MAP_HEAD_CHUNK", "4099")
    monkeypatch.setenv("DICEY_TIMING", "1")
    ix = dicey_amd.FmIndex(small_genome["fm9"], _lib=conftest.exp_lib())
    try:
        capfd.readouterr()
        got = ix.min_unique(max_k=64)
        err = capfd.readouterr().err
        launches = [int(x) for x in re.findall(r"min unique max_k=64: (\d+) launches", err)]
        assert launches == [-(-(len(text) + 1) // 4099)] and launches[0] > 20, err
        _same(got, U.by_values(text, 64), "chunks")
        _same(ix.min_unique(max_k=17, forward_only=True), U.by_values(text, 17, True), "chunks, forward")
    finally:
        ix.close()


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """4 Mb in two sequences with 200 segments copied on either strand, N runs and homopolymers"""
    rng = np.random.default_rng(23)
    seqs, copies, off = [], [], 0
    for length in (2_500_000, 1_500_000):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)].copy()
        for _ in range(100):
            a, m, d = int(rng.integers(0, length - 5000)), int(rng.integers(50, 3000)), int(rng.integers(0, length - 5000))
            piece = s[a:a + m].copy()
            if rng.random() < 0.5:
                piece = np.frombuffer(revcomp(piece.tobytes().decode()).encode(), dtype=np.uint8)
            s[d:d + m] = piece
            copies.append((off + d, m))
        for _ in range(20):
            a = int(rng.integers(0, length - 2000))
            s[a:a + int(rng.integers(1, 1500))] = ord("N")
        for _ in range(20):
            a = int(rng.integers(0, length - 500))
            s[a:a + int(rng.integers(10, 400))] = ord("ACGT"[int(rng.integers(0, 4))])
        seqs.append(s.tobytes())
        off += length + 1
    text = b"\n".join(seqs) + b"\n"
    path = str(tmp_path_factory.mktemp("mu4") / "gen.fm9")
    dicey_amd.build_index(text, path)
    return {"text": text, "fm9": path, "copies": copies}


def test_generated_genome(generated):
    text, max_k = generated["text"], 32
    run = U.run_lengths(text)
    with dicey_amd.FmIndex(generated["fm9"], compact=True, pre5=False) as ix:
        st = {}
        mul = ix.min_unique(max_k=max_k, stats=st)
        assert st["k"] == max_k and st["n"] == len(text) + 1 and st["rev_steps"] > 0
        for k in (16, 24, 32):
            one = ix.mappability(k=k) == 1
            ok = R.valid_positions(text, k)
            got = (mul != 0) & (mul <= k)
            bad = np.nonzero(got[ok] != one[ok])[0]
            assert len(bad) == 0, (k, len(bad), np.nonzero(ok)[0][bad[:10]])
            assert (~one[ok]).sum() > 10000
        # exact minimality through FmIndex.count: 1 at k = mul, more at k = mul - 1, more at the limit where mul == 0
        prs = np.random.default_rng(5)
        inside = np.concatenate([np.arange(d, d + m) for d, m in generated["copies"]])
        ps = np.concatenate([prs.choice(inside, 600, replace=False), prs.choice(len(text), 1400, replace=False)])
        ps = ps[run[ps] > 0]
        assert len(ps) > 1900 and (mul[ps] == 0).sum() > 200 and (mul[ps] > 0).sum() > 1000
        pats, what = [], []
        for p in ps.tolist():
            m, limit = int(mul[p]), min(int(run[p]), max_k)
            assert m <= limit
            for k, expect in ((m, "one"), (m - 1, "more")) if m else ((limit, "more"),):
                if k >= 1:
                    w = text[p:p + k]
                    pats += [w, revcomp(w.decode()).encode()]
                    what.append((p, k, expect))
        cnt = ix.count(pats)
        for j, (p, k, expect) in enumerate(what):
            tot = cnt[2 * j] + cnt[2 * j + 1]
            assert (tot == 1) if expect == "one" else (tot > 1), (p, k, expect, tot, int(mul[p]))
    assert not mul[run == 0].any()


def test_runs_stats_and_argument_checks(small_genome):
    text = small_genome["text"]
    n1 = len(text)
    L = dicey_amd._capi.load()
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        vals = U.by_values(text, 40)
        s0, l0, _ = R.runs(vals, 0, n1)
        long_runs = np.nonzero(l0 >= 5)[0]
        assert len(long_runs) >= 4
        a = int(s0[long_runs[1]] + 2)
        b = int(s0[long_runs[-2]] + 3)
        for lo, hi in ((0, n1), (a, b), (a, a + 1), (a, a), (n1 - 7, n1)):  # ranges that start and end inside runs
            got = ix.min_unique_runs(max_k=40, lo=lo, hi=hi)
            for x, y in zip(got, R.runs(vals, lo, hi)):
                assert x.dtype == y.dtype and (x == y).all(), (lo, hi)
        got = ix.min_unique_runs(max_k=12, forward_only=True)
        for x, y in zip(got, R.runs(U.by_values(text, 12, True), 0, n1)):
            assert (x == y).all()
        st, stf = {}, {}
        ix.min_unique(max_k=40, stats=st)
        ix.min_unique(max_k=40, forward_only=True, stats=stf)
        assert st["k"] == 40 and st["n"] == n1 + 1 and st["ms_scatter"] == 0 and st["ms_valid"] == 0
        assert st["rev_steps"] > 0 and stf["rev_steps"] == 0
        assert st["ms_total"] == pytest.approx(st["ms_forward"] + st["ms_reverse"], rel=1e-9) and st["transient_bytes"] >= 2 * n1
        for max_k in (9, 1001):
            with pytest.raises(dicey_amd.DgError) as e:
                ix.min_unique(max_k=max_k)
            assert e.value.code == -7
            with pytest.raises(dicey_amd.DgError) as e:
                ix.min_unique_runs(max_k=max_k)
            assert e.value.code == -7
        # the result is an ordinary map: the mismatch counters stay zero, the device pointer is there
        prm = dicey_amd._capi.MinUniqueParams(40, 0, 0, 0)
        m = C.c_void_p()
        assert L.dg_min_unique(ix.handle, C.byref(prm), C.byref(m)) == 0
        try:
            mm = dicey_amd._capi.MapMmStats()
            assert L.dg_map_mm_stats(m, C.byref(mm)) == 0
            assert not any(getattr(mm, f) for f, _ in dicey_amd._capi.MapMmStats._fields_)
            assert L.dg_map_device_values(m)
            buf = (C.c_uint32 * 4)()
            assert L.dg_map_values(m, n1 - 2, n1 + 2, buf) == -1
            assert L.dg_map_values(m, n1 - 4, n1, buf) == 0
        finally:
            L.dg_map_free(m)
        prm = dicey_amd._capi.MinUniqueParams(40, 0, 1, 0)
        assert L.dg_min_unique(ix.handle, C.byref(prm), C.byref(m)) == -1 and not m.value


def test_refused_while_a_hunt_batch_is_in_flight(small_genome):
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
                ix.min_unique(max_k=20)
            assert e.value.code == -1 and "in flight" in str(e.value) and "dg_min_unique" in str(e.value)
        finally:
            waited = flat(ix.hunt_wait(tk))
        assert waited == before
        _same(ix.min_unique(max_k=20), U.by_values(g["text"], 20), "after the batch")
        assert flat(ix.hunt(qs, g["seqlen"], distance=1)) == before
