"""dg_mappability / FmIndex.mappability against a brute-force count over the text (tests/mappability_ref.py), which knows
nothing of the FM-index: every position, both strands and forward only, across the K-mer table order, repeat groups that
span many rank tiles, palindromes, short sequences, the open flags, a 64 Mb genome, max_count, the run form and its chunk edges."""
import ctypes as C
import random

import numpy as np
import pytest

import conftest
import dicey_amd
import mappability_ref as R
import oracle_lib as O
from conftest import genome_text, make_genome, revcomp

pytestmark = pytest.mark.gpu
KS = [10, 11, 15, 16, 17, 20, 31, 32, 64, 100, 150]


@pytest.fixture(scope="module")
def small_k16(small_genome, monkeypatch_module):
    """the session genome opened with a K-mer table of order 16 (DICEY_KMER_K, a product tuning knob): k = 10..15 lie below the
    table's order, 16 at it, 17.. above"""
    monkeypatch_module.setenv("DICEY_KMER_K", "16")
    ix = dicey_amd.FmIndex(small_genome["fm9"])
    monkeypatch_module.delenv("DICEY_KMER_K")
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.mark.parametrize("k", KS)
def test_small_genome_every_position(small_genome, small_k16, k):
    text = small_genome["text"]
    for fo in (False, True):
        got = small_k16.mappability(k=k, forward_only=fo)
        exp = R.values(text, k, forward_only=fo)
        assert got.dtype == np.uint32 and len(got) == len(text)
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, (k, fo, bad[:10], got[bad[:10]], exp[bad[:10]])
        assert (got[R.valid_positions(text, k)] >= 1).all()


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    rng = random.Random(7)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    seg = rnd(2000)
    # sequence 1: a 2 kb segment 600 times and its reverse complement 400 times, random spacers between some copies
    parts = []
    for i in range(1000):
        parts.append(seg if i % 5 < 3 else revcomp(seg))
        if i % 7 == 0:
            parts.append(rnd(rng.randrange(1, 40)))
    s1 = "".join(parts)
    # sequence 2: random with planted even-length reverse-complement palindromes (20-mers and 32-mers), an N run, a 20 kb poly-A
    pal20 = [(lambda x: x + revcomp(x))(rnd(10)) for _ in range(5)]
    pal32 = [(lambda x: x + revcomp(x))(rnd(16)) for _ in range(3)]
    s2 = []
    for j in range(60):
        s2.append(rnd(rng.randrange(50, 400)))
        s2.append(pal20[j % 5] if j % 2 else pal32[j % 3])
    s2.append("N" * 37 + rnd(300) + "A" * 20000 + rnd(500))
    s2 = "".join(s2)
    seqs = [s1, s2, "ACGTAC", rnd(9), rnd(19), "AAAAAAAAAAA", rnd(33)]  # and sequences shorter than k
    text = genome_text(seqs)
    path = str(tmp_path_factory.mktemp("map") / "crafted.fm9")
    dicey_amd.build_index(text, path)
    return {"seqs": seqs, "text": text, "fm9": path, "pal20": pal20, "pal32": pal32}


@pytest.mark.parametrize("k", [10, 16, 20, 32, 64])
def test_crafted_genome(crafted, k):
    text = crafted["text"]
    with dicey_amd.FmIndex(crafted["fm9"]) as ix:
        for fo in (False, True):
            got = ix.mappability(k=k, forward_only=fo)
            exp = R.values(text, k, forward_only=fo)
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, (k, fo, bad[:10], got[bad[:10]], exp[bad[:10]])
        both = ix.mappability(k=k)
        fwd = ix.mappability(k=k, forward_only=True)
    if k in (20, 32):  # a palindrome of length k: both-strand value = 2 x its forward count
        for pal in crafted["pal%d" % k]:
            p = text.find(pal.encode())
            assert p >= 0 and both[p] == 2 * fwd[p] and fwd[p] >= 1, (pal, both[p], fwd[p])
    # the repeat groups are large: copies of the segment on both strands
    assert both[100] >= 1000
    polya = text.find(b"A" * 20000)
    assert fwd[polya] >= 20000 - k + 1


def test_k_longer_than_every_sequence(tmp_path):
    rng = random.Random(3)
    seqs = ["".join(rng.choice("ACGT") for _ in range(m)) for m in (5, 200, 999, 640)]
    text = genome_text(seqs)
    path = str(tmp_path / "short.fm9")
    dicey_amd.build_index(text, path)
    with dicey_amd.FmIndex(path) as ix:
        got = ix.mappability(k=1000)
        assert len(got) == len(text) and not got.any()
        s, ln, v = ix.mappability_runs(k=1000)
        assert len(s) == 0
        assert (ix.mappability(k=999) == R.values(text, 999)).all()


def test_open_flags_give_identical_arrays(small_genome):
    text = small_genome["text"]
    for k in (10, 20, 100):
        exp = R.values(text, k)
        for kw in ({}, {"compact": True, "pre5": False}, {"kmer_table": False}, {"big_table": True}):
            with dicey_amd.FmIndex(small_genome["fm9"], **kw) as ix:
                got = ix.mappability(k=k)
            assert (got == exp).all(), (k, kw)


def test_argument_checks(small_genome):
    L = dicey_amd._capi.load()
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        for k, code in ((9, -7), (1001, -7)):
            with pytest.raises(dicey_amd.DgError) as e:
                ix.mappability(k=k)
            assert e.value.code == code
        prm = dicey_amd._capi.MapParams(20, 0, 0, 1)
        m = C.c_void_p()
        assert L.dg_mappability(ix.handle, C.byref(prm), C.byref(m)) == -1 and not m.value
        # ranges outside the text are refused
        prm = dicey_amd._capi.MapParams(20, 0, 0, 0)
        assert L.dg_mappability(ix.handle, C.byref(prm), C.byref(m)) == 0
        try:
            n1 = len(small_genome["text"])
            buf = (C.c_uint32 * 4)()
            assert L.dg_map_values(m, n1 - 2, n1 + 2, buf) == -1
            assert L.dg_map_values(m, n1 - 4, n1, buf) == 0
            assert L.dg_map_device_values(m)
        finally:
            L.dg_map_free(m)


def test_max_count_and_runs(small_genome):
    text = small_genome["text"]
    n1 = len(text)
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        two = ix.mappability(k=12, max_count=2)
        exp = R.values(text, 12, max_count=2)
        assert (two == exp).all() and two.max() == 2 and set(np.unique(two)) == {0, 1, 2}
        vals = ix.mappability(k=12)
        assert (vals == R.values(text, 12)).all()
        # ranges that start and end inside runs
        s0, l0, _ = R.runs(vals, 0, n1)
        long_runs = np.nonzero(l0 >= 5)[0]
        assert len(long_runs) >= 4
        a = int(s0[long_runs[1]] + 2)
        b = int(s0[long_runs[-2]] + 3)
        for lo, hi in ((0, n1), (a, b), (a, a + 1), (a, a), (n1 - 7, n1)):
            got = ix.mappability_runs(k=12, lo=lo, hi=hi)
            ref = R.runs(vals, lo, hi)
            for x, y in zip(got, ref):
                assert (x == y).all(), (lo, hi)
        got = ix.mappability_runs(k=12, max_count=2)
        ref = R.runs(exp, 0, n1)
        for x, y in zip(got, ref):
            assert (x == y).all()


def test_run_chunks_on_the_development_build(small_genome, monkeypatch):
    """dg_map_runs goes through its range in chunks of positions; the development build takes the chunk size from
    DICEY_MAP_CHUNK: at 997 positions the 90 kb genome is ~90 chunks, and runs cross their edges"""
    text = small_genome["text"]
    n1 = len(text)
    vals = R.values(text, 10)
    chunk = 997
    monkeypatch.setenv("DICEY_MAP_CHUNK", str(chunk))
    ix = dicey_amd.FmIndex(small_genome["fm9"], _lib=conftest.exp_lib())
    try:
        for lo, hi in ((0, n1), (5, n1 - 3), (chunk - 1, 3 * chunk + 1)):
            s, ln, v = ix.mappability_runs(k=10, lo=lo, hi=hi)
            ref = R.runs(vals, lo, hi)
            for x, y in zip((s, ln, v), ref):
                assert (x == y).all(), (lo, hi)
            assert (hi - lo) // chunk >= 2
            # some run straddles a chunk edge (a chunk starts at lo + j * chunk)
            edges = np.arange(lo + chunk, hi, chunk)
            st = s.astype(np.int64)
            en = st + ln.astype(np.int64)
            assert any(((st < e) & (en > e)).any() for e in edges), (lo, hi)
        assert (ix.mappability(k=10) == vals).all()
    finally:
        ix.close()


def test_large_generated_genome(tmp_path):
    """~64 Mb, built on the device: exact at k = 24 and 32; at k = 100 on 2 000 seeded positions against FmIndex.count"""
    rng = np.random.default_rng(11)
    seqs = []
    for length in (30_000_000, 20_000_000, 14_000_000):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)].copy()
        # copied segments on both strands, N runs, homopolymers
        for _ in range(400):
            a, m, d = int(rng.integers(0, length - 5000)), int(rng.integers(50, 3000)), int(rng.integers(0, length - 5000))
            piece = s[a:a + m]
            if rng.random() < 0.5:
                piece = np.frombuffer(revcomp(piece.tobytes().decode()).encode(), dtype=np.uint8)
            s[d:d + m] = piece
        for _ in range(50):
            a = int(rng.integers(0, length - 2000))
            s[a:a + int(rng.integers(1, 1500))] = ord("N")
        for _ in range(50):
            a = int(rng.integers(0, length - 500))
            s[a:a + int(rng.integers(10, 400))] = ord("ACGT"[int(rng.integers(0, 4))])
        seqs.append(s.tobytes())
    text = b"\n".join(seqs) + b"\n"
    path = str(tmp_path / "big.fm9")
    dicey_amd.build_index(text, path)
    with dicey_amd.FmIndex(path, compact=True, pre5=False) as ix:
        for k in (24, 32):
            got = ix.mappability(k=k)
            exp = R.values(text, k)
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, (k, bad[:10], got[bad[:10]], exp[bad[:10]])
        got = ix.mappability(k=100)
        valid = R.valid_positions(text, 100)
        prs = np.random.default_rng(5)
        ps = np.sort(prs.choice(np.nonzero(valid)[0], 1500, replace=False)).tolist()
        ps += prs.choice(np.nonzero(~valid)[0], 500, replace=False).tolist()
        ws = [text[p:p + 100] for p in ps]
        pats = ws + [revcomp(w.decode()).encode() for w in ws]
        cnt = ix.count(pats)
        for j, p in enumerate(ps):
            exp = (cnt[j] + cnt[j + len(ps)]) if valid[p] else 0
            assert got[p] == exp, (p, got[p], exp)


def test_refused_while_a_hunt_batch_is_in_flight(small_genome):
    g = small_genome
    rng = random.Random(9)
    t = g["text"].decode()
    qs = []
    while len(qs) < 300:
        p = rng.randrange(len(t) - 20)
        if "\n" not in t[p:p + 20]:
            qs.append(t[p:p + 20])
    with dicey_amd.FmIndex(g["fm9"]) as ix:
        tk = ix.hunt_submit(qs, g["seqlen"], distance=1)
        try:
            with pytest.raises(dicey_amd.DgError) as e:
                ix.mappability(k=20)
            assert e.value.code == -1 and "in flight" in str(e.value)
        finally:
            ix.hunt_wait(tk)
        assert (ix.mappability(k=20) == R.values(g["text"], 20)).all()
        got = ix.hunt(qs, g["seqlen"], distance=1)
    _, hits = O.Index(g["fm9"]).hunt(g["seqlen"], g["names"], qs, distance=1, want_hits=True)
    per = {}
    for h in hits:
        per.setdefault(h[0], []).append(h[1:])
    for qi, qr in enumerate(got.queries):
        a = [(h.score, h.chr, h.start, h.strand, h.refalign, h.queryalign) for h in qr.hits]
        assert a == per.get(qi, []), qi
