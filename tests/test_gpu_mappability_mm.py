"""dg_mappability_mm / FmIndex.mappability(mismatches=e) / `dicey mappability -e` against the brute-force (k,e)-mappability of
tests/mappability_mm_ref.py, which knows nothing of the FM-index: every position of the session genome across the K-mer table order,
a crafted genome whose near-copies are shown (on the reference alone) to exercise the feature, the max_count / run / e = 0 properties,
the development-build switches, the open flags, a generated genome of a few Mb and the binary."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import conftest
import dicey_amd
import mappability_mm_ref as M
import mappability_ref as R
from conftest import genome_text, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def small_k16(small_genome, monkeypatch_module):
    """the session genome opened with a K-mer table of order 16 (DICEY_KMER_K, a product tuning knob): k = 12 lies below the table's
    order, 16 at it, 20 above"""
    monkeypatch_module.setenv("DICEY_KMER_K", "16")
    ix = dicey_amd.FmIndex(small_genome["fm9"])
    monkeypatch_module.delenv("DICEY_KMER_K")
    yield ix
    ix.close()


def _same(got, exp, what):
    assert got.dtype == np.uint32 and len(got) == len(exp)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:10]], exp[bad[:10]])


# ---- session genome --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [12, 16, 20])
def test_small_genome_every_position(small_genome, small_k16, k):
    text = small_genome["text"]
    prev = R.values(text, k).astype(np.uint64)
    for e in (1, 2):
        fwd, rev = M.parts_ball(text, k, e)
        for fo in (False, True):
            _same(small_k16.mappability(k=k, forward_only=fo, mismatches=e), M._finish(fwd, rev, fo, 0), (k, e, fo))
        assert ((fwd + rev) >= prev).all()
        prev = fwd + rev


@pytest.mark.parametrize("k", [64, 100])
def test_long_kmers_on_a_cut_of_the_small_genome(small_genome, k, tmp_path):
    """k above 32 against the diagonal reference: a 12 kb cut of the session text (with its N runs and IUPAC letters) and a planted
    one-substitution copy on each strand"""
    t = small_genome["text"][:12000].replace(b"\n", b"N").decode()
    a = next(a for a in range(1000, 6000) if set(t[a:a + 400]) <= set("ACGT"))
    src = t[a:a + 400]
    twin = src[:150] + ("A" if src[150] != "A" else "C") + src[151:]
    seqs = [t[:7000] + twin + t[7000:], t[8000:9000] + revcomp(twin) + "ACGTTGCAAC"]
    text = genome_text(seqs)
    path = str(tmp_path / "cut.fm9")
    dicey_amd.build_index(text, path)
    parts = M.parts_diagonal(text, k, (0, 1))
    assert ((parts[1][0] + parts[1][1]) > (parts[0][0] + parts[0][1])).sum() >= 3 * k
    with dicey_amd.FmIndex(path) as ix:
        for fo in (False, True):
            _same(ix.mappability(k=k, forward_only=fo, mismatches=1), M._finish(*parts[1], fo, 0), (k, fo))
        _same(ix.mappability(k=k, mismatches=0), M._finish(*parts[0], False, 0), (k, "e0"))


# ---- crafted genome --------------------------------------------------------------------------------------------------------------

def _subst(s, positions):
    s = list(s)
    for i in positions:
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + i % 3) % 4]
    return "".join(s)


def crafted_texts():
    rng = random.Random(17)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    base = rnd(4000)
    long1, long2 = rnd(1200), rnd(1200)
    A, B, Cc, D, E = base[100:500], base[700:1100], base[1300:1700], base[2000:2400], base[2600:3000]
    a1 = _subst(A, [200])                 # exactly one substitution
    b2 = _subst(B, [200, 207])            # exactly two, seven apart
    c3 = _subst(Cc, [200, 204, 208])      # exactly three, inside nine characters
    dn = D[:200] + "N" + D[201:]          # a copy with one base replaced by N
    e1 = _subst(E, [150])[:170]           # a near-copy that runs into its sequence's end
    l1 = revcomp(_subst(long1, range(15, 1200, 30)))  # reverse strand only, one substitution per window of up to 30
    l2 = _subst(long2, range(5, 1200, 11))            # two or three substitutions per 24-mer
    x12, x8 = rnd(12), rnd(8)
    pal24 = _subst(x12 + revcomp(x12), [3])  # a 24-mer two substitutions away from its own reverse complement
    pal16 = _subst(x8 + revcomp(x8), [2])

    def s1(c3_copy, c3_rc, n_char):
        parts = [base, rnd(50), a1, rnd(30), revcomp(a1), rnd(30), b2, rnd(30), revcomp(b2), rnd(30), c3_copy, rnd(30), c3_rc, rnd(30),
                 dn.replace("N", n_char), rnd(30), long1, rnd(20), long2, rnd(40), l1, rnd(20), l2]
        for j in range(6):
            parts += [rnd(40), pal24 if j % 2 else pal16]
        return "".join(parts)

    st = rng.getstate()
    seq1 = s1(c3, revcomp(c3), "N")
    rng.setstate(st)
    seq1_no3 = s1("N" * len(c3), "N" * len(c3), "N")   # the same text without the three-substitution copies
    rng.setstate(st)
    seq1_noN = s1(c3, revcomp(c3), D[200])             # the same text with the N put back
    seq2 = rnd(300) + "A" * 10000 + "C" + "A" * 9999 + rnd(300)
    seq3 = rnd(200) + e1
    rest = [seq2, seq3, "ACGTAC", rnd(9), rnd(15), "AAAAAAAAAAA"]  # and sequences shorter than k
    text = genome_text([seq1] + rest)
    assert len(text) == len(genome_text([seq1_no3] + rest)) == len(genome_text([seq1_noN] + rest))
    return {"text": text, "text_no3": genome_text([seq1_no3] + rest), "text_noN": genome_text([seq1_noN] + rest),
            "c_src": 1300, "d_src": 2000, "pal24": pal24, "polya": len(seq1) + 1 + 300}


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    c = crafted_texts()
    c["fm9"] = str(tmp_path_factory.mktemp("mapmm") / "crafted.fm9")
    dicey_amd.build_index(c["text"], c["fm9"])
    return c


@pytest.fixture(scope="module")
def crafted_ref(crafted):
    """the reference's fwd / rev parts at k = 24, per e"""
    parts = {0: M.parts_ball(crafted["text"], 24, 0)}
    parts[1] = M.parts_ball(crafted["text"], 24, 1)
    parts[2] = M.parts_ball(crafted["text"], 24, 2)
    return parts


def test_crafted_inputs_exercise_the_feature(crafted, crafted_ref):
    """conditions on the INPUTS, shown on the reference alone"""
    k, text = 24, crafted["text"]
    val = {e: crafted_ref[e][0] + crafted_ref[e][1] for e in (0, 1, 2)}
    for e in (1, 2):
        assert (val[e] > val[e - 1]).sum() >= 1000, e
    for e in (1, 2):  # an excess that comes from the reverse strand only
        only_rev = (crafted_ref[e][0] == crafted_ref[0][0]) & (crafted_ref[e][1] > crafted_ref[0][1])
        assert only_rev.sum() >= 50, e
    # would-be twins that hold an N: with the N put back the source windows over it have one more occurrence
    with_n = M.parts_ball(crafted["text_noN"], k, 1)
    valid = R.valid_positions(text, k)
    lost = valid & ((with_n[0] + with_n[1]) > val[1])
    assert lost.sum() >= 20
    src = np.arange(crafted["d_src"] + 200 - k + 1, crafted["d_src"] + 201)
    assert lost[src].all() and (val[2][src] == 1).all()
    # the copies with three substitutions add nothing at e = 2: the windows over all three see the same count without the copies
    ps = list(range(crafted["c_src"] + 208 - k + 1, crafted["c_src"] + 201))
    assert len(ps) == k - 8
    assert (M.direct(text, k, 2, ps) == M.direct(crafted["text_no3"], k, 2, ps)).all()
    assert (M.direct(text, k, 2, ps) == val[2][ps]).all()
    # ... while windows over two of the three do gain
    assert val[2][crafted["c_src"] + 204 - k + 1] > val[1][crafted["c_src"] + 204 - k + 1]
    # the near-palindrome meets its own reverse strand at e = 2 only
    p = text.find(crafted["pal24"].encode())
    assert p >= 0 and crafted_ref[2][1][p] > crafted_ref[1][1][p] == 0
    # poly-A: the windows with the interior C are one substitution away
    pa = crafted["polya"]
    assert crafted_ref[0][0][pa] >= 10000 - k + 1 + 9999 - k + 1 and crafted_ref[1][0][pa] >= crafted_ref[0][0][pa] + k


@pytest.mark.parametrize("e", [1, 2])
def test_crafted_genome(crafted, crafted_ref, e):
    fwd, rev = crafted_ref[e]
    with dicey_amd.FmIndex(crafted["fm9"]) as ix:
        for fo in (False, True):
            _same(ix.mappability(k=24, forward_only=fo, mismatches=e), M._finish(fwd, rev, fo, 0), (e, fo))
        _same(ix.mappability(k=16, mismatches=e), M.values(crafted["text"], 16, e), (16, e))
    with dicey_amd.FmIndex(crafted["fm9"], kmer_table=False) as ix:
        _same(ix.mappability(k=24, mismatches=e), M._finish(fwd, rev, False, 0), (e, "no table"))


# ---- properties ------------------------------------------------------------------------------------------------------------------

def test_properties(small_genome):
    text = small_genome["text"]
    n1 = len(text)
    k = 14
    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        v0 = ix.mappability(k=k)
        st = {}
        v = {0: ix.mappability(k=k, mismatches=0), 1: ix.mappability(k=k, mismatches=1, stats=st), 2: ix.mappability(k=k, mismatches=2)}
        assert (v[0] == v0).all() and (v0 == R.values(text, k)).all()
        assert (v[0] <= v[1]).all() and (v[1] <= v[2]).all() and (v[2] > v[1]).any() and (v[1] > v[0]).any()
        _same(v[1], M.values(text, k, 1), "e1")
        assert st["heads"] > 0 and st["launches"] >= 1 and st["table_reads"] >= st["heads"] and st["early_exits"] == 0
        assert st["ms_search"] == st["ms_reverse"] and st["steps"] == st["rev_steps"]
        st0 = {}
        ix.mappability(k=k, stats=st0)
        assert "heads" not in st0
        for e in (1, 2):
            for cap in (2, 5):
                stc = {}
                got = ix.mappability(k=k, mismatches=e, max_count=cap, stats=stc)
                _same(got, np.minimum(v[e], cap).astype(np.uint32), (e, cap))
                assert stc["early_exits"] > 0
            _same(ix.mappability(k=k, mismatches=e, max_count=2, forward_only=True),
                  np.minimum(ix.mappability(k=k, mismatches=e, forward_only=True), 2).astype(np.uint32), (e, "fo cap"))
        for lo, hi in ((0, n1), (1234, 56789), (n1 - 7, n1)):
            got = ix.mappability_runs(k=k, lo=lo, hi=hi, mismatches=1)
            for x, y in zip(got, R.runs(v[1], lo, hi)):
                assert (x == y).all(), (lo, hi)
        got = ix.mappability_runs(k=k, max_count=2, mismatches=2)
        for x, y in zip(got, R.runs(np.minimum(v[2], 2), 0, n1)):
            assert (x == y).all()
        for bad in (3, 7):
            with pytest.raises(dicey_amd.DgError) as err:
                ix.mappability(k=k, mismatches=bad)
            assert err.value.code == -7


def test_switches_of_the_development_build(small_genome, monkeypatch):
    """DICEY_MAP_HEAD_CHUNK (ranks per launch) and DICEY_MAP_NARROW (W) change how the search runs, never what it returns"""
    text = small_genome["text"]
    k = 20
    exp = {e: M.values(text, k, e) for e in (1, 2)}
    ix = dicey_amd.FmIndex(small_genome["fm9"], _lib=conftest.exp_lib())
    try:
        seen = {}
        for name, env in (("default", {}), ("chunk", {"DICEY_MAP_HEAD_CHUNK": "1024"}), ("never", {"DICEY_MAP_NARROW": "0"}),
                          ("always", {"DICEY_MAP_NARROW": "1000000000"}), ("both", {"DICEY_MAP_HEAD_CHUNK": "777", "DICEY_MAP_NARROW": "2"})):
            for kk, vv in env.items():
                monkeypatch.setenv(kk, vv)
            for e in (1, 2):
                st = {}
                _same(ix.mappability(k=k, mismatches=e, stats=st), exp[e], (name, e))
                seen[name, e] = st
            _same(ix.mappability(k=k, mismatches=1, max_count=2), np.minimum(exp[1], 2).astype(np.uint32), (name, "cap"))
            for kk in env:
                monkeypatch.delenv(kk)
        for e in (1, 2):
            assert seen["default", e]["launches"] == 1
            assert seen["chunk", e]["launches"] >= 50
            assert seen["never", e]["verified_rows"] == 0 and seen["never", e]["steps"] > 0
            assert seen["always", e]["verified_rows"] > 0 and seen["always", e]["steps"] == 0
            assert seen["default", e]["verified_rows"] > 0 and seen["default", e]["steps"] > 0
            assert len({s["heads"] for (_, ee), s in seen.items() if ee == e}) == 1
    finally:
        ix.close()


def test_open_flags_give_identical_arrays(small_genome):
    text = small_genome["text"]
    exp = {e: M.values(text, 18, e) for e in (1, 2)}
    for kw in ({}, {"compact": True}, {"compact": True, "pre5": False}, {"kmer_table": False}):
        with dicey_amd.FmIndex(small_genome["fm9"], **kw) as ix:
            for e in (1, 2):
                _same(ix.mappability(k=18, mismatches=e), exp[e], (kw, e))


# ---- a genome too large for brute force ------------------------------------------------------------------------------------------

def test_generated_genome_of_a_few_mb(tmp_path):
    """~6 Mb, built on the device, opened as the binary opens it; k = 36, e = 1 on 500 seeded valid positions (and some invalid ones)
    against the sum of FmIndex.count over the explicit Hamming ball of w and of revcomp(w).  A SECOND-LINE check: count is an older,
    separately tested path of the same library, not an independent reference — the brute-force comparisons are the tests above."""
    rng = np.random.default_rng(23)
    seqs = []
    for length in (3_000_000, 2_000_000, 1_000_000):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)].copy()
        for _ in range(300):  # copied segments on both strands with a few substitutions, N runs, homopolymers
            a, m, d = int(rng.integers(0, length - 5000)), int(rng.integers(50, 3000)), int(rng.integers(0, length - 5000))
            piece = s[a:a + m].copy()
            if rng.random() < 0.5:
                piece = np.frombuffer(revcomp(piece.tobytes().decode()).encode(), dtype=np.uint8).copy()
            hits = rng.integers(0, m, max(1, m // 40))
            piece[hits] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(hits))]
            s[d:d + m] = piece
        for _ in range(30):
            a = int(rng.integers(0, length - 2000))
            s[a:a + int(rng.integers(1, 1500))] = ord("N")
        for _ in range(30):
            a = int(rng.integers(0, length - 500))
            s[a:a + int(rng.integers(10, 400))] = ord("ACGT"[int(rng.integers(0, 4))])
        seqs.append(s.tobytes())
    text = b"\n".join(seqs) + b"\n"
    path = str(tmp_path / "mid.fm9")
    dicey_amd.build_index(text, path)
    k = 36
    with dicey_amd.FmIndex(path, compact=True, pre5=False) as ix:
        st = {}
        got = ix.mappability(k=k, mismatches=1, stats=st)
        exact = ix.mappability(k=k)
        assert (got >= exact).all() and (got > exact).sum() > 10000
        valid = R.valid_positions(text, k)
        assert ((got > 0) == valid).all()
        prs = np.random.default_rng(5)
        grew = np.nonzero(got > exact)[0]
        ps = prs.choice(np.nonzero(valid)[0], 350, replace=False).tolist() + prs.choice(grew, 150, replace=False).tolist()
        bad_ps = prs.choice(np.nonzero(~valid)[0], 100, replace=False).tolist()
        pats = []
        for p in ps:
            w = text[p:p + k]
            for u in (w, revcomp(w.decode()).encode()):
                pats.append(u)
                for i in range(k):
                    for c in b"ACGT":
                        if c != u[i]:
                            pats.append(u[:i] + bytes([c]) + u[i + 1:])
        per = 2 * (1 + 3 * k)
        cnt = np.array(ix.count(pats), dtype=np.int64).reshape(len(ps), per).sum(axis=1)
        for j, p in enumerate(ps):
            assert got[p] == cnt[j], (p, got[p], cnt[j], exact[p])
        assert not got[bad_ps].any()
        assert st["launches"] >= 1 and st["heads"] > 5_000_000


# ---- the binary ------------------------------------------------------------------------------------------------------------------

def test_binary_with_one_mismatch(small_genome, tmp_path):
    g = small_genome
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    fa = tmp_path / "session.fa.gz"
    with gzip.open(fa, "wt") as f:
        for n, s in zip(g["names"], g["seqs"]):
            f.write(">" + n + "\n")
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    r = subprocess.run([DICEY, "index", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fwd, rev = M.parts_ball(g["text"], 20, 1)
    exp = M.bedgraph(M._finish(fwd, rev, False, 0), g["text"], g["names"])
    assert len(exp) > 1000 and exp != R.bedgraph(g["text"], g["names"], 20)
    r = subprocess.run([DICEY, "mappability", "-g", str(fa), "-e", "1", "-k", "20"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp
    out = tmp_path / "x.gz"
    r = subprocess.run([DICEY, "mappability", "-g", str(fa), "--mismatches", "1", "-k", "20", "-o", str(out)], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert gzip.decompress(out.read_bytes()) == exp
    r = subprocess.run([DICEY, "mappability", "-g", str(fa), "-e", "1", "-k", "20", "-f", "-c", "2"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == M.bedgraph(M._finish(fwd, rev, True, 2), g["text"], g["names"])
    r = subprocess.run([DICEY, "mappability", "-g", str(fa), "-e", "0", "-k", "20"], capture_output=True)
    assert r.returncode == 0 and r.stdout == R.bedgraph(g["text"], g["names"], 20)
