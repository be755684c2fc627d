"""dg_query_map / FmIndex.query_mappability against the brute-force references of tests/query_map_ref.py, which know nothing of the
FM-index: every record shape on the session genome across the K-mer table order (the inputs shown, on the reference alone, to exercise
the feature), the genome track's values for a cut, long k-mers, the edges of the text, the max_count / count / strand properties, the
open flags and development-build switches, the argument checks and a generated genome of a few Mb."""
import ctypes as C
import random

import numpy as np
import pytest

import conftest
import dicey_amd
import mappability_mm_ref as M
import mappability_ref as R
import query_map_ref as Q
from conftest import genome_text, revcomp
from dicey_amd import _capi

pytestmark = pytest.mark.gpu
INV = Q.INVALID
KS, ES = (12, 16, 20), (0, 1, 2)


def _same(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for i, (g, x) in enumerate(zip(got, exp)):
        assert g.dtype == np.uint32 and len(g) == len(x), (what, i)
        bad = np.nonzero(g != x)[0]
        assert len(bad) == 0, (what, i, len(bad), bad[:10], g[bad[:10]], x[bad[:10]])


def _clean(t, start, m):
    """the first position >= start from which m characters of t are all A/C/G/T"""
    return next(a for a in range(start, len(t) - m) if set(t[a:a + m]) <= set("ACGT"))


def _subst_every(s, every):
    s = list(s)
    for i in range(every // 2, len(s), every):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + i % 3) % 4]
    return "".join(s)


def _kmers12_by_value(text, want, rng):
    """12-mers whose value at e = 2 (both strands) is each of `want`: the counts of the text's 12-mers of both strands, spread over the
    Hamming ball of radius 2 into a table of all 4^12 codes"""
    pos = np.nonzero(R.valid_positions(text, 12))[0]
    fw, rc = Q._codes(text, pos, 12)
    keys, cnt = np.unique(np.concatenate([fw, rc]), return_counts=True)  # count(revcomp(w)) in T = the count of w among the revcomps
    tot = np.zeros(1 << 24, dtype=np.uint32)
    for m in M._masks(12, 2):
        tot[keys ^ m] += cnt.astype(np.uint32)  # keys ^ m are distinct: no index repeats
    out = {}
    for v in want:
        codes = rng.choice(np.nonzero(tot == v)[0], 60, replace=False)
        out[v] = ["".join("ACGT"[(int(c) >> (2 * (11 - j))) & 3] for j in range(12)) for c in codes]
    return out


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
    """the records of every shape and, computed once, the ball reference's parts per (k, e)"""
    text = small_genome["text"]
    t = text.decode()
    s1, s2, s3 = small_genome["seqs"]
    rng = random.Random(41)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    a = next(a for a in range(1000, 25000) if "N" in s1[a + 100:a + 2900] and set(s1[a:a + 40] + s1[a + 2960:a + 3000]) <= set("ACGT"))
    b, c = _clean(s2, 5000, 600), _clean(s3, 9000, 800)
    j0, j1 = _clean(s1, 20000, 60), _clean(s3, 2000, 60)
    x12, x16, x20, z = _clean(s2, 12000, 12), _clean(s2, 13000, 16), _clean(s2, 14000, 20), _clean(s3, 20000, 300)
    recs = [s1[a:a + 3000],                                  # first record, buffer offset 0: a cut with an N run
            revcomp(s2[b:b + 600]),                          # the other strand of a cut
            _subst_every(s3[c:c + 800], 13),                 # one substitution every 13 nt
            s1[j0:j0 + 60] + s3[j1:j1 + 60],                 # a two-exon junction
            rnd(500),
            s2[x12:x12 + 12], s2[x16:x16 + 16], s2[x20:x20 + 20],  # records of exactly k
            rnd(9), "",                                      # shorter than every k, empty
            s1[j0:j0 + 100].lower()]                         # lower case: invalid (bytes go through as given)
    # copies the genome itself repeats: stretches whose 20-mers occur twice or more, until the values >= 2 are there at every k
    v20 = R.values(text, 20)
    starts, lens, _ = R.runs((v20 >= 2).astype(np.uint32), 0, len(text))
    order = np.argsort(-lens.astype(np.int64))[:6]
    for i in order:
        recs.append(t[int(starts[i]):int(starts[i]) + int(lens[i]) + 19])
    # 12-mers with no genome 12-mer within two substitutions on either strand, and with exactly one
    planted = _kmers12_by_value(text, (0, 1), np.random.default_rng(3))
    recs += planted[0] + planted[1]
    recs.append(s3[z:z + 300])                               # last record: a cut whose final window is valid
    recs = [r.encode() for r in recs]
    qbuf, _ = Q.buffer_of(recs)
    parts = {(k, e): Q.parts_ball(text, qbuf, k, e) for k in KS for e in ES}
    return {"recs": recs, "parts": parts, "cut0": a, "cut_last": 2 * 30001 + z, "junction": 3}


def _exp(shapes, k, e, fo=False, cap=0):
    return Q.split(Q.finish(*shapes["parts"][k, e], fo, cap), shapes["recs"])


# ---- session genome --------------------------------------------------------------------------------------------------------------

def test_inputs_exercise_the_feature(shapes):
    """conditions on the INPUTS, shown on the reference alone"""
    recs = shapes["recs"]
    assert len(recs[0]) == 3000 and b"N" in recs[0] and len(recs[9]) == 0 and recs[10].islower()
    for k in KS:
        val = {}
        for e in ES:
            fwd, rev, valid = shapes["parts"][k, e]
            v = (fwd + rev)[valid]
            val[e] = v
            assert (v == 0).sum() >= 50 and (v == 1).sum() >= 50 and (v >= 2).sum() >= 50, (k, e, (v == 0).sum(), (v == 1).sum(), (v >= 2).sum())
            assert (rev[valid] > 0).sum() >= 50 and (fwd[valid] > 0).sum() >= 50
        assert (val[1] > val[0]).sum() >= 50 and (val[2] > val[1]).sum() >= 50, k
        per = _exp(shapes, k, 0)
        assert per[0][0] != INV and per[-1][len(per[-1]) - k] != INV and (per[-1][len(per[-1]) - k + 1:] == INV).all()
        assert (per[0] == INV).sum() > k and (per[8] == INV).all() and (per[10] == INV).all()
        assert (per[5 + KS.index(k)] != INV).sum() == 1  # the record of exactly k has one window
        j = per[shapes["junction"]]
        assert (j[60 - k + 1:60] == 0).all() and (j[:60 - k + 1] >= 1).all()


@pytest.mark.parametrize("k", KS)
def test_session_genome_every_shape(shapes, small_k16, k):
    for e in ES:
        for fo in (False, True):
            st = {}
            got = small_k16.query_mappability(shapes["recs"], k=k, mismatches=e, forward_only=fo, stats=st)
            _same(got, _exp(shapes, k, e, fo), (k, e, fo))
            valid = shapes["parts"][k, e][2]
            assert st["positions"] == sum(len(r) for r in shapes["recs"]) and st["valid"] == valid.sum() and st["launches"] >= 1
            assert st["early_exits"] == 0 and st["ms_total"] == pytest.approx(st["ms_valid"] + st["ms_search"], rel=1e-9)
            assert st["table_reads"] >= (st["valid"] if k >= 16 else 0) and (k >= 16 or st["table_reads"] == 0)


def test_same_answer_as_the_genome_track(shapes, small_genome, small_k16):
    """for a cut of the genome the values at valid positions are the genome track's, sliced"""
    k = 16
    for e in ES:
        track = small_k16.mappability(k=k, mismatches=e)
        got = small_k16.query_mappability(shapes["recs"], k=k, mismatches=e)
        for rec, at in ((0, shapes["cut0"]), (len(shapes["recs"]) - 1, shapes["cut_last"])):
            g = got[rec]
            assert small_genome["text"][at:at + len(g)] == shapes["recs"][rec]
            ok = g != INV
            assert ok.sum() >= 250 and (g[ok] == track[at:at + len(g)][ok]).all() and (g[ok] >= 1).all(), (e, rec)
            inside = np.arange(len(g) - k + 1)
            assert ((track[at + inside] > 0) == ok[inside]).all()


# ---- long k ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [64, 100])
def test_long_kmers(small_genome, k, tmp_path):
    """k above 32 against the diagonal reference on the 12 kb cut-and-twin genome of test_gpu_mappability_mm: the narrow-interval check
    and the 8-byte pattern reads at record ends"""
    t = small_genome["text"][:12000].replace(b"\n", b"N").decode()
    a = next(a for a in range(1000, 6000) if set(t[a:a + 400]) <= set("ACGT"))
    src = t[a:a + 400]
    twin = src[:150] + ("A" if src[150] != "A" else "C") + src[151:]
    text = genome_text([t[:7000] + twin + t[7000:], t[8000:9000] + revcomp(twin) + "ACGTTGCAAC"])
    path = str(tmp_path / "cut.fm9")
    dicey_amd.build_index(text, path)
    recs = [src.encode(), twin.encode(), (src[:230] + twin[100:]).encode()]
    qbuf, _ = Q.buffer_of(recs)
    parts = Q.parts_diagonal(text, qbuf, k, (0, 1))
    v0, v1 = (parts[e][0] + parts[e][1] for e in (0, 1))
    assert (v1 > v0).sum() >= 2 * k and (v0[parts[0][2]] == 0).sum() >= 50 and (v0 >= 2).sum() >= 50
    with dicey_amd.FmIndex(path) as ix:
        for e in (0, 1):
            for fo in (False, True):
                _same(ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo), Q.split(Q.finish(*parts[e], fo), recs), (k, e, fo))


# ---- the edges of the text, and the properties ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    rng = random.Random(77)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    x10 = rnd(10)
    pal = x10 + revcomp(x10)  # its own reverse complement
    c1 = rnd(1500) + "N" + rnd(800) + pal + rnd(700)
    c2 = rnd(2000)
    text = genome_text([c1, c2])
    fm9 = str(tmp_path_factory.mktemp("qmap") / "edge.fm9")
    dicey_amd.build_index(text, fm9)
    return {"text": text, "fm9": fm9, "c1": c1, "c2": c2, "pal": pal, "rnd": rnd}


def test_edges_of_the_text(edge):
    c1, c2, text, k = edge["c1"], edge["c2"], edge["text"], 20
    recs = [c1[-10:] + c2[:10],                  # across the '\n' between two sequences
            c1[1490:1500] + "A" + c1[1501:1511],  # around the genome's N, the N replaced
            edge["rnd"](5) + c1[:15],             # the window would start five characters before position 0
            revcomp(edge["rnd"](5) + c1[:15]),
            c1[:20], c2[-20:]]                   # and the first and last windows themselves
    assert text[1500:1501] == b"N" and text[len(c1):len(c1) + 1] == b"\n"
    recs = [r.encode() for r in recs]
    with dicey_amd.FmIndex(edge["fm9"]) as ix:
        for e in ES:
            exp = Q.values(text, recs, k, e)
            assert [int(x[0]) for x in exp] == [0, 0, 0, 0, 1, 1], e  # the reference alone: none of the first four is counted
            for kw in ({}, {"forward_only": True}):
                _same(ix.query_mappability(recs, k=k, mismatches=e, **kw), Q.values(text, recs, k, e, **kw), (e, kw))


def test_properties(shapes, small_genome, small_k16, edge):
    recs, k = shapes["recs"], 16
    for e in ES:
        full = _exp(shapes, k, e)
        for cap in (1, 2, 5):
            st = {}
            got = small_k16.query_mappability(recs, k=k, mismatches=e, max_count=cap, stats=st)
            _same(got, [np.where(x == INV, INV, np.minimum(x, cap)).astype(np.uint32) for x in full], (e, cap))
            assert st["early_exits"] == sum(int(((x != INV) & (x >= cap)).sum()) for x in full) > 0
        both = small_k16.query_mappability(recs, k=k, mismatches=e)
        fwd = small_k16.query_mappability(recs, k=k, mismatches=e, forward_only=True)
        for x, y in zip(fwd, both):
            assert ((x == INV) == (y == INV)).all() and (x <= y).all()
    # e = 0 is count(w) + count(revcomp(w))
    got = small_k16.query_mappability(recs, k=k)
    rng = random.Random(5)
    where = [(i, p) for i, g in enumerate(got) for p in np.nonzero(g != INV)[0].tolist()]
    sample = rng.sample(where, 200)
    pats = []
    for i, p in sample:
        w = recs[i][p:p + k]
        pats += [w, revcomp(w.decode()).encode()]
    cnt = small_k16.count(pats)
    assert [int(got[i][p]) for i, p in sample] == [cnt[2 * j] + cnt[2 * j + 1] for j in range(len(sample))]
    # str input is upper-cased, bytes go through as given
    low = recs[-1].decode().lower()
    _same(small_k16.query_mappability([low], k=k), [got[-1]], "str")
    assert (small_k16.query_mappability([low.encode()], k=k)[0] == INV).all()
    assert small_k16.query_mappability([], k=k) == [] and dicey_amd.QMAP_INVALID == INV
    # a reverse-complement palindrome that the genome holds once counts on both strands
    with dicey_amd.FmIndex(edge["fm9"]) as ix:
        pal = edge["pal"].encode()
        assert edge["text"].count(pal) == 1 and Q.values(edge["text"], [pal], 20, 0)[0][0] == 2
        assert ix.query_mappability([pal], k=20)[0][0] == 2 and ix.query_mappability([pal], k=20, forward_only=True)[0][0] == 1


# ---- paths -----------------------------------------------------------------------------------------------------------------------

def test_open_flags_give_identical_arrays(shapes, small_genome):
    for kw in ({"kmer_table": False}, {"compact": True}, {"compact": True, "pre5": False}):
        with dicey_amd.FmIndex(small_genome["fm9"], **kw) as ix:
            for e in ES:
                _same(ix.query_mappability(shapes["recs"], k=20, mismatches=e), _exp(shapes, 20, e), (kw, e))


def test_switches_of_the_development_build(shapes, small_genome, monkeypatch):
    """DICEY_QMAP_CHUNK (positions per launch) and DICEY_MAP_NARROW (W) change how the search runs, never what it returns"""
    recs, k = shapes["recs"], 20
    npos = sum(len(r) + 1 for r in recs)
    ix = dicey_amd.FmIndex(small_genome["fm9"], _lib=conftest.exp_lib())
    try:
        seen = {}
        for name, env in (("default", {}), ("chunk", {"DICEY_QMAP_CHUNK": "64"}), ("never", {"DICEY_MAP_NARROW": "0"}),
                          ("both", {"DICEY_QMAP_CHUNK": "777", "DICEY_MAP_NARROW": "1000000000"})):
            for kk, vv in env.items():
                monkeypatch.setenv(kk, vv)
            for e in ES:
                st = {}
                _same(ix.query_mappability(recs, k=k, mismatches=e, stats=st), _exp(shapes, k, e), (name, e))
                seen[name, e] = st
            _same(ix.query_mappability(recs, k=k, mismatches=1, max_count=2, forward_only=True), _exp(shapes, k, 1, True, 2), (name, "cap"))
            for kk in env:
                monkeypatch.delenv(kk)
        for e in ES:
            assert seen["default", e]["launches"] == 1 and seen["default", e]["verified_rows"] > 0
            assert seen["chunk", e]["launches"] == -(-npos // 64) and seen["both", e]["launches"] == -(-npos // 777)
            assert seen["never", e]["verified_rows"] == 0 and seen["never", e]["steps"] > 0
            assert seen["both", e]["steps"] == 0 and seen["both", e]["verified_rows"] > 0
            assert len({s["valid"] for (_, ee), s in seen.items() if ee == e}) == 1
    finally:
        ix.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_argument_checks(small_genome):
    L = _capi.load()
    EINVAL, ELIMIT = -1, -7
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    seq = small_genome["seqs"][0][:40].encode()
    off = (C.c_uint64 * 2)(0, 40)
    vals = (C.c_uint32 * 40)(*([0xABCD1234] * 40))

    def prm(k=20, e=0, flags=0, res=(0, 0, 0)):
        return _capi.QmapParams(k, e, 0, 0, flags, (C.c_uint32 * 3)(*res))

    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        h = ix.handle

        def call(p, handle=h, s=seq, o=off, n=1, v=vals, st=None):
            rc = L.dg_query_map(handle, C.byref(p) if p is not None else None, s, o, n, v, st)
            if rc:
                assert L.dg_last_error() and b"dg_query_map" in L.dg_last_error()
            return rc

        assert call(None) == EINVAL
        assert call(prm(flags=1)) == EINVAL
        for r in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            assert call(prm(res=r)) == EINVAL
        assert call(prm(k=9)) == ELIMIT and call(prm(k=1001)) == ELIMIT and call(prm(e=3)) == ELIMIT
        big = (C.c_uint64 * 2)(0, 1 << 31)
        assert call(prm(), o=big) == ELIMIT
        assert call(prm(), o=(C.c_uint64 * 2)(0, (1 << 31) - 1)) == ELIMIT  # with its separator
        assert call(prm(), handle=None) == EINVAL
        assert call(prm(), s=None) == EINVAL and call(prm(), o=None) == EINVAL and call(prm(), v=None) == EINVAL
        assert call(prm(), o=(C.c_uint64 * 3)(0, 30, 20), n=2) == EINVAL
        # the order: parameter block, limits, then the handle
        assert call(prm(k=9, flags=1)) == EINVAL and call(prm(k=9), handle=None) == ELIMIT and call(prm(), o=big, handle=None) == ELIMIT
        assert list(vals) == [0xABCD1234] * 40
        # nothing to do is not an error, and writes nothing
        st = _capi.QmapStats()
        assert call(prm(), n=0, st=C.byref(st)) == 0 and call(prm(), s=None, o=None, n=0, v=None) == 0
        assert call(prm(), o=(C.c_uint64 * 3)(0, 0, 0), n=2, st=C.byref(st)) == 0 and st.positions == 0 and st.launches == 0
        assert list(vals) == [0xABCD1234] * 40
        assert call(prm(), st=C.byref(st)) == 0 and st.positions == 40 and st.valid == R.valid_positions(seq, 20).sum() and st.launches == 1
        assert list(vals) == [int(x) for x in Q.values(small_genome["text"], [seq], 20, 0)[0]] and list(vals[21:]) == [INV] * 19
        # offsets that do not start at 0: records are seqs[off[i] .. off[i+1]) and values[off[i] ..]
        v2 = (C.c_uint32 * 40)(*([7] * 40))
        assert call(prm(k=12), o=(C.c_uint64 * 3)(10, 25, 40), n=2, v=v2) == 0
        exp = Q.values(small_genome["text"], [seq[10:25], seq[25:40]], 12, 0)
        assert list(v2) == [7] * 10 + [int(x) for x in exp[0]] + [int(x) for x in exp[1]]


def test_refused_while_a_hunt_batch_is_in_flight(small_genome):
    g = small_genome
    rng = random.Random(9)
    t = g["text"].decode()
    qs = []
    while len(qs) < 300:
        p = rng.randrange(len(t) - 20)
        if "\n" not in t[p:p + 20]:
            qs.append(t[p:p + 20])
    rec = [t[_clean(t, 500, 200):][:200].encode()]
    with dicey_amd.FmIndex(g["fm9"]) as ix:
        before = ix.query_mappability(rec, k=20, mismatches=1)
        tk = ix.hunt_submit(qs, g["seqlen"], distance=1)
        try:
            with pytest.raises(dicey_amd.DgError) as e:
                ix.query_mappability(rec, k=20, mismatches=1)
            assert e.value.code == -1 and "in flight" in str(e.value) and "dg_query_map" in str(e.value)
        finally:
            ix.hunt_wait(tk)
        _same(ix.query_mappability(rec, k=20, mismatches=1), before, "after the batch")
        _same(before, Q.values(g["text"], rec, 20, 1), "reference")


# ---- a genome too large for brute force ------------------------------------------------------------------------------------------

def _direct(codes, w, k, e):
    """windows (2-bit codes, first character most significant) within e substitutions of the k-mer w, compared one by one"""
    c, _ = Q._codes(w, np.array([0]), k)
    x = codes ^ c[0]
    x = (x | (x >> np.uint64(1))) & np.uint64(0x5555555555555555)
    n = np.zeros(len(x), dtype=np.uint8)
    for b in range(0, 2 * k, 8):  # popcount by bytes
        n += _POP[(x >> np.uint64(b)).astype(np.uint8)]
    return int((n <= e).sum())


_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def test_generated_genome_of_a_few_mb(tmp_path):
    """~3 Mb with copied segments, N runs and homopolymers, built on the device and opened as the binary opens it; 20 kb of queries (cuts
    with 1 % substitutions, random sequence, a homopolymer) at k = 24, e = 2.  300 sampled positions against the sum of the text's
    window counts over the explicit Hamming ball, 12 of them also against a window-by-window comparison."""
    rng = np.random.default_rng(29)
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
    k, e = 24, 2
    recs = []
    for _ in range(6):
        a = int(rng.integers(0, len(seqs[0]) - 2500))
        piece = np.frombuffer(seqs[0][a:a + 2500], dtype=np.uint8).copy()
        hits = rng.integers(0, 2500, 25)
        piece[hits] = acgt[rng.integers(0, 4, 25)]
        recs.append(piece.tobytes())
    recs += [acgt[rng.integers(0, 4, 4800)].tobytes(), b"A" * 200]
    assert sum(map(len, recs)) == 20000
    with dicey_amd.FmIndex(path, compact=True, pre5=False) as ix:
        st = {}
        got = ix.query_mappability(recs, k=k, mismatches=e, stats=st)
        exact = ix.query_mappability(recs, k=k)
    assert st["launches"] > 0 and st["verified_rows"] > 0 and st["positions"] == 20000
    for g, x, r in zip(got, exact, recs):
        assert ((g == INV) == ~R.valid_positions(r, k)).all() and (g >= x).all()
    assert sum(int(((g > x) & (g != INV)).sum()) for g, x in zip(got, exact)) >= 1000
    prs = np.random.default_rng(5)
    where = [(i, p) for i, g in enumerate(got) for p in np.nonzero(g != INV)[0].tolist()]
    sample = [where[j] for j in prs.choice(len(where), 300, replace=False)]
    kmers = [recs[i][p:p + k] for i, p in sample]
    exp = Q.ball_at(text, kmers, k, e)
    assert [int(got[i][p]) for i, p in sample] == exp.tolist()
    assert (exp == 0).sum() >= 20 and (exp >= 1).sum() >= 100
    codes = Q._codes(text, np.nonzero(R.valid_positions(text, k))[0], k)[0]
    for w, x in list(zip(kmers, exp.tolist()))[:12]:
        assert _direct(codes, w, k, e) + _direct(codes, revcomp(w.decode()).encode(), k, e) == x
