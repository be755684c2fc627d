"""dg_query_map_iupac / FmIndex.query_mappability(iupac=True) against the brute-force model of tests/query_iupac_ref.py, which knows
nothing of the FM-index: the degenerate record set on the session genome across the K-mer table order, every strand option and the anchors
0, 1, 5 and k, with the statistics; max_count; max_degeneracy; A/C/G/T records against the plain and the anchored call, values and
counters; e = 0 against the sum of the plain call over explicit expansions; k = 64 and 63 with codes at every 8-byte edge of the narrow
finish, with and without the K-mer table and with the narrow finish forced and forbidden; the edges of the text; the argument checks."""
import ctypes as C
import random

import numpy as np
import pytest

import conftest
import dicey_amd
import query_iupac_ref as I
import query_map_ref as Q
from conftest import genome_text
from dicey_amd import _capi

pytestmark = pytest.mark.gpu
INV = I.INVALID
KS, ES = I.KS, I.ES


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
    return I.session(small_genome["seqs"], small_genome["text"])


def _exp(shapes, k, e, a, fo=False, cap=0, maxdeg=4096):
    f, r, valid = shapes["parts"][k, e, a]
    if maxdeg != 4096:
        valid = valid & (I.degeneracy(shapes["qbuf"], k)[1] <= maxdeg)
    return Q.split(I.finish(f, r, valid, fo, cap), shapes["recs"])


# ---- session genome --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_session_genome_every_anchor(shapes, small_k16, k):
    recs = shapes["recs"]
    npos = sum(len(r) for r in recs)
    letters, deg = I.degeneracy(shapes["qbuf"], k)
    valid = shapes["parts"][k, 0, 0][2]
    assert (letters & ~valid).sum() == 5 and (deg[valid] > 1).sum() >= 1000  # the seven N's; most k-mers are degenerate
    for e in ES:
        for a in I.anchors_of(k):
            for fo in (False, True):
                st = {}
                got = small_k16.query_mappability(recs, k=k, mismatches=e, forward_only=fo, anchor=a, iupac=True, max_degeneracy=4096, stats=st)
                _same(got, _exp(shapes, k, e, a, fo), (k, e, a, fo))
                assert st["positions"] == npos and st["valid"] == valid.sum() and st["launches"] >= 1 and st["early_exits"] == 0, (k, e, a, fo, st)
                assert st["too_degenerate"] == (letters & ~valid).sum() and st["degenerate"] == (deg[valid] > 1).sum(), (k, e, a, fo, st)
                assert st["expansions"] == deg[valid].sum() * (1 if fo else 2), (k, e, a, fo, st)
                assert st["ms_total"] == pytest.approx(st["ms_valid"] + st["ms_search"], rel=1e-9)


def test_max_count(shapes, small_k16):
    recs, k = shapes["recs"], 16
    for e in ES:
        for a in (0, 5):
            full = _exp(shapes, k, e, a)
            for cap in (1, 2, 5):
                st = {}
                got = small_k16.query_mappability(recs, k=k, mismatches=e, max_count=cap, anchor=a, iupac=True, max_degeneracy=4096, stats=st)
                _same(got, [np.where(x == INV, INV, np.minimum(x, cap)).astype(np.uint32) for x in full], (e, a, cap))
                assert st["early_exits"] == sum(int(((x != INV) & (x >= cap)).sum()) for x in full) > 0


def test_max_degeneracy(shapes, small_k16):
    recs, k = shapes["recs"], 20
    letters, deg = I.degeneracy(shapes["qbuf"], k)
    seen = set()
    for maxdeg in (1, 2, 64, 4096, 0):
        lim = maxdeg or 256
        st = {}
        got = small_k16.query_mappability(recs, k=k, mismatches=1, anchor=5, iupac=True, max_degeneracy=maxdeg, stats=st)
        _same(got, _exp(shapes, k, 1, 5, maxdeg=lim), maxdeg)
        ok = letters & (deg <= lim)
        assert st["valid"] == ok.sum() and st["too_degenerate"] == (letters & ~ok).sum() and st["degenerate"] == (ok & (deg > 1)).sum(), (maxdeg, st)
        assert st["expansions"] == 2 * deg[ok].sum()
        seen.add(int(ok.sum()))
    assert len(seen) >= 4  # every limit but the last cuts somewhere else
    st = {}
    got = small_k16.query_mappability(recs, k=k, iupac=True, max_degeneracy=1, stats=st)
    assert st["degenerate"] == 0 and st["expansions"] == 2 * st["valid"]
    flat = np.concatenate(got)
    buf = np.concatenate(Q.split(deg, recs))
    assert ((flat != INV) == (buf == 1)).all()  # only k-mers without a code have values


def test_acgt_records_are_the_plain_and_the_anchored_call(small_genome, small_k16):
    """on records of A/C/G/T the values and the shared counters are dg_query_map's at anchor 0 and dg_query_map_anchored's otherwise"""
    s1, s2, s3 = small_genome["seqs"]
    rng = random.Random(5)
    a, b = I._clean(s1, 8000, 400), I._clean(s3, 9000, 600)
    sub = lambda s: "".join(c if i % 13 else "ACGT"[("ACGT".index(c) + 1) % 4] for i, c in enumerate(s))
    recs = [s1[a:a + 400], conftest.revcomp(sub(s3[b:b + 600])), "".join(rng.choice("ACGT") for _ in range(300)), s2[a:a + 15].lower(), "", "ACGTACGTA"]
    recs = [r.encode() for r in recs]
    shared = ("positions", "valid", "steps", "table_reads", "verified_rows", "early_exits", "launches")
    for k in KS:
        for e in ES:
            for fo in (False, True):
                for anchor, cap in ((0, 0), (1, 0), (5, 0), (k, 0), (0, 2), (5, 2)):
                    s0, s1_ = {}, {}
                    exp = small_k16.query_mappability(recs, k=k, mismatches=e, forward_only=fo, max_count=cap, anchor=anchor or None, stats=s0)
                    got = small_k16.query_mappability(recs, k=k, mismatches=e, forward_only=fo, max_count=cap, anchor=anchor, iupac=True, stats=s1_)
                    _same(got, exp, (k, e, fo, anchor, cap))
                    assert [s1_[f] for f in shared] == [s0[f] for f in shared], (k, e, fo, anchor, cap, s0, s1_)
                    assert s1_["too_degenerate"] == 0 and s1_["degenerate"] == 0
                    if not cap:
                        assert s1_["expansions"] == s1_["valid"] * (1 if fo else 2)
    assert sum(int((x != INV).sum()) for x in exp) > 1000


def test_e0_is_the_sum_over_explicit_expansions(shapes, small_k16):
    """an independent path with no model: at e = 0 no window is near two expansions, so the plain call summed over them is the value"""
    recs = shapes["recs"]
    for k in KS:
        got = {fo: small_k16.query_mappability(recs, k=k, forward_only=fo, iupac=True, max_degeneracy=4096) for fo in (False, True)}
        kmers = []
        for ri in (0, 1, 2, 3, 4):
            r = recs[ri].decode()
            for p in range(0, len(r) - k + 1, 9):
                if 1 < I.deg(r[p:p + k]) <= 64:
                    kmers.append((ri, p, I.expansions(r[p:p + k])))
        assert len(kmers) >= 150 and max(len(x) for _, _, x in kmers) >= 9
        flat = [x.encode() for _, _, xs in kmers for x in xs]
        for fo in (False, True):
            vals = small_k16.query_mappability(flat, k=k, forward_only=fo)
            i, nonzero = 0, 0
            for ri, p, xs in kmers:
                tot = sum(int(v[0]) for v in vals[i:i + len(xs)])
                i += len(xs)
                assert int(got[fo][ri][p]) == tot, (k, fo, ri, p)
                nonzero += tot > 0
            assert nonzero >= 50


# ---- long k ----------------------------------------------------------------------------------------------------------------------

def _long_records(src, twin, k, rng):
    """windows of k with a code at index 0, 7, 8 and k - 1 (63: the last byte of the eighth word), a hit code and a miss code each, cut
    from src and from its twin (one substitution at offset 150), and one with all four"""
    recs = []
    for s in (src, twin):
        for i in (0, 7, 8, k - 1):
            for kind in ("hit", "miss"):
                w = list(s[120:120 + k])
                w[i] = I.put_codes(w[i], 1, kind, rng)
                recs.append("".join(w))
        w = list(s[120:120 + k])
        for i, kind in ((0, "hit"), (7, "miss"), (8, "hit"), (k - 1, "hit")):
            w[i] = I.put_codes(w[i], 1, kind, rng)
        recs.append("".join(w))
    recs.append(I.revcomp(recs[-1]))
    recs.append(I.put_codes(src[100:100 + k + 30], 9, "hit", rng))  # sliding: the codes pass every index
    return [r.encode() for r in recs]


@pytest.mark.parametrize("k", [64, 63])
def test_long_kmers(small_genome, k, tmp_path, monkeypatch):
    t = small_genome["text"][:12000].replace(b"\n", b"N").decode()
    a0 = next(a for a in range(1000, 6000) if set(t[a:a + 400]) <= set("ACGT"))
    src = t[a0:a0 + 400]
    twin = src[:150] + ("A" if src[150] != "A" else "C") + src[151:]
    text = genome_text([t[:7000] + twin + t[7000:], t[8000:9000] + conftest.revcomp(twin) + "ACGTTGCAAC"])
    path = str(tmp_path / "cut.fm9")
    dicey_amd.build_index(text, path)
    recs = _long_records(src, twin, k, random.Random(64))
    qbuf, _ = Q.buffer_of(recs)
    anchors = [0, 1, 8, 9, k]
    parts, _ = I.parts(text, qbuf, [k], ES, {k: anchors})
    tot = {key: parts[key][0] + parts[key][1] for key in parts}
    assert (tot[k, 1, 0] > tot[k, 0, 0]).sum() >= 8 and (tot[k, 1, 9] < tot[k, 1, 0]).sum() >= 3 and (tot[k, 0, 0] > 0).sum() >= 8
    runs = [("table", {}, None, {}), ("no table", {"kmer_table": False}, None, {})]
    runs += [(n, {}, conftest.exp_lib(), env) for n, env in (("never", {"DICEY_MAP_NARROW": "0"}), ("always", {"DICEY_MAP_NARROW": "1000000000"}))]
    for name, kw, lib, env in runs:
        for kk, vv in env.items():
            monkeypatch.setenv(kk, vv)
        with dicey_amd.FmIndex(path, _lib=lib, **kw) as ix:
            for e in ES:
                for a in anchors:
                    for fo in (False, True):
                        st = {}
                        got = ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo, anchor=a, iupac=True, max_degeneracy=4096, stats=st)
                        _same(got, Q.split(I.finish(*parts[k, e, a], fo), recs), (name, k, e, a, fo))
                        if name == "never":
                            assert st["verified_rows"] == 0 and st["steps"] > 0
                        if name == "always":
                            assert st["steps"] == 0 and st["verified_rows"] > 0
        for kk in env:
            monkeypatch.delenv(kk)


# ---- the edges of the text ---------------------------------------------------------------------------------------------------------

def test_edges_of_the_text(tmp_path):
    rng = random.Random(78)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    c1, c2 = rnd(1500) + "R" + rnd(1500), rnd(2000)
    text, k = genome_text([c1, c2]), 20
    fm9 = str(tmp_path / "edge.fm9")
    dicey_amd.build_index(text, fm9)
    code = lambda s, i, kind: s[:i] + I.put_codes(s[i], 1, kind, rng) + s[i + 1:]
    recs = [code(c1[:20], 0, "hit"), code(c1[:20], 3, "miss"), code(c2[-20:], 19, "hit"), code(c2[-20:], 12, "miss"),  # the first and last windows
            rnd(5) + code(c1[:15], 2, "hit"),            # the window would start five characters before position 0
            I.revcomp(rnd(5) + code(c1[:15], 2, "hit")),
            code(c1[-10:], 4, "hit") + c2[:10],          # across the '\n' between two sequences
            c1[1490:1500] + "R" + c1[1501:1510]]         # an IUPAC letter of the genome is never part of an occurrence
    recs = [r.encode() for r in recs]
    qbuf, _ = Q.buffer_of(recs)
    parts, _ = I.parts(text, qbuf, [k], ES, {k: [0, 1, 10]})
    with dicey_amd.FmIndex(fm9) as ix:
        for e in ES:
            for a in (0, 1, 10):
                exp = Q.split(I.finish(*parts[k, e, a]), recs)
                assert [int(x[0]) for x in exp] == [1, int(e > 0), 1, int(e > 0 and a <= 7), 0, 0, 0, 0], (e, a)  # the model alone
                for fo in (False, True):
                    _same(ix.query_mappability(recs, k=k, mismatches=e, forward_only=fo, anchor=a, iupac=True),
                          Q.split(I.finish(*parts[k, e, a], fo), recs), (e, a, fo))


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_argument_checks(small_genome):
    L = _capi.load()
    EINVAL, ELIMIT = -1, -7
    seq = small_genome["seqs"][0][:40].encode()
    off = (C.c_uint64 * 2)(0, 40)
    vals = (C.c_uint32 * 40)(*([0xABCD1234] * 40))
    assert set(seq) <= set(b"ACGT")

    def prm(k=20, e=0, a=5, maxdeg=0, flags=0, res=(0, 0, 0)):
        return _capi.QmapIupacParams(k, e, a, 0, 0, maxdeg, flags, (C.c_uint32 * 3)(*res))

    with dicey_amd.FmIndex(small_genome["fm9"]) as ix:
        h = ix.handle

        def call(p, handle=h, s=seq, o=off, n=1, v=vals, st=None):
            rc = L.dg_query_map_iupac(handle, C.byref(p) if p is not None else None, s, o, n, v, st)
            if rc:
                assert L.dg_last_error() and b"dg_query_map_iupac" in L.dg_last_error()
            return rc

        assert call(None) == EINVAL
        assert call(prm(flags=1)) == EINVAL
        for r in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            assert call(prm(res=r)) == EINVAL
        assert call(prm(k=9)) == ELIMIT and call(prm(k=65)) == ELIMIT and call(prm(e=3)) == ELIMIT
        assert call(prm(a=21)) == ELIMIT and call(prm(k=10, a=11)) == ELIMIT and call(prm(maxdeg=4097)) == ELIMIT
        big = (C.c_uint64 * 2)(0, 1 << 31)
        assert call(prm(), o=big) == ELIMIT
        assert call(prm(), o=(C.c_uint64 * 2)(0, (1 << 31) - 1)) == ELIMIT  # with its separator
        assert call(prm(), handle=None) == EINVAL
        assert call(prm(), s=None) == EINVAL and call(prm(), o=None) == EINVAL and call(prm(), v=None) == EINVAL
        assert call(prm(), o=(C.c_uint64 * 3)(0, 30, 20), n=2) == EINVAL
        # the order: parameter block, limits, then the handle
        assert call(prm(k=65, flags=1)) == EINVAL and call(prm(maxdeg=4097), handle=None) == ELIMIT and call(prm(), o=big, handle=None) == ELIMIT
        assert list(vals) == [0xABCD1234] * 40
        # nothing to do is not an error, and writes nothing
        st = _capi.QmapIupacStats()
        assert call(prm(), n=0, st=C.byref(st)) == 0 and call(prm(), s=None, o=None, n=0, v=None) == 0
        assert call(prm(), o=(C.c_uint64 * 3)(0, 0, 0), n=2, st=C.byref(st)) == 0 and st.positions == 0 and st.launches == 0
        assert list(vals) == [0xABCD1234] * 40
        assert call(prm(k=64, a=64, maxdeg=4096), st=C.byref(st)) == 0 and st.positions == 40 and st.valid == 0 and st.launches == 1
        assert list(vals) == [INV] * 40
        assert call(prm(a=20), st=C.byref(st)) == 0 and st.valid == I.degeneracy(seq, 20)[0].sum() > 0 and st.too_degenerate == 0
        assert list(vals) == [int(x) for x in Q.values(small_genome["text"], [seq], 20, 0)[0]]
        with pytest.raises(dicey_amd.DgError) as err:
            ix.query_mappability([seq], k=65, iupac=True)
        assert err.value.code == ELIMIT and "dg_query_map_iupac" in str(err.value)
