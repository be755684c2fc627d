"""Every layout an index open derives in HBM (dicey_amd/csrc/index.hip derive_layouts), read back through the development build's
dgx_index_layout and held against tests/index_layout_ref.py entry by entry: Occ blocks, text, suffix array, the packed K-mer table, every
copy of both presence filters, pre5, sax, the prefix levels' directories and records, the block minima with their padding, and the
scalars of FmView.  Most of these are accelerators with a correct slow path behind them: a copy with spurious bits, an escape bit that is
always set, a missing level or zero padding leave every query result equal to the oracle's, so the result suites cannot see them.

Texts: the three of tests/test_gpu_index_open.py (two walks / sorted suffix array, no / one / two prefix levels, default table orders 8 /
9 / 10: no kf below 17 bits, kf2 of order 10 / 11 / 12 through k_kf_generic0 and k_kf_transpose) and "wide" (index_layout_ref.wide_sequences):
A^9 occurs 65536 times — the first table entry in the wide format under test — and C^9 65535 times.  DICEY_KMER_K=12 / DICEY_KMER_K2=14
(k_kf_from_table, k_kf_generic, four copies) on the two larger ones.  Open flags and the switches that leave a layout out must remove
exactly that layout.  The last two tests run the consumers on the wide text: count / locate against a scan, a small hunt against the oracle.

All comparisons are exact; a failure names the layout and the first differing index."""
import ctypes as C
import os

import numpy as np
import pytest

import index_layout_ref as R
import oracle_lib as O
from conftest import exp_lib

pytestmark = pytest.mark.gpu

OCC, TEXT, SA, KTAB, KF, KF2, PRE5, SAX, PLV_DIR, PLV_REC, SAMIN = range(11)


class FilterInfo(C.Structure):
    _fields_ = [("k", C.c_uint32), ("nr", C.c_uint32), ("s", C.c_uint32 * 4), ("pick", C.c_uint64)]


class LayoutInfo(C.Structure):  # index.hip dgx_layout_info
    _fields_ = [("bytes", C.c_uint64), ("n", C.c_uint64), ("x", C.c_uint64), ("C4", C.c_uint32 * 4), ("K", C.c_uint32), ("nrun_min", C.c_uint32),
                ("nlev", C.c_uint32), ("nplv", C.c_uint32), ("pre5_null", C.c_uint32), ("sax_null", C.c_uint32), ("kf", FilterInfo), ("kf2", FilterInfo)]


def layout(ix, what, level=0, dtype=np.uint8):
    """(the layout as a numpy array, or None when the handle does not have it; info)"""
    L = ix._L
    L.dgx_index_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(LayoutInfo)]
    L.dgx_index_layout.restype = C.c_int
    info = LayoutInfo()
    assert L.dgx_index_layout(ix._h, what, level, None, 0, C.byref(info)) == 0, L.dg_last_error()
    if info.bytes == 0:
        return None, info
    buf = np.empty(info.bytes, np.uint8)
    assert L.dgx_index_layout(ix._h, what, level, buf.ctypes.data_as(C.c_void_p), info.bytes, C.byref(info)) == 0, L.dg_last_error()
    return buf.view(dtype), info


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    """per text, once: the .fm9 and the model (the module's cases share both and leave them unchanged)"""
    d = tmp_path_factory.mktemp("layout")
    out = {}
    for name in R.TEXT_NAMES:
        text, seqs = R.text_of(name)
        path = os.path.join(str(d), name + ".fm9")
        O.build_fm9(text, path)
        out[name] = {"text": text, "seqs": seqs, "fm9": path, "model": R.Model(text), "seqlen": [len(s) + 1 for s in seqs],
                     "names": ["chr%d" % (i + 1) for i in range(len(seqs))]}
    return out


K12 = {"DICEY_KMER_K": "12", "DICEY_KMER_K2": "14"}
CASES = [("%s/default" % t, t, {}, {}) for t in R.TEXT_NAMES] + \
        [("%s/K12_K2_14" % t, t, {}, K12) for t in ("n300k", "wide")] + \
        [("%s/%s" % (t, f), t, kw, {}) for t in R.TEXT_NAMES
         for f, kw in (("no_pre5", dict(pre5=False)), ("compact", dict(compact=True)), ("no_table", dict(kmer_table=False)))] + \
        [("%s/%s" % (t, v), t, {}, {v: "1"}) for t in ("n300k", "wide") for v in ("DICEY_NO_SAX", "DICEY_NO_PLV", "DICEY_NO_SA_MINIMA")]


def expected_presence(n, kw, env):
    """which layouts a handle has (derive_layouts' conditions on the flags and switches; the test devices have room for all of them)"""
    table = kw.get("kmer_table", True)
    K, K2 = R.default_orders(n)
    if "DICEY_KMER_K" in env:
        K, K2 = int(env["DICEY_KMER_K"]), int(env["DICEY_KMER_K2"])
    pre5 = table and kw.get("pre5", True)
    # the records ride on the block minima's top-k locate: without the minima there are none (stage_pre5_sax)
    sax = pre5 and not kw.get("compact", False) and "DICEY_NO_SAX" not in env and "DICEY_NO_SA_MINIMA" not in env
    return {"K": K if table else 0, "K2": K2 if table else 0, "kf": table and 2 * K >= 17, "pre5": pre5, "sax": sax,
            "plv": sax and "DICEY_NO_PLV" not in env, "samin": "DICEY_NO_SA_MINIMA" not in env}


def compare_all(ix, m, want):
    occ, info = layout(ix, OCC, dtype="<u8")
    assert info.n == m.n and list(info.C4) == m.C4(), "n / C4: device %d %s, model %d %s" % (info.n, list(info.C4), m.n, m.C4())
    assert info.nrun_min == m.nrun_min(), "nrun_min: device %d, model %d" % (info.nrun_min, m.nrun_min())
    R.compare_occ(m, occ)
    text, _ = layout(ix, TEXT)
    R._same("text", text, m.s)
    sa, _ = layout(ix, SA, dtype="<u4")
    R._same("sa", sa, m.sa.astype(np.uint32))
    # the K-mer table
    assert info.K == want["K"], "K: device %d, expected %d" % (info.K, want["K"])
    ktab, _ = layout(ix, KTAB, dtype="<u4")
    assert (ktab is not None) == (want["K"] > 0), "ktab"
    if ktab is not None:
        R.compare_ktab(m, info.K, ktab, with_pre5=want["pre5"])
    # the filters
    for name, what, fi, k in (("kf", KF, info.kf, want["K"] if want["kf"] else 0), ("kf2", KF2, info.kf2, want["K2"])):
        if k == 0:
            assert fi.nr == 0 and layout(ix, what, 0)[0] is None, "%s: present, expected none" % name
            continue
        assert fi.nr >= 1 and fi.k == k, "%s: order %d in %d copies, expected order %d" % (name, fi.k, fi.nr, k)
        assert fi.nr == min(4, (2 * k - 9 + 7) // 8 + 1), "%s: %d copies of a %d-bit code" % (name, fi.nr, 2 * k)
        copies = [layout(ix, what, r, dtype="<u4")[0] for r in range(fi.nr)]
        assert all(c is not None for c in copies) and layout(ix, what, fi.nr)[0] is None, "%s: copies" % name
        R.compare_filter(m, name, k, fi.nr, list(fi.s), fi.pick, copies)
    # pre5, sax, prefix levels
    pre5, _ = layout(ix, PRE5, dtype="<u2")
    assert (pre5 is not None) == want["pre5"] == (not info.pre5_null), "pre5: %s, expected %s" % (pre5 is not None, want["pre5"])
    if pre5 is not None:
        R.compare_pre5(m, pre5)
    sax, _ = layout(ix, SAX, dtype="<u4")
    assert (sax is not None) == want["sax"] == (not info.sax_null), "sax: %s, expected %s" % (sax is not None, want["sax"])
    if sax is not None:
        R.compare_sax(m, sax)
    xs = R.plv_sizes(m.n) if want["plv"] else []
    assert info.nplv == len(xs), "nplv: device %d, expected %d" % (info.nplv, len(xs))
    for lv, x in enumerate(xs):
        d, li = layout(ix, PLV_DIR, lv, dtype="<u8")
        rec, _ = layout(ix, PLV_REC, lv, dtype="<u4")
        assert li.x == x and d is not None and rec is not None, "plv[%d]: x %d, expected %d" % (lv, li.x, x)
        R.compare_plv(m, lv, x, d, rec, sax)
    assert layout(ix, PLV_DIR, len(xs))[0] is None and layout(ix, PLV_REC, len(xs))[0] is None, "plv: a level past nplv"
    # block minima
    nlev = 1 + len(m.samin()) if want["samin"] else 1
    assert info.nlev == nlev, "nlev: device %d, expected %d" % (info.nlev, nlev)
    if want["samin"]:
        R.compare_samin(m, [layout(ix, SAMIN, j, dtype="<u4")[0] for j in range(1, nlev)])
    assert layout(ix, SAMIN, nlev)[0] is None and layout(ix, SAMIN, 0)[0] is None, "samin: a level past nlev"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_layouts_equal_the_model(texts, monkeypatch, case):
    import dicey_amd
    _, tname, kw, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = texts[tname]
    with dicey_amd.FmIndex(t["fm9"], device=0, _lib=exp_lib(), **kw) as ix:
        compare_all(ix, t["model"], expected_presence(t["model"].n, kw, env))


def test_the_accessor_clips_and_reports(texts):
    import dicey_amd
    with dicey_amd.FmIndex(texts["n40k"]["fm9"], device=0, _lib=exp_lib()) as ix:
        sa, info = layout(ix, SA, dtype="<u4")
        buf = np.full(16, 0xAB, np.uint8)
        assert ix._L.dgx_index_layout(ix._h, SA, 0, buf.ctypes.data_as(C.c_void_p), 8, C.byref(info)) == 0
        assert info.bytes == 4 * info.n and buf[:8].view("<u4").tolist() == sa[:2].tolist() and (buf[8:] == 0xAB).all()
        assert ix._L.dgx_index_layout(ix._h, 99, 0, None, 0, C.byref(info)) != 0


def run_edges(seqs):
    """patterns on and across the ends of the two long runs"""
    first, last = seqs[0], seqs[2]
    a0, c0 = first.index("A" * 9), last.index("C" * 9)
    a1, c1 = a0 + R.WIDE_A_RUN, c0 + R.WIDE_C_RUN
    return first, last, a0, a1, c0, c1


def test_count_locate_on_the_wide_text(texts):
    import dicey_amd
    t = texts["wide"]
    first, last, a0, a1, c0, c1 = run_edges(t["seqs"])
    pats = ["A" * 9, "A" * 20, "C" * 9, "C" * 20, "A" * 10, "C" * 10, "A" * 8, "C" * 8, first[a0 - 4:a0 + 9], first[a1 - 9:a1 + 4], first[a0 - 1:a0 + 9],
            first[a1 - 9:a1 + 1], last[c0 - 4:c0 + 9], last[c1 - 9:c1 + 4], last[c0 - 1:c0 + 8], "A" * 9 + "C", "G" * 9, "A" * R.WIDE_A_RUN,
            "A" * (R.WIDE_A_RUN + 1), "C" * R.WIDE_C_RUN]
    pats = [p.encode() for p in pats]
    want = [O.bf_locate(t["text"], p) for p in pats]
    assert [len(w) for w in want[:4]] == [65536, 65525, 65535, 65524]
    for env_lib in (None, exp_lib()):
        with dicey_amd.FmIndex(t["fm9"], device=0, _lib=env_lib) as ix:
            assert ix.count(pats) == [len(w) for w in want]
            got = ix.locate(pats)
            for p, g, w in zip(pats, got, want):
                assert g == w, "locate %r: %d positions, the scan finds %d" % (p[:24], len(g), len(w))


def test_hunt_on_the_wide_text(texts):
    """distance 1, Hamming, forward only, five locations: the 20-mers inside the runs reach the wide and the largest narrow entry through
    the table, the run-edge ones the entries next to them (the oracle side of these eight queries takes 0.1 s)"""
    import dicey_amd
    import test_gpu_parity as P
    t = texts["wide"]
    first, last, a0, a1, c0, c1 = run_edges(t["seqs"])
    qs = ["A" * 20, "C" * 20, first[a0 - 10:a0 + 10], first[a1 - 10:a1 + 10], last[c0 - 10:c0 + 10], last[c1 - 10:c1 + 10], first[a0 - 1:a0 + 19],
          last[c1 - 19:c1 + 1]]
    with dicey_amd.FmIndex(t["fm9"], device=0) as ix:
        got = P._compare(ix, O.Index(t["fm9"]), t, qs, distance=1, hamming=True, forward_only=True, max_locations=5)
    assert [len(q.hits) > 0 for q in got.queries] == [True] * len(qs)
