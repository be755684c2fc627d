"""(k,e)-mappability on a box without a GPU: the two brute-force references of tests/mappability_mm_ref.py against each other and,
at e = 0, against tests/mappability_ref.py; the new structs; the argument checks of dg_mappability_mm / dg_map_mm_stats and of
`dicey mappability -e` that come before any device work."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import mappability_mm_ref as M
import mappability_ref as R
from conftest import genome_text, make_genome, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")


@pytest.fixture(scope="module")
def dicey():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "csrc"), "-s", "-j4"])
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    return DICEY


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "csrc"), "-s", "-j4"])
    from dicey_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def text():
    """3 kb in three sequences with N runs, IUPAC letters, copied segments, and near-copies on both strands"""
    rng = random.Random(5)
    seqs = make_genome(23, 3, 900, iupac=True)
    s = seqs[0]
    twin = list(s[100:220])
    for i in (17, 60, 63):
        twin[i] = "ACGT"[("ACGT".index(twin[i]) + 1) % 4] if twin[i] in "ACGT" else twin[i]
    twin = "".join(twin)
    seqs[1] = seqs[1][:300] + twin + seqs[1][300:]
    seqs[2] = seqs[2][:200] + revcomp(twin) + seqs[2][200:] + "".join(rng.choice("ACGT") for _ in range(40)) + s[100:130]
    seqs.append("ACGTAC")
    return genome_text(seqs)


@pytest.mark.parametrize("k", [10, 13, 24, 32])
def test_the_two_references_agree(text, k):
    diag = M.parts_diagonal(text, k, (0, 1, 2))
    grew = 0
    for e in (0, 1, 2):
        bf, br = M.parts_ball(text, k, e)
        assert (diag[e][0] == bf).all() and (diag[e][1] == br).all(), (k, e)
        if e:
            grew += int(((diag[e][0] + diag[e][1]) > (diag[e - 1][0] + diag[e - 1][1])).sum())
    assert grew > 50  # the near-copies are seen
    ps = list(range(90, 240, 7)) + [0, len(text) - 1, len(text) - k - 1]
    for e in (1, 2):
        assert (M.direct(text, k, e, ps) == (diag[e][0] + diag[e][1])[ps]).all()
        assert (M.direct(text, k, e, ps, forward_only=True) == diag[e][0][ps]).all()


@pytest.mark.parametrize("k", [10, 20, 32, 47])
def test_both_references_equal_the_exact_count_at_e0(text, k):
    for fo in (False, True):
        exp = R.values(text, k, forward_only=fo)
        assert (M.values(text, k, 0, forward_only=fo, method="diagonal") == exp).all()
        if k <= 32:
            assert (M.values(text, k, 0, forward_only=fo) == exp).all()
    assert (M.values(text, k, 0, max_count=2, method="diagonal") == R.values(text, k, max_count=2)).all()


def test_bedgraph_of_values_is_the_exact_writer_at_e0(text):
    names = ["a", "b", "c", "d"]
    assert M.bedgraph(R.values(text, 12), text, names) == R.bedgraph(text, names, 12)


def test_struct_sizes_match_the_header():
    from dicey_amd import _capi
    assert ctypes.sizeof(_capi.MapMmParams) == 24
    assert ctypes.sizeof(_capi.MapMmStats) == 56
    assert ctypes.sizeof(_capi.MapParams) == 16  # untouched


def test_entry_points_null_flag_and_limit_handling(lib):
    from dicey_amd import _capi
    DG_EINVAL, DG_ELIMIT = -1, -7

    def call(prm, ix=None):
        m = ctypes.c_void_p(1234)
        rc = lib.dg_mappability_mm(ix, ctypes.byref(prm) if prm is not None else None, ctypes.byref(m))
        assert not m.value  # cleared on every failure
        return rc

    assert call(_capi.MapMmParams(20, 1, 0, 0, 0, 0)) == DG_EINVAL  # null handle
    assert b"dg_mappability_mm" in lib.dg_last_error()
    assert call(None) == DG_EINVAL
    assert lib.dg_mappability_mm(None, ctypes.byref(_capi.MapMmParams(20, 1, 0, 0, 0, 0)), None) == DG_EINVAL
    assert call(_capi.MapMmParams(20, 1, 0, 0, 1, 0)) == DG_EINVAL  # flags
    assert call(_capi.MapMmParams(20, 1, 0, 0, 0, 1)) == DG_EINVAL  # reserved
    # the parameter block is checked before the handle: three mismatches are refused as a limit
    assert call(_capi.MapMmParams(20, 3, 0, 0, 0, 0)) == DG_ELIMIT
    assert b"outside 0..2" in lib.dg_last_error()
    assert call(_capi.MapMmParams(20, 0xFFFFFFFF, 0, 0, 0, 0)) == DG_ELIMIT
    st = _capi.MapMmStats()
    assert lib.dg_map_mm_stats(None, ctypes.byref(st)) == DG_EINVAL
    assert lib.dg_map_mm_stats(None, None) == DG_EINVAL


@pytest.mark.parametrize("e", ["3", "-1", "17"])
def test_mismatches_refused_before_device_work(dicey, tmp_path, e):
    fa = tmp_path / "g.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGT\n")  # no .fm9 next to it: a check that came later would say so instead
    r = subprocess.run([dicey, "mappability", "-g", str(fa), "-k", "10", "-e", e], capture_output=True, text=True)
    assert r.returncode == 1
    assert r.stderr.startswith("Error: ") and "outside 0..2!" in r.stderr
    assert r.stdout == ""
    r = subprocess.run([dicey, "mappability", "-g", str(fa), "-k", "10", "--mismatches=" + e], capture_output=True, text=True)
    assert r.returncode == 1 and "outside 0..2!" in r.stderr


def test_accepted_mismatches_reach_the_index_check(dicey, tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGT\n")
    for e in ("0", "1", "2"):
        r = subprocess.run([dicey, "mappability", "-g", str(fa), "-k", "10", "-e", e], capture_output=True, text=True)
        assert r.returncode == 1 and "g.fm9" in r.stderr


def test_usage_shows_mismatches(dicey):
    r = subprocess.run([dicey, "mappability"], capture_output=True, text=True)
    assert r.returncode == 255
    assert "-e [ --mismatches ] arg (=0)" in r.stdout and "--kmer" in r.stdout
    r = subprocess.run([dicey], capture_output=True, text=True)
    assert "chop is not part of this build." in r.stdout
