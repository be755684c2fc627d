"""Minimum unique length on a box without a GPU: the two models of tests/min_unique_ref.py against each other, the monotonicity the
definition rests on, the new struct, and the argument checks of dg_min_unique and of `dicey mappability -u` that come before any
device work."""
import ctypes
import os
import subprocess

import pytest

import min_unique_ref as U
from conftest import genome_text, make_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")
REFUSAL = "Error: --minunique cannot be combined with --mismatches or --maxcount!"


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
    """the first 3 000 characters of each sequence of the session genome (conftest.small_genome's recipe): N runs, IUPAC letters,
    copied segments and homopolymers"""
    return genome_text([s[:3000] for s in make_genome(101, 3, 30000, iupac=True)])


def test_the_session_genome_exercises_both_passes():
    """the input of tests/test_gpu_min_unique.py, by the reference alone: at max_k = 64 the session genome (conftest.small_genome's
    recipe) has unique positions, positions still repeated at their limit, positions that only the other strand decides (and some
    it keeps at 0), and values below the smallest max_k — no pass is tested on an empty set"""
    c = U.coverage(genome_text(make_genome(101, 3, 30000, iupac=True)), 64)
    assert c == {"acgt": 78406, "zeros": 3375, "raised": 24018, "kept_zero": 70, "smallest": 7}


@pytest.mark.parametrize("forward_only", [False, True])
def test_the_two_models_agree(text, forward_only):
    a = U.by_values(text, 40, forward_only)
    b = U.direct(text, 40, forward_only)
    bad = (a != b).nonzero()[0]
    assert len(bad) == 0, (bad[:10], a[bad[:10]], b[bad[:10]])
    run = U.run_lengths(text)
    assert len(a) == len(text) and not a[run == 0].any()
    assert (a[a > 0] <= run[a > 0]).all() and a.max() <= 40
    # the slice exercises what it should: unique positions, positions still repeated at the limit, and the other strand
    assert (a > 0).sum() > 5000 and ((a == 0) & (run > 0)).sum() > 100
    if not forward_only:
        assert (a > U.by_values(text, 40, True)).sum() > 1000


@pytest.mark.parametrize("forward_only", [False, True])
def test_the_value_falls_as_k_grows(text, forward_only):
    assert U.monotone(text, 40, forward_only)


def test_a_smaller_max_k_is_the_same_sweep_stopped_earlier(text):
    a40 = U.by_values(text, 40)
    a12 = U.by_values(text, 12)
    assert ((a12 == a40) | ((a12 == 0) & (a40 > 12))).all() and (a12 != a40).any()


def test_struct_size_matches_the_header():
    from dicey_amd import _capi
    assert ctypes.sizeof(_capi.MinUniqueParams) == 16
    assert [f for f, _ in _capi.MinUniqueParams._fields_] == ["max_k", "forward_only", "flags", "reserved"]


def test_entry_point_check_order(lib):
    from dicey_amd import _capi
    DG_EINVAL, DG_ELIMIT = -1, -7
    P = _capi.MinUniqueParams

    def call(prm, ix=None):
        m = ctypes.c_void_p(1234)
        rc = lib.dg_min_unique(ix, ctypes.byref(prm) if prm is not None else None, ctypes.byref(m))
        assert not m.value  # cleared on every failure
        return rc

    assert call(P(40, 0, 0, 0)) == DG_EINVAL  # null handle
    assert b"dg_min_unique" in lib.dg_last_error()
    assert call(None) == DG_EINVAL
    assert lib.dg_min_unique(None, ctypes.byref(P(40, 0, 0, 0)), None) == DG_EINVAL
    assert call(P(40, 0, 1, 0)) == DG_EINVAL  # flags
    assert call(P(40, 0, 0, 1)) == DG_EINVAL  # reserved
    # the parameter block is checked before the handle: a max_k out of range is refused as a limit ...
    for bad in (9, 1001, 0, 0xFFFFFFFF):
        assert call(P(bad, 0, 0, 0)) == DG_ELIMIT
        assert b"outside 10..1000" in lib.dg_last_error()
    for good in (10, 1000):
        assert call(P(good, 1, 0, 0)) == DG_EINVAL
    # ... and flags come before the range
    assert call(P(9, 0, 1, 0)) == DG_EINVAL
    assert call(P(1001, 0, 0, 7)) == DG_EINVAL


@pytest.mark.parametrize("extra", [["-e", "1"], ["-e", "2"], ["-c", "2"], ["--mismatches=1", "--maxcount=5"], ["-f", "-c", "1"]])
def test_minunique_refuses_mismatches_and_maxcount_before_device_work(dicey, tmp_path, extra):
    fa = tmp_path / "g.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGT\n")  # no .fm9 next to it: a check that came later would say so instead
    for flag in ("-u", "--minunique"):
        r = subprocess.run([dicey, "mappability", "-g", str(fa), flag, "-k", "10", *extra], capture_output=True, text=True)
        assert r.returncode == 1
        assert r.stderr == REFUSAL + "\n"
        assert r.stdout == ""


def test_minunique_keeps_the_range_check_of_k_and_reaches_the_index_check(dicey, tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGT\n")
    for k in ("9", "1001"):
        r = subprocess.run([dicey, "mappability", "-g", str(fa), "-u", "-k", k], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == ""
        assert r.stderr == "Error: k-mer length %s outside 10..1000!\n" % k
    for extra in ([], ["-e", "0", "-c", "0"], ["-f"]):
        r = subprocess.run([dicey, "mappability", "-g", str(fa), "-u", "-k", "10", *extra], capture_output=True, text=True)
        assert r.returncode == 1 and "g.fm9" in r.stderr and r.stdout == ""


def test_usage_names_minunique(dicey):
    r = subprocess.run([dicey, "mappability"], capture_output=True, text=True)
    assert r.returncode == 255
    assert "-u [ --minunique ]" in r.stdout and "-e [ --mismatches ] arg (=0)" in r.stdout
    assert "smallest length k" in r.stdout
