"""Minimum unique length with mismatches on a box without a GPU: the two models of tests/min_unique_mm_ref.py against each other and
against the exact models, what the crafted genome of tests/test_gpu_min_unique_mm.py exercises, the probe schedule of
dicey_amd/csrc/probe_schedule.hpp as a program of its own (plain and under the host sanitizers), the new structs, and the argument
checks of dg_min_unique_mm and of `dicey mappability -u -w` that come before any device work."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import min_unique_mm_ref as W
import min_unique_ref as U
from conftest import genome_text, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")
CRAFTED = W.crafted_seqs()


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
def tiny():
    """an N run, a near-copy (two substitutions), an inverted near-copy (one), a short sequence and an IUPAC letter"""
    a = "ACGTTGCAAGGCTTAACGTAGGCTAGCTAACGGATCGGATCAATTGGCCAGT"
    b = a[:12] + "A" + a[13:30] + "T" + a[31:]
    c = revcomp(a[5:45])
    c = c[:20] + ("A" if c[20] != "A" else "C") + c[21:]
    return genome_text([a + "GATTACA" + "NNNNN" + b + "C", "TTGACC" + c + "R" + a[8:30], "ACGTAC", a[30:]])


@pytest.mark.parametrize("forward_only", [False, True])
@pytest.mark.parametrize("e", [0, 1, 2])
def test_the_two_models_agree(tiny, e, forward_only):
    a = W.sweep(tiny, 32, e, forward_only)
    b = W.pairwise(tiny, 32, e, forward_only)
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, (bad[:10], a[bad[:10]], b[bad[:10]])
    run = U.run_lengths(tiny)
    assert not a[run == 0].any() and (a[a > 0] <= run[a > 0]).all() and a.max() <= 32
    assert (a > 0).sum() >= 20 and ((a == 0) & (run > 0)).sum() >= 20  # lengths and positions without one
    if e == 0:
        assert (b == U.by_values(tiny, 32, forward_only)).all()
    else:
        below = W.pairwise(tiny, 32, e - 1, forward_only)
        assert ((b == 0) | (b >= below)).all() and not b[below == 0].any() and (b > below).sum() >= 10
    for max_k in (10, 17):  # a smaller max_k is the same answer cut earlier
        c = W.pairwise(tiny, max_k, e, forward_only)
        assert (c == np.where(b <= max_k, b, 0)).all() and (c == W.sweep(tiny, max_k, e, forward_only)).all()


def test_pairwise_is_the_exact_model_at_e0_on_the_crafted_genome():
    text = genome_text(CRAFTED["seqs"])
    assert 4500 <= len(text) <= 8000
    for fo in (False, True):
        assert (W.pairwise(text, 40, 0, fo) == U.by_values(text, 40, fo)).all()


def test_the_crafted_genome_exercises_every_case():
    """the figures tests/test_gpu_min_unique_mm.py relies on, from the reference alone, at the largest max_k it runs"""
    text = genome_text(CRAFTED["seqs"])
    assert W.coverage(text, 64, 1) == {"raised": 4728, "became_zero": 96, "reverse_raises": 1208, "reverse_zeroes": 6}
    assert W.coverage(text, 64, 2) == {"raised": 3607, "became_zero": 1073, "reverse_raises": 1210, "reverse_zeroes": 3}
    # the partial near-copies: bases 0..69 of the stretch run into an N run with one substitution, bases 20..99 into a sequence end with
    # two.  Two mismatches alone would keep those pairs together up to the limit; the partner goes invalid first, so the original is
    # unique one base behind the partner's end
    p0 = text.find(CRAFTED["stretch"].encode())
    m2 = W.pairwise(text, 64, 2).astype(np.int64)
    assert (m2[p0 + 7:p0 + 18] == 71 - np.arange(7, 18)).all() and (m2[p0 + 37:p0 + 80] == 101 - np.arange(37, 80)).all()
    assert not m2[p0:p0 + 7].any() and not m2[p0 + 20:p0 + 37].any()
    # a k-mer within e of its own reverse complement counts itself on the other strand: never unique at that length on both strands
    for name, e in (("pal", 0), ("pal1", 2), ("odd", 1)):
        w = CRAFTED[name]
        assert sum(x != y for x, y in zip(w, revcomp(w))) == e
        p = text.find(w.encode())
        both, fwd = int(W.pairwise(text, 64, e)[p]), int(W.pairwise(text, 64, e, True)[p])
        assert both == 0 or both > len(w), (name, both, fwd)
        if name != "pal1":  # (whose own strand holds the unchanged palindrome, one mismatch away)
            assert 0 < fwd <= len(w), (name, both, fwd)


def test_probe_schedule_program(tmp_path):
    """probe_schedule.hpp for the host: every bracket of up to 200 lengths and every threshold, within the schedule's own probe bound;
    the same program again with the address and undefined-behaviour sanitizers"""
    src = os.path.join(ROOT, "tests", "host", "probe_schedule_main.cpp")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("probe_schedule_" + name))
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, r.stdout, r.stderr)
        assert re.fullmatch(r"ok 81200 cases, \d+ probes, worst 15\n", r.stdout), r.stdout


def test_struct_sizes_match_the_header():
    from dicey_amd import _capi
    assert ctypes.sizeof(_capi.MinUniqueMmParams) == 20
    assert [f for f, _ in _capi.MinUniqueMmParams._fields_] == ["max_k", "mismatches", "forward_only", "flags", "reserved"]
    assert ctypes.sizeof(_capi.MuMmStats) == 56
    assert [f for f, _ in _capi.MuMmStats._fields_] == ["candidates", "probes", "steps", "table_reads", "verified_rows", "launches", "ms_search"]
    hdr = open(os.path.join(ROOT, "include", "dicey_gpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} dg_mu_mm_stats_t;", hdr).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in _capi.MuMmStats._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} dg_min_unique_mm_params;", hdr).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in _capi.MinUniqueMmParams._fields_]


def test_entry_point_check_order(lib):
    from dicey_amd import _capi
    DG_EINVAL, DG_ELIMIT = -1, -7
    P = _capi.MinUniqueMmParams

    def call(prm, ix=None):
        m = ctypes.c_void_p(1234)
        rc = lib.dg_min_unique_mm(ix, ctypes.byref(prm) if prm is not None else None, ctypes.byref(m))
        assert not m.value  # cleared on every failure
        return rc

    for e in (0, 1, 2):
        assert call(P(40, e, 0, 0, 0)) == DG_EINVAL  # null handle
        assert b"dg_min_unique_mm" in lib.dg_last_error()
    assert call(None) == DG_EINVAL
    assert lib.dg_min_unique_mm(None, ctypes.byref(P(40, 1, 0, 0, 0)), None) == DG_EINVAL
    assert call(P(40, 1, 0, 1, 0)) == DG_EINVAL  # flags
    assert call(P(40, 1, 0, 0, 1)) == DG_EINVAL  # reserved
    # the parameter block is checked before the handle: values out of range are refused as a limit ...
    for bad in (9, 1001, 0, 0xFFFFFFFF):
        assert call(P(bad, 1, 0, 0, 0)) == DG_ELIMIT
        assert b"outside 10..1000" in lib.dg_last_error()
    for bad in (3, 0xFFFFFFFF):
        assert call(P(40, bad, 0, 0, 0)) == DG_ELIMIT
        assert b"outside 0..2" in lib.dg_last_error()
    for good in (10, 1000):
        assert call(P(good, 2, 1, 0, 0)) == DG_EINVAL
    # ... and flags come before the ranges
    assert call(P(9, 3, 0, 1, 0)) == DG_EINVAL
    assert call(P(1001, 0, 0, 0, 7)) == DG_EINVAL
    st = _capi.MuMmStats()
    assert lib.dg_map_mu_mm_stats(None, ctypes.byref(st)) == DG_EINVAL and lib.dg_map_mu_mm_stats(ctypes.c_void_p(8), None) == DG_EINVAL


def _run(dicey, fa, *args):
    return subprocess.run([dicey, "mappability", "-g", str(fa), *args], capture_output=True, text=True)


def test_within_is_refused_before_device_work(dicey, tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGT\n")  # no .fm9 next to it: a check that came later would say so instead
    for args in (["-w", "1"], ["--within", "0"], ["--within=2", "-k", "20"], ["-w", "1", "-e", "1"]):
        r = _run(dicey, fa, *args)
        assert (r.returncode, r.stderr, r.stdout) == (1, "Error: --within needs --minunique!\n", "")
    for v in ("3", "-1", "17"):
        for flag in ("-u", "--minunique"):
            r = _run(dicey, fa, flag, "-k", "10", "-w", v)
            assert (r.returncode, r.stderr, r.stdout) == (1, "Error: within %s outside 0..2!\n" % v, "")
    # the existing refusals keep their text and come first
    r = _run(dicey, fa, "-u", "-w", "1", "-e", "1")
    assert (r.returncode, r.stderr) == (1, "Error: --minunique cannot be combined with --mismatches or --maxcount!\n")
    r = _run(dicey, fa, "-u", "-w", "1", "-k", "9")
    assert (r.returncode, r.stderr) == (1, "Error: k-mer length 9 outside 10..1000!\n")
    r = _run(dicey, fa, "-u", "-w", "1", "-q", str(fa))
    assert (r.returncode, r.stderr) == (1, "Error: --minunique cannot be combined with --query!\n")
    r = _run(dicey, fa, "-u", "-w", "5", "-q", str(fa), "-I")
    assert (r.returncode, r.stderr) == (1, "Error: --minunique cannot be combined with --query!\n")
    # a good -w reaches the index check
    for v in ("0", "1", "2"):
        r = _run(dicey, fa, "-u", "-k", "10", "-w", v, "-f")
        assert r.returncode == 1 and "g.fm9" in r.stderr and r.stdout == ""


def test_usage_names_within(dicey):
    r = subprocess.run([dicey, "mappability"], capture_output=True, text=True)
    assert r.returncode == 255
    assert "  -w [ --within ] arg (=0)           with -u:" in r.stdout and "With -u -w 1 or -w 2" in r.stdout
    # every line that was there stays
    for line in ("-u [ --minunique ]                 write the minimum unique length instead; -k is then the largest length tried",
                 "-e [ --mismatches ] arg (=0)       count k-mers with up to this many mismatches (0..2)",
                 "-D [ --maxdegeneracy ] arg (=256)  with -I:", "With -u the value of a position is the smallest length k"):
        assert line in r.stdout
