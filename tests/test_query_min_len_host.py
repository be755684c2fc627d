"""The reference of tests/query_min_len_ref.py checked on the CPU (its two e = 0 routes against each other, the monotonicity of the per-k
values it scans), the refusals and the usage text of `dicey mappability -l`, and dg_query_min_len's check order as far as a machine
without a device shows it: what the GPU tests of the feature compare with is itself checked here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import query_map_ref as Q
import query_min_len_ref as ML
from conftest import genome_text, make_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")
MIN_K, MAX_K = 10, 24


@pytest.fixture(scope="module")
def case():
    """the session genome of conftest.small_genome (the text alone: no index is needed here) and the record set of the GPU tests"""
    seqs = make_genome(101, 3, 30000, iupac=True)
    text = genome_text(seqs)
    recs = ML.record_set(seqs, text, MIN_K, MAX_K)
    qbuf, offs = Q.buffer_of(recs)
    return {"text": text, "recs": recs, "qbuf": qbuf, "offs": offs}


def test_the_record_set_has_every_shape(case):
    recs = case["recs"]
    assert len(recs[0]) == 3000 and b"N" in recs[0] and case["offs"][0] == 0
    lens = [len(r) for r in recs]
    assert {MIN_K, MAX_K, 12, 16, 9, 0, 40}.issubset(lens) and recs[11].islower() and recs[-2] == b"A" * 40
    run = ML.run_lengths(case["qbuf"])
    assert run[case["offs"][-1] + lens[-1] - MIN_K] == MIN_K and case["qbuf"].endswith(b"\n")
    assert 5000 <= len(case["qbuf"]) <= 7000


def test_the_two_exact_routes_agree(case):
    parts = ML.parts_by_k(case["text"], case["qbuf"], range(MIN_K, MAX_K + 1), 0)
    seen = set()
    for t in (0, 1, 2):
        for fo in (False, True):
            a = ML.min_len(parts, case["qbuf"], MIN_K, MAX_K, t, fo)
            b = ML.min_len_dict(case["text"], case["qbuf"], MIN_K, MAX_K, t, fo)
            assert (a == b).all(), (t, fo, np.nonzero(a != b)[0][:10])
            seen |= set(np.unique(a).tolist())
    assert {0, MIN_K, MAX_K, ML.INVALID} <= seen and len(seen) >= 10
    a = ML.min_len(parts, case["qbuf"], 12, 16, 0)
    assert (a == ML.min_len_dict(case["text"], case["qbuf"], 12, 16, 0)).all() and set(np.unique(a).tolist()) <= {0, 12, 13, 14, 15, 16, ML.INVALID}


@pytest.mark.parametrize("e", [0, 1, 2])
def test_the_values_never_rise_with_k(case, e):
    """a condition on the INPUTS of the GPU tests, shown on the brute-force values alone: the scan and a search must agree on them"""
    parts = ML.parts_by_k(case["text"], case["qbuf"], range(MIN_K, MAX_K + 1), e)
    for fo in (False, True):
        assert ML.violations(parts, MIN_K, MAX_K, fo) == 0
    assert sum(int(parts[k][2].sum()) for k in parts) > 50000  # (position, k) pairs looked at


def test_bedgraph_drops_zero_and_invalid_runs():
    I = ML.INVALID
    vals = [np.array([0, 0, 12, 12, I, I, 0, 14], dtype=np.uint32), np.zeros(0, np.uint32), np.array([I, 0], dtype=np.uint32), np.array([10], dtype=np.uint32)]
    assert ML.bedgraph(vals, ["a", "b", "c", "d"]) == b"a\t2\t4\t12\na\t7\t8\t14\nd\t0\t1\t10\n"


# ---- the binary: refusals come before any device work, so they show without a device -----------------------------------------------

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("mlcli")
    fa = d / "g.fa"
    fa.write_text(">chr1\nACGTACGTACGTACGTACGTACGT\n")
    q = d / "q.fa"
    q.write_text(">t\nACGTACGTACGTTTGACGT\n")
    return {"g": str(fa), "q": str(q)}


def _run(*args):
    return subprocess.run([DICEY, "mappability"] + list(args), capture_output=True, text=True)


@pytest.mark.parametrize("args,msg", [
    (["-l"], "Error: --minlength needs --query!"),
    (["-l", "-q", "Q", "-c", "2"], "Error: --minlength cannot be combined with --maxcount!"),
    (["-q", "Q", "-s", "12"], "Error: --shortest and --atmost need --minlength!"),
    (["-q", "Q", "-t", "1"], "Error: --shortest and --atmost need --minlength!"),
    (["-t", "1"], "Error: --shortest and --atmost need --minlength!"),
    (["-l", "-q", "Q", "-k", "20", "-s", "21"], "Error: shortest length 21 above the largest length 20 (-k)!"),
    (["-l", "-q", "Q", "-s", "9"], "Error: shortest length 9 outside 10..1000!"),
    (["-l", "-q", "Q", "-t", "-1"], "Error: atmost -1 outside 0..4294967293!"),
    (["-l", "-q", "Q", "-t", "4294967294"], "Error: atmost 4294967294 outside 0..4294967293!"),
    # the refusals that existed keep their text and come first
    (["-u", "-q", "Q"], "Error: --minunique cannot be combined with --query!"),
    (["-u", "-q", "Q", "-l"], "Error: --minunique cannot be combined with --query!"),
    (["-u", "-l", "-e", "1"], "Error: --minunique cannot be combined with --mismatches or --maxcount!"),
    (["-l", "-q", "Q", "-k", "9"], "Error: k-mer length 9 outside 10..1000!"),
    (["-l", "-q", "Q", "-e", "3"], "Error: number of mismatches 3 outside 0..2!"),
])
def test_refusals(files, args, msg):
    r = _run("-g", files["g"], *[files["q"] if a == "Q" else a for a in args])
    assert r.returncode != 0 and r.stdout == "" and r.stderr.strip() == msg


def test_usage_names_the_new_options():
    r = _run("-?")
    for line in ("  -l [ --minlength ]", "  -s [ --shortest ] arg (=10)", "  -t [ --atmost ] arg (=0)"):
        assert line in r.stdout
    # and every line that was there still is
    for line in ("Usage: dicey mappability [OPTIONS] -g genome.fa.gz [-q targets.fa.gz]", "  -u [ --minunique ]                 write the minimum unique length instead",
                 "  -q [ --query ] arg                 FASTA file of sequences to rate against the genome instead of the genome itself",
                 "  -k [ --kmer ] arg (=100)           k-mer length (10..1000)", "-u cannot be combined with -q."):
        assert line in r.stdout


# ---- the library: the parameter block and the size limit are checked before a device is asked for ----------------------------------

def test_check_order_up_to_the_device():
    from dicey_amd import _capi
    L = _capi.load()
    EINVAL, ENODEV, ELIMIT = -1, -4, -7
    seq = b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT"
    off = (C.c_uint64 * 2)(0, 40)
    vals = (C.c_uint32 * 40)(*([0xABCD1234] * 40))

    def prm(min_k=10, max_k=24, e=0, t=0, flags=0, res=(0, 0)):
        return _capi.QminlenParams(min_k, max_k, e, 0, t, flags, (C.c_uint32 * 2)(*res))

    def call(p, o=off):
        rc = L.dg_query_min_len(None, C.byref(p) if p is not None else None, seq, o, 1, vals, None)
        assert rc != 0 and b"dg_query_min_len" in L.dg_last_error()
        return rc

    assert call(None) == EINVAL and call(prm(flags=1)) == EINVAL and call(prm(res=(1, 0))) == EINVAL and call(prm(res=(0, 1))) == EINVAL
    for p in (prm(min_k=9), prm(max_k=1001), prm(min_k=1001, max_k=1001), prm(min_k=9, max_k=9), prm(min_k=25), prm(e=3), prm(t=0xFFFFFFFE)):
        assert call(p) == ELIMIT
    assert call(prm(min_k=9, flags=1)) == EINVAL  # the block's form before its values
    assert call(prm(), o=(C.c_uint64 * 2)(0, (1 << 31) - 1)) == ELIMIT
    # valid parameters and a null handle: a machine without a device says so, one with a device reports the null handle
    assert call(prm(t=0xFFFFFFFD)) == (EINVAL if L.dg_device_count() > 0 else ENODEV)
    assert list(vals) == [0xABCD1234] * 40
