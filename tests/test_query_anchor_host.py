"""The reference of tests/query_anchor_ref.py checked on the CPU (its two methods against each other and against query_map_ref at a = 0
and a = k, the monotonicity in a, the orientation pinned by hand with literal strings, and the NON-monotonicity in k that makes
`dicey mappability -l` refuse `-a`), the refusals and the usage text of `dicey mappability -a`, and dg_query_map_anchored's check order as
far as a machine without a device shows it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import query_anchor_ref as A
import query_map_ref as Q
from conftest import genome_text, make_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")

# the orientation table: X occurs once in the text (forward strand) and nothing else is near it
X = "GATTACAGGCTTCAAGTCCA"
RC_X = "TGGACTTGAAGCCTGTAATC"
ORIENT_TEXT = ("TTTTTTTTTTTTTTTTTTTTTTTTT" + X + "TTTTTTTTTTTTTTTTTTTTTTTTT\n").encode()
ORIENT = [("GATTACAGGCTTCAAGTCCC", 0),   # X with its last base changed
          ("CATTACAGGCTTCAAGTCCA", 1),   # X with its first base changed
          ("TGGACTTGAAGCCTGTAATG", 0),   # revcomp(X) with its last base changed
          ("AGGACTTGAAGCCTGTAATC", 1)]   # revcomp(X) with its first base changed


@pytest.fixture(scope="module")
def case():
    """the session genome of conftest.small_genome (the text alone: no index is needed here) and the record set of the GPU tests"""
    seqs = make_genome(101, 3, 30000, iupac=True)
    text = genome_text(seqs)
    recs = A.record_set(seqs)
    qbuf, offs = Q.buffer_of(recs)
    return {"text": text, "recs": recs, "qbuf": qbuf, "offs": offs}


def test_the_record_set_has_every_shape(case):
    recs = case["recs"]
    lens = [len(r) for r in recs]
    assert lens[0] == 3000 and b"N" in recs[0] and case["offs"][0] == 0
    assert lens[1:8] == [600, 800, 400, 600, 400, 120, 500] and lens[8:13] == [12, 16, 20, 9, 0] and recs[13].islower()
    assert Q.values(case["text"], recs, 20, 0)[-1][lens[-1] - 20] != Q.INVALID  # the final window of the last record is valid


@pytest.mark.parametrize("k", [12, 16, 20])
def test_ball_equals_diagonal(case, k):
    """on the first 9 kb of the genome and records cut from them (the diagonal costs |Q| * |T|)"""
    text = case["text"][:9000] + b"\n"
    t = text.decode()
    c, d = A._clean(t, 2000, 300), A._clean(t, 5000, 300)
    recs = [A._subst_every(t[c:c + 300], 11), A._revcomp(A._subst_every(t[d:d + 300], 23)), t[c:c + k], t[c:c + 9], "", t[d:d + 40].lower()]
    qbuf, _ = Q.buffer_of([r.encode() for r in recs])
    anchors = sorted({0, 1, 5, 9, k - 1, k})
    diag = A.parts_diagonal(text, qbuf, k, (1, 2), anchors)
    for e in (1, 2):
        ball = A.parts_ball(text, qbuf, k, e, anchors)
        differ = 0
        for a in anchors:
            for j in (0, 1, 2):
                assert (ball[a][j] == diag[e, a][j]).all(), (k, e, a, j)
            differ += int((ball[a][0] != ball[0][0]).sum() + (ball[a][1] != ball[0][1]).sum())
        assert differ > 100, (k, e)  # the anchor matters on these records, on either strand
        assert (ball[k - 1][0] != ball[0][0]).any() and (ball[k - 1][1] != ball[0][1]).any()


@pytest.mark.parametrize("k", [12, 16, 20])
def test_anchor_0_and_k_and_monotone_in_a(case, k):
    text, qbuf = case["text"], case["qbuf"]
    exact = Q.parts_ball(text, qbuf, k, 0)
    for e in (0, 1, 2):
        parts = A.parts_ball(text, qbuf, k, e, list(range(k + 1)))
        plain = Q.parts_ball(text, qbuf, k, e)
        for j in (0, 1, 2):
            assert (parts[0][j] == plain[j]).all() and (parts[k][j] == exact[j]).all(), (k, e, j)
        for a in range(k):
            assert (parts[a + 1][0] <= parts[a][0]).all() and (parts[a + 1][1] <= parts[a][1]).all(), (k, e, a)


def test_orientation_pinned_by_hand():
    assert A._revcomp(X) == RC_X and ORIENT_TEXT.count(X.encode()) == 1 and RC_X.encode() not in ORIENT_TEXT
    recs = [w.encode() for w, _ in ORIENT]
    qbuf, offs = Q.buffer_of(recs)
    ball = A.parts_ball(ORIENT_TEXT, qbuf, 20, 1, [0, 1])
    diag = A.parts_diagonal(ORIENT_TEXT, qbuf, 20, (1,), [0, 1])
    for parts in (ball[1], diag[1, 1]):
        assert [int(parts[0][o] + parts[1][o]) for o in offs] == [v for _, v in ORIENT]
    # which strand holds the 1s: a changed first base of X is found forward, of revcomp(X) on the other strand
    assert [int(ball[1][0][o]) for o in offs] == [0, 1, 0, 0] and [int(ball[1][1][o]) for o in offs] == [0, 0, 0, 1]
    # without the anchor all four are one substitution from X
    assert [int(ball[0][0][o] + ball[0][1][o]) for o in offs] == [1, 1, 1, 1]


def test_values_rise_with_k(case):
    """Anchored values are NOT monotone in k for an oligo that grows at its 3' end: a site whose only mismatch is at offset k-1 is rejected
    at length k (a = 1) and accepted at k+1.  A scan for the smallest specific k could not stop at the first hit, which is why -l refuses -a."""
    text, qbuf = case["text"], case["qbuf"]
    for e, a, ks in ((1, 1, range(12, 21)), (1, 5, range(12, 21)), (2, 5, range(12, 15))):
        prev, rises = None, 0
        for k in ks:
            f, r, v = A.parts_ball(text, qbuf, k, e, [a])[a]
            if prev is not None:
                both = v & prev[1]
                rises += int(((f + r)[both] > prev[0][both]).sum())
            prev = (f + r, v)
        assert rises > 0, (e, a)
    # and the unanchored values never do
    prev = None
    for k in range(12, 21):
        f, r, v = Q.parts_ball(text, qbuf, k, 1)
        if prev is not None:
            assert ((f + r)[v & prev[1]] <= prev[0][v & prev[1]]).all()
        prev = (f + r, v)


def test_table_reads_formula():
    assert A.table_reads(20, 2, 0, 16, False) == 2 * (1 + 3 * 16 + 9 * 16 * 15 // 2)
    assert A.table_reads(20, 2, 16, 16, True) == 1 and A.table_reads(20, 2, 20, 16, False) == 2
    assert A.table_reads(20, 1, 5, 16, False) == (1 + 3 * 11) + (1 + 3 * 15) and A.table_reads(12, 2, 5, 16, False) == 0
    assert A.table_reads(20, 0, 5, 16, False) == 2


# ---- the binary: refusals come before any device work, so they show without a device -----------------------------------------------

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("anchcli")
    fa = d / "g.fa"
    fa.write_text(">chr1\nACGTACGTACGTACGTACGTACGT\n")
    q = d / "q.fa"
    q.write_text(">t\nACGTACGTACGTTTGACGT\n")
    return {"g": str(fa), "q": str(q)}


def _run(*args):
    return subprocess.run([DICEY, "mappability"] + list(args), capture_output=True, text=True)


@pytest.mark.parametrize("args,msg", [
    (["-a", "5"], "Error: --anchor needs --query!"),
    (["-a", "5", "-u"], "Error: --anchor needs --query!"),
    (["-q", "Q", "-l", "-a", "5"], "Error: --anchor cannot be combined with --minlength!"),
    (["-q", "Q", "-l", "--anchor", "0"], "Error: --anchor cannot be combined with --minlength!"),
    (["-q", "Q", "-k", "20", "-a", "21"], "Error: anchor 21 outside 0..20 (-k)!"),
    (["-q", "Q", "-k", "20", "-a", "-1"], "Error: anchor -1 outside 0..20 (-k)!"),
    (["-q", "Q", "-a", "101"], "Error: anchor 101 outside 0..100 (-k)!"),
    # the refusals that existed keep their text and come first
    (["-u", "-q", "Q", "-a", "5"], "Error: --minunique cannot be combined with --query!"),
    (["-l", "-a", "5"], "Error: --minlength needs --query!"),
    (["-q", "Q", "-a", "5", "-t", "1"], "Error: --shortest and --atmost need --minlength!"),
    (["-q", "Q", "-a", "5", "-k", "9"], "Error: k-mer length 9 outside 10..1000!"),
    (["-q", "Q", "-a", "5", "-e", "3"], "Error: number of mismatches 3 outside 0..2!"),
])
def test_refusals(files, args, msg):
    r = _run("-g", files["g"], *[files["q"] if a == "Q" else a for a in args])
    assert r.returncode != 0 and r.stdout == "" and r.stderr.strip() == msg


def test_usage_names_the_new_option():
    r = _run("-?")
    assert "  -a [ --anchor ] arg                with -q: the last arg bases of every k-mer must match exactly" in r.stdout
    assert "-a cannot be combined with -l" in r.stdout
    # and every line that was there still is
    for line in ("Usage: dicey mappability [OPTIONS] -g genome.fa.gz [-q targets.fa.gz]", "  -u [ --minunique ]                 write the minimum unique length instead",
                 "  -q [ --query ] arg                 FASTA file of sequences to rate against the genome instead of the genome itself",
                 "  -k [ --kmer ] arg (=100)           k-mer length (10..1000)", "-u cannot be combined with -q.", "  -l [ --minlength ]",
                 "  -s [ --shortest ] arg (=10)", "  -t [ --atmost ] arg (=0)", "  -o [ --outfile ] arg               gzipped output file"):
        assert line in r.stdout


# ---- the library: the parameter block and the size limit are checked before a device is asked for ----------------------------------

def test_params_field_list():
    from dicey_amd import _capi
    assert [(n, t) for n, t in _capi.QmapAnchorParams._fields_] == [
        ("k", C.c_uint32), ("mismatches", C.c_uint32), ("anchor", C.c_uint32), ("forward_only", C.c_int32), ("max_count", C.c_uint32),
        ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]
    assert C.sizeof(_capi.QmapAnchorParams) == 32 and "dg_query_map_anchored" in _capi.SYMBOLS
    assert _capi.load().dg_abi_version() == 7


def test_check_order_up_to_the_device():
    from dicey_amd import _capi
    L = _capi.load()
    EINVAL, ENODEV, ELIMIT = -1, -4, -7
    seq = b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT"
    off = (C.c_uint64 * 2)(0, 40)
    vals = (C.c_uint32 * 40)(*([0xABCD1234] * 40))

    def prm(k=20, e=0, a=5, flags=0, res=(0, 0)):
        return _capi.QmapAnchorParams(k, e, a, 0, 0, flags, (C.c_uint32 * 2)(*res))

    def call(p, o=off):
        rc = L.dg_query_map_anchored(None, C.byref(p) if p is not None else None, seq, o, 1, vals, None)
        assert rc != 0 and b"dg_query_map_anchored" in L.dg_last_error()
        return rc

    assert call(None) == EINVAL and call(prm(flags=1)) == EINVAL and call(prm(res=(1, 0))) == EINVAL and call(prm(res=(0, 1))) == EINVAL
    for p in (prm(k=9), prm(k=1001), prm(e=3), prm(a=21), prm(k=10, a=11), prm(a=0xFFFFFFFF)):
        assert call(p) == ELIMIT
    assert call(prm(k=9, flags=1)) == EINVAL and call(prm(a=21, res=(0, 1))) == EINVAL  # the block's form before its values
    assert call(prm(), o=(C.c_uint64 * 2)(0, (1 << 31) - 1)) == ELIMIT
    # valid parameters and a null handle: a machine without a device says so, one with a device reports the null handle
    for p in (prm(), prm(a=0), prm(a=20), prm(k=1000, a=1000, e=2)):
        assert call(p) == (EINVAL if L.dg_device_count() > 0 else ENODEV)
    assert list(vals) == [0xABCD1234] * 40
