"""The reference of tests/query_min_len_end_ref.py checked on the CPU: by END position the anchored values never rise with k (while by
start position, on the same records, they do: the contrast that makes `dicey mappability -l` take `-a` only with `-E`), its two routes
against each other, the monotonicity in the anchor, the orientation pinned by hand with literal strings; the refusals and the usage text of
`dicey mappability -E`, and dg_query_min_len_end's check order as far as a machine without a device shows it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import query_anchor_ref as A
import query_map_ref as Q
import query_min_len_end_ref as ME
from conftest import genome_text, make_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")
MIN_K, MAX_K = 10, 24
INV = ME.INVALID
ANCHORS = tuple(range(MIN_K + 1)) + (12,)  # one brute-force pass per (k, e) serves every test of this module

# the orientation table: X occurs once in the text (forward strand) and nothing else is near it
X = "GATTACAGGCTTCAAGTCCA"
RC_X = "TGGACTTGAAGCCTGTAATC"
ORIENT_TEXT = ("TTTTTTTTTTTTTTTTTTTTTTTTT" + X + "TTTTTTTTTTTTTTTTTTTTTTTTT\n").encode()
ORIENT = [("GATTACAGGCTTCAAGTCCC", 10, 10),   # X with its last base changed: no anchored place at any length
          ("CATTACAGGCTTCAAGTCCA", 0, 10),    # X with its first base changed: one place at every length, the changed base is a mismatch
          ("TGGACTTGAAGCCTGTAATG", 10, 10),   # revcomp(X) with its last base changed
          ("AGGACTTGAAGCCTGTAATC", 0, 10)]    # revcomp(X) with its first base changed


@pytest.fixture(scope="module")
def case():
    """the session genome of conftest.small_genome (the text alone: no index is needed here) and the record set of the GPU tests"""
    seqs = make_genome(101, 3, 30000, iupac=True)
    text = genome_text(seqs)
    recs = ME.record_set(seqs, MIN_K, MAX_K)
    qbuf, offs = Q.buffer_of(recs)
    return {"text": text, "seqs": seqs, "recs": recs, "qbuf": qbuf, "offs": offs}


def _parts(case, e):
    return ME.parts_by_k(case["text"], case["qbuf"], range(MIN_K, MAX_K + 1), e, ANCHORS)


def test_the_record_set_has_every_shape(case):
    recs, offs, qbuf = case["recs"], case["offs"], case["qbuf"]
    base = A.record_set(case["seqs"])
    assert recs[:len(base) - 1] == base[:-1] and recs[-1] == base[-1] and len(recs) == len(base) + 3
    brun = ME.brun_lengths(qbuf)
    # the first record: buffer offset 0, starts with A/C/G/T, longer than max_k: its runs end at the buffer's start, not at a '\n'
    assert offs[0] == 0 and len(recs[0]) > MAX_K and [int(x) for x in brun[:40]] == list(range(1, 41))
    lens = [len(r) for r in recs]
    assert lens[-4] == MIN_K and {12, 16, 20, 9, 0} <= set(lens) and int(brun[offs[-4] + MIN_K - 1]) == MIN_K
    # a run that fills one bitmap word: its first base at bit 0, its last at bit 63, neither A/C/G/T on either side
    word = [p for p in range(63, len(qbuf), 64) if brun[p] == 64]
    assert any(offs[-3] <= p < offs[-3] + lens[-3] and brun[p + 1] == 0 for p in word)
    # a run of 200 that starts at bit 40: its last bases look back over more than three words
    p = offs[-2] + lens[-2] - 1
    assert brun[p] == 200 and (p - 199) % 64 == 40 and p // 64 - (p - 199) // 64 == 3
    assert qbuf.endswith(b"\n") and brun[len(qbuf) - 2] >= MAX_K  # the last record's final base ends a run


@pytest.mark.parametrize("e,a", [(0, 0), (1, 1), (1, 5), (2, 5)])
def test_by_end_the_values_never_rise_with_k(case, e, a):
    """a condition on the INPUTS of the GPU tests, shown on the brute-force values alone: the scan and a search must agree on them"""
    parts = _parts(case, e)
    for fo in (False, True):
        assert ME.violations_by_end(parts, MIN_K, MAX_K, a, fo) == 0, (e, a, fo)
    assert sum(int(parts[k][a][2].sum()) for k in parts) > 50000  # (position, k) pairs looked at


def test_by_start_they_do_rise_on_the_same_records(case):
    """what tests/test_query_anchor_host.py shows on its records holds on these: the anchored count of the k-mer that STARTS at p rises
    somewhere with k, so a search by start position cannot take an anchor, and the by-end entry point is not a renamed by-start one"""
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


@pytest.mark.parametrize("lo,hi", [(12, 14), (18, 20)])
def test_ball_equals_diagonal(case, lo, hi):
    """on the first 9 kb of the genome and records cut from them (the diagonal costs |Q| * |T|)"""
    text = case["text"][:9000] + b"\n"
    t = text.decode()
    c, d = A._clean(t, 2000, 300), A._clean(t, 5000, 300)
    recs = [A._subst_every(t[c:c + 300], 11), A._revcomp(A._subst_every(t[d:d + 300], 23)), t[c:c + lo], t[c:c + 9], "", t[d:d + 40].lower()]
    qbuf, _ = Q.buffer_of([r.encode() for r in recs])
    anchors = (0, 1, 5, lo)
    for e in (1, 2):
        ball = ME.parts_by_k(text, qbuf, range(lo, hi + 1), e, anchors, "ball")
        diag = ME.parts_by_k(text, qbuf, range(lo, hi + 1), e, anchors, "diagonal")
        for a in anchors:
            for k in range(lo, hi + 1):
                for j in (0, 1, 2):
                    assert (ball[k][a][j] == diag[k][a][j]).all(), (k, e, a, j)
            for t_ in (0, 1):
                for fo in (False, True):
                    x, y = (ME.min_len_end(p, qbuf, lo, hi, a, t_, fo) for p in (ball, diag))
                    assert (x == y).all()
        plain = ME.min_len_end(ball, qbuf, lo, hi, 0, 0)
        assert (ME.min_len_end(ball, qbuf, lo, hi, 5, 0) != plain).any(), e  # the anchor matters on these records


@pytest.mark.parametrize("e", [0, 1, 2])
def test_len_never_grows_with_the_anchor(case, e):
    """if len at anchor a is not 0 then len at a + 1 is not 0 and not larger: the counted windows only shrink with a"""
    qbuf = case["qbuf"]
    parts = _parts(case, e)
    shorter = 0
    for t in (0, 1):
        for fo in (False, True):
            prev = ME.min_len_end(parts, qbuf, MIN_K, MAX_K, 0, t, fo)
            for a in range(1, MIN_K + 1):
                cur = ME.min_len_end(parts, qbuf, MIN_K, MAX_K, a, t, fo)
                assert ((prev == INV) == (cur == INV)).all()
                has = (prev != INV) & (prev != 0)
                assert (cur[has] != 0).all() and (cur[has] <= prev[has]).all(), (e, t, fo, a)
                shorter += int((cur[has] < prev[has]).sum())
                prev = cur
    assert e == 0 or shorter > 100  # (at e = 0 every base is exact already)


def test_orientation_pinned_by_hand():
    assert A._revcomp(X) == RC_X and ORIENT_TEXT.count(X.encode()) == 1 and RC_X.encode() not in ORIENT_TEXT
    recs = [w.encode() for w, _, _ in ORIENT]
    qbuf, offs = Q.buffer_of(recs)
    for route in ("ball", "diagonal"):
        parts = ME.parts_by_k(ORIENT_TEXT, qbuf, range(10, 21), 1, (0, 1), route)
        for t, col in ((0, 1), (1, 2)):
            got = ME.min_len_end(parts, qbuf, 10, 20, 1, t)
            assert [int(got[o + 19]) for o in offs] == [row[col] for row in ORIENT], (route, t)
            assert all((got[o:o + 9] == INV).all() and got[o + 9] != INV for o in offs)
        # which strand holds the place: a changed first base of X is found forward, of revcomp(X) on the other strand
        fo = ME.min_len_end(parts, qbuf, 10, 20, 1, 0, True)
        assert [int(fo[o + 19]) for o in offs] == [10, 0, 10, 10]
        # without the anchor all four are one substitution from X at every length
        assert [int(ME.min_len_end(parts, qbuf, 10, 20, 0, 0)[o + 19]) for o in offs] == [0, 0, 0, 0]


def test_bedgraph_is_at_the_last_base_and_drops_zero_and_invalid_runs():
    vals = [np.array([INV, INV, 0, 12, 12, INV, 0, 14], dtype=np.uint32), np.zeros(0, np.uint32), np.array([INV, 0], dtype=np.uint32),
            np.array([10], dtype=np.uint32)]
    assert ME.bedgraph(vals, ["a", "b", "c", "d"]) == b"a\t3\t5\t12\na\t7\t8\t14\nd\t0\t1\t10\n"


# ---- the binary: refusals come before any device work, so they show without a device -----------------------------------------------

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("mlecli")
    fa = d / "g.fa"
    fa.write_text(">chr1\nACGTACGTACGTACGTACGTACGT\n")
    q = d / "q.fa"
    q.write_text(">t\nACGTACGTACGTTTGACGT\n")
    return {"g": str(fa), "q": str(q)}


def _run(*args):
    return subprocess.run([DICEY, "mappability"] + list(args), capture_output=True, text=True)


@pytest.mark.parametrize("args,msg", [
    (["-E"], "Error: --byend needs --minlength!"),
    (["-q", "Q", "--byend"], "Error: --byend needs --minlength!"),
    (["-q", "Q", "-E", "-a", "5"], "Error: --byend needs --minlength!"),
    (["-q", "Q", "-l", "-E", "-a", "11"], "Error: anchor 11 above the shortest length 10 (-s)!"),
    (["-q", "Q", "-l", "--byend", "-s", "12", "-k", "20", "--anchor", "13"], "Error: anchor 13 above the shortest length 12 (-s)!"),
    # the refusals that existed keep their text and come first
    (["-q", "Q", "-l", "-a", "5"], "Error: --anchor cannot be combined with --minlength!"),
    (["-q", "Q", "-l", "-a", "0"], "Error: --anchor cannot be combined with --minlength!"),
    (["-l", "-E"], "Error: --minlength needs --query!"),
    (["-E", "-a", "5"], "Error: --anchor needs --query!"),
    (["-q", "Q", "-l", "-E", "-k", "20", "-a", "21"], "Error: anchor 21 outside 0..20 (-k)!"),
    (["-q", "Q", "-l", "-E", "-a", "-1"], "Error: anchor -1 outside 0..100 (-k)!"),
    (["-q", "Q", "-l", "-E", "-c", "2"], "Error: --minlength cannot be combined with --maxcount!"),
    (["-q", "Q", "-E", "-t", "1"], "Error: --shortest and --atmost need --minlength!"),
    (["-q", "Q", "-l", "-E", "-s", "9"], "Error: shortest length 9 outside 10..1000!"),
    (["-q", "Q", "-l", "-E", "-k", "20", "-s", "21"], "Error: shortest length 21 above the largest length 20 (-k)!"),
    (["-u", "-q", "Q", "-l", "-E"], "Error: --minunique cannot be combined with --query!"),
    (["-q", "Q", "-l", "-E", "-e", "3"], "Error: number of mismatches 3 outside 0..2!"),
])
def test_refusals(files, args, msg):
    r = _run("-g", files["g"], *[files["q"] if a == "Q" else a for a in args])
    assert r.returncode != 0 and r.stdout == "" and r.stderr.strip() == msg


def test_usage_names_the_new_option():
    r = _run("-?")
    assert "  -E [ --byend ]                     with -l: the length of the shortest specific k-mer that ENDS at the position" in r.stdout
    assert "With -q -l -E the value of a position" in r.stdout and "the coordinates of the oligo's LAST base" in r.stdout
    # and every line that was there still is
    for line in ("Usage: dicey mappability [OPTIONS] -g genome.fa.gz [-q targets.fa.gz]", "  -u [ --minunique ]                 write the minimum unique length instead",
                 "  -q [ --query ] arg                 FASTA file of sequences to rate against the genome instead of the genome itself",
                 "  -k [ --kmer ] arg (=100)           k-mer length (10..1000)", "-u cannot be combined with -q.", "  -l [ --minlength ]",
                 "  -s [ --shortest ] arg (=10)", "  -t [ --atmost ] arg (=0)", "  -o [ --outfile ] arg               gzipped output file",
                 "  -a [ --anchor ] arg                with -q: the last arg bases of every k-mer must match exactly", "-a cannot be combined with -l"):
        assert line in r.stdout


# ---- the library: the parameter block and the size limit are checked before a device is asked for ----------------------------------

def test_params_field_list():
    from dicey_amd import _capi
    assert [(n, t) for n, t in _capi.QminlenEndParams._fields_] == [
        ("min_k", C.c_uint32), ("max_k", C.c_uint32), ("mismatches", C.c_uint32), ("anchor", C.c_uint32), ("forward_only", C.c_int32),
        ("at_most", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]
    assert C.sizeof(_capi.QminlenEndParams) == 36 and "dg_query_min_len_end" in _capi.SYMBOLS
    assert _capi.load().dg_abi_version() == 7


def test_check_order_up_to_the_device():
    from dicey_amd import _capi
    L = _capi.load()
    EINVAL, ENODEV, ELIMIT = -1, -4, -7
    seq = b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT"
    off = (C.c_uint64 * 2)(0, 40)
    vals = (C.c_uint32 * 40)(*([0xABCD1234] * 40))

    def prm(min_k=10, max_k=24, e=0, a=5, t=0, flags=0, res=(0, 0)):
        return _capi.QminlenEndParams(min_k, max_k, e, a, 0, t, flags, (C.c_uint32 * 2)(*res))

    def call(p, o=off):
        rc = L.dg_query_min_len_end(None, C.byref(p) if p is not None else None, seq, o, 1, vals, None)
        assert rc != 0 and b"dg_query_min_len_end" in L.dg_last_error()
        return rc

    assert call(None) == EINVAL and call(prm(flags=1)) == EINVAL and call(prm(res=(1, 0))) == EINVAL and call(prm(res=(0, 1))) == EINVAL
    for p in (prm(min_k=9), prm(max_k=1001), prm(min_k=1001, max_k=1001), prm(min_k=9, max_k=9), prm(min_k=25), prm(e=3), prm(t=0xFFFFFFFE),
              prm(a=11), prm(min_k=12, a=13), prm(a=0xFFFFFFFF)):
        assert call(p) == ELIMIT
    assert call(prm(a=24)) == ELIMIT and b"anchor" in L.dg_last_error()  # within max_k is not enough: the anchor is bounded by min_k
    assert call(prm(min_k=9, flags=1)) == EINVAL and call(prm(a=11, res=(0, 1))) == EINVAL  # the block's form before its values
    assert call(prm(), o=(C.c_uint64 * 2)(0, (1 << 31) - 1)) == ELIMIT
    # valid parameters and a null handle: a machine without a device says so, one with a device reports the null handle
    for p in (prm(), prm(a=0), prm(a=10), prm(min_k=1000, max_k=1000, a=1000, e=2, t=0xFFFFFFFD)):
        assert call(p) == (EINVAL if L.dg_device_count() > 0 else ENODEV)
    assert list(vals) == [0xABCD1234] * 40
