"""`dicey mappability -q -l -E`: the binary's bedGraph of minimum lengths by end position for the records of a query FASTA against the
writer of tests/query_min_len_end_ref.py (runs of equal lengths at the coordinates of the oligo's last base; no line where there is no
length), plain and gzipped, with and without -a and -f; every refusal of the new option, and `-l -a` without `-E` still refused with the
text it had."""
import gzip
import os
import random
import subprocess

import pytest

import query_map_ref as Q
import query_min_len_end_ref as ME
import query_min_len_ref as ML
from conftest import revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")


def _records(seqs):
    """a cut with every eleventh base substituted next to a junction, a lower-case record with a description in its header (the binary
    upper-cases it) that is a cut of the other strand with every 23rd base substituted, random sequence with an N, and a cut of exactly
    the smallest length: lengths, zero runs and invalid stretches"""
    rng = random.Random(3)
    s1, s2, _ = seqs
    clean = lambda s, a, m: next(x for x in range(a, len(s) - m) if set(s[x:x + m]) <= set("ACGT"))
    a, b = clean(s1, 3000, 300), clean(s2, 8000, 200)

    def subst(s, first, every):
        s = list(s)
        for i in range(first, len(s), every):
            s[i] = "ACGT"[("ACGT".index(s[i]) + 1) % 4]
        return "".join(s)

    return [("tx1", "", subst(s1[a:a + 300], 8, 11) + s2[b:b + 60]), ("low", " a lower-case record", revcomp(subst(s2[b:b + 200], 5, 23)).lower()),
            ("rnd", "\tx=1", "".join(rng.choice("ACGT") for _ in range(90)) + "N" + "".join(rng.choice("ACGT") for _ in range(60))),
            ("ten", "", s1[a:a + 10])]


@pytest.fixture(scope="module")
def indexed(small_genome, tmp_path_factory):
    g = small_genome
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("mlecli")
    fa = d / "session.fa.gz"
    with gzip.open(fa, "wt") as f:
        for n, s in zip(g["names"], g["seqs"]):
            f.write(">" + n + "\n")
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    r = subprocess.run([DICEY, "index", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    recs = _records(g["seqs"])
    q = d / "targets.fa"
    with open(q, "w") as f:
        for name, desc, s in recs:
            f.write(">" + name + desc + "\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    qgz = d / "targets.fa.gz"
    qgz.write_bytes(gzip.compress(q.read_bytes()))
    return {"fa": str(fa), "q": str(q), "qgz": str(qgz), "names": [r[0] for r in recs], "recs": [r[2].upper().encode() for r in recs], "dir": d}


def _expected(text, recs, names, lo, hi, e, a, t, fo):
    qbuf, _ = Q.buffer_of(recs)
    parts = ME.parts_by_k(text, qbuf, range(lo, hi + 1), e, (a,))
    return ME.bedgraph(ME.split(ME.min_len_end(parts, qbuf, lo, hi, a, t, fo), recs), names)


@pytest.mark.parametrize("args,lo,hi,e,a,t,fo", [
    (["-k", "24"], 10, 24, 0, 0, 0, False),
    (["-k", "24", "-e", "1", "-a", "5"], 10, 24, 1, 5, 0, False),
    (["-k", "20", "-s", "12", "-t", "1", "-e", "1", "-f"], 12, 20, 1, 0, 1, True),
    (["-k", "20", "-s", "12", "-e", "2", "--anchor", "7", "-f"], 12, 20, 2, 7, 0, True)])
def test_bedgraph_of_minimum_lengths_by_end(small_genome, indexed, args, lo, hi, e, a, t, fo):
    exp = _expected(small_genome["text"], indexed["recs"], indexed["names"], lo, hi, e, a, t, fo)
    lines = exp.splitlines()
    # the expectation itself: several lengths, lines for the records that have some, none with 0 or the invalid mark, none in front of
    # the first base at which an oligo of the smallest length ends
    vals = {int(l.split(b"\t")[3]) for l in lines}
    assert len(vals) >= 3 and min(vals) >= lo and max(vals) <= hi and len({l.split(b"\t")[0] for l in lines}) >= 3 and len(lines) >= 10
    first = min(int(l.split(b"\t")[1]) for l in lines)
    assert first >= lo - 1 and (e > 0 or first == lo - 1)
    # and it is not what -l without -E writes for the same records
    by_start = ML.bedgraph(ML.split(ML.min_len(ML.parts_by_k(small_genome["text"], Q.buffer_of(indexed["recs"])[0], range(lo, hi + 1), e),
                                               Q.buffer_of(indexed["recs"])[0], lo, hi, t, fo), indexed["recs"]), indexed["names"])
    assert by_start != exp
    base = [DICEY, "mappability", "-g", indexed["fa"], "-l", "-E"] + args
    r = subprocess.run(base + ["-q", indexed["q"]], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp
    out = indexed["dir"] / ("out%d%d%d.gz" % (e, a, t))
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"], "--minlength", "--byend"] + args + ["--query", indexed["qgz"], "-o", str(out)],
                       capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert gzip.decompress(out.read_bytes()) == exp


@pytest.mark.parametrize("args,msg", [
    (["-E"], "Error: --byend needs --minlength!"),
    (["-q", "Q", "--byend", "-a", "5"], "Error: --byend needs --minlength!"),
    (["-q", "Q", "-l", "-E", "-a", "11"], "Error: anchor 11 above the shortest length 10 (-s)!"),
    (["-q", "Q", "-l", "-E", "-s", "12", "-k", "20", "-a", "13"], "Error: anchor 13 above the shortest length 12 (-s)!"),
    # the refusal of -l -a without -E keeps its text
    (["-q", "Q", "-l", "-a", "5"], "Error: --anchor cannot be combined with --minlength!"),
    (["-q", "Q", "--minlength", "--anchor", "0"], "Error: --anchor cannot be combined with --minlength!"),
])
def test_refusals_with_an_index_at_hand(indexed, args, msg):
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"]] + [indexed["q"] if x == "Q" else x for x in args], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout == "" and r.stderr.strip() == msg
