"""`dicey mappability -q -a`: the binary's bedGraph of anchored counts for the records of a query FASTA against the values of
tests/query_anchor_ref.py written by query_map_ref.bedgraph, plain and gzipped; `-a 0` byte for byte what `-q` alone writes; and -f, -c
and -e 2 with the anchor."""
import gzip
import os
import random
import subprocess

import pytest

import query_anchor_ref as A
import query_map_ref as Q
from conftest import revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")


@pytest.fixture(scope="module")
def indexed(small_genome, tmp_path_factory):
    g = small_genome
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("anchcli")
    fa = d / "session.fa.gz"
    with gzip.open(fa, "wt") as f:
        for n, s in zip(g["names"], g["seqs"]):
            f.write(">" + n + "\n")
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    r = subprocess.run([DICEY, "index", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # a cut with a substitution every 11 nt next to a junction, the other strand of a cut with one every 23 as a lower-case record with a
    # description in its header (the binary upper-cases it), random sequence with an N, and a record of exactly k
    rng = random.Random(3)
    s1, s2, _ = g["seqs"]
    a, b, c = A._clean(s1, 3000, 300), A._clean(s2, 8000, 300), A._clean(s2, 14000, 20)
    recs = [("tx1", "", A._subst_every(s1[a:a + 300], 11) + s2[b:b + 60]), ("low", " a lower-case record", revcomp(A._subst_every(s2[b:b + 300], 23)).lower()),
            ("rnd", "\tx=1", "".join(rng.choice("ACGT") for _ in range(90)) + "N" + "".join(rng.choice("ACGT") for _ in range(60))),
            ("k20", "", s2[c:c + 20])]
    q = d / "targets.fa"
    with open(q, "w") as f:
        for name, desc, s in recs:
            f.write(">" + name + desc + "\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    qgz = d / "targets.fa.gz"
    qgz.write_bytes(gzip.compress(q.read_bytes()))
    return {"fa": str(fa), "q": str(q), "qgz": str(qgz), "names": [r[0] for r in recs], "recs": [r[2].upper().encode() for r in recs], "dir": d}


def _expected(text, ind, k, e, a, fo=False, cap=0):
    qbuf, _ = Q.buffer_of(ind["recs"])
    return Q.bedgraph(Q.split(Q.finish(*A.parts_ball(text, qbuf, k, e, [a])[a], fo, cap), ind["recs"]), ind["names"])


def test_bedgraph_of_anchored_counts(small_genome, indexed):
    exp = _expected(small_genome["text"], indexed, 20, 1, 5)
    plain = Q.bedgraph(Q.values(small_genome["text"], indexed["recs"], 20, 1), indexed["names"])
    exact = Q.bedgraph(Q.values(small_genome["text"], indexed["recs"], 20, 0), indexed["names"])
    assert exp != plain and exp != exact and len(exp.splitlines()) >= 20 and len({l.split(b"\t")[0] for l in exp.splitlines()}) == 4
    base = [DICEY, "mappability", "-g", indexed["fa"], "-k", "20", "-e", "1"]
    r = subprocess.run(base + ["-q", indexed["q"], "-a", "5"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp
    out = indexed["dir"] / "out.gz"
    r = subprocess.run(base + ["--query", indexed["qgz"], "--anchor", "5", "-o", str(out)], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert gzip.decompress(out.read_bytes()) == exp


def test_anchor_0_writes_what_query_alone_writes(small_genome, indexed):
    base = [DICEY, "mappability", "-g", indexed["fa"], "-q", indexed["q"], "-k", "20", "-e", "2"]
    r0 = subprocess.run(base, capture_output=True)
    r1 = subprocess.run(base + ["-a", "0"], capture_output=True)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr, r1.stderr)
    assert r1.stdout == r0.stdout == Q.bedgraph(Q.values(small_genome["text"], indexed["recs"], 20, 2), indexed["names"])


@pytest.mark.parametrize("args,e,a,fo,cap", [(["-e", "1", "-a", "5", "-f"], 1, 5, True, 0), (["-e", "1", "-a", "5", "-c", "2"], 1, 5, False, 2),
                                             (["-e", "2", "-a", "19"], 2, 19, False, 0)])
def test_forward_maxcount_and_two_mismatches(small_genome, indexed, args, e, a, fo, cap):
    exp = _expected(small_genome["text"], indexed, 20, e, a, fo, cap)
    assert len(exp.splitlines()) >= 10
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"], "-q", indexed["q"], "-k", "20"] + args, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp
