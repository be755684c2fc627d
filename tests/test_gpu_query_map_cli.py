"""`dicey mappability -q`: the binary's bedGraph for the records of a query FASTA against the reference writer of tests/query_map_ref.py
(runs of equal values over valid positions, zero included), plain and gzipped, and its refusals."""
import gzip
import os
import random
import subprocess

import pytest

import query_map_ref as Q
from conftest import revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")


@pytest.fixture(scope="module")
def indexed(small_genome, tmp_path_factory):
    g = small_genome
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("qcli")
    fa = d / "session.fa.gz"
    with gzip.open(fa, "wt") as f:
        for n, s in zip(g["names"], g["seqs"]):
            f.write(">" + n + "\n")
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    r = subprocess.run([DICEY, "index", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # three records: a cut with every fortieth base substituted next to a junction, a lower-case record with a description in its
    # header (the binary upper-cases it, as `dicey index` does), and random sequence with an N
    rng = random.Random(3)
    s1, s2, _ = g["seqs"]
    clean = lambda s, a, m: next(x for x in range(a, len(s) - m) if set(s[x:x + m]) <= set("ACGT"))
    a, b = clean(s1, 3000, 300), clean(s2, 8000, 200)
    cut = list(s1[a:a + 300])
    for i in range(8, 300, 40):
        cut[i] = "ACGT"[("ACGT".index(cut[i]) + 1) % 4]
    recs = [("tx1", "", "".join(cut) + s2[b:b + 60]), ("low", " a lower-case record", revcomp(s2[b:b + 200]).lower()),
            ("rnd", "\tx=1", "".join(rng.choice("ACGT") for _ in range(90)) + "N" + "".join(rng.choice("ACGT") for _ in range(60)))]
    q = d / "targets.fa"
    with open(q, "w") as f:
        for name, desc, s in recs:
            f.write(">" + name + desc + "\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    qgz = d / "targets.fa.gz"
    qgz.write_bytes(gzip.compress(q.read_bytes()))
    return {"fa": str(fa), "q": str(q), "qgz": str(qgz), "names": [r[0] for r in recs], "recs": [r[2].upper().encode() for r in recs], "dir": d}


@pytest.mark.parametrize("args,e,fo,cap", [(["-e", "0"], 0, False, 0), (["-e", "1", "-c", "2", "-f"], 1, True, 2)])
def test_bedgraph_of_a_query_file(small_genome, indexed, args, e, fo, cap):
    k = 20
    exp = Q.bedgraph(Q.values(small_genome["text"], indexed["recs"], k, e, forward_only=fo, max_count=cap), indexed["names"])
    lines = exp.splitlines()
    # the expectation itself: zero runs and non-zero runs, lines for every record, the description and the N left out
    assert any(l.endswith(b"\t0") for l in lines) and any(not l.endswith(b"\t0") for l in lines)
    assert {l.split(b"\t")[0] for l in lines} == {b"tx1", b"low", b"rnd"} and b"rnd\t0\t71\t0" in lines and b"rnd\t91\t132\t0" in lines
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"], "-q", indexed["q"], "-k", str(k)] + args, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp
    out = indexed["dir"] / ("out%d.gz" % e)
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"], "--query", indexed["qgz"], "-k", str(k), "-o", str(out)] + args, capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert gzip.decompress(out.read_bytes()) == exp


def test_refusals(indexed):
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"], "-q", indexed["q"], "-u"], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout == "" and "Error: --minunique cannot be combined with --query!" in r.stderr
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"], "-q", str(indexed["dir"] / "missing.fa")], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout == "" and "Error: Query file" in r.stderr and "does not exist or is empty!" in r.stderr
    empty = indexed["dir"] / "empty.fa"
    empty.write_text("")
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"], "-q", str(empty)], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout == "" and "does not exist or is empty!" in r.stderr
    norec = indexed["dir"] / "norecord.fa"
    norec.write_text("ACGTACGTACGT\n")
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"], "-q", str(norec)], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout == "" and "Error: Could not read any sequence" in r.stderr
    r = subprocess.run([DICEY, "mappability", "-?"], capture_output=True, text=True)
    assert "--query" in r.stdout
