"""`dicey mappability -q -l`: the binary's bedGraph of minimum lengths for the records of a query FASTA against the writer of
tests/query_min_len_ref.py (runs of equal lengths; no line where there is no length), plain and gzipped, in the default build and with a
small DICEY_MAP_PIECE, and `-q` without `-l` still byte for byte what tests/query_map_ref.py writes."""
import gzip
import os
import random
import subprocess

import pytest

import query_map_ref as Q
import query_min_len_ref as ML
from conftest import revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")


@pytest.fixture(scope="module")
def indexed(small_genome, tmp_path_factory):
    g = small_genome
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("mlcli")
    fa = d / "session.fa.gz"
    with gzip.open(fa, "wt") as f:
        for n, s in zip(g["names"], g["seqs"]):
            f.write(">" + n + "\n")
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    r = subprocess.run([DICEY, "index", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # a cut with every fortieth base substituted next to a junction, a lower-case record with a description in its header (the binary
    # upper-cases it), random sequence with an N, and one of the genome's own repeats: lengths, zero runs and invalid stretches
    rng = random.Random(3)
    s1, s2, _ = g["seqs"]
    clean = lambda s, a, m: next(x for x in range(a, len(s) - m) if set(s[x:x + m]) <= set("ACGT"))
    a, b = clean(s1, 3000, 300), clean(s2, 8000, 200)
    cut = list(s1[a:a + 300])
    for i in range(8, 300, 40):
        cut[i] = "ACGT"[("ACGT".index(cut[i]) + 1) % 4]
    rep = next(r for r in ML.record_set(g["seqs"], g["text"]) if 90 <= len(r) <= 200 and r.isupper() and r != b"A" * 40).decode()
    recs = [("tx1", "", "".join(cut) + s2[b:b + 60]), ("low", " a lower-case record", revcomp(s2[b:b + 200]).lower()),
            ("rnd", "\tx=1", "".join(rng.choice("ACGT") for _ in range(90)) + "N" + "".join(rng.choice("ACGT") for _ in range(60))),
            ("rep", "", rep)]
    q = d / "targets.fa"
    with open(q, "w") as f:
        for name, desc, s in recs:
            f.write(">" + name + desc + "\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    qgz = d / "targets.fa.gz"
    qgz.write_bytes(gzip.compress(q.read_bytes()))
    return {"fa": str(fa), "q": str(q), "qgz": str(qgz), "names": [r[0] for r in recs], "recs": [r[2].upper().encode() for r in recs], "dir": d}


def _expected(text, recs, names, lo, hi, e, t, fo):
    qbuf, _ = Q.buffer_of(recs)
    parts = ML.parts_by_k(text, qbuf, range(lo, hi + 1), e)
    return ML.bedgraph(ML.split(ML.min_len(parts, qbuf, lo, hi, t, fo), recs), names)


@pytest.mark.parametrize("args,lo,hi,e,t,fo", [(["-k", "24"], 10, 24, 0, 0, False), (["-k", "20", "-s", "12", "-t", "1", "-e", "1", "-f"], 12, 20, 1, 1, True)])
def test_bedgraph_of_minimum_lengths(small_genome, indexed, args, lo, hi, e, t, fo):
    exp = _expected(small_genome["text"], indexed["recs"], indexed["names"], lo, hi, e, t, fo)
    lines = exp.splitlines()
    # the expectation itself: several lengths, lines for the records that have some, none with 0 or the invalid mark
    vals = {int(l.split(b"\t")[3]) for l in lines}
    assert len(vals) >= 3 and min(vals) >= lo and max(vals) <= hi and len({l.split(b"\t")[0] for l in lines}) >= 3 and len(lines) >= 10
    base = [DICEY, "mappability", "-g", indexed["fa"], "-l"] + args
    for env in ({}, {"DICEY_MAP_PIECE": "50"}):
        r = subprocess.run(base + ["-q", indexed["q"]], capture_output=True, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr
        assert r.stdout == exp
        out = indexed["dir"] / ("out%d%s.gz" % (e, "p" if env else ""))
        r = subprocess.run(base + ["--query", indexed["qgz"], "--minlength", "-o", str(out)], capture_output=True, env=dict(os.environ, **env))
        assert r.returncode == 0 and r.stdout == b"", r.stderr
        assert gzip.decompress(out.read_bytes()) == exp


def test_query_without_minlength_writes_what_it_wrote(small_genome, indexed):
    exp = Q.bedgraph(Q.values(small_genome["text"], indexed["recs"], 20, 1, max_count=3), indexed["names"])
    assert any(l.endswith(b"\t0") for l in exp.splitlines())
    r = subprocess.run([DICEY, "mappability", "-g", indexed["fa"], "-q", indexed["q"], "-k", "20", "-e", "1", "-c", "3"], capture_output=True)
    assert r.returncode == 0 and r.stdout == exp, r.stderr
