"""`dicey mappability` end to end: a gz FASTA with mixed case and descriptions in its names, indexed with `dicey index`; stdout and
the gzip file (-o) against the bedGraph built from a brute-force count over the text (tests/mappability_ref.py), byte for byte."""
import gzip
import os
import subprocess

import pytest

import mappability_ref as R
from conftest import genome_text, make_genome

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")


@pytest.fixture(scope="module")
def map_genome(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("mapcli")
    seqs = make_genome(77, 3, 20000, iupac=True)
    seqs.append("ACGTTGCA")  # shorter than every k below
    names = ["chr1", "chr2 some description", "scaffold_3\tmore", "tiny"]
    fa = d / "genome.fa.gz"
    with gzip.open(fa, "wt") as f:
        for n, s in zip(names, seqs):
            f.write(">" + n + "\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60].lower() if i % 120 else s[i:i + 60])
                f.write("\n")
    r = subprocess.run([DICEY, "index", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(str(d / "genome.fa.fm9"))
    return {"fa": str(fa), "dir": d, "seqs": seqs, "names": ["chr1", "chr2", "scaffold_3", "tiny"], "text": genome_text(seqs)}


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([DICEY, "mappability", *args], capture_output=True, env=e)


@pytest.mark.parametrize("extra,kw", [([], {}), (["-f"], {"forward_only": True}), (["-c", "2"], {"max_count": 2}),
                                      (["--forward", "--maxcount=3"], {"forward_only": True, "max_count": 3})])
def test_stdout_equals_brute_force(map_genome, extra, kw):
    g = map_genome
    exp = R.bedgraph(g["text"], g["names"], 20, **kw)
    r = _run(["-g", g["fa"], "-k", "20", *extra])
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp
    assert len(exp) > 1000


def test_gzip_output_and_piece_edges(map_genome, tmp_path):
    g = map_genome
    exp = R.bedgraph(g["text"], g["names"], 20)
    out = tmp_path / "x.gz"
    r = _run(["-g", g["fa"], "-k", "20", "-o", str(out)])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == b""
    assert gzip.decompress(out.read_bytes()) == exp
    # pieces of 1 000 positions: runs that cross a piece edge are joined again (the default piece is 4 M positions)
    for piece in ("1000", "7"):
        r = _run(["-g", g["fa"], "-k", "12", "-o", str(out)], env={"DICEY_MAP_PIECE": piece})
        assert r.returncode == 0, r.stderr.decode()
        assert gzip.decompress(out.read_bytes()) == R.bedgraph(g["text"], g["names"], 12)
        r = _run(["-g", g["fa"], "-k", "12", "-c", "2"], env={"DICEY_MAP_PIECE": piece})
        assert r.stdout == R.bedgraph(g["text"], g["names"], 12, max_count=2)


def test_with_a_fai(map_genome, tmp_path):
    g = map_genome
    d = tmp_path
    fa = d / "g2.fa.gz"
    with gzip.open(fa, "wt") as f:
        for n, s in zip(["c1 desc", "c2", "c3", "c4"], g["seqs"]):
            f.write(">" + n + "\n" + s + "\n")
    r = subprocess.run([DICEY, "index", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(str(fa) + ".fai", "w") as f:  # names from the .fai, not the FASTA
        for n, s in zip(["n1", "n2", "n3", "n4"], g["seqs"]):
            f.write("%s\t%d\t%d\t%d\t%d\n" % (n, len(s), 0, len(s), len(s) + 1))
    r = _run(["-g", str(fa), "-k", "31", "-f"])
    assert r.returncode == 0, r.stderr
    assert r.stdout == R.bedgraph(g["text"], ["n1", "n2", "n3", "n4"], 31, forward_only=True)
    # a .fai whose lengths do not add up to the index: refused
    with open(str(fa) + ".fai", "w") as f:
        f.write("n1\t%d\t0\t1\t2\n" % len(g["seqs"][0]))
    r = _run(["-g", str(fa), "-k", "31"])
    assert r.returncode == 1 and b"do not match" in r.stderr and r.stdout == b""


def test_missing_genome(map_genome, tmp_path):
    r = _run(["-g", str(tmp_path / "absent.fa.gz"), "-k", "20"])
    assert r.returncode == 1 and b"Genome does not exist" in r.stderr
