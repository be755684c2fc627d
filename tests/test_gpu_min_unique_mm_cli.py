"""`dicey mappability -u -w` end to end: the gz FASTA recipe of test_gpu_min_unique_cli.py (mixed case, descriptions in the names) cut
to 3 x 2 000 bases, a size the pairwise model serves, indexed with `dicey index`; stdout and the gzip file (-o) against the bedGraph
built from the model (tests/min_unique_mm_ref.py), byte for byte."""
import gzip
import os
import subprocess

import pytest

import min_unique_mm_ref as W
import min_unique_ref as U
from conftest import genome_text, make_genome

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")


@pytest.fixture(scope="module")
def map_genome(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("mummcli")
    seqs = make_genome(77, 3, 2000, iupac=True)
    seqs.append("ACGTTGCA")  # shorter than 10
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


@pytest.mark.parametrize("extra,e,fo", [(["-u", "-w", "1"], 1, False), (["-u", "-w", "2", "-f"], 2, True), (["--minunique", "--within=2"], 2, False)])
def test_stdout_gzip_and_piece_edges(map_genome, tmp_path, extra, e, fo):
    g = map_genome
    exp = W.bedgraph(g["text"], g["names"], 40, e, forward_only=fo)
    assert len(exp.splitlines()) > 1000 and exp != U.bedgraph(g["text"], g["names"], 40, forward_only=fo)
    r = _run(["-g", g["fa"], "-k", "40", *extra])
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp
    out = tmp_path / "x.gz"
    r = _run(["-g", g["fa"], "-k", "40", *extra, "-o", str(out)])
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert gzip.decompress(out.read_bytes()) == exp
    # pieces of 1 000 positions: runs that cross a piece edge are joined again (the default piece is 4 M positions)
    r = _run(["-g", g["fa"], "-k", "40", *extra], env={"DICEY_MAP_PIECE": "1000"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp


def test_within_zero_is_minunique(map_genome):
    g = map_genome
    exp = U.bedgraph(g["text"], g["names"], 40)
    a = _run(["-g", g["fa"], "-u", "-k", "40"])
    b = _run(["-g", g["fa"], "-u", "-k", "40", "-w", "0"])
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout == exp and len(exp) > 10000
