"""`dicey mappability -p` end to end: the gz FASTA recipe of test_gpu_min_unique_mm_cli.py (mixed case, descriptions in the names, a
sequence shorter than 10), indexed with `dicey index`; stdout and the gzip file (-o) against the bedGraph built from the models
(tests/cover_ref.py), byte for byte."""
import gzip
import os
import subprocess

import pytest

import cover_ref as V
import mappability_mm_ref as MM
import mappability_ref as R
import min_unique_mm_ref as W
import min_unique_ref as U
from conftest import genome_text, make_genome

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")
K = 24


@pytest.fixture(scope="module")
def map_genome(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("covercli")
    seqs = make_genome(78, 3, 2000, iupac=True)
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
    return {"fa": str(fa), "dir": d, "seqs": seqs, "names": ["chr1", "chr2", "scaffold_3", "tiny"], "text": genome_text(seqs)}


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([DICEY, "mappability", *args], capture_output=True, env=e)


def _expected(text, what):
    if what == "cover":
        return V.cover(R.values(text, K), K)
    if what == "cover-t2-c1":
        return V.cover(R.values(text, K), K, 2, 1)
    if what == "cover-e1":
        return V.cover(MM.values(text, K, 1), K)
    if what == "min-cover":
        return V.min_cover(text, U.by_values(text, K), K)
    return V.min_cover(text, W.pairwise(text, K, 1, True), K)


@pytest.mark.parametrize("what,extra", [("cover", ["-p"]), ("cover-t2-c1", ["-p", "-t", "2", "-c", "1"]), ("cover-e1", ["-e", "1", "--perbase"]),
                                        ("min-cover", ["-u", "-p"]), ("min-cover-w1-f", ["-u", "-w", "1", "-p", "-f"])])
def test_stdout_gzip_and_piece_edges(map_genome, tmp_path, what, extra):
    g = map_genome
    exp = V.bedgraph(_expected(g["text"], what), g["text"], g["names"])
    # (clamped at 1 the track has one line per covered stretch: a handful per sequence)
    assert len(exp.splitlines()) > (10 if what == "cover-t2-c1" else 200), len(exp.splitlines())
    r = _run(["-g", g["fa"], "-k", str(K), *extra])
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp
    out = tmp_path / "x.gz"
    r = _run(["-g", g["fa"], "-k", str(K), *extra, "-o", str(out)])
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert gzip.decompress(out.read_bytes()) == exp
    # pieces of 1 000 positions: runs that cross a piece edge are joined again
    r = _run(["-g", g["fa"], "-k", str(K), *extra], env={"DICEY_MAP_PIECE": "1000"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp


def test_the_tracks_differ_from_the_start_position_ones(map_genome):
    g = map_genome
    a, b = _run(["-g", g["fa"], "-k", str(K)]), _run(["-g", g["fa"], "-k", str(K), "-p"])
    assert a.returncode == 0 and b.returncode == 0 and a.stdout != b.stdout and len(b.stdout) > 1000


@pytest.mark.parametrize("args,msg", [
    (["-p", "-q", "FA"], b"Error: --perbase cannot be combined with --query!"),
    (["-u", "-p", "-t", "1"], b"Error: --perbase --minunique cannot be combined with --atmost!"),
    (["-p", "-t", "0"], b"Error: atmost 0 outside 1..4294967293!"),
    (["-t", "1"], b"Error: --shortest and --atmost need --minlength!"),
])
def test_refusals(map_genome, args, msg):
    r = _run(["-g", map_genome["fa"]] + [map_genome["fa"] if a == "FA" else a for a in args])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.strip() == msg
