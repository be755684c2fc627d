"""`dicey mappability -u` end to end: the gz FASTA recipe of test_gpu_mappability_cli.py (mixed case, descriptions in the names),
indexed with `dicey index`; stdout and the gzip file (-o) against the bedGraph built from the definition (tests/min_unique_ref.py),
byte for byte."""
import gzip
import os
import subprocess

import pytest

import min_unique_ref as U
from conftest import genome_text, make_genome

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")


@pytest.fixture(scope="module")
def map_genome(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("mucli")
    seqs = make_genome(77, 3, 20000, iupac=True)
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


@pytest.mark.parametrize("extra,fo", [(["-u"], False), (["-u", "-f"], True), (["--minunique", "--forward", "-e", "0", "-c", "0"], True)])
def test_stdout_equals_the_definition(map_genome, extra, fo):
    g = map_genome
    exp = U.bedgraph(g["text"], g["names"], 40, forward_only=fo)
    r = _run(["-g", g["fa"], "-k", "40", *extra])
    assert r.returncode == 0, r.stderr
    assert r.stdout == exp
    assert len(exp) > 100000  # the value changes from position to position: most runs are short


def test_gzip_output_and_piece_edges(map_genome, tmp_path):
    g = map_genome
    exp = U.bedgraph(g["text"], g["names"], 40)
    out = tmp_path / "x.gz"
    r = _run(["-g", g["fa"], "-u", "-k", "40", "-o", str(out)])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == b""
    assert gzip.decompress(out.read_bytes()) == exp
    # pieces of 1 000 positions: runs that cross a piece edge are joined again (the default piece is 4 M positions)
    r = _run(["-g", g["fa"], "-u", "-k", "40"], env={"DICEY_MAP_PIECE": "1000"})
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == exp
    r = _run(["-g", g["fa"], "-u", "-k", "40", "-f", "-o", str(out)], env={"DICEY_MAP_PIECE": "1000"})
    assert r.returncode == 0, r.stderr.decode()
    assert gzip.decompress(out.read_bytes()) == U.bedgraph(g["text"], g["names"], 40, forward_only=True)


def test_without_the_flag_the_output_is_the_count_track(map_genome):
    import mappability_ref as R
    g = map_genome
    r = _run(["-g", g["fa"], "-k", "40"])
    assert r.returncode == 0 and r.stdout == R.bedgraph(g["text"], g["names"], 40)
