"""The per-base tracks without a GPU: the two models of each track in tests/cover_ref.py against each other, the identity that ties the
cover count to the minimum covering length, what the crafted text exercises, the arithmetic of dicey_amd/csrc/map_cover.hpp as a host
program against the models, and the refusals of `dicey mappability -p`."""
import os
import random
import subprocess

import numpy as np
import pytest

import cover_ref as V
import genome_shapes as S
import mappability_mm_ref as MM
import mappability_ref as R
import min_unique_mm_ref as W
import min_unique_ref as U
from conftest import genome_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICEY = os.path.join(ROOT, "dicey_amd", "dicey")
CXX = os.environ.get("CXX", "g++")
MAX_K = 40


@pytest.fixture(scope="module")
def crafted():
    return genome_text(V.crafted_seqs())


def _mul(text, max_k, e, fo):
    return U.by_values(text, max_k, fo) if e == 0 else W.pairwise(text, max_k, e, fo)


def _same(a, b, what):
    bad = np.nonzero(a != b)[0]
    assert len(a) == len(b) and len(bad) == 0, (what, len(bad), bad[:10], a[bad[:10]], b[bad[:10]])


# ---- the two models of each track ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fo", [False, True])
@pytest.mark.parametrize("e", [0, 1])
def test_models_agree_on_the_crafted_text(crafted, e, fo):
    for k in (10, 20, 40):
        base = V._values(crafted, k, e, fo)
        for at_most, max_count in ((1, 0), (2, 0), (5, 3), (1, 1), (2, k)):
            _same(V.cover(base, k, at_most, max_count), V.cover_by_windows(crafted, k, at_most, max_count, e, fo), ("cover", k, e, fo, at_most, max_count))
    for max_k in (10, 16, MAX_K):
        _same(V.min_cover(crafted, _mul(crafted, max_k, e, fo), max_k), V.min_cover_by_windows(crafted, max_k, e, fo), ("min cover", max_k, e, fo))


@pytest.mark.parametrize("name", [n for n in S.TINY_NAMES if len(S.all_shapes()[n]["text"]) <= 600])
def test_models_agree_on_the_tiny_shapes(name):
    text = S.all_shapes()[name]["text"]
    for e in (0, 1):
        for k in (10, 24):
            _same(V.cover(V._values(text, k, e, False), k), V.cover_by_windows(text, k, e=e), (name, "cover", k, e))
        _same(V.min_cover(text, _mul(text, 24, e, False), 24), V.min_cover_by_windows(text, 24, e), (name, "min cover", e))


# ---- the identity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fo", [False, True])
@pytest.mark.parametrize("e", [0, 1])
def test_identity_and_its_restriction(crafted, e, fo):
    """for every k in 10..max_k and every p in at least one valid k-window: cover_1 at k >= 1  <=>  mcl != 0 and mcl <= k"""
    mcl = V.min_cover(crafted, _mul(crafted, MAX_K, e, fo), MAX_K)
    outside = {}
    for k in range(10, MAX_K + 1):
        cov = V.cover(V._values(crafted, k, e, fo), k) >= 1
        short = (mcl != 0) & (mcl <= k)
        ok = V.coverable(crafted, k)
        bad = np.nonzero(cov[ok] != short[ok])[0]
        assert len(bad) == 0, (k, e, fo, np.nonzero(ok)[0][bad[:10]])
        assert not cov[~ok].any()
        outside[k] = int(short[~ok].sum())
    # the restriction is needed: bases of runs shorter than k with a unique shorter window over them
    assert outside[20] >= 1 and outside[40] >= outside[20], outside


# ---- what the crafted text exercises, by the reference alone -----------------------------------------------------------------------------

def test_the_crafted_text_exercises_every_class(crafted):
    text = crafted
    acgt = U.run_lengths(text) > 0
    k = MAX_K
    cov = V.cover(R.values(text, k), k)
    figures = {"partial": int(((cov > 0) & (cov < k)).sum()), "full": int((cov == k).sum()), "acgt_uncovered": int((acgt & (cov == 0)).sum())}
    assert figures["partial"] >= 100 and figures["full"] >= 100 and figures["acgt_uncovered"] >= 50, figures
    mul = U.by_values(text, k)
    mcl = V.min_cover(text, mul, k)
    L = len(text)
    p = np.arange(L)
    figures["short_outside_coverable"] = int(((mcl != 0) & (mcl <= k) & ~V.coverable(text, k)).sum())
    # the minimiser is not q = p: the start at p itself gives max(mul(p), 1) = mul(p), or nothing
    own = np.where(mul != 0, mul, 1 << 30)
    figures["minimiser_elsewhere"] = int(((mcl != 0) & (mcl < own)).sum())
    # the reach decides: no start q over p has mul(q) == mcl(p) with p-q+1 <= mul(q); walk the definition once more, keeping the best pair
    run = U.run_lengths(text)
    reach = 0
    for pp in np.nonzero(mcl)[0].tolist():
        by_len = False
        for d in range(1, min(k, pp + 1) + 1):
            q = pp - d + 1
            if mul[q] != 0 and run[q] >= d and max(int(mul[q]), d) == mcl[pp] and mul[q] >= d:
                by_len = True
                break
        reach += not by_len
    figures["reach_decides"] = reach
    figures["zero_inside_run"] = int((acgt & (mcl == 0)).sum())
    assert figures["short_outside_coverable"] >= 1 and figures["minimiser_elsewhere"] >= 100 and figures["reach_decides"] >= 1 and \
        figures["zero_inside_run"] >= 50, figures
    assert not mcl[~acgt].any() and p[mcl != 0].size > 500


# ---- the header's arithmetic as a host program ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host", "map_cover_main.cpp")
    exe = str(tmp_path_factory.mktemp("mapcover") / "map_cover_main")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, src])
    return exe


def _ask(program, jobs):
    r = subprocess.run([program], input="".join(jobs), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return [np.array(line.split(), dtype=np.int64) for line in r.stdout.split("\n")[:-1]]


def test_host_program_window_counts(program):
    rng = random.Random(7)
    jobs, exp = [], []
    for k in (10, 63, 64, 65, 128, 1000):
        for nbits in (1, 9, 63, 65, 127, 129, 1000, 1001, 2500, 4099):
            for density in (0.02, 0.5, 0.97):
                bits = np.array([rng.random() < density for _ in range(nbits)], dtype=np.uint32)
                jobs.append("count %d %d\n%s\n" % (nbits, k, "".join("01"[b] for b in bits)))
                exp.append(V.cover(bits, k))
    got = _ask(program, jobs)
    assert len(got) == len(exp) == 180
    for j, (a, b) in enumerate(zip(got, exp)):
        _same(a, b.astype(np.int64), jobs[j][:20])


def test_host_program_walk(program, crafted):
    rng = random.Random(8)
    jobs, exp = [], []

    def add(text, mul, max_k):
        acgt = U.run_lengths(text) > 0
        cells = np.where(acgt, np.asarray(mul).astype(np.int64), -1)
        jobs.append("walk %d %d\n%s\n" % (len(text), max_k, " ".join(map(str, cells.tolist()))))
        exp.append(V.min_cover(text, mul, max_k))

    for max_k in (10, 40, 100, 1000):
        for L in (1, 9, 64, 700, 3000):
            # random lengths with zeros and breaks: a length never exceeds the run it starts in, as in a real map
            text = bytes(rng.choice(b"ACGT") if rng.random() > 0.01 else ord("N") for _ in range(L))
            run = U.run_lengths(text)
            mul = np.array([0 if rng.random() < 0.6 else rng.randint(1, max_k) for _ in range(L)], dtype=np.int64)
            mul[mul > run] = 0
            add(text, mul, max_k)
    add(crafted, U.by_values(crafted, MAX_K), MAX_K)
    got = _ask(program, jobs)
    assert len(got) == len(exp) == 21
    assert sum(int((e != 0).sum()) for e in exp) > 5000
    for j, (a, b) in enumerate(zip(got, exp)):
        _same(a, b.astype(np.int64), jobs[j][:20])


# ---- the command line --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dicey_amd", "cli"), "-s"])
    d = tmp_path_factory.mktemp("covercli")
    (d / "g.fa").write_text(">a\nACGTACGTACGTAAACCCGGGTTT\n")
    (d / "q.fa").write_text(">q\nACGTACGTACGTAAACCCGGGTTT\n")
    return {"g": str(d / "g.fa"), "q": str(d / "q.fa")}


@pytest.mark.parametrize("args,msg", [
    (["-p", "-q", "Q"], "Error: --perbase cannot be combined with --query!"),
    (["-p", "-q", "Q", "-l"], "Error: --perbase cannot be combined with --query!"),
    (["-u", "-p", "-t", "1"], "Error: --perbase --minunique cannot be combined with --atmost!"),
    (["--perbase", "--minunique", "--atmost=3"], "Error: --perbase --minunique cannot be combined with --atmost!"),
    (["-p", "-t", "0"], "Error: atmost 0 outside 1..4294967293!"),
    (["-p", "-t", "4294967294"], "Error: atmost 4294967294 outside 1..4294967293!"),
    (["-p", "-s", "12"], "Error: --shortest and --atmost need --minlength!"),
    # every argument vector that existed keeps its message
    (["-t", "1"], "Error: --shortest and --atmost need --minlength!"),
    (["-t", "0"], "Error: --shortest and --atmost need --minlength!"),
    (["-u", "-t", "1"], "Error: --shortest and --atmost need --minlength!"),
    (["-u", "-q", "Q"], "Error: --minunique cannot be combined with --query!"),
    (["-u", "-p", "-q", "Q"], "Error: --minunique cannot be combined with --query!"),
    (["-u", "-p", "-c", "2"], "Error: --minunique cannot be combined with --mismatches or --maxcount!"),
])
def test_cli_refusals(files, args, msg):
    r = subprocess.run([DICEY, "mappability", "-g", files["g"]] + [files["q"] if a == "Q" else a for a in args], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.strip() == msg


def test_cli_accepts_atmost_with_perbase_and_names_the_option(files):
    """-p -t 2 passes the option checks (the run ends at the missing index, the first thing behind them)"""
    r = subprocess.run([DICEY, "mappability", "-g", files["g"], "-p", "-t", "2", "-c", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Error: Index "), r.stderr
    u = subprocess.run([DICEY, "mappability", "-?"], capture_output=True, text=True).stdout
    for line in ("  -p [ --perbase ]", "       dicey mappability -g genome.fa.gz -u -p [-k 100] [-w 0] [-f]", "With -u -p the value of a base"):
        assert line in u
