"""The locate stage of `dicey hunt` (hunt_locate.hpp: k_locate, k_locate_small, k_locate_topk<576> / <1152>, k_locate_big) on the families
of tests/locate_shapes.py, hit by hit against the oracle: every occurrence count and `max_locations` either side of a threshold the
stage has, positions spread and clustered, the product library, the development build with its job lists dumped and held against
the route tests/test_locate_shapes_host.py derived from a scan of the text, and the development build without prefix levels, records
and block minima (one fresh child process per switch)."""
import os
import pickle
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # the child processes below start this file as a script
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

try:  # torch bundles its own HIP runtime: it only finds the GPU if it initialises before libdiceygpu's (system) runtime does
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import dicey_amd
import locate_shapes as S
from conftest import revcomp
from test_gpu_locate_topk import _compare

pytestmark = pytest.mark.gpu
REF = S.Reference()
SWITCHES = ["DICEY_NO_PLV", "DICEY_NO_SAX", "DICEY_NO_SA_MINIMA"]
MIDLVL = ["mid_4607", "mid_4608", "mid_4609", "lvl_9215", "lvl_9216", "lvl_9217", "small_257", "small_256", "n17", "n16"]


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    g = dict(S.genome())
    d = tmp_path_factory.mktemp("locate_shapes")
    g.update(dir=d, fm9=str(d / "locate.fm9"))
    dicey_amd.build_index(g["text"], g["fm9"])      # the GPU builder (byte-identical to the oracle's, tests/test_gpu_parity.py)
    return g


@pytest.fixture(scope="module")
def ix(shapes):
    with dicey_amd.FmIndex(shapes["fm9"]) as h:
        yield h


def _exact(ix, g, table):
    n = 0
    for m, names in table.items():
        got = _compare(ix, REF, g, S.units(names), max_locations=m, **S.D0)
        for name, q in zip(names, got.queries):
            assert len(q.hits) == min(m, len(g["fam"][name]["pos"])), (name, m)
        n += sum(len(q.hits) for q in got.queries)
    return n


def test_exact_units_at_every_count_and_mark(shapes, ix):
    """every family's unit at 1, occs - 1, occs, occs + 1 and at 4, 5, 16, 17, 256, 257, 576, 577, 927, 928, 929, 1024, 1025"""
    print("%d hits equal, in order" % _exact(ix, shapes, S.exact_batches()))


def test_more_than_1024_positions(shapes, ix):
    """k_locate_big: limit 2 050, 5 120, 9 216 (9 216 copies sorted whole), 9 218 (9 217 copies sorted whole, 9 215 too), CAP"""
    print("%d hits equal, in order" % _exact(ix, shapes, S.big_batches()))


def test_batches_with_a_40_nt_query_sort_plain_positions(shapes, ix):
    print("%d hits equal, in order" % _exact(ix, shapes, S.long_batches()))


@pytest.mark.parametrize("hamming", [False, True])
def test_star_takes_end_inside_at_the_end_and_before_each_string(shapes, ix, hamming):
    q = shapes["star"]["q"]
    for m in S.star_marks():
        _compare(ix, REF, shapes, [q], distance=1, hamming=hamming, max_locations=m)
    # among other queries: the strings' hit slots start behind another query's
    others = [shapes["fam"]["small_33"]["unit"], revcomp(q), shapes["fam"]["n5"]["unit"], q]
    for m in S.star_marks()[::4]:
        _compare(ix, REF, shapes, others, distance=1, hamming=hamming, max_locations=m)


def test_filtered_intervals_keep_the_suffixes_of_their_mask(shapes, monkeypatch):
    """tails: with a table of order 16 a 20-mer's last 16 characters have 2 .. 16 suffixes, and 1, 2, 4, 5, 15 or 16 of them are
    preceded by the query's first characters (Sel's filtered form: locate_in_registers<4> / <16> with a mask, and the record path for
    one occurrence)"""
    monkeypatch.setenv("DICEY_KMER_K", str(S.TAIL_K))
    monkeypatch.setenv("DICEY_KMER_K2", "18")
    qs = [q for q, _ in S.tails_queries()]
    with dicey_amd.FmIndex(shapes["fm9"]) as h:
        for kw in (dict(distance=1), dict(distance=1, hamming=True), dict(distance=0), dict(distance=1, max_locations=1),
                   dict(distance=1, max_locations=3), dict(distance=1, forward_only=True, max_locations=14)):
            got = _compare(h, REF, shapes, qs, **kw)
            print(kw, sum(len(q.hits) for q in got.queries), "hits equal")


def test_small_buffer_list_after_a_batch_of_workgroup_jobs(shapes):
    """mid_* / lvl_* on a fresh handle (no small-buffer list: k_locate_topk<1152> at level 0), then right behind 2 304 workgroup jobs
    (k_locate_topk<576> takes intervals and runs of up to 4 608 entries)"""
    jobs = S.jobs_batch(2304)
    with dicey_amd.FmIndex(shapes["fm9"]) as h:
        for m in (1000, 577):
            _compare(h, REF, shapes, S.units(MIDLVL), max_locations=m, **S.D0)
            got = _compare(h, REF, shapes, jobs, distance=1, max_locations=20)
            assert sum(len(q.hits) for q in got.queries) == 20 * len(jobs)
            _compare(h, REF, shapes, S.units(MIDLVL), max_locations=m, **S.D0)


def test_job_kernels_come_and_go_on_one_handle(shapes):
    plain, small = S.plain_batch(), S.units(["small_%d" % c for c in S.SMALL_COUNTS] + ["n16", "n17"])
    with dicey_amd.FmIndex(shapes["fm9"]) as h:
        for qs in (plain, small, plain, plain, small, small, plain):
            _compare(h, REF, shapes, qs, distance=1, max_locations=1000)


# ---- the development build: which list, which level ------------------------------------------------------------------------------------------

def _dumped(h, g, path, names, m, mid_max=0, levels=S.LEVELS):
    """one exact batch on the development build: hits against the oracle, job lists against route()"""
    if os.path.exists(path):
        os.remove(path)
    _compare(h, REF, g, S.units(names), max_locations=m, **S.D0)
    got, want = S.read_jobs(path), S.expected_jobs(names, m, mid_max, levels)
    assert got == want, (m, [x for x in got if x not in want], [x for x in want if x not in got])
    return got


def test_every_case_reaches_the_list_and_level_derived_for_it(shapes, monkeypatch):
    from conftest import exp_lib
    path = str(shapes["dir"] / "jobs.bin")
    monkeypatch.setenv("DICEY_DUMP_JOBS", path)
    fam = shapes["fam"]
    with dicey_amd.FmIndex(shapes["fm9"], _lib=exp_lib()) as h:
        seen = []
        for table in (S.exact_batches(), S.big_batches()):
            for m, names in table.items():
                seen += _dumped(h, shapes, path, names, m)
        lists = {x[0] for x in seen}
        assert lists == {0, 2}                                     # never a small-buffer job on this handle so far
        whole = [x for x in seen if x[1] is None]                  # (a run of a prefix level may be as short as its take)
        assert min(x[2] for x in whole) == 17 and max(x[2] for x in whole if x[0] == 0) == 256 and min(x[2] for x in whole if x[0] == 2) == 257
        assert all(x[0] == 2 and x[3] <= x[2] <= S.WALK_MAX for x in seen if x[1] is not None)
        print("case                 list level  occs  take")
        for name, m in S.plv_cases() + [("lvl_9216", 1000), ("lvl_9217", 1000), ("lvl_9217", 1), ("topk_skew", 501)]:
            (job,) = _dumped(h, shapes, path, [name], m)
            print("%-20s %4d %5s %5d %5d" % (name, job[0], job[1], job[2], job[3]))
            if job[1] is not None:                                 # a run: as many records as copies lie below that level's X
                assert job[2] == sum(1 for p in fam[name]["pos"] if p < S.LEVELS[job[1]])
        # the small-buffer list exists only right behind a batch with >= 2 048 workgroup jobs
        jobs = S.jobs_batch(2304)
        os.remove(path)
        _compare(h, REF, shapes, jobs, distance=1, max_locations=20)
        assert S.read_jobs(path) == [(2, None, 300, 20, 20)] * len(jobs)
        mid = _dumped(h, shapes, path, MIDLVL, 1000, mid_max=S.MID_MAX)
        for x in mid:
            print("%-20s %4d %5s %5d %5d" % ("after 2304 jobs", x[0], x[1], x[2], x[3]))
        assert (1, None, 4608, 1000, 16) in mid and (2, None, 4609, 1000, 16) in mid and (1, None, 257, 257, len(fam["small_257"]["unit"])) in mid
        assert not any(x[2] <= 16 for x in mid)
        again = _dumped(h, shapes, path, MIDLVL, 1000)            # that batch queued ten jobs: the list is gone
        assert {x[0] for x in again} == {0, 2}


# ---- the development build, one switch per fresh process ---------------------------------------------------------------------------------------

def _child(fm9, blob):
    """runs in a child whose environment holds one DICEY_* switch: conftest.open_index then opens the development build"""
    from conftest import exp_lib, open_index
    batches, g, dump = pickle.load(open(blob, "rb"))
    os.environ["DICEY_DUMP_JOBS"] = dump
    with open_index(fm9) as h:
        assert h._L is exp_lib()
        for m, names, qs, per, want in batches:
            if os.path.exists(dump):
                os.remove(dump)
            _compare(h, S.Canned(per), g, qs, max_locations=m, **S.D0)
            got = S.read_jobs(dump)
            assert got == want, (m, names, got, want)    # no prefix level in any job: the interval itself, whatever its size
            print("batch %d: %d jobs, hits equal" % (m, len(got)), flush=True)


def test_development_build_without_levels_records_and_minima(shapes):
    from conftest import build_exp_lib
    build_exp_lib()
    g = {k: shapes[k] for k in ("seqlen", "names")}
    batches = []
    for m, names in S.walk_batches().items():
        qs = S.units(names)
        batches.append((m, names, qs, S.per_query(qs, max_locations=m, **S.D0), S.expected_jobs(names, m, 0, ())))
    for switch in SWITCHES:      # one at a time; the first failure stops the rest
        blob = str(shapes["dir"] / (switch + ".pickle"))
        pickle.dump((batches, g, str(shapes["dir"] / (switch + ".jobs"))), open(blob, "wb"))
        env = dict(os.environ)
        env[switch] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shapes["fm9"], blob], env=env, capture_output=True,
                           text=True, timeout=180)
        print(switch, r.stdout.replace("\n", "; "))
        assert r.returncode == 0, (switch, r.stdout[-1500:], r.stderr[-1500:])
        assert r.stdout.count("hits equal") == len(batches), (switch, r.stdout)


# ---- a full job region ---------------------------------------------------------------------------------------------------------------------------

def test_strings_a_full_job_region_turns_away_are_served_by_their_lane(shapes, monkeypatch):
    """3 500 times the crowd's centre: 105 000 wavefront jobs for 64 regions of 1 568 slots (100 352), so at least 4 648 strings are
    served by the lane that queued them (17 of 17 occurrences each)"""
    from conftest import exp_lib
    path = str(shapes["dir"] / "crowd.bin")
    monkeypatch.setenv("DICEY_DUMP_JOBS", path)
    qs = S.crowd_batch()
    with dicey_amd.FmIndex(shapes["fm9"], _lib=exp_lib()) as h:
        t0 = time.time()
        got = _compare(h, REF, shapes, qs, distance=1, hamming=True, forward_only=True, max_locations=1000)
        print("crowd batch: %.1f s" % (time.time() - t0))
        assert all(len(q.hits) == S.CROWD * S.CROWD_COPIES for q in got.queries)
        jobs = S.read_jobs(path)
        assert set(jobs) == {(0, None, 17, 17, 20)}
        assert len(jobs) <= 64 * 1568 < len(qs) * S.CROWD, len(jobs)
        print("jobs in the list: %d of %d strings" % (len(jobs), len(qs) * S.CROWD))


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "--child":
    _child(sys.argv[2], sys.argv[3])
