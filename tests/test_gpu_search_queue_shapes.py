"""k_search1s (dicey_amd/csrc/hunt_search.hpp) on the texts of tests/search_queue_shapes.py: workgroups with a chosen number of candidates
that pass the last-K2 window and a chosen number that pass the first-K2 window as well — 0, 1, 63 / 64 / 65 (the first wavefront's
share and the bound up to which the wavefronts 1-3 end behind the dense phase), 128 / 129, 255 - 257, 512 / 513 (the queue's second round) —
one lane whose eight operations all survive both windows or the last one only, lengths K2 - 1 .. K2 + 2 in both modes, and a list
that overflows beside entries that fail the first window.

Each case runs on a handle's first batch (the form with k_take a launch of its own, generic kernels beside it) and on a handle
settled by one batch of padding (the TAKE form), at max_locations 1, 3 and 1000: hits hit by hit against the oracle, the leaves
counter against the census of occurring candidates, the filter-probe counter against (valid candidates) + (tail survivors longer
than K2) — both numbers as tests/test_search_queue_shapes_host.py holds them against the recorded counters."""
import tempfile

import pytest

try:  # torch bundles its own HIP runtime: it only finds the GPU if it initialises before libdiceygpu's (system) runtime does
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import dicey_amd
import oracle_lib as O
import search_queue_shapes as Q
import select_shapes as S
from test_gpu_locate_topk import _compare

pytestmark = pytest.mark.gpu
_refs = {}


@pytest.fixture(scope="module", autouse=True)
def table_orders():
    mp = pytest.MonkeyPatch()
    mp.setenv("DICEY_KMER_K", str(S.K))
    mp.setenv("DICEY_KMER_K2", str(S.K2))
    yield
    mp.undo()


class _Ref(S.Reference):
    """select_shapes.Reference on a case of search_queue_shapes"""

    def __init__(self, g):
        import os
        self.g = g
        self.dir = tempfile.mkdtemp(prefix="search_queue_shapes_")
        self.path = os.path.join(self.dir, g["name"] + ".fm9")
        O.build_fm9(g["text"], self.path)
        self.orc = O.Index(self.path)
        self.memo = {}


def reference(name):
    if name not in _refs:
        _refs[name] = _Ref(Q.case(name))
    return _refs[name]


@pytest.fixture(scope="module")
def fm9(tmp_path_factory):
    d = tmp_path_factory.mktemp("search_queue_shapes")
    built = {}

    def path(name):
        if name not in built:
            built[name] = str(d / (name + ".fm9"))
            dicey_amd.build_index(Q.case(name)["text"], built[name])
        return built[name]
    return path


def expected(name):
    c = Q.census(Q.case(name))
    return Q.probes(c), c["occurring"]


def run(h, name, qs, form, probes, leaves, gating=Q.GATING):
    g, ref = Q.case(name), reference(name)
    for m in gating:
        got = _compare(h, ref, g, qs, distance=1, hamming=g["hamming"], max_locations=m)
        print("%s max_locations %d: form %d, counters %r" % (name, m, got.path["flat_kernel_form"], got.counters))
        assert got.path["flat_kernel_form"] == form, (m, got.path)
        assert got.counters["leaves"] == leaves, (m, got.counters)
        assert got.counters["filter_probes"] == probes, (m, got.counters)
        # the same probes, made earlier: table reads and extension steps as the parent of that change counted them
        assert (got.counters["tab_reads"], got.counters["ext_steps"]) == tuple(Q.PARENT_COUNTERS[name][2:]), (m, got.counters)


@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_first_batch_of_a_handle(fm9, name):
    """k_search1s<., false>: the generic kernels run beside it, k_take is a launch of its own (a batch without work for them settles
    the handle: a fresh one per limit)"""
    g = Q.case(name)
    probes, leaves = expected(name)
    for m in Q.GATING:
        with dicey_amd.FmIndex(fm9(name)) as h:
            run(h, name, g["qs"], 2, probes, leaves, gating=(m,))


@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_settled_handle(fm9, name):
    """k_search1s<., true> after one batch of the case's padding; a list that overflows repeats the batch with the generic kernels"""
    g = Q.case(name)
    probes, leaves = expected(name)
    pads = [q for i, q in enumerate(g["qs"]) if i not in g["sat"]]
    pc = Q.census(dict(g, qs=pads))
    with dicey_amd.FmIndex(fm9(name)) as h:
        got = _compare(h, reference(name), g, pads, distance=1, hamming=g["hamming"], max_locations=1000)
        assert got.path["flat_kernel_form"] == 2 and got.counters["leaves"] == 0 and got.counters["filter_probes"] == Q.probes(pc)
        run(h, name, g["qs"], 2 if g["want"]["occurring"] > Q.LCAP0 else 3, probes, leaves)
