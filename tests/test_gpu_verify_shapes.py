"""The verify stage of dg_hunt on the PRODUCT library against the oracle, on the batches of tests/verify_shapes.py (proved without a GPU
by tests/test_verify_shapes_host.py): every hit in push order — score, chr, start, strand and both rows (cut at aln_len) — and the
compact delivery against the classic one.  Equality only.  A failure names the batch, the query, the hit and its class: (kept string,
pre_eff, post_eff, context bytes), the key under which k_verify_memo shares one alignment among hits.

Every test asserts the form that ran (dg_hunt_result::verify_kernel_form: (band width << 8) | hits per lane for k_verify_memo, 0 for
the other kernels, where the batch's longest query and its distance select the kernel: hunt.hip run_batch), so a passing test proves
the kernel.  No test switch is read (conftest.EXP_VARS must be unset): all nine forms are reached from data and history.

run_batch sizes the hit buffer as hit_cap = max(hint, 4 nq + 1024), where hint is nhits * 5 / 4 + 1024 of the handle's largest batch so
far; a batch with more hits than room is repeated with nhits * 5 / 4 + 1024.  k_verify_memo's hits per lane follow hit_cap / nq:
distance <= 1: >= 24 -> 4 (8 on a handle without context records, DG_OPEN_COMPACT), >= 12 -> 4, else 1; distance 2: >= 192 -> 8,
>= 96 -> 4, else 1.  (test_verify_shapes_host.py::test_the_schedules_reach_the_widths_they_name holds the arithmetic below against the
oracle's hit counts.)

| form                    | where                          | schedule on the product library                                           |
|-------------------------|--------------------------------|---------------------------------------------------------------------------|
| k_verify_memo<7,1>      | asserted on the product library | fresh handle, ties + clean in one call: 178 queries, 1 736 / 178 = 9     |
| k_verify_memo<7,4>      | asserted on the product library | classes20 (2 700 hits, repeated with room for 4 399: 549 per query); then ties + clean again (4 399 / 178 = 24), ties alone |
| k_verify_memo<7,8>      | asserted on the product library | handle opened with DG_OPEN_COMPACT: ties alone (1 096 / 18 = 60), classes20, classes20 + clean (4 399 / 168 = 26) |
| k_verify_memo<13,1>     | asserted on the product library | fresh handle, clean_d2: 48 queries, 1 216 / 48 = 25                      |
| k_verify_memo<13,8>     | asserted on the product library | classes14 (3 006 hits, repeated with room for 4 781: 478 per query)       |
| k_verify_memo<13,4>     | asserted on the product library | after classes14: classes14 + 20 clean queries (4 781 / 30 = 159), clean_d2 (4 781 / 48 = 99), classes20_d2 + 28 clean queries |
| k_verify<1,true,24>     | asserted on the product library | form 0, longest query <= 24 at distance 3 / 4: len24_d3, deep3, deep4    |
| k_verify<1,true,32>     | asserted on the product library | form 0, longest query 25 / 32 at distance 3: len25_d3, len32_d3          |
| k_verify<160,false>     | asserted on the product library | form 0, longest query 33 and the last length with cells <= 32 * 160       |
| k_verify<2200,false>    | asserted on the product library | form 0, the first length with cells > 32 * 160, and 255                   |
| k_verify_long           | asserted on the product library | form 0, longest query 256 and 300                                         |
| k_rows_to_ops, k_hits_to_compact | asserted on the product library | behind every form-0 batch but k_verify_long's: the compact and the classic delivery of each are compared |

Nothing is left to the development library: DICEY_VERIFY_CH is not needed to reach a form."""
import os

import pytest

import conftest
import dicey_amd
import verify_shapes as V
from dicey_amd import _capi

pytestmark = pytest.mark.gpu

assert not [k for k in conftest.EXP_VARS if k in os.environ], "test switches set: this module runs the product library only"


@pytest.fixture(autouse=True)
def _product_only():
    assert not [k for k in conftest.EXP_VARS if k in os.environ]
    yield


def open_product(**kw):
    ix = dicey_amd.FmIndex(V.oracle_index()[1], **kw)
    assert ix._L is _capi.load()
    return ix


@pytest.fixture(scope="module")
def shared():
    """one handle for the batches whose kernel does not depend on history (the length and deep batches)"""
    ix = open_product()
    yield ix
    ix.close()


def _tuples(qr):
    return [(h.score, h.chr, h.start, h.strand, h.refalign, h.queryalign) for h in qr.hits]


def _key(batch):
    return [_tuples(q) + [q.flags, q.nondna, q.sequence, q.distance] for q in batch.queries]


def check(name, got, tag, offset=0, count=None):
    """queries offset.. of the result against batch `name` (its first `count` queries), hit by hit in push order"""
    exp, pl = V.expected(name), V.push_list(name)
    per = {}
    for k, e in enumerate(exp):
        per.setdefault(e[0], []).append(k)
    qs = V.batches()[name]["queries"]
    for qi in range(len(qs) if count is None else count):
        a = _tuples(got.queries[offset + qi])
        ks = per.get(qi, [])
        want = [exp[k][1:] for k in ks]
        if a == want:      # (FmIndex._unpack cuts both rows at dg_hit::aln_len: the rows' lengths are aln_len)
            assert all(len(h[4]) == len(h[5]) == len(w[4]) for h, w in zip(a, want))
            continue
        j = next((i for i in range(min(len(a), len(want))) if a[i] != want[i]), min(len(a), len(want)))
        if j < len(ks):
            where = "hit %d of the query, %d of the batch, class (kept string, pre_eff, post_eff, context) %r at text position %d" % \
                (j, ks[j], pl[ks[j]]["cls"], pl[ks[j]]["loc"])
        else:
            where = "hit %d of the query: the oracle has %d" % (j, len(ks))
        raise AssertionError("batch %s (%s), form %#x, query %d %r, %s\n  library: %r\n  oracle:  %r" %
                             (name, tag, got.path["verify_kernel_form"], qi, qs[qi], where, a[j] if j < len(a) else None,
                              want[j] if j < len(want) else None))
    return got


def hunt(ix, names, counts=None, **over):
    """the named batches in one call (they share their hunt parameters); each part compared with its own oracle answer"""
    g = V.genome()
    counts = counts or [None] * len(names)
    qs, parts = [], []
    for name, c in zip(names, counts):
        q = V.batches()[name]["queries"]
        q = q if c is None else q[:c]
        parts.append((name, len(qs), len(q)))
        qs += q
    kw = dict(V.batches()[names[0]]["kw"])
    for name in names[1:]:
        k2 = V.batches()[name]["kw"]
        assert k2["distance"] == kw["distance"]
        kw["max_locations"] = max(kw.get("max_locations", 1000), k2.get("max_locations", 1000))
        kw["max_neighborhood"] = max(kw.get("max_neighborhood", 10000), k2.get("max_neighborhood", 10000))
    for name in names:      # a larger cap than a batch's own must not change its answer: nothing of it is cut
        b = V.batches()[name]
        n = {}
        for e in V.expected(name):
            n[e[0]] = n.get(e[0], 0) + 1
        assert max(n.values(), default=0) < b["kw"].get("max_locations", 1000), name
    got = ix.hunt(qs, g["seqlen"], **dict(dict(kw, compact=True), **over))
    for name, off, cnt in parts:
        check(name, got, "+".join(names), off, cnt)
    return got


def form(got):
    f = got.path["verify_kernel_form"]
    return (f >> 8, f & 0xff)


def _part(got, lo, n):
    return [_tuples(q) for q in got.queries[lo:lo + n]]


# ------------------------------------------------------------------------------------------------------------ the band, distance 1

def test_band7_one_hit_per_lane_then_four():
    """k_verify_memo<7,1> on a fresh handle, <7,4> after the 20-nt family; the clean queries and the ties keep their answers when
    they share workgroups with the family's classes"""
    n_t, n_c, n_f = (len(V.batches()[b]["queries"]) for b in ("ties", "clean", "classes20"))
    ix = open_product()
    a = hunt(ix, ["ties", "clean"])
    assert form(a) == (7, 1), a.path
    f = hunt(ix, ["classes20"])
    assert form(f) == (7, 4), f.path
    b = hunt(ix, ["ties", "clean"])
    assert form(b) == (7, 4), b.path
    assert _part(a, 0, n_t + n_c) == _part(b, 0, n_t + n_c)
    t = hunt(ix, ["ties"])
    assert form(t) == (7, 4), t.path
    assert _part(t, 0, n_t) == _part(a, 0, n_t)
    both = hunt(ix, ["classes20", "clean"])
    assert form(both) == (7, 4), both.path
    assert _part(both, n_f, n_c) == _part(a, n_t, n_c)
    assert _part(both, 0, n_f) == _part(f, 0, n_f)
    classic = hunt(ix, ["classes20", "clean"], compact=False)
    assert _key(classic) == _key(both)
    assert form(hunt(ix, ["classes14_d1"])) == (7, 4)      # the 14-nt family (it closes the text) at band width 7
    ix.close()


def test_band7_eight_hits_per_lane_without_context_records():
    """a handle opened with DG_OPEN_COMPACT has no context records (FmView::sax): every hit reads its flanks from the text and the
    rich width is 8.  <7,8> on the ties, on the family and on the family next to clean queries"""
    n_t, n_c, n_f = (len(V.batches()[b]["queries"]) for b in ("ties", "clean", "classes20"))
    ix = open_product(compact=True, pre5=False)
    t = hunt(ix, ["ties"])
    assert form(t) == (7, 8), t.path
    f = hunt(ix, ["classes20"])
    assert form(f) == (7, 8), f.path
    both = hunt(ix, ["classes20", "clean"])
    assert form(both) == (7, 8), both.path
    classic = hunt(ix, ["classes20", "clean"], compact=False)
    assert _key(classic) == _key(both)
    assert form(hunt(ix, ["classes14_d1"])) == (7, 8)
    ix.close()
    fresh = open_product(compact=True, pre5=False)
    a = hunt(fresh, ["ties", "clean"])
    assert form(a) == (7, 1), a.path
    fresh.close()
    assert _part(both, n_f, n_c) == _part(a, n_t, n_c) and _part(t, 0, n_t) == _part(a, 0, n_t)


# ------------------------------------------------------------------------------------------------------------ the band, distance 2

def test_band13_one_eight_and_four_hits_per_lane():
    """k_verify_memo<13,1> on a fresh handle, <13,8> on the 14-nt family, <13,4> on the family next to 20 clean queries and on the
    clean batch afterwards; the clean queries keep their answers"""
    n_f = len(V.batches()["classes14"]["queries"])
    ix = open_product()
    a = hunt(ix, ["clean_d2"])
    assert form(a) == (13, 1), a.path
    f = hunt(ix, ["classes14"])
    assert form(f) == (13, 8), f.path
    both = hunt(ix, ["classes14", "clean_d2"], counts=[None, 20])
    assert form(both) == (13, 4), both.path
    assert _part(both, n_f, 20) == _part(a, 0, 20) and _part(both, 0, n_f) == _part(f, 0, n_f)
    b = hunt(ix, ["clean_d2"])
    assert form(b) == (13, 4), b.path
    assert _key(a) == _key(b)
    classic = hunt(ix, ["classes14", "clean_d2"], counts=[None, 20], compact=False)
    assert _key(classic) == _key(both)
    # the 20-nt family (it opens the text) at band width 13: 4 queries alone, then beside 28 clean ones (4 781 / 32 = 149)
    assert form(hunt(ix, ["classes20_d2"])) == (13, 8)
    assert form(hunt(ix, ["classes20_d2", "clean_d2"], counts=[None, 28])) == (13, 4)
    ix.close()


# ------------------------------------------------------------------------------------------------ the other kernels: form 0 by length

_kernel_of = V.kernel_of


E1, E2 = V.cells_edge(1), V.cells_edge(2)
KERNELS = {"len24_d3": "k_verify<1,true,24>", "len25_d3": "k_verify<1,true,32>", "len32_d3": "k_verify<1,true,32>",
           "len24_d1": "k_verify_memo", "len25_d1": "k_verify_memo", "len32_d1": "k_verify_memo", "len33_d1": "k_verify<160,false>",
           "len%d_d1" % E1[0]: "k_verify<160,false>", "len%d_d1" % E1[1]: "k_verify<2200,false>",
           "len%d_d2" % E2[0]: "k_verify<160,false>", "len%d_d2" % E2[1]: "k_verify<2200,false>",
           "len255_d1": "k_verify<2200,false>", "len256_d1": "k_verify_long", "len300_d1": "k_verify_long",
           "len255_d2": "k_verify<2200,false>", "len256_d2": "k_verify_long", "len300_d2": "k_verify_long",
           "deep3": "k_verify<1,true,24>", "deep4": "k_verify<1,true,24>"}


@pytest.mark.parametrize("name", V.LENGTH_BATCHES + V.DEEP_BATCHES)
def test_the_longest_query_selects_the_kernel(shared, name):
    """each length batch alone, so that its longest query selects the kernel: compact and classic delivery, then the forward-only
    Hamming variant.  verify_kernel_form is 0 for every kernel but the band's; the batch's maxlen beside it names the kernel"""
    b = V.batches()[name]
    maxlen, d = max(len(q) for q in b["queries"]), b["kw"]["distance"]
    assert maxlen == b["maxlen"] and _kernel_of(maxlen, d) == KERNELS[name], (name, maxlen, d)
    band = KERNELS[name] == "k_verify_memo"
    got = hunt(shared, [name])
    classic = hunt(shared, [name], compact=False)
    assert _key(classic) == _key(got), name
    for r in (got, classic):
        assert (form(r)[0] == 7 and form(r)[1] in (1, 4, 8)) if band else r.path["verify_kernel_form"] == 0, (name, maxlen, r.path)
    if name + "_ham" in V.batches():
        ham = hunt(shared, [name + "_ham"])
        hc = hunt(shared, [name + "_ham"], compact=False)
        assert _key(hc) == _key(ham), name
        assert (form(ham)[0] == 7) if band else ham.path["verify_kernel_form"] == 0, (name, ham.path)
    assert sum(len(q.hits) for q in got.queries) == len(V.expected(name)) >= 3
