"""dg_padlock_scan against the plain model of tests/padlock_shapes.py: every slot of the six per-position arrays and the three
work counters, for every entry of the parameter matrix; then what a second call on the same handles can get wrong (the result
pool hands back a block that still holds the previous result, the per-thread buffers keep their contents), batch order, and
the empty batches.  Doubles compare by bit pattern, integers exactly.

The model's temperatures come from the reference's own thal() where oracle/_ref is present, else from dicey_amd.Thal.tm on
explicit pairs (dg_thal_batch, which test_gpu_thal_reference.py pins to the reference) so that the filter and count stages are
still tested; its counts come from the oracle on an index the oracle built itself.  tests/test_padlock_shapes_host.py holds
the conditions that make these comparisons worth something.  No test switches: product library only."""
import gc

import numpy as np
import pytest

import oracle_lib as O
import padlock_shapes as P
import thal_expect as TE

pytestmark = pytest.mark.gpu
DOUBLES = ("arm_gc", "arm_tm", "probe_gc", "probe_tm")
INTS = ("arm_count", "arm_nbcount")
COUNTERS = ("n_arm_thal", "n_probe_thal", "n_arms_counted")
DEFAULTS = P.MATRIX[0]
DG_EINVAL = -1                 # include/dicey_gpu.h


class Scanner:
    def __init__(self, d):
        import dicey_amd
        text = P.genome()["text"]
        fm9, ofm9 = str(d / "gpu.fm9"), str(d / "oracle.fm9")
        dicey_amd.build_index(text, fm9)
        O.build_fm9(text, ofm9)
        self.orc = O.Index(ofm9)
        self.ix = dicey_amd.FmIndex(fm9)
        self.th = dicey_amd.Thal(O.PRIMER3_CONFIG)
        pairs = P.ref_thal_pairs if TE.have_ref() else lambda ps: [t for t, _, _ in self.th.tm(ps)]
        self.memo = P.oracle_memo(self.orc, pairs)
        self._models = {}

    def scan(self, exons, params):
        import dicey_amd
        L, distance, hamming, tmdiff, gc_min, gc_max = params
        return dicey_amd.padlock_scan(self.ix, self.th, [e.encode() for e in exons], armlen=L, distance=distance, hamming=hamming,
                                      tmdiff=tmdiff, gc_min=gc_min, gc_max=gc_max)

    def model(self, exons, params):
        key = (tuple(exons), params)
        if key not in self._models:
            self._models[key] = self.memo.model(exons, params)
        return self._models[key]

    def close(self):
        self.th.close()
        self.ix.close()
        self.orc.close()


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    s = Scanner(tmp_path_factory.mktemp("padlock_shapes"))
    yield s
    s.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _equal(R, m, what):
    """every slot of every array, and the counters, against a model (or a dict shaped like one)"""
    assert [int(x) for x in R["pos_off"]] == [int(x) for x in m["pos_off"]], what
    n = int(m["pos_off"][-1])
    for k in DOUBLES:
        assert len(R[k]) == n, (what, k)
        bad = np.nonzero(_bits(R[k]) != _bits(m[k]))[0]
        assert not len(bad), (what, k, len(bad), [(int(i), TE.hexd(R[k][i]), TE.hexd(m[k][i]), R[k][i], m[k][i]) for i in bad[:4]])
    for k in INTS:
        assert len(R[k]) == n and R[k].dtype == np.int64, (what, k)
        bad = np.nonzero(R[k] != np.asarray(m[k], dtype=np.int64))[0]
        assert not len(bad), (what, k, len(bad), [(int(i), int(R[k][i]), int(m[k][i])) for i in bad[:4]])
        assert not (R[k] == -2).any(), (what, k)        # "queued" never leaves the library
    for k in COUNTERS:
        assert R[k] == m[k], (what, k, R[k], m[k])


def _copy(R):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in R.items()}


def _slices(R):
    """per exon: the six array slices"""
    off = [int(x) for x in R["pos_off"]]
    return [tuple(R[k][off[e]:off[e + 1]].tobytes() for k in DOUBLES + INTS) for e in range(len(off) - 1)]


@pytest.mark.parametrize("params", P.MATRIX, ids=P.entry_id)
def test_scan_equals_model_in_every_slot(S, params):
    exons = P.exons(params)
    m = S.model(exons, params)
    R = S.scan(exons, params)
    _equal(R, m, P.entry_id(params))
    assert m["n_arms_counted"] >= 10
    if params[1] == 0:
        assert (R["arm_nbcount"] == -1).all()


def test_a_result_owes_nothing_to_the_one_before(S):
    """Full list, a list of under a tenth of its positions, the full list again, each after the last result went back to the pool
    (a block of at most twice the positions asked for + 4096 is taken again: the small scan is sized to take the full one's)."""
    full = P.exons(DEFAULTS)
    named = dict(P.named_exons(DEFAULTS[0]))
    small = [named[n] for n in ("two_arms", "near_piece", "short", "empty", "identical_1")]
    m_full, m_small = S.model(full, DEFAULTS), S.model(small, DEFAULTS)
    n_full, n_small = m_full["pos_off"][-1], m_small["pos_off"][-1]
    assert 0 < 10 * n_small < n_full and m_small["n_arms_counted"] > 0
    where = []
    for exons, m, what in ((full, m_full, "full"), (small, m_small, "small after full"), (full, m_full, "full after small")):
        R = S.scan(exons, DEFAULTS)
        where.append(R["arm_gc"].ctypes.data)
        _equal(R, m, what)
        del R
        gc.collect()
    print("result blocks at", [hex(a) for a in where])


def test_exon_order_and_batch_cuts_do_not_change_an_exon(S):
    full = P.exons(DEFAULTS)
    want = _slices(_copy(S.scan(full, DEFAULTS)))
    m = S.model(full, DEFAULTS)
    assert len({w for w in want if w[0]}) >= 10
    got = _slices(S.scan(full[::-1], DEFAULTS))
    assert got[::-1] == want
    cut = len(full) // 2
    a, b = S.scan(full[:cut], DEFAULTS), S.scan(full[cut:], DEFAULTS)
    assert _slices(a) + _slices(b) == want
    for k in COUNTERS:      # (no arm belongs to two exons)
        assert a[k] + b[k] == m[k], k
    names = [n for n, _ in P.named_exons(DEFAULTS[0])]
    assert want[names.index("identical_1")] == want[names.index("identical_2")]      # same arms, slots of their own, both counted


def test_distance_0_right_after_distance_1_leaves_no_neighbourhood_count(S):
    full = P.exons(DEFAULTS)
    d0 = (DEFAULTS[0], 0) + DEFAULTS[2:]
    R1 = S.scan(full, DEFAULTS)
    assert (R1["arm_nbcount"] >= 0).sum() >= 100
    del R1
    gc.collect()
    R0 = S.scan(full, d0)
    assert (R0["arm_nbcount"] == -1).all() and (R0["arm_count"] >= 0).sum() >= 100
    _equal(R0, S.model(full, d0), "distance 0 after distance 1")


def test_batches_without_a_position(S):
    T = 2 * DEFAULTS[0]
    named = dict(P.named_exons(DEFAULTS[0]))
    for exons in ([], [named["short"]], [named["empty"], named["short"], "ACGT", named["short"][:T - 2]]):
        R = S.scan(exons, DEFAULTS)
        assert [int(x) for x in R["pos_off"]] == [0] * (len(exons) + 1)
        assert all(len(R[k]) == 0 for k in DOUBLES + INTS) and all(R[k] == 0 for k in COUNTERS)
        _equal(R, S.model(exons, DEFAULTS), "no position")
    full = P.exons(DEFAULTS)
    _equal(S.scan(full, DEFAULTS), S.model(full, DEFAULTS), "full after the empty batches")


def test_arms_under_10_nt_with_a_distance_are_refused_before_any_work(S):
    """dg_neighborhood_count takes 10 nt or more; the scan refuses the combination at once with DG_EINVAL (include/dicey_gpu.h)
    and the handles serve the next scan"""
    from dicey_amd import _capi
    exons = P.exons((8, 1, False, 2, 0.4, 0.6))
    for hamming in (False, True):
        with pytest.raises(_capi.DgError) as ei:
            S.scan(exons, (8, 1, hamming, 2, 0.4, 0.6))
        assert ei.value.code == DG_EINVAL and "10 nt" in str(ei.value)
    with pytest.raises(_capi.DgError) as ei:
        S.scan(exons, (9, 2, True, 2, 0.4, 0.6))
    assert ei.value.code == DG_EINVAL
    full = P.exons(DEFAULTS)
    _equal(S.scan(full, DEFAULTS), S.model(full, DEFAULTS), "after the refusal")
