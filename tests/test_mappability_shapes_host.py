"""No GPU: the inputs of tests/mappability_shapes.py exercise what they claim, shown on the brute-force references alone, and the
references that tests/test_gpu_mappability_shapes.py trusts agree with their independent second routes on these texts."""
import random

import numpy as np
import pytest

import mappability_mm_ref as M
import mappability_ref as R
import mappability_shapes as P
import min_unique_ref as U
import query_iupac_ref as I
import query_map_ref as Q
import query_min_len_ref as QL

_memo = {}


def _track(name, k, e):
    """fwd + rev of the ball reference over the shape's text, once per process"""
    key = (name, k, e)
    if key not in _memo:
        fwd, rev = M.parts_ball(P.get(name)["text"], k, e)
        _memo[key] = fwd + rev
    return _memo[key]


def _query(name, text, k, e, tag=""):
    """(values, valid) of the plain records against `text`"""
    key = (name, k, e, tag)
    if key not in _memo:
        qbuf, _ = Q.buffer_of(P.as_bytes(P.records(name, P.get(name))["plain"]))
        fwd, rev, valid = Q.parts_ball(text, qbuf, k, e)
        _memo[key] = (fwd + rev, valid, qbuf)
    return _memo[key]


def test_the_cut_keeps_what_many_short_is_for():
    g = P.get("many_short_800")
    lens = [len(s) for s in g["seqs"]]
    assert len(lens) == 800 and lens[0] == lens[5] == lens[700] == lens[701] == 0 and lens.count(0) == 4
    assert 80 <= sum(1 for m in lens if 1 <= m <= 19) <= 90
    assert g["text"].startswith(b"\n") and b"\n\n\n" in g["text"]
    assert g["seqs"] == P.S.all_shapes()["many_short"]["seqs"][:800]


@pytest.mark.parametrize("name", P.SHAPES)
def test_records_are_seeded_small_and_of_every_kind(name):
    g = P.get(name)
    recs = P.records(name, g)
    assert recs == P.records(name, g)
    for key in ("plain", "iupac"):
        b = P.as_bytes(recs[key])
        # (a tiny shape's records are its text twice and a 30-mer: 8.2 kb at 4 097 symbols, against a text of 4 kb)
        assert sum(len(r) + 1 for r in b) < (2 * len(g["text"]) + 40 if name in P.TINY else P.BUFFER_LIMIT) and all(b"\n" not in r for r in b)
    if name in P.TINY:
        whole = P.as_bytes(recs["plain"])[0]
        assert len(whole) == len(g["text"]) and whole.count(b"N") >= g["text"].count(b"\n") and len(recs["plain"][2]) == 30
        return
    plain = recs["plain"]
    assert set(plain[0]) <= set(b"ACGT") and set(plain[1]) <= set(b"ACGT") and len(plain[0]) >= 40
    assert any(isinstance(r, str) and r.islower() for r in plain) and b"" in plain and any(len(r) == 9 for r in plain)
    assert plain[3] == P.revcomp(plain[2].decode()).encode() and plain[2] != plain[3]
    t = g["text"].decode()
    assert plain[0].decode() in t and plain[1].decode() in t and plain[2].decode() not in t
    coded = [r for r in P.as_bytes(recs["iupac"]) if set(r) & set(b"RYSWKMBDHV")]
    assert len(coded) >= 4
    if name in P.ABSENT:
        assert not set(P.ABSENT[name].encode()) & set(g["text"])
        assert any(set(P.ABSENT[name].encode()) <= set(r) for r in P.as_bytes(plain))
    if name == "iupac_rich":  # a record whose code letters are the genome's own bytes at that place
        own = [r for r in P.as_bytes(recs["iupac"]) if r.decode() in t and set(r) & set(P.S.AMBIG.encode())]
        assert len(own) == 2 and all(0 < I.deg(r.decode()[:12]) <= 16 or 0 < I.deg(r.decode()[-12:]) <= 16 for r in own)
    if name == "hard_masked":
        assert any(b"N" * 50 in r for r in plain)
    if name == "at_tandem":   # a record over the join of two unit lengths: its two halves have different periods
        j = P._unit_join(g["seqs"][0])
        assert g["seqs"][0][j - 150:j + 150].encode() in plain and j >= 20000


@pytest.mark.parametrize("name", P.BIG)
def test_values_grow_with_the_budget(name):
    """at k = 12 at least 1 000 positions gain at e = 1 and at least 1 000 more at e = 2 (measured on the full shapes: at least 6 108).
    No floor at k = 20 on iupac_rich, where e = 1 adds 11 positions."""
    v = {e: _track(name, 12, e) for e in (0, 1, 2)}
    g1, g2 = int((v[1] > v[0]).sum()), int((v[2] > v[1]).sum())
    print("growth %s k=12: e1 %d, e2 %d" % (name, g1, g2))
    assert g1 >= 1000 and g2 >= 1000, (name, g1, g2)
    assert (v[1] >= v[0]).all() and (v[2] >= v[1]).all()


@pytest.mark.parametrize("name", P.BIG)
def test_record_kmers_have_twins_behind_a_special_byte(name):
    """record 12-mers that have, within one substitution, a window of the text that holds an N, an ambiguity letter or a '\\n': with the
    byte put back (mappability_shapes.restored) their count rises, and nothing else differs between the two texts"""
    text = P.get(name)["text"]
    back = P.restored(text)
    assert len(back) == len(text) and back[-1:] == b"\n" and set(back[:-1]) <= set(b"ACGT")
    diff = np.frombuffer(back, np.uint8) != np.frombuffer(text, np.uint8)
    assert (R._CODE[np.frombuffer(text, np.uint8)][diff] == 255).all()
    v0, valid, _ = _query(name, text, 12, 1)
    v1, valid1, _ = _query(name, back, 12, 1, "restored")
    assert (valid == valid1).all() and (v1 >= v0).all()
    rise = int((v1 > v0)[valid].sum())
    print("special bytes %s: %d record 12-mers rise" % (name, rise))
    assert rise >= (5 if name in ("at_tandem", "bisulfite") else 50), (name, rise)


@pytest.mark.parametrize("name", sorted(P.ABSENT))
def test_kmers_with_a_letter_the_text_lacks_still_count(name):
    absent = np.isin(np.frombuffer(_query(name, P.get(name)["text"], 12, 1)[2], np.uint8), list(P.ABSENT[name].encode()))
    cs = np.concatenate([[0], np.cumsum(absent)])
    n = 0
    for e in (1, 2):
        v, valid, qbuf = _query(name, P.get(name)["text"], 12, e)
        holds = np.zeros(len(qbuf), bool)
        holds[:len(qbuf) - 11] = (cs[12:] - cs[:-12]) > 0
        n = max(n, int((valid & holds & (v > 0)).sum()))
    print("absent letters %s: %d record 12-mers" % (name, n))
    assert n >= 100, (name, n)


def test_minimum_unique_length_meets_its_cap_and_its_runs():
    t = P.get("at_tandem")["text"]
    v = U.by_values(t, 100)
    acgt = U.run_lengths(t) > 0
    assert int((v > 0).sum()) == 8311 and int((v[acgt] == 0).sum()) >= 1000   # still repeated at max_k = 100
    t = P.get("hard_masked")["text"]
    v, run = U.by_values(t, 100), U.run_lengths(t)
    near = (v > 0) & (run - v <= 3)
    assert near.sum() >= 1 and (v <= np.minimum(run, 100)).all()
    t = P.get("single_no_n")["text"]
    assert (U.run_lengths(t)[:-1] == np.arange(len(t) - 1, 0, -1)).all()     # no byte outside A/C/G/T before the end of the text


@pytest.mark.parametrize("name", P.TINY)
def test_tiny_shapes(name):
    g = P.get(name)
    text = g["text"]
    recs = P.as_bytes(P.records(name, g)["plain"])
    qbuf, _ = Q.buffer_of(recs)
    if len(text) < 20:   # nothing to count, nothing valid, apart from the random 30-mer
        for k, e in P.count_cells(name):
            assert not M.values(text, k, e).any()
            got = Q.values(text, recs, k, e)
            assert all((x == Q.INVALID).all() for x in got[:2]) and not (got[2][got[2] != Q.INVALID]).any()
        parts = QL.parts_by_k(text, qbuf, range(P.MIN_K, P.MAX_K + 1), 0)
        ml = QL.split(QL.min_len(parts, qbuf, P.MIN_K, P.MAX_K), recs)
        assert all((x == QL.INVALID).all() for x in ml[:2]) and set(ml[2].tolist()) <= {P.MIN_K, QL.INVALID}
    if len(text) >= 62:
        # valid 32-mers, what min_unique at max_k = 100 can walk: 7 on tiny_62, 6 on tiny_63, 10 on tiny_64, 5 on tiny_65 (two of its four
        # sequences are shorter than 12), 18 and more from tiny_127 on; valid 12-mers: 25 (tiny_65) and more
        n32, n12 = int(R.valid_positions(text, 32).sum()), int(R.valid_positions(text, 12).sum())
        assert n32 >= {62: 7, 63: 6, 64: 10, 65: 5}.get(len(text), 18) and n12 >= 25, (name, n32, n12)
        assert M.values(text, 12, 0).any()


@pytest.mark.parametrize("name", ["many_short_800", "bisulfite"])
def test_the_references_agree_with_their_second_routes(name):
    text = P.get(name)["text"]
    rng = random.Random(P.S.hash_name(name) + 5)
    for k, e in ((12, 2), (20, 1)):
        ok = np.nonzero(R.valid_positions(text, k))[0]
        grew = np.nonzero(_track(name, k, e) > _track(name, k, 0))[0]
        assert len(grew) >= 80, (name, k, e, len(grew))
        ps = sorted(rng.sample(ok.tolist(), 120) + rng.sample(grew.tolist(), 80))
        assert (M.direct(text, k, e, ps) == _track(name, k, e)[ps]).all(), (name, k, e)
    # the whole array on the forward strand; both strands (direct searches the text once per position and length for the reverse
    # complement: 51 s on the 107 kb cut) on the text of the first records, up to 30 kb
    seqs = P.get(name)["seqs"]
    head = P.S._shape(seqs[:next(i for i in range(1, len(seqs) + 1) if sum(len(s) + 1 for s in seqs[:i]) >= 30000 or i == len(seqs))])["text"]
    for t, fo, floor in ((text, True, 50000), (head, False, 20000)):
        a, b = U.by_values(t, 24, fo), U.direct(t, 24, fo)
        assert (a == b).all() and (a > 0).sum() >= floor, (name, fo, np.nonzero(a != b)[0][:10])
