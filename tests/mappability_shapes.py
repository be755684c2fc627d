"""Inputs for the mappability family (-e 1|2, -u, -q, -q -l, -q -a, -q -l -E, -q -I) on the genome shapes of tests/genome_shapes.py: which
shapes, the query records cut from each shape's own sequences, and the parameter grids.  tests/test_mappability_shapes_host.py shows on
the references alone that these inputs exercise what they claim; tests/test_gpu_mappability_shapes.py runs the library on them.  A plain
module: no fixtures, no pytest hooks."""
import random
import re

import numpy as np

import genome_shapes as S
import mappability_ref as R
import query_anchor_ref as A
import query_iupac_ref as I
from conftest import revcomp

CUT = 800                        # many_short_800: the first 800 records of many_short (the ball reference at k = 12, e = 2 takes 15 s on
                                 # the full 400 kb text and 2 to 4 s on texts of 55 to 160 kb)
BIG = ["many_short_800", "hard_masked", "bisulfite", "at_tandem", "iupac_rich"]
FOUR = ["hard_masked", "bisulfite", "at_tandem", "iupac_rich"]     # the open-flag and development-build matrices
MU_ONLY = ["single_no_n"]        # minimum unique length only
TINY = list(S.TINY_NAMES)
SHAPES = BIG + TINY              # every call but min_unique, which runs on SHAPES + MU_ONLY
ABSENT = {"bisulfite": "C", "at_tandem": "CG"}   # the letters the text lacks
# the IUPAC model (query_iupac_ref.parts) walks every shift between the records and the text, and on the tandem text no shift is ruled
# out early: 31 s against the 100 kb text even for 600 bytes of records.  The IUPAC call alone runs against a 30 kb cut of that shape
IUPAC_TEXT = {"at_tandem": "at_tandem_30k"}
BUFFER_LIMIT = 6000              # bytes of a shape's whole query buffer: every query reference stays cheap

_cache = {}


def get(name):
    """the shape: one of genome_shapes.all_shapes(), or the cut of many_short"""
    if name not in _cache:
        if name == "many_short_800":
            g = S._shape(S.all_shapes()["many_short"]["seqs"][:CUT], "ctg")
            lens = [len(s) for s in g["seqs"]]
            assert [i for i, m in enumerate(lens) if m == 0] == [0, 5, 700, 701]     # the first record, and an adjacent pair
            assert 80 <= sum(1 for m in lens if 1 <= m <= 19) <= 90
            assert g["text"][:1] == b"\n" and 55000 <= len(g["text"]) <= 160000
            _cache[name] = g
        elif name == "at_tandem_30k":
            s0, s1 = S.all_shapes()["at_tandem"]["seqs"]
            _cache[name] = S._shape([s0[24000:44000], s1[:10000]], "sat")     # the last 6 kb of the 30 kb repeat and what follows
        else:
            _cache[name] = S.all_shapes()[name]
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------------------------------
# parameter grids

def count_cells(name):
    """(k, e) of the count calls: k in {12, 20} at e in {0, 1}; e = 2 at k = 12 everywhere and at k = 20 where the ball reference is
    cheap (measured: 0.5 s on at_tandem, 6 s on bisulfite, up to 10 s elsewhere)"""
    return [(12, 0), (12, 1), (20, 0), (20, 1), (12, 2)] + ([(20, 2)] if name in ("at_tandem", "bisulfite") else [])


STRANDS = (False, True)          # forward_only
MAX_COUNTS = (0, 2)


def anchors_of(k):
    return [0, 1, 5, 8, 9, k]


MIN_K, MAX_K = 10, 24            # query_min_length / query_min_length_end
AT_MOST = (0, 1, 50)             # 50: on at_tandem nothing is rare
MINLEN_ES = (0, 1)
END_ANCHORS = (0, 5, 10)
MAX_DEGENERACY = 4096


def mu_max_ks(name):
    return (24,) if name in MU_ONLY else (24, 100)


# ---------------------------------------------------------------------------------------------------------------------------------
# the text with its special bytes put back

def restored(text: bytes) -> bytes:
    """the text with every byte that is not A/C/G/T (N, ambiguity letters, the '\\n' between records; not the final '\\n') replaced by a
    base that depends on the position alone: the windows these bytes kept from counting are there again"""
    t = np.frombuffer(text, dtype=np.uint8).copy()
    bad = R._CODE[t] == 255
    bad[-1] = False
    pos = np.nonzero(bad)[0]
    t[pos] = np.frombuffer(b"ACGT", dtype=np.uint8)[((pos * 2654435761) >> 13) & 3]
    return t.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# query records

def as_bytes(recs):
    """the records as the library sees them: str records are upper-cased, bytes go through as given"""
    return [r.upper().encode() if isinstance(r, str) else bytes(r) for r in recs]


_rnd = S._rnd


def _special(name, g, t):
    """byte ranges [a, b) of the text at which the shape is special, each with 60 bases of A/C/G/T on either side"""
    flank = 60
    ok = lambda a, b: a >= flank and set(t[a - flank:a] + t[b:b + flank]) <= set("ACGT") and len(t[b:b + flank]) == flank
    if name in ("hard_masked", "bisulfite"):            # the two shortest N runs
        runs = [(m.end() - m.start(), m.start()) for m in re.finditer("N+", t)]
        return [(a, a + n) for n, a in sorted(runs) if ok(a, a + n)][:2]
    if name == "iupac_rich":                            # three ambiguity stretches
        runs = [(m.start(), m.end()) for m in re.finditer("[%s]+" % S.AMBIG, t)]
        return [(a, b) for a, b in runs if ok(a, b)][:3]
    if name == "many_short_800":                        # six '\n' between two records
        seps = [i for i in range(1, len(t) - 1) if t[i] == "\n"]
        return [(i, i + 1) for i in seps if ok(i, i + 1)][10:16]
    if name == "at_tandem":                             # the '\n' between the two sequences
        i = t.index("\n")
        return [(i, i + 1)] if ok(i, i + 1) else []
    return []


def _unit_join(s):
    """the place where the first tandem repeat of the sequence ends: the first index that breaks its period"""
    u = next(u for u in range(1, 8) if s[:70] == (s[:u] * 70)[:70])
    return next(i for i in range(u, len(s)) if s[i] != s[i - u])


def records(name, g):
    """{"plain": records for the count, anchored and minimum-length calls, "iupac": records for the IUPAC call}; bytes, and one str.
    Seeded by the shape's name and cut from the shape's own sequences, no fixed offsets.  plain: two cuts of 150-400 nt from the longest
    A/C/G/T stretches as they are; a third with a substitution every 13th base, and its reverse complement; cuts straight across the
    places where the shape is special (_special; on the tandem text also across the join of two unit lengths), as the text shows them and
    with the special bytes put back; 200 random bases; a lower-case str, an empty record and a 9-mer.  iupac: copies of the cuts with hit
    and miss codes every 9th base, on iupac_rich two cuts whose code letters are the genome's own ambiguity bytes, and the short records.
    A tiny shape gets its whole text with N for '\\n', the reverse complement of that and a random 30-mer, for both calls."""
    rng = random.Random(S.hash_name(name) + 77)
    t = g["text"].decode()
    if name.startswith("tiny_"):
        whole = t.replace("\n", "N")
        recs = [whole.encode(), revcomp(whole).encode(), _rnd(rng, 30).encode()]
        return {"plain": recs, "iupac": list(recs)}
    stretches = sorted(((m.end() - m.start(), m.start()) for m in re.finditer("[ACGT]+", t)), reverse=True)[:6]

    def cut(i):
        ln, a = stretches[i % len(stretches)]
        m = min(ln, rng.randint(150, 400))
        o = a + rng.randrange(ln - m + 1)
        return t[o:o + m]

    c1, c2, c3 = cut(0), cut(1), cut(2)
    sub = A._subst_every(c3, 13)
    plain = [c1, c2, sub, revcomp(sub)]
    # across the places where the shape is special: as the text shows them, and with the special bytes put back
    tr = restored(g["text"]).decode()
    places = _special(name, g, t)
    for a, b in places:
        if name in ("many_short_800", "at_tandem"):
            plain.append(t[a - 60:a] + t[b:b + 60])     # the neighbours concatenated without the '\n'
        else:
            plain.append(t[a - 60:b + 60])
        plain.append(tr[a - 60:b + 60])
    if name == "at_tandem":
        j = _unit_join(g["seqs"][0])
        plain.append(g["seqs"][0][j - 150:j + 150])
    plain.append(_rnd(rng, 200))                        # on bisulfite and at_tandem it holds the letters the text lacks
    low = c1[:100].lower()                              # a str record: the library upper-cases it
    # for the IUPAC call: hit and miss codes every 9th base.  The model's cost follows the number of shifts with a near window: on the
    # three- and two-letter texts most shifts have one, so their copies are shorter
    m = {"at_tandem": 90, "bisulfite": 120}.get(name, 250)
    coded = [I.put_codes(c1[:m], 9, "hit", rng), I.put_codes(c2[:m], 9, "miss", rng), I.put_codes(sub[:m], 9, "hit", rng),
             I.revcomp(I.put_codes(sub[:m], 9, "miss", rng))]
    if name == "iupac_rich":                            # the code letters are the very ambiguity bytes the genome shows at that place
        a, b = places[0]
        coded.append(t[b - 2:b + 40])
        coded.append(t[a - 40:a + 2])
    iupac = coded + [c1[:m // 2], _rnd(rng, 60)]
    out = {"plain": [r.encode() for r in plain] + [low, b"", _rnd(rng, 9).encode()],
           "iupac": [r.encode() for r in iupac] + [low, b"", b"ACGTRYKMA"]}
    for recs in out.values():
        assert sum(len(r) + 1 for r in recs) < BUFFER_LIMIT, (name, sum(len(r) + 1 for r in recs))
    return out
