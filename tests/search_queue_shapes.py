"""Inputs for the survivor queue of k_search1s (dicey_amd/csrc/hunt_search.hpp) — from the reference side only: nothing here touches a
GPU or the library under test.

k_search1s asks the long presence filter (order K2) about the LAST K2 characters of every candidate of a (query, strand) group, then
about the FIRST K2 characters of every survivor longer than K2, and only what passes both windows is looked up in the K-mer table.
How many candidates of one workgroup pass the first window and how many pass both decides how the kernel's queue, its rounds and its
wavefronts behave, whether or not the whole string occurs.  The texts here fix both numbers per workgroup: a candidate's two windows
are planted as two pieces APART from each other (random spacers between all pieces), so that it passes both filters and dies at the
table entry or the pre5 line; a candidate's last window alone makes it a tail-only survivor.  Whole candidates are planted only
where a case wants occurring strings.

Pieces are planted one at a time against a running census of every candidate of the saturated workgroup (neighbouring candidates
share windows: the last K2 characters of a query are the last window of every candidate edited left of them), and a piece that
would move a census past its target is left out.  A case whose targets are not met raises: seeds are fixed, nothing is retried.
tests/test_search_queue_shapes_host.py repeats every census from scratch on the finished text, over all queries of the batch.

The planting, the candidate order, the batch layout and the oracle are those of tests/select_shapes.py."""
import random

import select_shapes as S
from conftest import revcomp
from select_shapes import K, K2, flat_candidates, gpw_of, layout  # noqa: F401  (the layout model the cases are built on)

FUSED_QCAP = 512
T_LEAVE = 64                     # hunt_search.hpp FUSED_TLEAVE: up to this many queue entries the wavefronts 1-3 end behind the dense phase
T_OTHER = 256                    # a bound the development build can be given (DICEY_EXP), and the size of a fresh handle's LDS list
LCAP0 = 256                      # a fresh handle's LDS list (hunt.hip, launch_flat1)
_memo = {}


def windows(w):
    """(what the first probe asks about, what the second one asks about or None) for a candidate string: strings of at least K2
    characters ask the long filter about their last K2, shorter ones the table's filter about their last K; strings longer than K2 are
    asked again about their first K2 (head_window_occurs)"""
    tail = w[-K2:] if len(w) >= K2 else w[-K:]
    return tail, (w[:K2] if len(w) > K2 else None)


def strands(q):
    return (q, revcomp(q))


class _Line:
    """the planted line with the census of one workgroup's candidates kept up to date piece by piece"""

    def __init__(self, rng, cands):
        self.rng, self.cands = rng, cands
        self.line = "".join(S._spacer(rng) for _ in range(16))     # (a text is never shorter than this: nothing planted is a case too)
        self.cuts = [len(self.line) // 2]
        self.index = {}
        for i, w in enumerate(cands):
            t, h = windows(w)
            self.index.setdefault(t, []).append((i, 0))
            if h is not None:
                self.index.setdefault(h, []).append((i, 1))
            self.index.setdefault(w, []).append((i, 2))
        self.lens = sorted({len(k) for k in self.index})
        self.flag = [[False, windows(w)[1] is None, False] for w in cands]   # tail window occurs, head window occurs (or none asked), string occurs

    def census(self, flag=None):
        flag = self.flag if flag is None else flag
        tail = sum(1 for f in flag if f[0])
        both = sum(1 for f in flag if f[0] and f[1])
        return tail - both, both, sum(1 for f in flag if f[2])

    def _new(self, piece):
        t, out = self.line + piece, []
        for k in self.lens:
            for i in range(max(0, len(self.line) - k + 1), len(t) - k + 1):
                if t[i:i + k] in self.index:
                    out += self.index[t[i:i + k]]
        return out

    def put(self, pieces, ok):
        """plant the pieces (each behind a spacer of its own) when ok(census afterwards) holds"""
        for again in range(4):      # (the line's last spacer can complete a string by accident: another one in front then)
            lead = S._spacer(self.rng) if again else ""
            piece = lead + "".join(p + S._spacer(self.rng) for p in pieces)
            hits = self._new(piece)
            flag = self.flag
            if hits:
                flag = [list(f) for f in self.flag]
                for i, kind in hits:
                    flag[i][kind] = True
            if ok(self.census(flag)):
                at = len(self.line) + len(lead)
                for p in pieces:
                    at += len(p)
                    self.cuts.append(at + S.SPACER // 2)
                    at += S.SPACER
                self.line += piece
                self.flag = flag
                return True
        return False


def _workgroup_queries(rng, m, take=True):
    """the queries of one whole workgroup (both strands of a query side by side)"""
    return [S._query(rng, m) for _ in range(gpw_of(m, take) // 2)]


def _case(seed, m, hamming, tail_only, both, occurring=0, pick=None):
    """One text and one batch of three workgroups of m-mers whose SECOND workgroup has exactly `tail_only` candidates that pass the last
    window alone, `both` that pass both windows without occurring, and `occurring` whole strings (which pass both as well).  pick:
    restricts the candidates that may be planted, (query index in the workgroup, strand, position) -> bool."""
    rng = random.Random(seed)
    sat = _workgroup_queries(rng, m)
    cands, where = [], []
    for qi, q in enumerate(sat):
        for st, s in enumerate(strands(q)):
            for w in flat_candidates(s, hamming):
                cands.append(w)
                where.append((qi, st))
    L = _Line(rng, cands)
    order = list(range(len(cands)))
    rng.shuffle(order)
    if pick is not None:
        order = [i for i in order if pick(i, cands[i], where[i])]
    for i in order:                                   # whole strings first: each brings both of its windows along
        t, b, o = L.census()
        if o >= occurring:
            break
        if not L.flag[i][2]:
            L.put([cands[i]], lambda c: c[2] <= occurring and c[1] <= both + occurring and c[0] <= tail_only)
    for i in order:                                   # both windows, apart from each other
        t, b, o = L.census()
        if b >= both + occurring:
            break
        f = L.flag[i]
        if not (f[0] and f[1]):
            tw, hw = windows(cands[i])       # (a string of at most K2 characters has one window)
            L.put([tw] if hw is None else [hw, tw], lambda c: c[2] == o and c[1] <= both + occurring and c[0] <= tail_only)
    for i in order:                                   # the last window alone
        t, b, o = L.census()
        if t >= tail_only:
            break
        if not L.flag[i][0]:
            L.put([windows(cands[i])[0]], lambda c: c[2] == o and c[1] == b and c[0] <= tail_only)
    got = L.census()
    if got != (tail_only, both + occurring, occurring):
        raise AssertionError("case (seed %d, %d nt, hamming %d) could not be built: census %r, wanted %r" % (seed, m, hamming, got, (tail_only, both + occurring, occurring)))
    text, seqlen = S._finish(L.line, L.cuts)
    per = len(sat)
    pads = S._padding(rng, m, 2 * per, text, 1, hamming, avoid=sat)
    qs = pads[:per] + sat + pads[per:]
    return {"text": text, "seqlen": seqlen, "names": ["sq_1", "sq_2"], "d": 1, "hamming": hamming, "qs": qs, "sat": list(range(per, 2 * per)),
            "m": m, "want": {"tail_only": tail_only, "both": both + occurring, "occurring": occurring}}


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------

# double survivors of the saturated workgroup: nothing, one, the leave boundary of the first wavefront (which is T_LEAVE), wavefront 2's
# first entry, around T_OTHER, and the second round.  Tail-only survivors are three times as many where a workgroup has that many candidates: 12 groups
# of 20-mers have about 1 800, of which about 1 280 can be given a window of their own, so from 313 double survivors on the tail-only ones are what is left of 1 250 (the parent's queue, which
# held both kinds, is past its second round there anyway).
DOUBLE = (0, 1, T_LEAVE - 1, T_LEAVE, T_LEAVE + 1, 128, 129, T_OTHER - 1, T_OTHER, T_OTHER + 1, FUSED_QCAP, FUSED_QCAP + 1)
LENGTHS = (K2 - 1, K2, K2 + 1, K2 + 2)


def _tail_only_for(n):
    return min(3 * n, 1250 - n)


def _one_lane(seed, tail_only_case):
    """One lane with all eight operations valid — position 1 of a 20-mer (query 2 of the workgroup, forward strand): a deletion, three
    substitutions, four insertions — whose eight strings all pass both windows, or all pass the last one only.  The edit sits left of
    the last window, which is the query's own last K2 characters: the candidates of the positions up to m - K2 pass it with them (and
    fail the first window)."""
    rng = random.Random(seed)
    m = 20
    sat = _workgroup_queries(rng, m)
    cands, first = [], {}
    for qi, q in enumerate(sat):
        for st, s in enumerate(strands(q)):
            first[qi, st] = len(cands)
            cands += flat_candidates(s, False)
    s = sat[2]
    mine = [s[1:]] + [a + s[1:] for a in "ACGT" if a != s[0]] + [s[0] + c + s[1:] for c in "ACGT"]
    if cands[first[2, 0]:first[2, 0] + 8] != mine:
        raise AssertionError("one-lane case: the lane of position 1 does not hold the eight strings expected")
    L = _Line(rng, cands)
    ok = L.put([s[-K2:]], lambda c: c[2] == 0)
    for w in mine if not tail_only_case else ():
        ok = ok and L.put([w[:K2]], lambda c: c[2] == 0)
    t, b, o = L.census()
    lane = L.flag[first[2, 0]:first[2, 0] + 8]
    if not ok or o or any(f[0] is not True or f[1] is tail_only_case for f in lane) or (b != 0 if tail_only_case else b < 8):   # (a spacer's character beside a window may spell a neighbour's window: the census says so)
        raise AssertionError("one-lane case could not be built: census %r" % ((t, b, o),))
    text, seqlen = S._finish(L.line, L.cuts)
    per = len(sat)
    pads = S._padding(rng, m, 2 * per, text, 1, False, avoid=sat)
    return {"text": text, "seqlen": seqlen, "names": ["sq_1", "sq_2"], "d": 1, "hamming": False, "qs": pads[:per] + sat + pads[per:],
            "sat": list(range(per, 2 * per)), "m": m, "want": {"tail_only": t, "both": b, "occurring": 0}}


def _cases():
    c = {}
    for n in DOUBLE:
        c["double%d" % n] = lambda n=n: _case(7000 + n, 20, False, _tail_only_for(n), n)
    for m in LENGTHS:
        for ham in (False, True):
            # (a head window exists for strings longer than K2 only: the insertions of a K2-mer, no string of a shorter query)
            # and the last window of a string of exactly K2 characters is the string: in Hamming mode a K2-mer's survivors all occur)
            tail_only = 10 if m + (0 if ham else 1) > K2 else 0
            both = 0 if (ham and m == K2) else 10
            c["len%d_%s" % (m, "ham" if ham else "edit")] = lambda m=m, ham=ham, t=tail_only, b=both: _case(7600 + 2 * m + ham, m, ham, t, b, 5)
    c["lane_both"] = lambda: _one_lane(7700, False)
    c["lane_tail"] = lambda: _one_lane(7701, True)
    c["overflow257"] = lambda: _case(7800, 20, False, 120, 40, LCAP0 + 1)
    return c


CASES = _cases()
GATING = (1, 3, 1000)            # max_locations: what the TAKE form's gating sees


def case(name):
    """{"text", "seqlen", "names", "d", "hamming", "qs", "sat": the saturated workgroup's queries, "m", "want": the census the case was
    built for (second workgroup alone)}, built once per process"""
    if name not in _memo:
        g = dict(CASES[name]())
        g["name"] = name
        _memo[name] = g
    return _memo[name]


def census(g):
    """From scratch on the finished text, over every query of the batch: {"valid": candidates (each asks a filter), "tail": those whose
    last window occurs, "head_asked": tail survivors longer than K2, "both": those that pass both windows, "occurring": candidates whose
    string occurs, "per_wg": {workgroup: (tail only, both, occurring)}}.  The filters hold the windows of the text's own sequences."""
    have = {}

    def occurs(w):
        if len(w) not in have:
            have[len(w)] = S.substrings(g["text"], len(w))
        return w in have[len(w)]
    out = {"valid": 0, "tail": 0, "head_asked": 0, "both": 0, "occurring": 0, "per_wg": {}}
    lay = layout(g["qs"], True)
    for qi, q in enumerate(g["qs"]):
        for st, s in enumerate(strands(q)):
            wg = lay[2 * qi + st][0]
            acc = out["per_wg"].setdefault(wg, [0, 0, 0])
            for w in flat_candidates(s, g["hamming"]):
                tw, hw = windows(w)
                out["valid"] += 1
                if not occurs(tw):
                    continue
                out["tail"] += 1
                out["head_asked"] += hw is not None
                if hw is None or occurs(hw):
                    out["both"] += 1
                    acc[1] += 1
                else:
                    acc[0] += 1
                if occurs(w):
                    out["occurring"] += 1
                    acc[2] += 1
    out["per_wg"] = {k: tuple(v) for k, v in out["per_wg"].items()}
    return out


def probes(c):
    """what ctr_filter_probes counts: every valid candidate asks a filter once, every survivor of that longer than K2 once more"""
    return c["valid"] + c["head_asked"]


# ctr_filter_probes, ctr_leaves, ctr_tab_reads and ctr_ext_steps of each case's batch as the PARENT of the commit that moved the head probe in front of the queue
# reported them on an MI355X (fresh handle settled by the batch's padding, max_locations 1000): the probe formula above was held
# against these before any build with the moved probe ran.  {case: (filter probes, leaves, table reads, extension steps)}: the first two follow from the census, the other two are the parent's word
PARENT_COUNTERS = {
    "double0": (4876, 0, 0, 0),
    "double1": (4860, 0, 1, 3),
    "double128": (5364, 0, 128, 462),
    "double129": (5362, 0, 129, 457),
    "double255": (5864, 0, 255, 897),
    "double256": (5883, 0, 256, 980),
    "double257": (5895, 0, 257, 948),
    "double512": (6106, 0, 512, 1950),
    "double513": (6121, 0, 513, 1996),
    "double63": (5120, 0, 63, 213),
    "double64": (5080, 0, 64, 221),
    "double65": (5118, 0, 65, 230),
    "lane_both": (4896, 0, 9, 28),
    "lane_tail": (4891, 0, 0, 0),
    "len13_edit": (4146, 5, 15, 0),
    "len13_ham": (1920, 5, 15, 0),
    "len14_edit": (4503, 5, 15, 0),
    "len14_ham": (2064, 5, 5, 0),
    "len15_edit": (4850, 5, 15, 0),
    "len15_ham": (2233, 5, 15, 0),
    "len16_edit": (5205, 5, 15, 0),
    "len16_ham": (2377, 5, 15, 0),
    "overflow257": (5261, 257, 297, 2240),
}
