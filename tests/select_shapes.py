"""Inputs for the search and select stages of `dicey hunt` (dicey_amd/csrc/hunt_search.hpp: k_search1s, k_search2p<true, .>;
hunt_select.hpp: k_group_pack, k_group_select, k_leaf_alive, k_leaf_rank, k_group, k_select, k_take) at the occupancies where the two
stages change the code that answers — from the reference side only: nothing here touches a GPU or the library under test.

The mechanism is a SATURATED text.  For a query q the search stage enumerates candidate strings (distance 1: deletions, substitutions,
insertions; distance 2: pairs of those) and the select stage keeps the candidates that occur, without duplicates and without any string
that contains another one, in std::set order.  On a random text almost no candidate occurs; saturated() plants a chosen subset of q's
candidates between short random spacers, so the number of occurring strings of one (query, strand) group — and of one workgroup of
k_search1s, which owns `gpw` consecutive groups — is whatever a case asks for.  Spacers can complete a candidate by accident and a
planted string can contain another candidate (the substitution of q's first character contains the deletion of it), so strings are
planted one at a time against a running census of every candidate of every saturated group, and a string that would move a census
past its target is planted with another spacer or left out.  tests/test_select_shapes_host.py repeats the census from scratch on
the finished text.

The batch layout restated (dicey_amd/csrc/hunt.hip launch_flat1, hunt_hints.hpp start_caps):

    const u32 ipg = std::min(pl.maxlen, 31u), ...                                                               // hunt.hip:843
    const u32 gpw = at.prep_in ? (std::min(16u, 256u / ipg) & ~1u) : std::min(16u, 256u / ipg);                 // hunt.hip:845
    const dim3 g1(ceil_div(pl.ngrp, gpw)), b1(256);                                                             // hunt.hip:854
    const u32 lcap = ... (ix->hints.fused_leaves > 48ull * g1.x ? FUSED_LCAP : FUSED_LCAP / 2);                 // launch_flat1
    at.shard_cap = std::max<u32>(h.shard_cap, (u32)std::max<u64>(64, (16 * f.nq + f.nxs / 8) / NSHARD));       // start_caps
    at.flat_req = h.flat_cap ? h.flat_cap : at.shard_cap;                                                       // start_caps
    const u32 g_first = blockIdx.x * gpw;  ...  const u32 shard = blockIdx.x & (NSHARD - 1);                    // hunt_search.hpp:685, 745

group 2 i + strand belongs to query i; workgroup = group // gpw; Sel slice = workgroup & 1023; a slice of a fresh handle holds 64 kept
strings while the batch has fewer than 4 096 queries.  Distance 2: one workgroup per group (hunt.hip:890)."""
import os
import random
import tempfile

import oracle_lib as O
from conftest import revcomp

K, K2 = 12, 14                   # the table orders every case opens its index with (DICEY_KMER_K / DICEY_KMER_K2)
SPACER = 14
# the stages' capacities (hunt_search.hpp:648-649, 1114-1115; hunt_select.hpp:195, 383; hunt_internal.hpp:70)
FUSED_LCAP, FUSED_QCAP, FUSED2_LCAP, SELCAP, PACK_MAX_LEN, NSHARD, FLAT_CAP0 = 512, 512, 512, 1024, 42, 1024, 64
_memo = {}


class _Retry(Exception):
    pass


# ---- the batch layout model ----------------------------------------------------------------------------------------------------------------

def gpw_of(maxlen, take):
    """groups per workgroup of k_search1s (hunt.hip:843-845); take: the TAKE form (both strands of a query in one workgroup)"""
    ipg = min(maxlen, 31)
    g = min(16, 256 // ipg)
    return g & ~1 if take else g


def layout(qs, take):
    """[(workgroup, local slot)] per group 2 i + strand of a distance-1 batch"""
    gpw = gpw_of(max(len(q) for q in qs), take)
    return [(g // gpw, g % gpw) for g in range(2 * len(qs))]


def per_workgroup(batch, key, take):
    """{workgroup: sum of batch[key][group]} under the layout model"""
    out = {}
    lay = layout(batch["qs"], take)
    for g, v in batch[key].items():
        out[lay[g][0]] = out.get(lay[g][0], 0) + v
    return out


def flat_cap(nq):
    """entries per slice of the flat Sel region on a fresh handle (hunt.hip:738, 742)"""
    return max(FLAT_CAP0, 16 * nq // NSHARD)


# ---- candidates ----------------------------------------------------------------------------------------------------------------------------

def candidates(q, d, hamming):
    """every string the reference's walk generates for q (neighbors.h:47-83: delete, keep, substitute, insert in front, position by
    position; a leaf is taken when an edit was spent), duplicates included; the query itself is not among them unless an edit path
    spells it"""
    out = []

    def walk(s, dist, pos):
        if pos >= len(s):
            if dist < d:
                out.append(s)
            return
        if dist > 0 and not hamming:
            walk(s[:pos] + s[pos + 1:], dist - 1, pos)
        walk(s, dist, pos + 1)
        if dist > 0:
            for a in "ACGT":
                if a != s[pos]:
                    walk(s[:pos] + a + s[pos + 1:], dist - 1, pos + 1)
            if not hamming:
                for a in "ACGT":
                    walk(s[:pos] + a + s[pos:], dist - 1, pos + 1)
    walk(q, d, 0)
    return out


def flat_candidates(q, hamming):
    """the (position, operation) candidates k_search1s looks up for one strand, in its own order (cand1, hunt_search.hpp:376-407:
    "deleting either of two equal neighbours gives the same string: the right-most character of a run does it"; "nothing after the
    last character; and a base inserted right of an equal one is the string of the insertion one position further left (which exists
    from the second position on)"; Hamming mode: the sequence itself on the lane of position 1) — what l_n counts when they occur"""
    m, out = len(q), []
    for pos in range(1, m + 1):
        i, old = pos - 1, q[pos - 1]
        if hamming:
            if pos == 1:
                out.append(q)
        elif not (pos < m and q[i + 1] == old):
            out.append(q[:i] + q[i + 1:])
        out += [q[:i] + a + q[i + 1:] for a in "ACGT" if a != old]
        if not hamming and pos < m:
            out += [q[:pos] + c + q[pos:] for c in "ACGT" if not (pos >= 2 and c == old)]
    return out


def language(q, d, hamming):
    """the distinct candidates the search stage looks for: candidates(), plus the query itself in Hamming mode (neighbors.h:88 puts it
    into the set; in edit mode its deletions remove it again, and no kernel searches it)"""
    key = ("lang", q, d, hamming)
    if key not in _memo:
        s = set(candidates(q, d, hamming))
        if hamming:
            s.add(q)
        else:
            s.discard(q)
        _memo[key] = frozenset(s)
    return _memo[key]


def kept_set(q, d, hamming):
    """the reference's neighbourhood of q (distance 2: the hash-set form, the same set while it stays below the cap)"""
    key = ("kept", q, d, hamming)
    if key not in _memo:
        _memo[key] = frozenset((O.neighbors if d < 2 else O.neighbors_fast)(q, d, not hamming))
    return _memo[key]


def dels(s):
    return [s[:i] + s[i + 1:] for i in range(len(s))]


def subs(s):
    return [s[:i] + a + s[i + 1:] for i in range(len(s)) for a in "ACGT" if a != s[i]]


def substrings(text, k):
    """every k-mer of the text's sequences (bytes -> set of str)"""
    out = set()
    for seq in text.decode().split("\n"):
        out.update(seq[i:i + k] for i in range(len(seq) - k + 1))
    return out


def scan(text, pat):
    """occurrences of pat in text, overlapping ones included: bytes.find in a loop"""
    n, p = 0, text.find(pat)
    while p >= 0:
        n += 1
        p = text.find(pat, p + 1)
    return n


# ---- planting ------------------------------------------------------------------------------------------------------------------------------

def _query(rng, m):
    """a random m-mer without equal neighbouring characters: every deletion and substitution of it is a different string"""
    s = rng.choice("ACGT")
    while len(s) < m:
        s += rng.choice([x for x in "ACGT" if x != s[-1]])
    return s


def _spacer(rng):
    return "".join(rng.choices("ACGT", k=SPACER))


def _finish(s, cuts):
    """the planted line as a text of two sequences, cut in the middle of the spacer nearest to its middle"""
    c = min(cuts, key=lambda x: abs(x - len(s) // 2))
    seqs = [s[:c], s[c:]]
    return ("\n".join(seqs) + "\n").encode(), [len(x) + 1 for x in seqs]


def saturated(q, d, hamming, which, seed=0):
    """(text, seqlen): the strings `which` — candidates of q at distance d — each between two random spacers of 14 nt, in the order
    given.  Nothing is checked here: what occurs in the result is for the caller to count."""
    rng = random.Random("%s/%d/%d/%d" % (q, d, hamming, seed))
    s, cuts = _spacer(rng), []
    for w in which:
        s += w
        cuts.append(len(s) + SPACER // 2)
        s += _spacer(rng)
    return _finish(s, cuts or [len(s) // 2])


def _plant(seed, groups, copies=0):
    """One line with every group's strings.  groups: [{"s": the strand's string, "watch": strings whose occurrence is counted, "bad":
    strings that must not occur, "pool": what may be planted, "target": how many of `watch` are to occur}]; a group's pool is planted
    string by string until its census stands at the target, and no string goes in that moves another group's census past its own or
    makes a `bad` string occur.  copies: every fourth planted string of a group's first 4 * copies gets two more copies.
    Returns (text, seqlen, [set of occurring watch strings per group])."""
    rng = random.Random(seed)
    watch = {}
    for gi, g in enumerate(groups):
        for w in g["watch"]:
            watch.setdefault(w, []).append((gi, False))
        for w in g.get("bad", ()):
            watch.setdefault(w, []).append((gi, True))
    lens = sorted({len(w) for w in watch})
    occ = [set() for _ in groups]
    line, cuts = _spacer(rng), []

    def found_by(piece):
        t, out = line + piece, set()
        for k in lens:
            for i in range(max(0, len(line) - k + 1), len(t) - k + 1):
                if t[i:i + k] in watch:
                    out.add(t[i:i + k])
        return out

    def fits(found, only_known):
        add = [set() for _ in groups]
        for w in found:
            for gi, bad in watch[w]:
                if bad:
                    return None
                if w not in occ[gi]:
                    add[gi].add(w)
        for gi, a in enumerate(add):
            if a and (only_known or len(occ[gi]) + len(a) > groups[gi]["target"]):
                return None
        return add

    def put(w, only_known=False):
        nonlocal line
        for _ in range(4):
            piece = w + _spacer(rng)
            add = fits(found_by(piece), only_known)
            if add is not None:
                cuts.append(len(line) + len(w) + SPACER // 2)
                line += piece
                for gi, a in enumerate(add):
                    occ[gi] |= a
                return True
        return False

    for gi, g in enumerate(groups):
        pool, planted = list(g["pool"]), []
        rng.shuffle(pool)
        for w in pool:
            if len(occ[gi]) >= g["target"]:
                break
            if w not in occ[gi] and put(w):
                planted.append(w)
        if len(occ[gi]) != g["target"]:
            raise _Retry
        for w in planted[:4 * copies:4]:
            for _ in range(2):
                if not put(w, only_known=True):
                    raise _Retry
    text, seqlen = _finish(line, cuts or [len(line) // 2])
    return text, seqlen, occ


def _group(s, d, hamming, target, pool=None, exact=True):
    """the planting order for one strand.  exact (distance 1 in edit mode; Hamming mode at either distance): the census runs over
    every candidate, and in edit mode the insertions and the string itself must stay away, so that the occurring (position,
    operation) candidates are as many as the distinct occurring strings.  not exact (edit distance 2): the census runs over the
    reference's kept strings."""
    if not exact:
        watch, bad = kept_set(s, d, hamming), ()
    elif hamming:
        watch, bad = language(s, d, hamming), ()
    else:
        lang = language(s, d, hamming)
        watch, bad = {w for w in lang if len(w) <= len(s)}, {w for w in lang if len(w) > len(s)} | {s}
    if pool is None:
        pool = sorted(language(s, d, hamming)) if hamming else dels(s) + subs(s)
    return {"s": s, "watch": watch, "bad": bad, "pool": pool, "target": target}


def _padding(rng, m, n, text, d, hamming, avoid=()):
    """n random m-mers none of whose candidates occurs on either strand: none of the reference's kept strings does (every candidate
    is one of them or contains one)"""
    subs_of = {}
    out = []
    while len(out) < n:
        q = "".join(rng.choices("ACGT", k=m))
        ok = q not in avoid and q not in out
        for s in (q, revcomp(q)):
            for w in kept_set(s, d, hamming) if ok else ():
                if len(w) not in subs_of:
                    subs_of[len(w)] = substrings(text, len(w))
                if w in subs_of[len(w)]:
                    ok = False
                    break
        if ok:
            out.append(q)
    return out


def _spread(total, n, swing=4):
    """`total` over n groups, no two neighbours equal"""
    base, rem = divmod(total, n)
    t = [base + (i < rem) for i in range(n)]
    for i in range(0, n - 1, 2):
        k = 1 + (i // 2) % swing
        t[i] += k
        t[i + 1] -= k
    assert sum(t) == total
    return t


def _batch(nq, at, pads, groups_of, **more):
    """nq queries: `at` = {index: saturated query}, padding elsewhere; groups_of = {query: (forward census, reverse census)}"""
    pads = iter(pads)
    qs = [at[i] if i in at else next(pads) for i in range(nq)]
    L = {}
    for i, q in at.items():
        for strand, c in enumerate(groups_of[q]):
            if c:
                L[2 * i + strand] = c
    b = {"qs": qs, "sat": sorted(at), "L": L, "leaves": sum(L.values())}
    b.update(more)
    return b


def _retrying(fn, seed):
    while True:
        try:
            return fn(seed)
        except _Retry:
            seed += 1


# ---- distance 1: the occupancy texts (rows a - e) ------------------------------------------------------------------------------------------

def _occupancy(hamming):
    """one text per mode with the sets x (1 string), b (64), c (256), d (512) and e (64 KEPT strings), each set's queries at the
    start of the second workgroup of a batch of 24 20-mers (gpw 12: six queries per workgroup, four workgroups, so that a census of 513
    is above 48 per workgroup: hunt.hip:859); the batches of 65, 257, 513 and 65 kept add x's query behind their set's own"""
    def build(seed):
        rng = random.Random(seed)
        cap = 52 if hamming else 68
        sets, census, groups = {}, {}, []

        def add(name, total, kept_only=False):
            ng = 2 * -(-total // (2 * cap))
            t = _spread(total, ng) if ng > 2 else [total * 5 // 8, total - total * 5 // 8]
            sets[name] = []
            for j in range(0, ng, 2):
                q = _query(rng, 20)
                sets[name].append(q)
                census[q] = (t[j], t[j + 1])
                for s, c in ((q, t[j]), (revcomp(q), t[j + 1])):
                    grp = _group(s, 1, hamming, c)
                    if kept_only:   # (a spacer in front of the deletion of the first character spells a substitution of it: not kept)
                        grp["pool"] = sorted(w for w in kept_set(s, 1, hamming) if len(w) <= 20)
                        grp["bad"] = set(grp["bad"]) | (set(grp["watch"]) - kept_set(s, 1, hamming))
                    groups.append((name, grp))
        q = _query(rng, 20)
        sets["x"], census[q] = [q], (1, 0)
        groups.append(("x", _group(q, 1, hamming, 1, subs(q)[3:-3] if hamming else dels(q)[1:-1])))
        groups.append(("x", _group(revcomp(q), 1, hamming, 0)))
        add("b", 64)
        add("c", 256)
        add("d", 512)
        add("e", 64, kept_only=True)
        text, seqlen, occ = _plant(seed, [g for _, g in groups], copies=3)
        pads = _padding(rng, 20, 24, text, 1, hamming, avoid=census)
        x = sets["x"][0]
        batches = {"a0": _batch(24, {}, pads, census), "a1": _batch(24, {6: x}, pads, census)}
        for name, n in (("b", 64), ("c", 256), ("d", 512), ("e", 64)):
            at = {6 + j: q for j, q in enumerate(sets[name])}
            batches["%s%d" % (name, n)] = _batch(24, at, pads, census)
            at[6 + len(sets[name])] = x
            batches["%s%d" % (name, n + 1)] = _batch(24, at, pads, census)
        for name in ("e64", "e65"):       # every planted string of set e (and of x) is one the reference keeps
            batches[name]["kept"] = dict(batches[name]["L"])
        return {"text": text, "seqlen": seqlen, "d": 1, "hamming": hamming, "batches": batches}
    return _retrying(build, 4100 + hamming)


# ---- distance 1: where a group sits in its workgroup (row f) ----------------------------------------------------------------------------------

LAY_LENGTHS = (16, 17, 31, K + 1)
LAY_CENSUS = ((9, 5), (7, 11), (6, 8))


def _layouts(hamming):
    """per length one batch of three workgroups (TAKE form) whose second workgroup holds three saturated queries: in its first two
    slots (side by side, different censuses) and in its last; length 17 has gpw 14 in the TAKE form and 15 without, where the first of
    the three has its forward strand in the last slot of workgroup 0 and its reverse strand in the first slot of workgroup 1"""
    def build(seed):
        rng = random.Random(seed)
        census, groups, at_of = {}, [], {}
        for m in LAY_LENGTHS:
            per = gpw_of(m, True) // 2
            at_of[m] = {}
            for idx, c in zip((per, per + 1, 2 * per - 1), LAY_CENSUS):
                q = _query(rng, m)
                at_of[m][idx], census[q] = q, c
                groups += [_group(q, 1, hamming, c[0]), _group(revcomp(q), 1, hamming, c[1])]
        text, seqlen, occ = _plant(seed, groups, copies=1)
        batches = {}
        for m in LAY_LENGTHS:
            per = gpw_of(m, True) // 2
            batches["f%d" % m] = _batch(3 * per, at_of[m], _padding(rng, m, 3 * per, text, 1, hamming, avoid=census), census)
        return {"text": text, "seqlen": seqlen, "d": 1, "hamming": hamming, "batches": batches}
    return _retrying(build, 4200 + hamming)


# ---- distance 1: everything planted (row g), long queries (row h) ----------------------------------------------------------------------------------

LOW_QUERIES = ("ACGTAGAAAAAACTGATCGT",      # a homopolymer run inside
               "ACACACACACACACACACAC",      # a dinucleotide repeat
               "GATCCGTAGCTAAGCTTACG")      # plain, first and last character equal


def _low():
    """every candidate of three low-complexity queries and the queries themselves (both modes read this text): most strings contain
    one another, equal strings come from several operations.  A query per workgroup, so that no LDS list overflows."""
    key = "low"
    if key not in _memo:
        rng = random.Random(4300)
        line_of = []
        for q in LOW_QUERIES:
            which = sorted(language(q, 1, False) | {q}) + sorted(language(revcomp(q), 1, True))[:9]
            rng.shuffle(which)
            line_of += which
        text, seqlen = saturated("low", 1, False, line_of, seed=4300)
        batches = {}
        for hamming in (False, True):
            pads = _padding(rng, 20, 18, text, 1, hamming, avoid=LOW_QUERIES)
            batches[hamming] = _batch(18, {0: LOW_QUERIES[0], 7: LOW_QUERIES[1], 17: LOW_QUERIES[2]}, pads, {q: (0, 0) for q in LOW_QUERIES})
        _memo[key] = {"text": text, "seqlen": seqlen, "d": 1, "batches": batches}
    return _memo[key]


def _long():
    """a 41-mer and a 42-mer with 100 of their deletions and substitutions each (both modes read this text)"""
    def build(seed):
        rng = random.Random(seed)
        q41, q42 = _query(rng, 41), _query(rng, 42)
        groups = [dict(_group(q, 1, False, 100), bad=()) for q in (q41, q42)]
        text, seqlen, occ = _plant(seed, groups)
        batches = {}
        for hamming in (False, True):
            pads = _padding(rng, 20, 10, text, 1, hamming)
            for q in (q41, q42):
                batches[len(q), hamming] = _batch(11, {5: q}, pads, {q: (0, 0)})
        return {"text": text, "seqlen": seqlen, "d": 1, "batches": batches}
    if "long" not in _memo:
        _memo["long"] = _retrying(build, 4400)
    return _memo["long"]


# ---- distance 2 (rows i - k) -----------------------------------------------------------------------------------------------------------------

REV2 = 5    # strings of the reverse strand's ball planted beside every saturated forward group


def _ham2(counts, seed0):
    """Hamming distance 2: per count one 20-mer with exactly that many strings of its ball planted, REV2 of its reverse strand's"""
    def build(seed):
        rng = random.Random(seed)
        census, groups, qs = {}, [], []
        for c in counts:
            q = _query(rng, 20)
            qs.append(q)
            census[q] = (c, REV2)
            groups += [_group(q, 2, True, c), _group(revcomp(q), 2, True, REV2)]
        text, seqlen, occ = _plant(seed, groups)
        pads = _padding(rng, 20, 7, text, 2, True, avoid=census)
        batches = {c: _batch(8, {3: q}, pads, census) for c, q in zip(counts, qs)}
        return {"text": text, "seqlen": seqlen, "d": 2, "hamming": True, "batches": batches}
    return _retrying(build, seed0)


def _double_subs(s):
    """two substitutions at positions 2 .. m - 3 that are no neighbours: one pair of operations spells each"""
    out = []
    for i in range(2, len(s) - 2):
        for j in range(i + 2, len(s) - 2):
            for a in "ACGT":
                for b in "ACGT":
                    if a != s[i] and b != s[j]:
                        out.append(s[:i] + a + s[i + 1:j] + b + s[j + 1:])
    return out


def _edit2():
    """edit distance 2, 16-mers (the hash-set form of the reference's neighbourhood stays below its cap): one query with 513 of its
    KEPT strings planted — at least 513 occurring candidates, whatever repeated operations a kernel skips — and one with 400 double
    substitutions, each spelt by one pair of operations; and a 15-mer (shorter than K2 + 2) nothing of which occurs"""
    def build(seed):
        rng = random.Random(seed)
        q513, q400 = _query(rng, 16), _query(rng, 16)
        census = {q513: (513, REV2), q400: (400, REV2)}
        kept400 = kept_set(q400, 2, False)
        groups = [_group(q513, 2, False, 513, sorted(kept_set(q513, 2, False)), exact=False),
                  _group(revcomp(q513), 2, False, REV2, sorted(kept_set(revcomp(q513), 2, False)), exact=False),
                  _group(q400, 2, False, 400, [w for w in _double_subs(q400) if w in kept400], exact=False),
                  _group(revcomp(q400), 2, False, REV2, [w for w in _double_subs(revcomp(q400)) if w in kept_set(revcomp(q400), 2, False)], exact=False)]
        text, seqlen, occ = _plant(seed, groups)
        pads = _padding(rng, 16, 7, text, 2, False, avoid=census)
        short = _padding(rng, K2 + 1, 1, text, 2, False)[0]
        batches = {}
        for c, q in ((513, q513), (400, q400)):
            batches[c, "long2"] = _batch(8, {3: q}, pads, census)
            batches[c, "r04"] = _batch(8, {3: q, 6: short}, pads, dict(census, **{short: (0, 0)}))
        return {"text": text, "seqlen": seqlen, "d": 2, "hamming": False, "batches": batches, "short": short}
    return _retrying(build, 4700)


GENOMES = {"occ_edit": lambda: _occupancy(False), "occ_ham": lambda: _occupancy(True), "lay_edit": lambda: _layouts(False),
           "lay_ham": lambda: _layouts(True), "low": _low, "long": _long, "ham2_i": lambda: _ham2((512, 513), 4500),
           "ham2_j1024": lambda: _ham2((1024,), 4600), "ham2_j1025": lambda: _ham2((1025,), 4650), "edit2": _edit2}


def genome(name):
    """{"text", "seqlen", "names", "d", "batches": {label: {"qs", "sat": indices of the saturated queries, "L": {group: occurring
    candidates}, "leaves": their sum, "kept": {group: kept strings} where the row states it}}}, built once per process"""
    key = ("genome", name)
    if key not in _memo:
        g = dict(GENOMES[name]())
        g["name"] = name
        g["names"] = ["%s_%d" % (name, i + 1) for i in range(len(g["seqlen"]))]
        _memo[key] = g
    return _memo[key]


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------------------

class Reference:
    """the oracle on one text behind the interface tests/test_gpu_locate_topk.py's _compare asks for, every query answered once per
    parameter set; sums(): what count mode reports, per query and strand"""

    def __init__(self, name):
        self.g = genome(name)
        self.dir = tempfile.mkdtemp(prefix="select_shapes_")
        self.path = os.path.join(self.dir, name + ".fm9")
        O.build_fm9(self.g["text"], self.path)
        self.orc = O.Index(self.path)
        self.memo = {}

    def hunt(self, seqlen, names, qs, want_hits=True, **kw):
        memo = self.memo.setdefault(tuple(sorted(kw.items())), {})
        todo = [q for q in dict.fromkeys(qs) if q not in memo]
        if todo:
            O.fast_neighbors(kw.get("distance", 1) >= 2)
            try:
                _, hits = self.orc.hunt(seqlen, names, todo, want_hits=True, **kw)
            finally:
                O.fast_neighbors(False)
            for q in todo:
                memo[q] = []
            for h in hits:
                memo[todo[h[0]]].append(h[1:])
        return None, [(qi,) + h for qi, q in enumerate(qs) for h in memo[q]]

    def sums(self, qs, d, hamming):
        memo = self.memo.setdefault(("sums", d, hamming), {})
        for q in qs:
            if q not in memo:
                memo[q] = tuple(sum(self.orc.count(w.encode()) for w in kept_set(s, d, hamming)) for s in (q, revcomp(q)))
        return [memo[q] for q in qs]


def reference(name):
    key = ("ref", name)
    if key not in _memo:
        _memo[key] = Reference(name)
    return _memo[key]


def bracket(g, batch):
    """edit distance 2, where the occurring (position pair, operation pair) candidates depend on which repeated operations a kernel
    skips: (distinct occurring candidates, occurring candidates with every duplicate of the reference's walk) summed over the batch's
    saturated queries — the search stage's leaf counter lies between the two"""
    key = ("bracket", g["name"], tuple(batch["qs"]))
    if key not in _memo:
        lo = hi = 0
        have = {}
        for i in batch["sat"]:
            for s in (batch["qs"][i], revcomp(batch["qs"][i])):
                for w in candidates(s, g["d"], False):
                    if len(w) not in have:
                        have[len(w)] = substrings(g["text"], len(w))
                lo += sum(1 for w in language(s, g["d"], False) if w in have[len(w)])
                hi += sum(1 for w in candidates(s, g["d"], False) if w != s and w in have[len(w)])
        _memo[key] = (lo, hi)
    return _memo[key]


def limits(ref, batch, d, hamming):
    """max_locations above every query's total, and inside the forward and inside the reverse strand's strings of the batch's first
    saturated query"""
    sums = ref.sums(batch["qs"], d, hamming)
    fw, rv = sums[batch["sat"][0]] if batch["sat"] else (0, 0)
    out = [max(a + b for a, b in sums) + 7]
    if fw > 1:
        out.append(fw // 2)
    if rv > 1:
        out.append(fw + rv // 2)
    return out
