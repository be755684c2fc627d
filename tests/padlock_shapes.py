"""Inputs and a plain model for dg_padlock_scan (dicey_amd/csrc/padlock.hip), whose six per-position arrays and three counters the
binary's replay only samples: it skips 2*armlen - 1 positions after every accepted probe and stops at the first refusal.

Everything comes from seeds; nothing here touches a GPU or the library under test.  genome() is a text of three sequences with
an exact duplicate, a near-duplicate, a reverse-complemented copy, an N run and two IUPAC letters; exons(armlen) the exon list
cut from it; MATRIX the parameter sets; model() the nine result fields written from the reference's loop (src/padlock.h:321-428)
and the comment above dg_padlock_scan in include/dicey_gpu.h, one position after the other, with thal(), count() and
neighbors() handed in.  tests/test_padlock_shapes_host.py asserts, from the model over the reference's thal() and the oracle's
count() alone, that the inputs reach what they were built for; tests/test_gpu_padlock_shapes.py compares the library with it."""
import random
import struct

NAMES = ["chrA", "chrB", "chrC"]
LENGTHS = [30000, 30000, 20000]
DUP = (2000, 5000, 600)          # chrA[2000:2600] copied to chrB[5000:5600]
NEAR = (7000, 12000, 600)        # chrA[7000:7600] to chrB[12000:12600], a substitution every 37 nt
RC = (11000, 3000, 600)          # the reverse complement of chrA[11000:11600] at chrC[3000:3600]
N_RUN = (15000, 10)              # chrA[15000:15010]
IUPAC_EXON = (20000, 20400)      # in chrB, with an 'R' and a 'Y' inside
R_AT, Y_AT = 20117, 20262
NOT_COMPUTED = -1e300            # DG_PADLOCK_NOT_COMPUTED
THAL_ERROR = -999999.0           # THAL_ERROR_SCORE: thal() refused the pair
NB_CAP = 10000                   # neighbors()' size cap in padlock.h:396

# (armlen, distance, hamming, tmdiff, gc_min, gc_max).  Probes of up to 48 nt (armlen <= 24) are paired on the device, the 50 nt
# probe of armlen 25 goes through dg_thal_batch; edit distance 2 only up to 20 nt (the oracle's enumeration above that takes
# seconds per arm).  k/armlen computed in double equals the literal of the same decimal (both are the nearest double), so
# 0.45 = 9/20 = 18/40 and 0.55 = 11/20 = 22/40 are attained exactly by arms and probes of the boundary entry.
MATRIX = [
    (20, 1, False, 2, 0.4, 0.6),       # the command line's defaults
    (20, 1, True, 2, 0.4, 0.6),
    (20, 2, True, 2, 0.4, 0.6),        # (exon list capped)
    (20, 0, False, 4, 0.45, 0.55),     # boundary: gc_min and gc_max are attainable values of k/20
    (15, 1, True, 10, 0.3, 0.7),       # the wide filter
    (15, 1, False, 2, 0.4, 0.6),
    (10, 2, False, 10, 0.3, 0.7),      # edit distance 2 (capped to EDIT2_EXONS)
    (10, 1, False, 10, 0.3, 0.7),
    (10, 2, True, 2, 0.4, 0.6),
    (24, 1, False, 2, 0.4, 0.6),       # (capped)
    (24, 2, True, 2, 0.4, 0.6),        # (capped)
    (25, 1, False, 2, 0.4, 0.6),       # (capped)
    (25, 1, True, 2, 0.4, 0.6),
    (25, 0, False, 2, 0.4, 0.6),
]
BOUNDARY = MATRIX[3]
# The oracle's enumeration decides what an entry can afford.  neighbors() at edit distance 2 takes 0.05 s for a 10-mer (2 s for a
# 20-mer); at edit distance 1 it takes 2 ms from 24 nt on; the 1 700 to 2 500 strings of a Hamming-2 neighbourhood of 20 to 24 nt
# cost 10 ms per arm to count one by one.  Those entries scan a part of the list that still holds every length around 2*armlen.
EDIT2_EXONS = ("two_arms", "near_piece", "short", "empty", "two_arms_plus_1")
CAPPED_EXONS = ("two_arms", "near", "short", "empty", "identical_1", "two_arms_plus_1")
_memo = {}
_COMP = dict(zip("ACGTURYSWKMBVDHN", "TGCAAYRSWMKVBHDN"))   # util.h complement(), upper case; anything else -> 'N'


def entry_id(p):
    return "arm%d_%s%d_z%d_gc%g-%g" % (p[0], "h" if p[2] else "e", p[1], p[3], p[4], p[5])


def revcomp(s):
    return "".join(_COMP.get(c, "N") for c in reversed(s))


def _rand(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def genome():
    """{"seqs", "names", "text"}: built once per process, upper case throughout"""
    if "g" in _memo:
        return _memo["g"]
    rng = random.Random(20262)
    a, b, c = (_rand(rng, n) for n in LENGTHS)
    src, dst, n = DUP
    b = b[:dst] + a[src:src + n] + b[dst + n:]
    src, dst, n = NEAR
    nd = list(a[src:src + n])
    for k in range(10, n, 37):
        nd[k] = rng.choice([x for x in "ACGT" if x != nd[k]])
    b = b[:dst] + "".join(nd) + b[dst + n:]
    src, dst, n = RC
    c = c[:dst] + revcomp(a[src:src + n]) + c[dst + n:]
    a = a[:N_RUN[0]] + "N" * N_RUN[1] + a[N_RUN[0] + N_RUN[1]:]
    b = b[:R_AT] + "R" + b[R_AT + 1:Y_AT] + "Y" + b[Y_AT + 1:]
    seqs = [a, b, c]
    assert [len(s) for s in seqs] == LENGTHS
    _memo["g"] = dict(seqs=seqs, names=NAMES, text=("\n".join(seqs) + "\n").encode())
    return _memo["g"]


def named_exons(armlen):
    """[(name, sequence)] in list order.  The three lengths around 2*armlen sit first (2L: one probe, L+1 arm slots), adjacent in
    the middle (2L-1 and the empty exon: no slot) and last (2L+1)."""
    a, b, c = genome()["seqs"]
    L, T = armlen, 2 * armlen
    n0 = N_RUN[0]
    identical = c[1000:1300]
    return [
        ("two_arms", a[500:500 + T]),
        ("dup", a[1950:2450]),                       # over the exact duplicate: arm_count 2 from chrA[2000:]
        ("near", a[6990:7440]),                      # over the near-duplicate: neighbourhood hits beyond the exact ones
        ("rc_copy", a[11050:11450]),                 # its reverse complement stands in chrC: a reverse-strand count
        ("minus_strand", revcomp(b[8000:8350])),     # given as the reverse complement of its genome stretch
        ("near_piece", a[7100:7190]),                # (all that an edit-distance-2 entry scans of it)
        ("short", c[7000:7000 + T - 1]),
        ("empty", ""),
        ("n_inside", a[n0 - 110:n0 + 120]),          # the N run strictly inside
        ("n_last", a[n0 - 3 * L:n0 + 1]),            # one N, the last character of the last arm window
        ("iupac", b[IUPAC_EXON[0]:IUPAC_EXON[1]]),
        ("identical_1", identical),
        ("overlap_1", a[2100:2500]),                 # overlaps "dup" and the next one
        ("overlap_2", a[2400:2800]),
        ("identical_2", identical),                  # same arms as identical_1, slots of its own
        ("foreign", _rand(random.Random(977), 300)),  # not from the genome: counts 0
        ("two_arms_plus_1", c[5000:5000 + T + 1]),
    ]


def exons(params):
    """the exon list of a matrix entry"""
    ex = named_exons(params[0])
    L, distance, hamming = params[:3]
    if distance >= 2 and not hamming:
        ex = [(n, s) for n, s in ex if n in EDIT2_EXONS]
    elif (distance == 2 and L >= 20) or (distance == 1 and not hamming and L >= 24):
        ex = [(n, s) for n, s in ex if n in CAPPED_EXONS]
    return [s for _, s in ex]


def unhex(h):
    return struct.unpack(">d", bytes.fromhex(h))[0]


def gc(w):
    """util.h gccontent(): -1 with an N in the window; any other letter that is not C or G counts as not G/C"""
    if not w or "N" in w:
        return -1.0
    return (w.count("C") + w.count("G")) / len(w)


def model(exons, params, thal, count, neighbors):
    """The nine fields of a dg_padlock_result as plain Python lists and ints.
      thal(windows)       -> [temperature of thal(w, revcomp(w)) for w in windows]
      count(s)            -> occurrences of the string s in the text
      neighbors(s, d, indel) -> the strings of neighbors(s, "ACGT", d, indel, 10000)"""
    L, distance, hamming, tmdiff, gc_min, gc_max = params
    T = 2 * L
    passes = lambda g: not (g < gc_min or g > gc_max)
    pos_off, npos = [], 0
    for ex in exons:
        pos_off.append(npos)
        if len(ex) >= T:
            npos += len(ex) - L + 1
    pos_off.append(npos)
    arm_gc, probe_gc = [0.0] * npos, [0.0] * npos
    arm_tm, probe_tm = [NOT_COMPUTED] * npos, [NOT_COMPUTED] * npos
    arm_count, arm_nbcount = [-1] * npos, [-1] * npos
    arm_seq = {}                                  # slot -> arm window
    for e, ex in enumerate(exons):
        if len(ex) < T:
            continue
        for q in range(len(ex) - L + 1):
            at = pos_off[e] + q
            arm_seq[at] = ex[q:q + L]
            arm_gc[at] = gc(ex[q:q + L])
    arm_thal = [at for at in sorted(arm_seq) if passes(arm_gc[at])]
    for at, t in zip(arm_thal, thal([arm_seq[at] for at in arm_thal])):
        arm_tm[at] = t
    arm_ok = lambda at: passes(arm_gc[at]) and not (arm_tm[at] > 93 + arm_gc[at] - 675.0 / L)
    probe_thal, probe_seq = [], {}
    for e, ex in enumerate(exons):
        if len(ex) < T:
            continue
        for q in range(len(ex) - T + 1):
            at = pos_off[e] + q
            probe_gc[at] = gc(ex[q:q + T])
            if arm_ok(at) and arm_ok(at + L) and not abs(arm_tm[at] - arm_tm[at + L]) > tmdiff and passes(probe_gc[at]):
                probe_thal.append(at)
                probe_seq[at] = ex[q:q + T]
    for at, t in zip(probe_thal, thal([probe_seq[at] for at in probe_thal])):
        probe_tm[at] = t
    counted = set()
    for at in probe_thal:
        if in_window(probe_tm[at], probe_gc[at], L):
            counted |= {at, at + L}
    for at in sorted(counted):
        arm = arm_seq[at]
        arm_count[at] = count(arm) + count(revcomp(arm))
        if distance > 0:
            arm_nbcount[at] = sum(count(s) for s in neighbors(arm, distance, not hamming)) + \
                sum(count(s) for s in neighbors(revcomp(arm), distance, not hamming))
    return dict(pos_off=pos_off, arm_gc=arm_gc, arm_tm=arm_tm, probe_gc=probe_gc, probe_tm=probe_tm, arm_count=arm_count,
                arm_nbcount=arm_nbcount, n_arm_thal=len(arm_thal), n_probe_thal=len(probe_thal), n_arms_counted=len(counted))


def in_window(tm, probe_gc, armlen):
    """padlock.h:376-378: the probe's Tm window; a refused thal() is the reference's error path, never a probe"""
    lo = 81.5 + probe_gc - 675.0 / (2 * armlen)
    return tm != THAL_ERROR and tm != NOT_COMPUTED and lo <= tm <= lo + 10


class Memo:
    """model() over one thal() provider that takes explicit pairs, with the temperatures kept per window: the matrix entries
    share arm lengths, hence windows.  count and neighbors go to the model as they are."""

    def __init__(self, thal_pairs, count, neighbors):
        self._thal, self._count, self._nb = thal_pairs, count, neighbors
        self.tm = {}

    def thal(self, windows):
        new = sorted(set(windows) - set(self.tm))
        if new:
            self.tm.update(zip(new, self._thal([(w, revcomp(w)) for w in new])))
        return [self.tm[w] for w in windows]

    def model(self, exons, params):
        return model(exons, params, self.thal, self._count, self._nb)


def oracle_memo(orc, thal_pairs):
    """Memo over the oracle's count() and neighbors() on the open oracle_lib.Index orc"""
    import oracle_lib as O
    return Memo(thal_pairs, lambda s: orc.count(s.encode()), lambda s, d, indel: O.neighbors(s, d, indel, NB_CAP))


def ref_thal_pairs(pairs):
    """the reference's own thal() (oracle/_ref) at the default environment"""
    import thal_corpus as TC
    import thal_expect as TE
    return [unhex(v[0]) for v in TE.ref_values(pairs, TC.ENVS["default"])]
