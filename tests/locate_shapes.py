"""Inputs for the locate stage of `dicey hunt` (dicey_amd/csrc/hunt_locate.hpp) at the occurrence counts, `take` values and position
layouts where the stage changes the code that answers: the in-lane routes of k_locate (<= 4, <= 16 occurrences), the wavefront job
(17 .. 256), the workgroup jobs (small buffer up to 4 608, walk from 9 217 on), the prefix levels (FmView::plv), k_locate_big
(take above 1 024) and both sorts of the job kernels (by buckets, or by the network when the positions cluster).

Everything comes from seeds; nothing here touches a GPU or the library under test.  genome() is ONE text of four sequences (6 Mb, so
that the index has the four prefix levels X = 2^16 .. 2^22) with every family planted at positions this module chose and remembers;
the module also restates, in plain Python, the arithmetic the kernels use to choose a route (route(), bucket_lanes()), so that
tests/test_locate_shapes_host.py can prove from a scan of the text that each family lands on the side of a threshold it was built for,
and tests/test_gpu_locate_shapes.py can hold the job lists a development build dumps against it."""
import bisect
import os
import random
import tempfile

import oracle_lib as O
from conftest import revcomp

NAMES = ["locA", "locB", "locC", "locD"]
LENGTHS = [1_500_000, 1_500_000, 1_500_000, 1_500_000]
LEVELS = (1 << 16, 1 << 18, 1 << 20, 1 << 22)   # FmView::plv[l].x: 2^(16 + 2 l) below n
# the stage's constants (hunt_locate.hpp)
LOC_SMALL_MAX, TOPK_KMAX, TOPK_KCAP, TOPK_KCAP_MID, BUCKET_SKEW, BIG_CAP = 256, 1024, 1152, 576, 32, 16384
MID_MAX = 8 * TOPK_KCAP_MID      # 4 608: LocJobs::mid_max after a batch with >= 2 048 workgroup jobs, else 0
WALK_MAX = 8 * TOPK_KCAP         # 9 216
MARKS = (4, 5, 16, 17, 256, 257, 576, 577, 927, 928, 929, 1024, 1025)
BIG_TAKES = (1025, 2560, 4608, 4609, 8192, 8193, 16384)
N_COUNTS = (1, 2, 3, 4, 5, 15, 16, 17)
SMALL_COUNTS = (18, 31, 32, 33, 63, 64, 65, 128, 129, 255, 256, 257)
SKEW_C = (31, 32, 33, 34, 64)
STAR_FWD = (1, 4, 5, 16, 17, 256, 257, 600)
STAR_REV = (3, 40)
# (suffixes in the table window's interval, how many of them are preceded by the query's own first characters)
TAILS = ((2, 1), (3, 2), (4, 4), (4, 1), (6, 4), (8, 5), (9, 2), (16, 15), (16, 16), (16, 1), (5, 5))
TAIL_K = 16                      # the table order the tails batches are opened with (DICEY_KMER_K)
CROWD, CROWD_COPIES = 30, 17     # substitutions of a second centre, each a wavefront job
_memo = {}


class _Retry(Exception):
    pass


def _rand(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def _unit(rng, n):
    """a random unit no two neighbouring characters of which are equal: it has no period, so a tandem array of c units holds it exactly
    c times, and none of its one-character deletions or insertions is found inside a copy of one of its substitutions"""
    while True:
        u = _rand(rng, n)
        if all(u[i] != u[i + 1] for i in range(n - 1)) and all(u[:p] != u[-p:] for p in range(n // 2, n)):
            return u


def scan(text, pat):
    """every position of `pat` in `text`, overlapping ones included: bytes.find in a loop"""
    out, p = [], text.find(pat)
    while p >= 0:
        out.append(p)
        p = text.find(pat, p + 1)
    return out


def _build(seed):
    rng = random.Random(seed)
    total = sum(LENGTHS) + len(LENGTHS)
    text = bytearray(rng.randbytes(total).translate(bytes(b"ACGT"[i & 3] for i in range(256))))
    cum = [0]
    for n in LENGTHS:
        cum.append(cum[-1] + n + 1)
        text[cum[-1] - 1] = 10
    used = bytearray(total)
    for c in cum[1:]:
        used[c - 1] = 1
    fam = {}

    def free(p, n, gap=1):
        return p >= 0 and p + n <= total and used.find(1, max(0, p - gap), p + n + gap) < 0

    def put(name, p):
        u = fam[name]["unit"].encode()
        text[p:p + len(u)] = u
        used[p:p + len(u)] = b"\x01" * len(u)
        fam[name]["pos"].append(p)

    def new(name, n, unit=None):
        fam[name] = {"unit": unit or _unit(rng, n), "pos": []}
        return fam[name]

    def edge(name, p):          # a copy that touches a separator or the text's first character: no gap asked
        if not free(p, len(fam[name]["unit"]), gap=0):
            raise _Retry
        put(name, p)

    def tandem(name, p, c):
        n = len(fam[name]["unit"])
        if not free(p, n * c):
            raise _Retry
        for i in range(c):
            put(name, p + i * n)

    def spread(name, count, a, b):
        """one copy in each of `count` equal slots of [a, b)"""
        n = len(fam[name]["unit"])
        w = (b - a) / count
        if w < n + 3:
            raise _Retry
        for i in range(count):
            s0, s1 = int(a + i * w), int(a + (i + 1) * w) - n - 1
            for _ in range(400):
                p = rng.randrange(s0, max(s0 + 1, s1))
                if free(p, n):
                    put(name, p)
                    break
            else:                                     # the slot is taken (a tandem array lies there): anywhere in [a, b)
                for _ in range(4000):
                    p = rng.randrange(a, b - n - 1)
                    if free(p, n):
                        put(name, p)
                        break
                else:
                    raise _Retry

    end = total - 1                                   # the final separator
    # ---- n1 .. n17: one copy each at a place where a hit's neighbour is the text's start or a separator, the others anywhere
    edges = [lambda n: 0, lambda n: end - n, lambda n: cum[1], lambda n: cum[2] - 1 - n, lambda n: cum[2], lambda n: cum[3] - 1 - n,
             lambda n: cum[3], lambda n: cum[1] - 1 - n]
    for c, at in zip(N_COUNTS, edges):
        f = new("n%d" % c, rng.randrange(16, 21))
        edge("n%d" % c, at(len(f["unit"])))
    # ---- tandem arrays first (they need a stretch of their own)
    for c in SKEW_C:                                  # the array, then nothing for 200 kb, then the others over 1.5 Mb
        name = "skew_%d" % c
        new(name, 20)
        a = rng.randrange(100_000, 3_000_000)
        tandem(name, a, c)
        fam[name]["array"] = (a, c)
    new("skew_flat", 16, unit="A" * 16)               # 200 overlapping copies inside one run of 215 A: the span is 199 positions
    a = rng.randrange(100_000, 5_000_000)
    if not free(a, 217):
        raise _Retry
    text[a] = ord("C")
    text[a + 1:a + 216] = b"A" * 215
    text[a + 216] = ord("G")
    used[a:a + 217] = b"\x01" * 217
    fam["skew_flat"]["pos"] = list(range(a + 1, a + 201))
    new("run_600", 16, unit="C" * 16)                 # 600 consecutive positions, the first at 100 (mod 256): see threshold_exit()
    a = (rng.randrange(300_000, 5_000_000) & ~255) + 99
    if not free(a, 617):
        raise _Retry
    text[a] = ord("A")
    text[a + 1:a + 616] = b"C" * 615
    text[a + 616] = ord("T")
    used[a:a + 617] = b"\x01" * 617
    fam["run_600"]["pos"] = list(range(a + 1, a + 601))
    new("topk_skew", 20)
    a = rng.randrange(70_000, 200_000)
    tandem("topk_skew", a, 500)
    fam["topk_skew"]["array"] = (a, 500)
    # ---- the prefix-level families (16-nt units: they are the bulk of what is planted)
    X1, X2, X3 = LEVELS[1], LEVELS[2], LEVELS[3]
    new("plv_run", 16)                                # even density: the level asked first holds take .. 9 216 records
    spread("plv_run", 12000, 2000, end)
    new("plv_next", 16)                               # 10 copies below 2^20, 5 000 up to 2^22: the asked run is short, the next one serves
    spread("plv_next", 10, 70_000, X2 - 100)
    spread("plv_next", 5000, X2 + 100, X3 - 100)
    spread("plv_next", 6990, X3 + 100, end)
    new("plv_dense", 16)                              # 9 500 copies below the asked 2^20: the run is refused, the walk serves
    spread("plv_dense", 9500, 70_000, X2 - 100)
    spread("plv_dense", 2500, X2 + 100, end)
    new("plv_exact", 16)                              # exactly 400 copies below 2^18
    spread("plv_exact", 400, 2000, X1 - 100)
    spread("plv_exact", 1600, X1 + 100, X2 - 100)
    spread("plv_exact", 18000, X2 + 100, end)
    # ---- the others of the tandem families
    for c in SKEW_C:
        name = "skew_%d" % c
        a = fam[name]["array"][0]
        spread(name, 200 - c, a + 200_000, a + 1_700_000)
    a = fam["topk_skew"]["array"][0]
    spread("topk_skew", 2500, a + 10_000 + 1_100_000, end)
    # ---- spread families
    for c in N_COUNTS:
        if c > 1:
            spread("n%d" % c, c - 1, 5000, end - 5000)
    for c in SMALL_COUNTS:
        new("small_%d" % c, rng.randrange(16, 21))
        a = rng.randrange(1000, 2_000_000)
        spread("small_%d" % c, c, a, a + rng.randrange(1_100_000, 3_900_000))
    for c in (4607, 4608, 4609):
        new("mid_%d" % c, 16)
        spread("mid_%d" % c, c, 1000, end)
    for c in (9215, 9216, 9217):
        new("lvl_%d" % c, 16)
        spread("lvl_%d" % c, c, 1000, end)
    new("huge_16400", 16)                             # the smallest family that can be asked for more than 16 384 positions
    spread("huge_16400", 16400, 1000, end)
    for c in (300, 5000):
        new("long40_%d" % c, 40)
        spread("long40_%d" % c, c, 1000, end)
    for c in (1024, 1025):                            # DICEY_NO_SA_MINIMA: k_locate_big sorts 1 024 whole and selects from 1 025
        new("flat_%d" % c, 18)
        spread("flat_%d" % c, c, 1000, end)
    new("fam300", 20)                                 # the family the 2 048-job batch is asked against
    spread("fam300", 300, 1000, end)
    # ---- star: a centre that does not occur, substitutions of it and of its reverse complement that do
    q = _unit(rng, 20)
    star = {"q": q, "fwd": [], "rev": []}
    spots = rng.sample(range(3, 17), len(STAR_FWD))
    # (a substitution of revcomp(q) at 19 - i could be the reverse complement of q's substitution at i: other places)
    spots += rng.sample([j for j in range(3, 17) if 19 - j not in spots], len(STAR_REV))
    for k, c in enumerate(STAR_FWD + STAR_REV):
        src = q if k < len(STAR_FWD) else revcomp(q)
        i = spots[k]
        s = src[:i] + rng.choice([x for x in "ACGT" if x != src[i]]) + src[i + 1:]
        name = "star_%s%d" % ("f" if k < len(STAR_FWD) else "r", c)
        new(name, 20, unit=s)
        a = rng.randrange(1000, 2_000_000)
        spread(name, c, a, a + 3_000_000)
        star["fwd" if k < len(STAR_FWD) else "rev"].append(name)
    # ---- crowd: a second centre with 30 substitutions of 17 copies each (the batch that fills a job region)
    q2 = _unit(rng, 20)
    crowd = {"q": q2, "names": []}
    for k, (i, x) in enumerate(rng.sample([(i, x) for i in range(2, 18) for x in "ACGT" if x != q2[i]], CROWD)):
        name = "crowd_%02d" % k
        new(name, 20, unit=q2[:i] + x + q2[i + 1:])
        a = rng.randrange(1000, 2_000_000)
        spread(name, CROWD_COPIES, a, a + 3_000_000)
        crowd["names"].append(name)
    # ---- tails: w 20-mers that share their last 16 characters, b of them with the same four characters in front
    tails = []
    for w, b in TAILS:
        tail, head = _unit(rng, TAIL_K), _rand(rng, 4)
        grp = {"tail": tail, "head": head, "w": w, "b": b, "pos": []}
        for j in range(w):
            h = head
            if j >= b:                                # another head: it differs next to the tail, or only in its first character
                i = 3 if (j - b) % 2 == 0 else 0
                h = head[:i] + rng.choice([x for x in "ACGT" if x != head[i]]) + head[i + 1:]
            for _ in range(1000):
                p = rng.randrange(5000, end - 5000)
                if free(p, 20):
                    break
            else:
                raise _Retry
            text[p:p + 20] = (h + tail).encode()
            used[p:p + 20] = b"\x01" * 20
            grp["pos"].append((p + 4, h))
        grp["pos"].sort()
        tails.append(grp)
    text = bytes(text)
    for t in tails:
        if scan(text, t["tail"].encode()) != [p for p, _ in t["pos"]] or text.find(revcomp(t["tail"]).encode()) >= 0:
            raise _Retry
    for s2 in (q2, revcomp(q2)):
        if text.find(s2.encode()) >= 0:
            raise _Retry
    # ---- every unit, and its reverse complement, occurs where it was planted and nowhere else
    for name, f in fam.items():
        f["pos"].sort()
        if scan(text, f["unit"].encode()) != f["pos"]:
            raise _Retry
        rc = revcomp(f["unit"]).encode()
        if text.find(rc) >= 0:
            raise _Retry
    for s in (q, revcomp(q)):
        if text.find(s.encode()) >= 0:
            raise _Retry
    seqs = [text[cum[i]:cum[i + 1] - 1].decode() for i in range(len(LENGTHS))]
    return {"seqs": seqs, "names": NAMES, "text": text, "seqlen": [n + 1 for n in LENGTHS], "cum": cum, "n": total + 1, "fam": fam,
            "star": star, "crowd": crowd, "tails": tails, "seed": seed}


def genome():
    """{"seqs", "names", "text", "seqlen", "cum", "n", "fam": {name: {"unit", "pos"}}, "star"}: built once per process.  n counts the
    suffix array's entries: the text, its separators and the sentinel."""
    if "g" not in _memo:
        seed = 20270
        while True:
            try:
                _memo["g"] = _build(seed)
                break
            except _Retry:
                seed += 1
    return _memo["g"]


# ---- the stage's arithmetic, restated -----------------------------------------------------------------------------------------------------

def route(pos, take, n, mid_max=0, levels=LEVELS):
    """what k_locate does with a kept string whose occurrences are `pos` (ascending) when it may report `take` of them:
    None (served in the lane: <= 16 occurrences), or {"list": 0 wavefront / 1 small buffer / 2 workgroup / 3 the lane's own selection,
    "level": prefix level of the run or None, "occs": entries the job names, "take"}"""
    occs = len(pos)
    if take == 0 or occs <= 16:
        return None
    if take > BIG_CAP:
        return {"list": 3, "level": None, "occs": occs, "take": take}
    lst = 0 if occs <= LOC_SMALL_MAX else 1 if (occs <= mid_max and take <= TOPK_KMAX) else 2
    level, jo = None, occs
    if lst == 2 and take <= TOPK_KMAX and levels and occs > WALK_MAX:
        lv = 0
        while lv < len(levels) and occs * levels[lv] < 2 * take * n:
            lv += 1
        while lv < len(levels):
            r = bisect.bisect_left(pos, levels[lv])
            if r > WALK_MAX:
                break
            if r >= take:
                level, jo, lst = lv, r, (1 if r <= mid_max else 2)
                break
            lv += 1
    return {"list": lst, "level": level, "occs": jo, "take": take}


def bucket_lanes(pos, lanes):
    """bucket_sort_keys<lanes>: (span, sh, keys per lane) for the positions it is given; it sorts by buckets when no lane holds more
    than BUCKET_SKEW keys and answers false (the caller runs its network) otherwise"""
    nbk, logb = 4 * lanes, 8 if lanes == 64 else 10
    mn, span = min(pos), max(pos) - min(pos)
    sh = 0 if span < nbk else span.bit_length() - logb
    per = [0] * lanes
    for p in pos:
        b = (p - mn) >> sh
        assert b < nbk
        per[b >> 2] += 1
    return span, sh, per


def threshold_exit(vals, k, limit):
    """topk_threshold (k_locate_topk's radix select over `vals`, len(vals) > limit): (the byte shift it returns at, how many values lie
    under its threshold) — it stops as soon as everything up to the end of the k-th value's bin fits `limit`, at shift 0 with exactly k"""
    assert len(vals) > limit >= k
    prefix = mask = below = 0
    kk = k - 1
    for shift in (24, 16, 8, 0):
        hist = [0] * 256
        for x in vals:
            if x & mask == prefix:
                hist[(x >> shift) & 255] += 1
        ex = 0
        for b in range(256):
            if ex <= kk < ex + hist[b]:
                break
            ex += hist[b]
        prefix |= b << shift
        mask |= 255 << shift
        if below + ex + hist[b] <= limit or shift == 0:
            t = prefix | ((1 << shift) - 1 if shift else 0)
            return shift, sum(1 for x in vals if x <= t)
        below += ex
        kk -= ex


def topk_survivors(pos, take):
    """k_locate_topk at the entries keeps `take` .. min(take + 96, 1 024) of the smallest positions (how many is the radix select's
    business): both ends of that range"""
    limit = min(take + 96, TOPK_KMAX)
    return [pos[:h] for h in range(min(take, len(pos)), min(limit, len(pos)) + 1)]


# ---- batches --------------------------------------------------------------------------------------------------------------------------------

D0 = dict(distance=0, forward_only=True)


def exact_families():
    g = genome()
    return [k for k in g["fam"] if not k.startswith(("star_", "long40_", "crowd_"))] + g["star"]["fwd"]


def exact_batches():
    """{max_locations: [family, ...]}: every family's unit at 1, occs - 1, occs, occs + 1 and at the stage's marks below occs"""
    g = genome()
    out = {}
    for name in exact_families():
        occs = len(g["fam"][name]["pos"])
        # (a take above 16 384 is served by ONE lane, 30 s for 16 385 of 16 400 copies: DESIGN.md §16 — the two largest families are
        #  not asked at their own counts)
        own = {m for m in (1, occs - 1, occs, occs + 1) if min(m, occs) <= BIG_CAP}
        for m in sorted(own | {x for x in MARKS if x < occs}):
            if m >= 1:
                out.setdefault(m, []).append(name)
    return dict(sorted(out.items()))


def big_batches():
    """k_locate_big: {max_locations: [family, ...]}"""
    out = {m: ["lvl_9217", "plv_exact"] for m in BIG_TAKES}
    out[4608] = ["lvl_9217", "plv_exact", "lvl_9216"]
    out[4609] = ["lvl_9217", "plv_exact", "lvl_9215"]
    out[16384] = ["lvl_9217", "plv_exact", "huge_16400"]
    return out


def long_batches():
    """the 40-nt unit: a batch whose longest query exceeds 32 nt sorts plain suffix-array values in every job kernel, for all its
    queries — so a wavefront job, a small-buffer job, a clustered one and a run of a prefix level ride along"""
    names = ["long40_300", "long40_5000", "small_64", "skew_33", "mid_4608", "topk_skew", "lvl_9217"]
    return {m: names for m in (1, 5, 17, 299, 300, 301, 501, 577, 928, 1024, 4999, 5000, 5001)}


def plv_cases():
    """(family, max_locations) of the prefix-level decision"""
    return [("plv_run", 1000), ("plv_next", 700), ("plv_dense", 1000), ("plv_exact", 400), ("plv_exact", 401)]


def walk_batches():
    """the batches that run again without prefix levels, without records and without block minima: {max_locations: [family, ...]}"""
    out = {}
    for name, m in plv_cases() + [("topk_skew", 501), ("topk_skew", 500), ("topk_skew", 1024), ("topk_skew", 100), ("run_600", 300), ("run_600", 257)] + \
            [(f, m) for f in ("lvl_9215", "lvl_9216", "lvl_9217") for m in (1, 577, 928, 1024)] + [("flat_1024", 3), ("flat_1025", 3)]:
        out.setdefault(m, []).append(name)
    return dict(sorted(out.items()))


def star_strings():
    """the ten kept strings of hunt(q, distance=1) in the reference's order (a std::set per strand, forward strand first) with their
    counts: [(family, count)]"""
    g = genome()
    out = []
    for side in ("fwd", "rev"):
        for name in sorted(g["star"][side], key=lambda k: g["fam"][k]["unit"]):
            out.append((name, len(g["fam"][name]["pos"])))
    return out


def star_marks():
    """max_locations at every prefix sum of the ten counts, one below and one above"""
    out, acc = set(), 0
    for _, c in star_strings():
        acc += c
        out |= {acc - 1, acc, acc + 1}
    return sorted(m for m in out if m >= 1)


def tails_queries():
    """per group: the planted 20-mer whose head is the group's own (the table window of order 16 holds w suffixes, b of them behind that
    head), its last 19, 18 and 17 characters (fewer characters in front of the window), and the 20-mer with one substitution in the
    head and one in the tail — [(query, group index)]"""
    g, rng, out = genome(), random.Random(41), []
    for gi, t in enumerate(g["tails"]):
        s = t["head"] + t["tail"]
        out += [(s, gi), (s[1:], gi), (s[2:], gi), (s[3:], gi)]
        for i in (rng.randrange(0, 4), rng.randrange(4, 20)):
            out.append((s[:i] + rng.choice([x for x in "ACGT" if x != s[i]]) + s[i + 1:], gi))
    return out


def crowd_batch(nq=3500):
    """`nq` times the crowd's centre: CROWD wavefront jobs each"""
    return [genome()["crowd"]["q"]] * nq


def units(names):
    g = genome()
    return [g["fam"][k]["unit"] for k in names]


def hit_of(p, unit):
    """the hit of an exact forward occurrence at text position p, as the oracle pushes it"""
    cum = genome()["cum"]
    c = bisect.bisect_right(cum, p) - 1
    return (0, c, p - cum[c] + 1, "+", unit, unit)


def scan_expectation(names, m):
    """per query: the first m positions of a scan of the text, as hits"""
    g = genome()
    return [[hit_of(p, g["fam"][k]["unit"]) for p in g["fam"][k]["pos"][:m]] for k in names]


def jobs_batch(nq=2048, seed=5):
    """`nq` queries with one substitution each against fam300: at distance 1 every one keeps the unit itself, 300 occurrences"""
    rng = random.Random(seed)
    u = genome()["fam"]["fam300"]["unit"]
    out = []
    for _ in range(nq):
        i = rng.randrange(1, 19)
        out.append(u[:i] + rng.choice([x for x in "ACGT" if x != u[i]]) + u[i + 1:])
    return out


def plain_batch(nq=64, seed=6):
    """random 20-mers: no string of theirs has more than a stray occurrence, so no job is queued"""
    rng = random.Random(seed)
    return [_rand(rng, 20) for _ in range(nq)]


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------------

def oracle_index():
    if "orc" not in _memo:
        g = genome()
        d = tempfile.mkdtemp(prefix="locate_shapes_")
        path = os.path.join(d, "locate.fm9")
        O.build_fm9(g["text"], path)
        _memo["orc"] = O.Index(path)
        _memo["orc_path"] = path
    return _memo["orc"]


class Reference:
    """the oracle behind the interface tests/test_gpu_locate_topk.py's _compare asks for; a query is answered once per parameter set
    however often it is asked or repeated inside a batch"""

    def hunt(self, seqlen, names, qs, want_hits=True, **kw):
        key = tuple(sorted(kw.items()))
        memo = _memo.setdefault(("hunt", key), {})
        todo = [q for q in dict.fromkeys(qs) if q not in memo]
        if todo:
            _, hits = oracle_index().hunt(seqlen, names, todo, want_hits=True, **kw)
            for q in todo:
                memo[q] = []
            for h in hits:
                memo[todo[h[0]]].append(h[1:])
        return None, [(qi,) + h for qi, q in enumerate(qs) for h in memo[q]]


class Canned:
    """the same interface over hits computed before (a child process gets its expectation pickled: [per-query hit lists])"""

    def __init__(self, per):
        self.per = per

    def hunt(self, seqlen, names, qs, want_hits=True, **kw):
        assert len(qs) == len(self.per)
        return None, [(qi,) + tuple(h) for qi, hs in enumerate(self.per) for h in hs]


def per_query(qs, **kw):
    """the oracle's hits as one list per query"""
    g = genome()
    per = [[] for _ in qs]
    for h in Reference().hunt(g["seqlen"], g["names"], qs, **kw)[1]:
        per[h[0]].append(h[1:])
    return per


def read_jobs(path):
    """the job lists a development build dumped: [(list, level or None, occs, take, string length)], sorted"""
    import struct
    out = []
    if os.path.exists(path):
        for lo, occs, take, w in struct.iter_unpack("<4I", open(path, "rb").read()):
            lv = (w >> 24) & 15
            out.append((w >> 28, lv - 1 if lv else None, occs, take, w & 0xFFFFFF))
    return sorted(out, key=repr)


def expected_jobs(names, m, mid_max=0, levels=LEVELS):
    """what route() says about an exact forward batch: the same tuples"""
    g, out = genome(), []
    for k in names:
        f = g["fam"][k]
        r = route(f["pos"], min(m, len(f["pos"])), g["n"], mid_max, levels)
        if r is not None and r["list"] != 3:
            out.append((r["list"], r["level"], r["occs"], r["take"], len(f["unit"])))
    return sorted(out, key=repr)


def first_difference(got, want):
    """(query index, hit index) of the first hit two per-query hit lists disagree on, None when they are equal"""
    for qi, (a, b) in enumerate(zip(got, want)):
        if a != b:
            k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
            return qi, k
    return None
