"""Generated oligo pairs for the thal kernels (test_thal_corpus.py on the CPU, test_gpu_thal_reference.py on the GPU).

groups() returns named lists of (oligo1, oligo2); every group is meant to be sent to dg_thal_batch as a batch of its own,
because the wave kernel's LDS layout (row stride, cell capacity, wavefronts per workgroup) follows the batch's longest
oligo 1 / oligo 2 (thal_api.hip, dg_thal_batch).  Deterministic: the same seed gives the same corpus.  Pure Python, no GPU.

Empty oligos are left out on purpose: the reference refuses them and only then sets the temperature (0.0); what
dg_thal_batch does with one is not part of this corpus.
"""
import random
from collections import OrderedDict

SEED = 20261016
WAVE_LEN_CAP = 48   # kWaveLenCap in dg_thal_batch: longer oligos go to the sequential kernel
MAX_ALIGN = 60      # THAL_MAX_ALIGN: thal() refuses a pair with both oligos longer

GEOMETRIES = [(8, 8), (20, 20), (20, 48), (48, 20), (33, 41), (48, 48)]
CAP_SIZES = [(20, 20), (32, 48), (48, 48)]
N_GEOMETRY = 2000
N_SHARED = 300

# (mv, dv, dntp, dna_conc): primer3's defaults and the second golden set's, then the settings that reach the corners of the
# salt correction (dv = 0 makes dntp irrelevant; dntp > dv goes through the fmax) and very low / high concentrations
ENVS = OrderedDict([
    ("default", dict(mv=50.0, dv=1.5, dntp=0.6, dna_conc=50.0)),
    ("golden_long", dict(mv=40.0, dv=2.5, dntp=0.8, dna_conc=100.0)),
    ("no_divalent", dict(mv=50.0, dv=0.0, dntp=0.0, dna_conc=50.0)),
    ("dntp_above_dv", dict(mv=50.0, dv=1.5, dntp=3.0, dna_conc=50.0)),
    ("low", dict(mv=1.0, dv=0.0, dntp=0.0, dna_conc=1.0)),
    ("high", dict(mv=1000.0, dv=10.0, dntp=0.0, dna_conc=1000.0)),
    # the `dv <= 0` rule of saltCorrectS (thal.h:357) only shows when dntp lies below a non-positive dv: everywhere else the fmax gives
    # the same 0.  Not a meaningful buffer, but the only input that tells the rule from its absence.
    ("negative", dict(mv=50.0, dv=-1.0, dntp=-2.0, dna_conc=50.0)),
])
N_ENV = 500

_COMP = str.maketrans("ACGTN", "TGCAN")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def code(ch):
    """str2int (thal.h:260-275): everything but ACGT, in either case, is 4"""
    return "ACGT".find(ch.upper()) if ch.upper() in "ACGT" else 4


def pairing_cells(a, b):
    """number of DP cells (i, j) whose bases pair, a[i] + b_rev[j] == 3 with both < 4: what the wave kernel's table stores"""
    ca, cb = [0] * 5, [0] * 5
    for ch in a:
        ca[code(ch)] += 1
    for ch in b:
        cb[code(ch)] += 1
    return sum(ca[c] * cb[3 - c] for c in range(4))


def wave_cell_cap(len1, stride):
    """wave_cell_cap of dicey_amd/csrc/thal_wave.hpp:55, restated: 7/16 of the full table plus one row plus 16.  A pair
    with MORE pairing cells is handed to the sequential kernel (thal_wave.hpp:248: exactly `cap` cells still fit)."""
    return (len1 * stride * 7) // 16 + stride + 16


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _near_complement(rng, a, maxlen, edits=4):
    """reverse complement of `a` with up to `edits` substitutions / insertions / deletions (as test_gpu_thal_wave.py)"""
    b = list(revcomp(a))
    for _ in range(rng.randint(0, edits)):
        k = rng.randrange(len(b))
        r = rng.random()
        if r < 0.4:
            b[k] = rng.choice("ACGTN")
        elif r < 0.7:
            b.insert(k, rng.choice("ACGT"))
        elif len(b) > 1:
            del b[k]
    return "".join(b)[:maxlen]


def _mixed_pair(rng, L1, L2):
    l1, l2 = rng.randint(1, L1), rng.randint(1, L2)
    a = _rand(rng, l1)
    if rng.random() < 0.6:   # mostly near-complementary: long duplexes with loops and bulges
        return a, _near_complement(rng, a, L2)
    return a, _rand(rng, l2, "ACGTN")


def shared_pairs(seed=SEED):
    """(shared8, shared20): 300 pairs of at most 8 nt that every geometry group holds, and 300 of 9-20 nt that every geometry
    group with maxima of at least (20, 20) holds — all but (8, 8), whose maxima they would break."""
    rng = random.Random(seed * 7 + 1)
    s8 = [_mixed_pair(rng, 8, 8) for _ in range(N_SHARED)]
    s20 = []
    while len(s20) < N_SHARED:
        l1 = rng.randint(9, 20)
        a = _rand(rng, l1)
        b = _near_complement(rng, a, 20) if rng.random() < 0.6 else _rand(rng, rng.randint(9, 20), "ACGTN")
        if len(b) >= 9:
            s20.append((a, b))
    return s8, s20


def _geometry_group(rng, L1, L2, s8, s20):
    pairs = list(s8)
    if L1 >= 20 and L2 >= 20:
        pairs += s20
    pairs.append((_rand(rng, L1), _rand(rng, L2)))          # the pair that sets the batch maxima
    a = _rand(rng, L1)
    pairs.append((a, (revcomp(a) * 2)[:L2] if L2 > L1 else revcomp(a)[:L2]))
    while len(pairs) < N_GEOMETRY:
        pairs.append(_mixed_pair(rng, L1, L2))
    rng.shuffle(pairs)
    return pairs


def _biased(rng, n, letters, weights):
    return "".join(rng.choices(letters, weights)[0] for _ in range(n))


def _cap_group(rng, L1, L2):
    """Pairs of exactly L1 x L2 whose number of pairing cells lies around wave_cell_cap(L1, L2).  Returns the list and the
    pairs found at exact counts {count: pair} for cap-2 .. cap+2."""
    cap, area = wave_cell_cap(L1, L2), L1 * L2
    band = (3 * area) // 100
    below, above, runs_back = [], [], []
    tries = 0
    while (len(below) < 40 or len(above) < 40 or len(runs_back) < 24) and tries < 400000:
        tries += 1
        r = rng.random()
        if r < 0.5:    # two letters against their partners: p*q + (1-p)*(1-q) of the table
            p, q = rng.uniform(0.55, 0.95), rng.uniform(0.55, 0.95)
            x, y = rng.choice(["AC", "AG", "CT", "GT", "CA", "TG"])
            a = _biased(rng, L1, x + y, [p, 1 - p])
            b = _biased(rng, L2, revcomp(x) + revcomp(y), [q, 1 - q])
        elif r < 0.75:  # three letters
            w = [rng.uniform(0.5, 0.8), rng.uniform(0.1, 0.3), rng.uniform(0.02, 0.2)]
            ls = rng.sample("ACGT", 3)
            a = _biased(rng, L1, ls, w)
            b = _biased(rng, L2, [revcomp(c) for c in ls], w)
        else:           # a perfect or near-perfect duplex from position 1 on: its traceback runs back into the first rows,
            w = [rng.uniform(0.5, 0.8), rng.uniform(0.1, 0.3), rng.uniform(0.02, 0.2)]   # whose records sit right behind the cells
            ls = rng.sample("ACGT", 3)
            a = _biased(rng, L1, ls, w)
            b = revcomp(a)
            b = (b + _biased(rng, L2, [revcomp(c) for c in ls], w))[:L2] if L2 >= L1 else b[:L2]
            n = pairing_cells(a, b)
            if cap - 8 <= n <= cap + 8 and len(runs_back) < 24:
                runs_back.append((a, b))
            continue
        n = pairing_cells(a, b)
        if cap - band <= n <= cap and len(below) < 40:
            below.append((a, b))
        elif cap < n <= cap + band and len(above) < 40:
            above.append((a, b))
    # exact counts: oligo 1 over two letters (k of the first), oligo 2 over the partners plus one letter that pairs with nothing in
    # oligo 1, so cells = k * m1 + (L1 - k) * m2; the letters are then shuffled
    exact = {}
    for target in range(cap - 2, cap + 3):
        found = None
        for k in range(L1, L1 // 2 - 1, -1):
            for m1 in range(L2, -1, -1):
                rest = target - k * m1
                if rest < 0:
                    continue
                if L1 - k == 0:
                    m2 = 0
                    if rest != 0:
                        continue
                elif rest % (L1 - k) == 0:
                    m2 = rest // (L1 - k)
                else:
                    continue
                if m1 + m2 <= L2:
                    found = (k, m1, m2)
                    break
            if found:
                break
        if found:
            k, m1, m2 = found
            a = list("A" * k + "C" * (L1 - k))
            b = list("T" * m1 + "G" * m2 + "A" * (L2 - m1 - m2))
            rng.shuffle(a)
            rng.shuffle(b)
            pair = ("".join(a), "".join(b))
            assert pairing_cells(*pair) == target
            exact[target] = pair
    pairs = below + above + runs_back + list(exact.values())
    return pairs, exact


def cap_groups(seed=SEED):
    """{(L1, L2): (pairs, exact)} — see _cap_group"""
    out = OrderedDict()
    for L1, L2 in CAP_SIZES:
        out[(L1, L2)] = _cap_group(random.Random(seed * 11 + L1 * 100 + L2), L1, L2)
    return out


def _structure_group(rng):
    pairs = []
    for n in range(1, WAVE_LEN_CAP + 1):     # homopolymers at every length
        pairs += [("A" * n, "T" * n), ("G" * n, "C" * n), ("A" * n, "A" * n), ("C" * n, "G" * WAVE_LEN_CAP)]
    for n in range(1, WAVE_LEN_CAP // 2 + 1):
        pairs += [("AT" * n, "AT" * n), ("GC" * n, "GC" * n), ("TA" * n, "AT" * n), ("CG" * n, "GC" * n)]
    for n in range(1, WAVE_LEN_CAP // 4 + 1):
        pairs += [("ACGT" * n, "ACGT" * n), ("ACGTTGCA" * (n // 2), "TGCAACGT" * (n // 2))][:2 if n > 1 else 1]
    for _ in range(150):   # both oligos self-complementary, even length: the symmetric RC
        h1, h2 = _rand(rng, rng.randint(1, 24)), _rand(rng, rng.randint(1, 24))
        p, q = h1 + revcomp(h1), h2 + revcomp(h2)
        pairs += [(p, p), (p, q)]
    for _ in range(100):   # hairpin-prone: stem, loop, stem — and one self-complementary oligo against one that is not
        stem, loop = _rand(rng, rng.randint(3, 12)), _rand(rng, rng.randint(3, 8))
        p = (stem + loop + revcomp(stem))[:WAVE_LEN_CAP]
        pairs += [(p, p), (p, revcomp(p)), (stem + revcomp(stem), p)]
    for _ in range(100):   # N at either end, N inside, N only
        a = _rand(rng, rng.randint(2, 46))
        b = revcomp(a)
        pairs += [("N" + a, b + "N"), (a + "N", "N" + b), ("N" + a + "N", b), (a, "N" + b + "N")]
    for n in range(1, WAVE_LEN_CAP + 1, 3):
        pairs += [("N" * n, "N" * n), ("N" * n, _rand(rng, n)), (_rand(rng, n), "N" * n)]
    return pairs


def _alphabet_group(rng):
    pairs = []
    iupac = "URYKMSWBDHVNX-*"
    for _ in range(150):
        a = _rand(rng, rng.randint(4, 40))
        b = _near_complement(rng, a, WAVE_LEN_CAP, 2)
        k = rng.randrange(len(a))
        pairs += [(a.lower(), b), (a, b.lower()), (a.lower(), b.lower()),
                  ("".join(c.lower() if rng.random() < 0.5 else c for c in a), b),
                  (a.replace("T", "U"), b), (a, b.replace("T", "u")),
                  (a[:k] + rng.choice(iupac) + a[k + 1:], b),
                  (a, "".join(rng.choice(iupac + iupac.lower()) if rng.random() < 0.15 else c for c in b))]
    for _ in range(40):    # lower-case self-complementary oligos: the symmetry test upper-cases (thal.h:1992)
        h = _rand(rng, rng.randint(2, 20))
        p = h + revcomp(h)
        pairs += [(p.lower(), p), (p.lower(), p.lower())]
    return pairs


def _long_groups(rng):
    mid = []
    for l1 in range(WAVE_LEN_CAP + 1, 65):     # 49 .. 64 x 1 .. 64: the sequential kernel's own pairs
        for _ in range(12):
            a = _rand(rng, l1)
            l2 = rng.randint(1, 64)
            if l1 > MAX_ALIGN:
                l2 = min(l2, MAX_ALIGN)
            b = _near_complement(rng, a, l2) if rng.random() < 0.6 else _rand(rng, l2, "ACGTN")
            mid.append((a, b))
            if len(b) <= MAX_ALIGN or l1 <= MAX_ALIGN:
                mid.append((b, a))
    mid = [(a, b) for a, b in mid if not (len(a) > MAX_ALIGN and len(b) > MAX_ALIGN)]
    refused = []
    for _ in range(30):
        a = _rand(rng, rng.randint(MAX_ALIGN + 1, 90))
        refused += [(a, revcomp(a)), (a, _rand(rng, rng.randint(MAX_ALIGN + 1, 200)))]
    refused += [("A" * 61, "T" * 61), ("ACGT" * 16, "ACGT" * 16)]
    long_short = []
    for _ in range(100):                       # long x short in both orders (a primer against a long target and back)
        l1, l2 = rng.randint(MAX_ALIGN + 1, 400), rng.randint(1, MAX_ALIGN)
        a = _rand(rng, l1)
        if rng.random() < 0.7:                 # the short oligo binds somewhere inside the long one
            p = rng.randrange(0, l1 - min(l2, l1) + 1)
            b = _near_complement(rng, a[p:p + l2], MAX_ALIGN, 3)
        else:
            b = _rand(rng, l2, "ACGTN")
        long_short += [(a, b), (b, a)]
    return mid, refused, long_short


def env_pairs(seed=SEED):
    """the 500 mixed pairs every environment of ENVS is run on (1-48 nt, a few longer, some self-complementary)"""
    rng = random.Random(seed * 13 + 5)
    pairs = [("GCCCCATAGGTTTTGAACTCA", revcomp("GCCCCATAGGTTTTGAACTCA"))]   # SURVEY.md known-answer primer
    while len(pairs) < N_ENV - 60:
        pairs.append(_mixed_pair(rng, WAVE_LEN_CAP, WAVE_LEN_CAP))
    for _ in range(30):
        h = _rand(rng, rng.randint(2, 24))
        pairs.append((h + revcomp(h), h + revcomp(h)))
    while len(pairs) < N_ENV:
        a = _rand(rng, rng.randint(49, 64))
        pairs.append((a, _near_complement(rng, a, MAX_ALIGN)))
    return pairs


_cache = {}


def groups(seed=SEED):
    """OrderedDict name -> list of (oligo1, oligo2), all for the default environment"""
    if seed in _cache:
        return _cache[seed]
    g = OrderedDict()
    s8, s20 = shared_pairs(seed)
    for L1, L2 in GEOMETRIES:
        g["geometry_%dx%d" % (L1, L2)] = _geometry_group(random.Random(seed * 3 + L1 * 100 + L2), L1, L2, s8, s20)
    for (L1, L2), (pairs, _) in cap_groups(seed).items():
        g["cap_%dx%d" % (L1, L2)] = pairs
    g["structure"] = _structure_group(random.Random(seed * 5 + 1))
    g["alphabet"] = _alphabet_group(random.Random(seed * 5 + 2))
    mid, refused, long_short = _long_groups(random.Random(seed * 5 + 3))
    g["long_49_64"] = mid
    g["both_over_60"] = refused
    g["long_x_short"] = long_short
    for k, (a, b) in enumerate(CUTOFF_PAIRS):
        g.setdefault("entropy_cutoff", []).append((a, b))
    for name, pairs in REGRESSIONS.items():
        g["regression_" + name] = list(pairs)
    _cache[seed] = g
    return g


REFUSED_GROUPS = ("both_over_60",)   # the only group whose pairs the reference refuses

# Pairs in which an opening candidate with S < -2500 wins (thal.h:1322-1330), the case the wave kernel hands back: found by
# cutoff_search() below with the host build's counter.  Empty: the search met none (thal section).
CUTOFF_PAIRS = []

# named pairs that once failed, {name: [pairs]}
REGRESSIONS = OrderedDict()


def cutoff_search_pairs(n, seed=SEED):
    """`n` ACGT pairs of 30-48 nt built to hold long AT-rich interior loops between GC stems: the search for inputs that reach
    the entropy cut-off of the table fill"""
    rng = random.Random(seed * 17 + 3)
    out = []
    for _ in range(n):
        L = rng.randint(30, 48)
        s1 = rng.randint(3, 8)
        s2 = rng.randint(3, 8)
        loop1 = max(1, min(L - s1 - s2, rng.randint(4, 30)))
        a = _rand(rng, s1, "GC") + _biased(rng, loop1, "ATGC", [0.45, 0.45, 0.05, 0.05]) + _rand(rng, s2, "GC")
        a = (a + _biased(rng, L, "ATGC", [0.4, 0.4, 0.1, 0.1]))[:L]
        r = rng.random()
        if r < 0.5:     # the stems pair, the loop of oligo 2 is a different AT-rich run
            loop2 = rng.randint(1, 30)
            b = revcomp(a[s1 + loop1:s1 + loop1 + s2]) + _biased(rng, loop2, "ATGC", [0.45, 0.45, 0.05, 0.05]) + revcomp(a[:s1])
            b = (b + _biased(rng, 48, "ATGC", [0.4, 0.4, 0.1, 0.1]))[:rng.randint(30, 48)]
        elif r < 0.8:
            b = _near_complement(rng, a, 48, 6)
            b = (b + _biased(rng, 48, "AT", [0.5, 0.5]))[:rng.randint(30, 48)]
        else:
            b = _biased(rng, rng.randint(30, 48), "ATGC", [0.4, 0.4, 0.1, 0.1])
        out.append((a, b))
    return out
