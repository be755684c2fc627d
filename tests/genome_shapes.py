"""Seeded genomes of the shapes real FASTA files have and `make_genome` (tests/conftest.py) never makes: one sequence, hundreds
and thousands of sequences, empty records, texts without N, hard-masked and bisulfite-converted texts, A/T tandem repeats, N runs
of one exact length, all IUPAC letters, texts of a few symbols and texts over (almost) every byte value.

Every generator returns {"seqs", "text", "seqlen", "names"} with `genome_text` (src/index.h:105-113) as the text rule.  The
pattern and query lists the GPU module runs are made here as well, so that tests/test_genome_shapes_host.py validates the
reference side on exactly those inputs.  A plain module: no fixtures, no pytest hooks."""
import random

from conftest import genome_text, make_genome, make_queries, revcomp

AMBIG = "RYKMSWBDHVN"       # with A, C, G, T: the 15 IUPAC nucleotide letters
TINY_SIZES = (5, 62, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4095, 4096, 4097)


def _shape(seqs, prefix="s"):
    return {"seqs": seqs, "text": genome_text(seqs), "seqlen": [len(s) + 1 for s in seqs],
            "names": ["%s%d" % (prefix, i + 1) for i in range(len(seqs))]}


def _rnd(rng, m, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(m))


def n_run_lengths(text):
    """the set of lengths of the maximal runs of 'N' in a text (bytes)"""
    out, run = set(), 0
    for c in text + b"\n":
        if c == 78:
            run += 1
        elif run:
            out.add(run)
            run = 0
    return out


def single_no_n(seed=201):
    """1 sequence, 300 kb, A/C/G/T only, copied segments on both strands: nseq = 1, no N run at all, sigma 6"""
    rng = random.Random(seed)
    s = list(_rnd(rng, 300000))
    for _ in range(150):
        a, m, d = rng.randrange(290000), rng.randint(20, 600), rng.randrange(290000)
        piece = "".join(s[a:a + m])
        s[d:d + m] = piece if rng.random() < 0.5 else revcomp(piece)
    for _ in range(40):
        a = rng.randrange(299000)
        m = rng.randint(5, 40)
        s[a:a + m] = rng.choice("ACGT") * m
    return _shape(["".join(s[:300000])], "chrom")


def _many(rng, lengths, nrate=0.002):
    """sequences of the given lengths: random A/C/G/T, pieces copied from earlier sequences (both strands), sparse N"""
    seqs, pool = [], ""
    for m in lengths:
        s = []
        while len(s) < m:
            r = rng.random()
            if r < nrate:
                s.extend("N" * rng.randint(1, 6))
            elif r < nrate + 0.004 and len(pool) > 400:
                a = rng.randrange(len(pool) - 60)
                piece = pool[a:a + rng.randint(15, 60)]
                s.extend(piece if rng.random() < 0.6 else revcomp(piece))
            else:
                s.append(rng.choice("ACGT"))
        s = "".join(s[:m])
        seqs.append(s)
        if len(pool) < 200000:
            pool += s
    return seqs


def seq_count(nseq, seed=None):
    """nseq sequences of 60-150 nt (512 / 513: the two sides of k_verify_memo's LDS / global sequence-start lookup)"""
    rng = random.Random(300 + nseq if seed is None else seed)
    lengths = [rng.randint(60, 150) for _ in range(nseq)]
    lengths[-1] = 150   # the last sequence (index 512 of seq513) is the only one above the edge: room for the queries aimed at it
    return _shape(_many(rng, lengths), "scaf")


def seq512():
    return seq_count(512)


def seq513():
    return seq_count(513)


MANY_SHORT_EMPTY = (0, 5, 700, 701, 1500, 2000, 2600, 2999)   # 700 / 701 are adjacent; the first and the last record are empty


def many_short(seed=404):
    """3 000 sequences, ~400 kb: 8 empty records (two adjacent, the first and the last one), more than 300 of 1-19 nt (one of exactly 12
    at index 1201), the rest of 20-400 nt; sparse N"""
    rng = random.Random(seed)
    lengths = []
    for i in range(3000):
        if i in MANY_SHORT_EMPTY:
            lengths.append(0)
        elif i == 1201:
            lengths.append(12)
        elif i % 9 == 4 and len([x for x in lengths if 0 < x < 20]) < 319:
            lengths.append(rng.randint(1, 19))
        else:
            lengths.append(rng.randint(20, 400) if rng.random() < 0.35 else rng.randint(20, 200))
    seqs = _many(rng, lengths)
    seqs[1201] = _rnd(rng, 12)    # pure A/C/G/T; its neighbours are at least 20 nt long (1200 and 1202 are not 4 mod 9)
    return _shape(seqs, "ctg")


def hard_masked(seed=505):
    """4 sequences of 40 kb, 55-65 % N in runs of 50-5 000: N is the most frequent symbol, the shortest N run is 50"""
    rng = random.Random(seed)
    seqs = []
    for c in range(4):
        want_n = rng.uniform(0.57, 0.63)
        s = list(_rnd(rng, rng.randint(30, 300)) if c % 2 else "N" * (50 if c == 0 else 731))   # sequences that begin with a run, too
        n_n = s.count("N")
        while len(s) < 40000:
            if n_n < want_n * (len(s) + 300) and s[-1] != "N":
                m = rng.choice((50, 51, 64, 65, rng.randint(50, 400), rng.randint(400, 2000), rng.randint(400, 5000)))
                s.extend("N" * m)
                n_n += m
            if len(seqs) and rng.random() < 0.3:      # unmasked pieces that occur elsewhere, either strand
                src = rng.choice(seqs).replace("N", "")
                a = rng.randrange(len(src) - 200)
                piece = src[a:a + rng.randint(20, 200)]
                s.extend(piece if rng.random() < 0.5 else revcomp(piece))
            else:
                s.extend(_rnd(rng, rng.randint(1, 400)))
        s = s[:40000]
        # a cut inside a run may leave a short one: restore the property at the end of the sequence
        k = len(s)
        while k and s[k - 1] == "N":
            k -= 1
        if 0 < len(s) - k < 50:
            s[k:] = _rnd(rng, len(s) - k)
        seqs.append("".join(s))
    return _shape(seqs, "masked")


def bisulfite(seed=606):
    """3 sequences of 30 kb over A/G/T/N (every C converted to T): the code of C is absent from the wavelet tree"""
    seqs = [s.replace("C", "T") for s in make_genome(seed, 3, 30000)]
    return _shape(seqs, "bs")


def at_tandem(seed=707):
    """2 sequences, ~100 kb, A/T only: tandem repeats of 1-7 nt units (up to 30 kb long) and a few unique islands: sigma 4,
    SA intervals of thousands of rows, many prefix-doubling rounds in the builder"""
    rng = random.Random(seed)
    seqs = []
    for c in range(2):
        s = []
        first = True
        while len(s) < 50000:
            unit = _rnd(rng, rng.randint(1, 7), "AT")
            copies = (30000 if first and c == 0 else rng.randint(50, 4000)) // len(unit)
            s.extend(unit * copies)
            first = False
            if rng.random() < 0.5:
                s.extend(_rnd(rng, rng.randint(200, 500), "AT"))
        seqs.append("".join(s[:50000]))
    return _shape(seqs, "sat")


def nrun(r, seed=None):
    """3 sequences of 30 kb like the small genome (copies, homopolymers, six IUPAC letters), every N run of length exactly r;
    runs at the very start of a sequence, at the very end of one, and 1 and 2 nt from an end"""
    rng = random.Random(800 + r if seed is None else seed)
    seqs = []
    for s in make_genome(rng.randrange(1 << 30), 3, 30000, nrate=0.0, iupac=True):
        s = list(s)
        starts = {0, len(s) - r} if len(seqs) == 0 else ({1, len(s) - r - 1} if len(seqs) == 1 else {2, len(s) - r - 2})
        while len(starts) < 70:
            starts.add(rng.randrange(3 * r, len(s) - 3 * r))
        last = -10
        for a in sorted(starts):
            if a <= last + r:          # keep a gap of at least one other letter between two runs
                continue
            s[a:a + r] = "N" * r
            for j in (a - 1, a + r):   # and no N next to a run
                if 0 <= j < len(s) and s[j] == "N":
                    s[j] = rng.choice("ACGT")
            last = a
        seqs.append("".join(s))
    return _shape(seqs, "chr")


def nrun2():
    return nrun(2)


def nrun3():
    return nrun(3)


def iupac_rich(seed=909):
    """3 sequences of 20 kb: stretches of A/C/G/T (40-120 nt) between stretches of the 11 ambiguity letters (10-40 nt), which come
    from one shuffled pool with the same count of every letter: ~2 % each, sigma 17, bps 5, Huffman ties"""
    rng = random.Random(seed)
    seqs = []
    for _ in range(3):
        s = []
        while len(s) < 20000:
            s.extend(_rnd(rng, rng.randint(40, 120)))
            s.extend("?" * rng.randint(10, 40))
        seqs.append(s[:20000])
    holes = sum(s.count("?") for s in seqs)
    pool = list(AMBIG * (holes // len(AMBIG))) + list(AMBIG[:holes % len(AMBIG)])
    rng.shuffle(pool)
    seqs = ["".join(pool.pop() if c == "?" else c for c in s) for s in seqs]
    for c in range(3):   # a repeated piece per sequence, so that hunts have more than one hit per query
        a = rng.randrange(15000)
        seqs[(c + 1) % 3] = seqs[(c + 1) % 3][:5000 + 97 * c] + seqs[c][a:a + 300] + seqs[(c + 1) % 3][5300 + 97 * c:]
    return _shape(seqs, "amb")


def tiny():
    """name -> shape for texts of 1, 2, 5, 62 ... 4 097 symbols (the sentinel not counted): arrays shorter than a wavefront, the
    64-bit word and 512-bit superblock edges of the bit vector, the ISA sample count (n - 1) / 64 + 1"""
    out = {"tiny_1": _shape([""]), "tiny_2a": _shape(["A"]), "tiny_2n": _shape(["", ""])}
    for size in TINY_SIZES:
        rng = random.Random(1000 + size)
        nseq = 1 if size < 20 else rng.randint(2, 4)
        left = size - nseq
        lengths = []
        for i in range(nseq):
            m = left if i == nseq - 1 else rng.randint(left // (2 * nseq), left // nseq)
            lengths.append(m)
            left -= m
        seqs = []
        for m in lengths:
            s = list(_rnd(rng, m))
            if m > 40:
                a = rng.randrange(m - 4)
                s[a:a + 2] = "NN"
            if m > 200:                      # a piece that occurs twice
                s[m - 60:m - 30] = s[20:50]
            seqs.append("".join(s))
        g = _shape(seqs)
        assert len(g["text"]) == size
        out["tiny_%d" % size] = g
    return out


def _bytes_shape(data):
    """text rule of genome_text over raw bytes: the sequences are what stands between the '\\n' bytes; the text ends with one"""
    assert data.endswith(b"\n") and 0 not in data
    seqs = data[:-1].split(b"\n")
    return {"seqs": seqs, "text": data, "seqlen": [len(s) + 1 for s in seqs], "names": ["b%d" % (i + 1) for i in range(len(seqs))]}


def bytes_wide(seed=111):
    """builder and seam only.  "wide": 20 kb over the byte values 1-255, every value present (sigma 256, bps 8, K 8); "w70": 20 kb
    over 70 values (sigma 71 with the sentinel, bps 7, K 9).  The oracle's writer takes every value from 1 to 255, so nothing had to be
    narrowed; 0 is the sentinel and is refused by both writers."""
    rng = random.Random(seed)
    allv = list(range(1, 256))
    a = allv + [rng.choice(allv) if rng.random() < 0.7 else rng.choice(allv[:16]) for _ in range(20000 - 256)]
    rng.shuffle(a)
    vals70 = sorted(rng.sample([v for v in allv if v != 10], 69) + [10])
    b = vals70 + [rng.choice(vals70) for _ in range(20000 - 71)]
    rng.shuffle(b)
    return {"bytes_wide": _bytes_shape(bytes(a) + b"\n"), "bytes_w70": _bytes_shape(bytes(b) + b"\n")}


DNA_SHAPES = {"single_no_n": single_no_n, "seq512": seq512, "seq513": seq513, "many_short": many_short, "hard_masked": hard_masked,
              "bisulfite": bisulfite, "at_tandem": at_tandem, "nrun2": nrun2, "nrun3": nrun3, "iupac_rich": iupac_rich}
TINY_NAMES = ["tiny_1", "tiny_2a", "tiny_2n"] + ["tiny_%d" % n for n in TINY_SIZES]
BYTES_NAMES = ["bytes_wide", "bytes_w70"]
NAMES = list(DNA_SHAPES) + TINY_NAMES + BYTES_NAMES
_cache = {}


def all_shapes():
    """name -> shape, every shape of this module (generated once per process)"""
    if not _cache:
        for name, fn in DNA_SHAPES.items():
            _cache[name] = fn()
        _cache.update(tiny())
        _cache.update(bytes_wide())
        assert list(_cache) == NAMES
    return _cache


def is_dna(name):
    return not name.startswith("bytes_")


# ---------------------------------------------------------------------------------------------------------------------------------
# patterns for count / locate / extract


def seam_patterns(name, g, n=160):
    """bytes patterns: sampled from the text (1-40 long; on the many-sequence shapes many of them cross a '\\n'), windows over
    separators and over empty records, letters the text may lack, whole short sequences with and without their separators, random
    strings, and one pattern longer than the text"""
    rng = random.Random(hash_name(name))
    text = g["text"]
    L = len(text)
    pats = []
    for _ in range(n):
        m = rng.randint(1, min(40, L))
        p = rng.randrange(L - m + 1)
        pats.append(text[p:p + m])
    seps = [i for i in range(L) if text[i] == 10]
    for p in [seps[0], seps[-1]] + rng.sample(seps, min(20, len(seps))):      # across a separator
        for a, b in ((3, 4), (1, 2), (0, 1), (12, 12)):
            pats.append(text[max(0, p - a):p + b])
    empty = [i for i in range(1, L) if text[i] == 10 and text[i - 1] == 10] + ([0] if text[:1] == b"\n" else [])
    for p in empty[:12]:                                                       # across an empty record
        pats += [text[max(0, p - 3):p + 4], text[max(0, p - 1):p + 1], text[max(0, p - 2):p + 2], text[max(0, p - 10):p + 9]]
    alphabet = b"ACGTN" if is_dna(name) else bytes(range(1, 256))
    pats += [bytes([c]) for c in (b"ACGTNRY\n" if is_dna(name) else alphabet[::9])]
    pats += [b"C" * 3, b"N" * 2, b"N" * 30, b"NNN", b"CG", b"\n\n", b"\n\n\n", b"A\n", b"\nA"]
    for _ in range(30):
        pats.append(bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 8))))
    short = [s for s in g["seqs"] if 0 < len(s) <= 40][:15]
    for s in short:                                                            # whole short sequences
        s = s if isinstance(s, bytes) else s.encode()
        pats += [s, b"\n" + s + b"\n", s + b"\n"]
    pats += [text + b"A", text, text[:40], text[-40:]]
    return [p for p in pats if p]


def hash_name(name):
    import zlib
    return zlib.crc32(name.encode())


def extract_ranges(name, g, n=80):
    rng = random.Random(hash_name(name) + 1)
    L = len(g["text"])
    rs = []
    for _ in range(n):
        b = rng.randrange(L)
        rs.append((b, min(L, b + rng.randint(0, 60))))
    return rs + [(0, 0), (L, L), (0, min(L, 5000)), (max(0, L - 70), L)]


# ---------------------------------------------------------------------------------------------------------------------------------
# queries for hunt

# (key, hunt parameters, query lengths, share of the shape's query count)
MODES = [("d0", dict(distance=0), (18, 20), 0.4),
         ("edit1", dict(distance=1), (20, 14, 25), 1.0),
         ("ham1", dict(distance=1, hamming=True), (20, 15), 0.5),
         ("ham2", dict(distance=2, hamming=True), (20,), 0.15),
         ("fwd1", dict(distance=1, forward_only=True), (12, 25, 31), 0.3),
         ("maxloc3", dict(distance=1, max_locations=3), (10, 11, 12), 0.4),
         ("edit2", dict(distance=2), (12, 15), 0.06)]
# make_queries draws per mode: the checker's cost per query follows the number of occurrences, and the tandem shape has thousands
QUERY_COUNT = {"at_tandem": 30, "hard_masked": 50}
DEFAULT_QUERY_COUNT = 120


def _sampled(name, g, seed, n, lens):
    """make_queries where it can draw (it needs windows free of '\\n'), for the tiny texts random strings and cut-outs"""
    seqs = [s for s in g["seqs"] if len(s) >= 2 * max(lens)]
    if len(seqs) * 4 >= len(g["seqs"]) and len(g["text"]) > 500:
        return make_queries(seed, g["text"], n, lens)
    rng = random.Random(seed)
    out = []
    for _ in range(min(n, 12)):
        m = rng.choice(lens)
        s = rng.choice(g["seqs"])
        if len(s) >= m and rng.random() < 0.7:
            a = rng.randrange(len(s) - m + 1)
            out.append(s[a:a + m])
        else:
            out.append(_rnd(rng, m))
    return out


def _with(q, k, ins):
    """q with the letter(s) `ins` in place of position k (negative k counts from the end)"""
    k = k % len(q)
    return q[:k] + ins + q[k + len(ins):]


def edge_queries(name, g):
    """the per-shape edge cases: sequence ends (sequences 0, 511, 512, 513 and the last one), queries longer than the sequence they land
    in, whole short sequences and one letter more on either side, queries next to and across empty records, N's and letters the text
    lacks at and near both ends of a query"""
    rng = random.Random(hash_name(name) + 2)
    seqs = g["seqs"]
    qs = []
    for i in sorted({0, 511, 512, 513, len(seqs) - 1, len(seqs) - 2}):
        if 0 <= i < len(seqs) and seqs[i]:
            s = seqs[i]
            qs += [s[:20], s[-20:], s[1:21], s[-21:-1], s[:19] + "A", "T" + s[-19:]]
    # a 20-mer over a sequence of 12 nt, whole short sequences, one letter more on either side
    short = [i for i, s in enumerate(seqs) if 10 <= len(s) <= 19][:6]
    for i in short:
        s = seqs[i]
        before = seqs[i - 1][-4:] if i else "ACGT"
        after = seqs[i + 1][:4] if i + 1 < len(seqs) else "ACGT"
        qs += [s, "A" + s, s + "C", "G" + s + "T", before + s + after, s + _rnd(rng, 20 - len(s)), s[1:], s[:-1]]
    twelve = [i for i, s in enumerate(seqs) if len(s) == 12][:2]
    for i in twelve:
        qs += [seqs[i - 1][-4:] + seqs[i] + seqs[i + 1][:4], seqs[i - 1][-8:] + seqs[i], seqs[i] + seqs[i + 1][:8]]
    # next to and across empty records
    for i in [i for i, s in enumerate(seqs) if not s][:8]:
        prev = next((seqs[j] for j in range(i - 1, -1, -1) if seqs[j]), "")
        nxt = next((seqs[j] for j in range(i + 1, len(seqs)) if seqs[j]), "")
        qs += [prev[-20:], nxt[:20], prev[-10:] + nxt[:10], prev[-19:] + "A", "A" + nxt[:19]]
    # N runs of the text inside the query window at every offset class, and windows that end inside a run
    text = g["text"].decode()
    runs = []
    k = text.find("N")
    while k >= 0 and len(runs) < 400:
        e = k
        while e < len(text) and text[e] == "N":
            e += 1
        runs.append((k, e - k))
        k = text.find("N", e)
    for a, r in (runs[:3] + rng.sample(runs, min(5, len(runs))) + runs[-3:] if runs else []):
        if r <= 6:
            offs = [a - off for off in (0, 1, 2, 3, 9, 20 - r - 3, 20 - r - 2, 20 - r - 1, 20 - r, 19, 20)]
        else:     # a long run: windows that end 1-3 letters inside it, and windows that begin 1-3 letters before its end
            offs = [a - 20 + j for j in (0, 1, 2, 3)] + [a + r - j for j in (0, 1, 2, 3)]
        for b in offs:
            w = text[max(0, b):max(0, b) + 20]
            if "\n" not in w and len(w) == 20:
                qs.append(w)
    # one, two and three N's (and the letters the text lacks) put into text 20-mers at and near both ends
    base = [q for q in _sampled(name, g, hash_name(name) + 3, 40, (20,)) if len(q) == 20 and set(q) <= set("ACGT")][:3]
    letters = ["N", "NN", "NNN"] + (["C", "CC"] if name == "bisulfite" else []) + (["G", "C"] if name == "at_tandem" else [])
    for j, q in enumerate(base):
        for ins in letters:
            for k in (0, 1, 2, 9, -3 - len(ins) + 1, -2 - len(ins) + 1, -len(ins)):
                qs.append(_with(q, k, ins))
        qs.append(q[:7] + "N" + q[7:])          # inserted, not substituted: only a deletion brings it back
        qs.append("N" + q[:10] + "N" + q[10:] + "N")
        if name in ("bisulfite", "single_no_n", "at_tandem"):
            qs.append(q[:5] + "C" + q[5:])
            qs.append(q[:-1] + "C" + q[-1:])
    qs = [q for q in qs if q]
    seen, out = set(), []
    for q in qs:
        if q not in seen:
            seen.add(q)
            out.append(q)
    return out


def tail_queries(name, g, n, lens):
    """queries cut from the sequences with index >= 512 (for seq513: from its last sequence alone), a third of them with one substitution"""
    rng = random.Random(hash_name(name) + 4)
    src = [s for s in g["seqs"][512:] if len(s) >= max(lens)]
    out = []
    while src and len(out) < n:
        s = rng.choice(src)
        m = rng.choice(lens)
        a = rng.randrange(len(s) - m + 1)
        q = s[a:a + m]
        if rng.random() < 0.33:
            q = _with(q, rng.randrange(m), rng.choice("ACGT"))
        out.append(q)
    return out


def hunt_queries(name, g, mode):
    """the batch of one shape and mode: make_queries' recipe, the queries aimed at sequences above index 511, and the edge cases
    (cut to 12 / 15 nt for edit distance 2, where the checker enumerates the neighbourhood)"""
    key, kw, lens, share = next(m for m in MODES if m[0] == mode)
    n = max(24, int(QUERY_COUNT.get(name, DEFAULT_QUERY_COUNT) * share))
    seed = hash_name(name + mode) % 100000
    qs = _sampled(name, g, seed, n, lens)
    if len(g["seqs"]) > 512:
        qs += tail_queries(name, g, 90, lens)
    edges = edge_queries(name, g)
    if mode == "edit2":
        cut = []
        for i, q in enumerate(edges):
            m = (12, 15)[i % 2]
            if len(q) >= m:
                cut.append(q[:m] if i % 4 < 2 else q[-m:])
        step = -(-len(cut) // 40)
        edges = cut[::step]
        qs = [q[:15] for q in qs]
    elif mode in ("fwd1", "maxloc3"):
        edges = edges[::3]
    elif mode == "ham2":
        edges = edges[::2]
    return qs + edges
