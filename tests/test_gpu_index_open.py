"""The index open, stage by stage (dicey_amd/csrc/index.hip derive_layouts): three texts sized so that every branch of the open is
taken — about 40 k symbols (n <= 2^16: text and suffix array by the two walks, no prefix level), 3 x 60 000 (2^17 < n < 2^18: suffix
array by sorting, one prefix level, DG_OPEN_BIG_TABLE raises the table order from 9 to 10) and 3 x 100 000 (n > 2^18: two levels) —
each under every open flag and in two layouts, the default one and DICEY_KMER_K=12 with DICEY_KMER_K2=14.

Every handle must report exactly the resident bytes recorded in tests/golden/index_open_bytes.json (taken from the commit before the
open became stages: the refactor may not move a byte), the text's n, sigma and code lengths, answer count / locate / extract like a
scan of the text and a distance-1 hunt like the oracle, and report the same bytes when it is closed and opened again."""
import json
import os
import random

import pytest

try:
    import torch
    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import oracle_lib as O
from conftest import ROOT, genome_text, make_genome

pytestmark = pytest.mark.gpu

GENOMES = {"n40k": (211, 2, 20000), "n180k": (212, 3, 60000), "n300k": (213, 3, 100000)}  # make_genome(seed, sequences, length)
FLAGS = {"default": {}, "no_table": dict(kmer_table=False), "compact_no_pre5": dict(compact=True, pre5=False), "no_pre5": dict(pre5=False),
         "big_table": dict(big_table=True), "no_selfcheck": dict(selfcheck=False)}
LAYOUTS = {"auto": {}, "K12_K2_14": {"DICEY_KMER_K": "12", "DICEY_KMER_K2": "14"}}
GOLDEN = os.path.join(ROOT, "tests", "golden", "index_open_bytes.json")


def build_genome(name, directory):
    seed, nchr, length = GENOMES[name]
    seqs = make_genome(seed, nchr, length)
    text = genome_text(seqs)
    path = os.path.join(str(directory), name + ".fm9")
    O.build_fm9(text, path)
    return {"seqs": seqs, "text": text, "fm9": path, "seqlen": [len(s) + 1 for s in seqs], "names": ["chr%d" % (i + 1) for i in range(nchr)]}


def case_id(genome, flags, layout):
    return "%s/%s/%s" % (genome, flags, layout)


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    d = tmp_path_factory.mktemp("open")
    return {name: build_genome(name, d) for name in GENOMES}


@pytest.fixture(scope="module")
def scans(genomes):
    """per text, once for all its cases: the patterns and ranges of test_gpu_parity.test_count_locate_extract_match_bruteforce (fewer
    of them) with what a scan of the text finds"""
    out = {}
    for name, g in genomes.items():
        text, rng = g["text"], random.Random(17)
        pats = []
        for _ in range(500):
            if rng.random() < 0.7:
                p = rng.randrange(len(text) - 14)
                pats.append(text[p:p + rng.randint(1, 14)])
            else:
                pats.append("".join(rng.choice("ACGTNRY") for _ in range(rng.randint(1, 8))).encode())
        pats += [b"\n", b"N" * 30, b"A", text[:40], text[-40:]]
        rs = []
        for _ in range(200):
            b = rng.randrange(len(text))
            rs.append((b, min(len(text), b + rng.randint(0, 60))))
        rs += [(0, 0), (len(text), len(text)), (0, len(text))]
        full = text + b"\0"
        out[name] = (pats, [O.bf_locate(text, p) for p in pats], rs, [full[a:b + 1] for a, b in rs])
    return out


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["hbm_bytes"]


def test_the_texts_take_every_branch(genomes):
    n = {k: len(g["text"]) + 1 for k, g in genomes.items()}
    assert n["n40k"] <= 1 << 16 and (1 << 17) < n["n180k"] < (1 << 18) < n["n300k"]
    assert (1 << 18) < 2 * n["n180k"]  # 4^9 < 2 n: the larger table exists for this one


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("genome", list(GENOMES))
def test_open(genomes, scans, golden, monkeypatch, genome, flags, layout):
    import dicey_amd
    import test_gpu_parity as P
    g = genomes[genome]
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    want = golden[case_id(genome, flags, layout)]
    with dicey_amd.FmIndex(g["fm9"], device=0, **FLAGS[flags]) as ix:
        st = ix.stats()
        print("%s: hbm_bytes %d, recorded %d" % (case_id(genome, flags, layout), st["hbm_bytes"], want))
        assert st["hbm_bytes"] == want
        orc = O.Index(g["fm9"])
        assert st["n"] == len(g["text"]) + 1 and st["sigma"] == len(set(g["text"])) + 1
        assert all(st["code_len"].get(b, 0) == orc.code_len(b) for b in b"ACGTN\nRYKMSW")
        assert {b for b in st["code_len"] if b} == set(g["text"])
        pats, found, ranges, pieces = scans[genome]
        assert ix.count(pats) == [len(w) for w in found]
        assert ix.locate(pats) == found
        assert ix.extract(ranges) == pieces
        P.test_hunt_hits_equal_oracle_push_order(ix, g, dict(distance=1), 200, (20,))
    with dicey_amd.FmIndex(g["fm9"], device=0, **FLAGS[flags]) as ix:
        assert ix.stats()["hbm_bytes"] == want
