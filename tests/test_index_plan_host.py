"""What an index open decides before it allocates (dicey_amd/csrc/index_plan.hpp), on the host: the header's own functions behind
tests/host/libindexplanhost.so, held against a model of the rules as they stood inline in index.hip's derive_layouts before the open
became stages — the table order K and the long filter's order K2 from (n, free bytes, open flags, DICEY_KMER_K, DICEY_KMER_K2,
DICEY_NO_KMER_FILTER), whether the suffix array with context fits, whether one more prefix level fits, the level sizes below n.

Seeded random fact sets, every threshold at the byte and one byte to either side (the comparisons are strict), hipMemGetInfo
failed, every forced order, and the layouts a GRCh38-size genome gets on a 288 GB device, by value."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
W = C.c_ulonglong
GIB = 1 << 30
ROOM = 4 * GIB


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host")])
    L = C.CDLL(os.path.join(HERE, "host", "libindexplanhost.so"))
    L.ip_table_orders.argtypes = [W, C.c_int, W, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.ip_table_orders.restype = None
    L.ip_sax_fits.argtypes = [W, C.c_int, W]
    L.ip_plv_level_fits.argtypes = [W, W, C.c_int, W]
    L.ip_plv_sizes.argtypes = [W, C.POINTER(W), C.c_int]
    L.ip_bytes.argtypes = [C.c_int, W]
    L.ip_bytes.restype = W
    return L


def orders(L, n, free_b, have=True, flags=0, env_k=None, env_k2=None, no_filter=False):
    """env_k / env_k2: None = the variable is not set, else what atoi makes of it"""
    K, K2 = C.c_uint(), C.c_uint()
    L.ip_table_orders(n, int(have), free_b, flags, env_k or 0, int(env_k2 is not None), env_k2 or 0, int(no_filter), C.byref(K), C.byref(K2))
    return K.value, K2.value


# ------------------------------------------------------------------------------------------------------------------- the model

def base_k(n):
    K = 8
    while K < 16 and (1 << (2 * K)) < n:
        K += 1
    return K


def model_orders(n, free_b, have=True, flags=0, env_k=None, env_k2=None, no_filter=False, big_flag=8):
    K = base_k(n)
    K2 = 0
    slack = min(48 << 30, n * 16 + (64 << 20))
    f2_b = 4 * ((1 << (2 * (K + 2))) >> 3)
    need = (8 << (2 * K)) + slack
    if have and free_b > need + f2_b:
        K2 = K + 2
        need += f2_b
    if (flags & big_flag) and have and (1 << (2 * K)) < n * 2 and free_b > need - (8 << (2 * K)) + (8 << (2 * (K + 1))):
        K += 1
    if env_k is not None and 8 <= env_k <= 17:
        K = env_k
        if K2 and K2 <= K:
            K2 = K + 1
    if env_k2 is not None:
        K2 = env_k2 if (env_k2 > K and env_k2 <= 20) else 0
    if no_filter or 2 * K2 < 17:
        K2 = 0
    return K, K2


def filter_threshold(n):
    """the long filter is planned when MORE than this is free"""
    K = base_k(n)
    return (8 << (2 * K)) + min(48 << 30, n * 16 + (64 << 20)) + 4 * ((1 << (2 * (K + 2))) >> 3)


def big_threshold(n, with_filter):
    """DG_OPEN_BIG_TABLE raises K when MORE than this is free (and 4^K < 2 n)"""
    K = base_k(n)
    rest = min(48 << 30, n * 16 + (64 << 20)) + (4 * ((1 << (2 * (K + 2))) >> 3) if with_filter else 0)
    return rest + (8 << (2 * (K + 1)))


def model_sax_fits(n, have, free_b):
    return have and free_b > n * 8 + n * 2 + ROOM


def model_level_fits(n, x, have, free_b):
    return not (not have or free_b < (n // 448 + 1) * 64 + x * 8 + ROOM)


def model_level_sizes(n):
    xs = []
    for lv in range(8):
        x = 1 << (16 + 2 * lv)
        if x >= n:
            break
        xs.append(x)
    return xs


def level_sizes(L, n):
    out = (W * 16)()
    k = L.ip_plv_sizes(n, out, 16)
    return list(out[:k])


SIZES = [lambda n: ((n >> 7) + 1) * 64, lambda n: n + 64, lambda n: n * 4 + 64, lambda K: 8 << (2 * K), lambda k: ((1 << (2 * k)) >> 3) + 64,
         lambda n: n * 2 + 64, lambda n: n * 8 + 64, lambda n: (n // 448 + 1) * 64, lambda x: x * 8 + 64]
NS = [1, 2, 127, 128, 447, 448, 449, 40003, 65535, 65536, 65537, 180004, 262143, 262144, 262145, 300004, 10 ** 6, 104 * 10 ** 6, 3_100_000_000, (1 << 32) - 1]


# ------------------------------------------------------------------------------------------------------------------- the tests

def test_flag_and_limits(lib):
    assert lib.ip_big_table_flag() == 8 and lib.ip_max_levels() == 8


def test_random_fact_sets_against_the_model(lib):
    rng = random.Random(20261)
    for _ in range(6000):
        n = rng.choice(NS) if rng.random() < 0.3 else int(2 ** rng.uniform(0, 32))
        n = max(1, min(n, (1 << 32) - 1))
        r = rng.random()
        if r < 0.4:
            free_b = int(2 ** rng.uniform(0, 39))
        elif r < 0.7:
            free_b = filter_threshold(n) + rng.randint(-2, 2)
        else:
            free_b = big_threshold(n, rng.random() < 0.7) + rng.randint(-2, 2)
        kw = dict(have=rng.random() < 0.9, flags=rng.randrange(32), env_k=rng.choice([None, None, 0, -3, 99] + list(range(7, 19))),
                  env_k2=rng.choice([None, None, 0, -1, 5] + list(range(8, 23))), no_filter=rng.random() < 0.1)
        assert orders(lib, n, free_b, **kw) == model_orders(n, free_b, **kw), (n, free_b, kw)
        x = 1 << (16 + 2 * rng.randrange(8))
        for fb in (free_b, n * 10 + ROOM + rng.randint(-2, 2), (n // 448 + 1) * 64 + x * 8 + ROOM + rng.randint(-2, 2)):
            assert bool(lib.ip_sax_fits(n, int(kw["have"]), fb)) == model_sax_fits(n, kw["have"], fb), (n, fb)
            assert bool(lib.ip_plv_level_fits(n, x, int(kw["have"]), fb)) == model_level_fits(n, x, kw["have"], fb), (n, x, fb)
        assert level_sizes(lib, n) == model_level_sizes(n)


@pytest.mark.parametrize("n", [40003, 180004, 300004, 104 * 10 ** 6, 3_100_000_000])
def test_every_threshold_is_strict(lib, n):
    K = base_k(n)
    # the long filter: more than table + slack + four copies
    t = filter_threshold(n)
    assert [orders(lib, n, t + d) for d in (-1, 0, 1)] == [(K, 0), (K, 0), (K, K + 2)]
    # DG_OPEN_BIG_TABLE: one order more for the table when 4^K < 2 n and more than slack + four copies + the larger table is free
    # (the long filter is planned first: the four copies of order K + 2 are as large as the table of order K, so a device
    # without room for them has none for the larger table either)
    grows = (1 << (2 * K)) < 2 * n
    assert [orders(lib, n, t + d, flags=8) for d in (-1, 0, 1)] == [(K, 0), (K, 0), (K, K + 2)]
    t = big_threshold(n, True)
    assert [orders(lib, n, t + d, flags=8) for d in (-1, 0, 1)] == [(K, K + 2), (K, K + 2), (K + 1 if grows else K, K + 2)]
    assert [orders(lib, n, t + d) for d in (-1, 0, 1)] == [(K, K + 2)] * 3
    # the suffix array with context: more than 8 n + 2 n + 4 GiB
    t = n * 10 + ROOM
    assert [lib.ip_sax_fits(n, 1, t + d) for d in (-1, 0, 1)] == [0, 0, 1]
    # a prefix level: not less than directory + records + 4 GiB
    for x in model_level_sizes(n):
        t = (n // 448 + 1) * 64 + x * 8 + ROOM
        assert [lib.ip_plv_level_fits(n, x, 1, t + d) for d in (-1, 0, 1)] == [0, 1, 1]


def test_without_the_free_byte_count_nothing_optional_is_planned(lib):
    for n in NS:
        assert orders(lib, n, 1 << 40, have=False) == (base_k(n), 0)
        assert orders(lib, n, 1 << 40, have=False, flags=8) == (base_k(n), 0)
        assert orders(lib, n, 1 << 40, have=False, env_k2=base_k(n) + 2) == (base_k(n), base_k(n) + 2)  # a forced filter needs no count
        assert not lib.ip_sax_fits(n, 0, 1 << 40) and not lib.ip_plv_level_fits(n, 1 << 16, 0, 1 << 40)


def test_forced_table_order(lib):
    n, free_b = 180004, 200 * GIB  # K / K2 = 9 / 11 on its own
    assert orders(lib, n, free_b) == (9, 11)
    for v in range(-1, 25):
        want_k = v if 8 <= v <= 17 else 9
        want_k2 = 11 if want_k < 11 else want_k + 1  # a long filter at or below the forced table order moves right above it
        assert orders(lib, n, free_b, env_k=v) == (want_k, want_k2), v
        assert orders(lib, n, 0, env_k=v) == (want_k, 0), v  # no room for the filter: none, whatever the table order
    assert orders(lib, n, free_b, flags=8) == (10, 11) and orders(lib, n, free_b, flags=8, env_k=12) == (12, 13)


def test_forced_long_filter_order(lib):
    n, free_b = 180004, 200 * GIB
    for K in (None, 9, 12):
        k = K or 9
        for v in range(-2, 24):
            want = v if k < v <= 20 else 0  # 0, at or below K, 21 and above: no long filter
            assert orders(lib, n, free_b, env_k=K, env_k2=v) == (k, want), (K, v)
            assert orders(lib, n, 0, env_k=K, env_k2=v) == (k, want), (K, v)
    assert orders(lib, n, free_b, env_k=12, env_k2=14) == (12, 14)
    assert orders(lib, n, free_b, env_k=8, env_k2=8) == (8, 0)  # 2 K2 < 17 would be no filter anyway


def test_no_filter_switch(lib):
    for n in NS:
        for kw in (dict(), dict(flags=8), dict(env_k=12, env_k2=14), dict(env_k2=20)):
            K, _ = model_orders(n, 250 * GIB, **kw)
            assert orders(lib, n, 250 * GIB, no_filter=True, **kw) == (K, 0)


def test_grch38_size_layouts_by_value(lib):
    """what every benchmark number rests on: 3.1 G symbols on a device with 270 GB free"""
    n = 3_100_000_000
    assert orders(lib, n, 270 * 10 ** 9) == (16, 18)
    assert orders(lib, n, 270 * 10 ** 9, flags=8) == (17, 18)
    assert orders(lib, n, 60 * 10 ** 9) == (16, 0)
    assert orders(lib, n, 60 * 10 ** 9, flags=8) == (16, 0)
    assert lib.ip_sax_fits(n, 1, 100 * 10 ** 9) == 1 and lib.ip_sax_fits(n, 1, 35 * 10 ** 9) == 0
    assert level_sizes(lib, n) == [1 << (16 + 2 * i) for i in range(8)]


def test_level_sizes(lib):
    for n in (1, 40003, 65535, 65536):
        assert level_sizes(lib, n) == []
    for n in (65537, 180004, 1 << 18):
        assert level_sizes(lib, n) == [1 << 16]
    assert level_sizes(lib, (1 << 18) + 1) == [1 << 16, 1 << 18] == level_sizes(lib, 300004)
    assert level_sizes(lib, (1 << 30) + 1) == [1 << (16 + 2 * i) for i in range(8)]
    for n in ((1 << 32) - 1, 1 << 40):  # never more than MAXPLV
        assert len(level_sizes(lib, n)) == 8 and level_sizes(lib, n)[-1] == 1 << 30


def test_layout_sizes(lib):
    for which, f in enumerate(SIZES):
        for v in (range(8, 21) if which in (3, 4) else NS):
            assert lib.ip_bytes(which, v) == f(v), (which, v)
