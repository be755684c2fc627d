"""Expected values for the thal corpus: the reference's own thal() (oracle/_ref/libthalref.so, the unmodified thal.h built by
oracle/Makefile) and the host build of the product's sequential formulation (tests/host/libthalhost.so).  A value is the triple
(big-endian hex of the temperature, align_end_1, align_end_2): comparisons are bit for bit.  Where the reference refuses a pair
the ends are not compared (it leaves them unset); they are reported as None."""
import ctypes as C
import os
import struct
import subprocess

import oracle_lib as O
import thal_corpus as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = O.REF_THAL
HOST_DIR = os.path.join(ROOT, "tests", "host")
HOST_SO = os.path.join(HOST_DIR, "libthalhost.so")


def have_ref():
    return os.path.exists(REF_SO)


def hexd(t):
    return struct.pack(">d", t).hex()


_ref = {}


def ref_values(pairs, env):
    """[(hex, end1 or None, end2 or None, ok)] from the reference.  The reference keeps its settings in globals, so they are set
    on every call."""
    if "lib" not in _ref:
        R = C.CDLL(REF_SO)
        R.ref_thal_init.argtypes = [C.c_char_p] + [C.c_double] * 5
        R.ref_thal.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _ref["lib"] = R
    R = _ref["lib"]
    assert R.ref_thal_init(O.PRIMER3_CONFIG.encode(), 37.0, env["mv"], env["dv"], env["dna_conc"], env["dntp"]) == 0
    t, a, b = C.c_double(), C.c_int(), C.c_int()
    out = []
    # the reference announces every refusal on stderr; keep the test log readable
    saved = os.dup(2)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 2)
    try:
        for o1, o2 in pairs:
            ok = R.ref_thal(o1.encode("latin-1"), o2.encode("latin-1"), C.byref(t), C.byref(a), C.byref(b))
            out.append((hexd(t.value), a.value if ok else None, b.value if ok else None, bool(ok)))
    finally:
        os.dup2(saved, 2)
        os.close(saved)
        os.close(null)
    return out


_host = {}


def host_lib():
    if "lib" not in _host:
        srcs = [os.path.join(HOST_DIR, "thal_host.cpp"), os.path.join(ROOT, "dicey_amd", "csrc", "thal.hpp"),
                os.path.join(ROOT, "dicey_amd", "csrc", "thal_tables.hpp")]
        if not os.path.exists(HOST_SO) or any(os.path.getmtime(s) > os.path.getmtime(HOST_SO) for s in srcs):
            subprocess.check_call(["make", "-C", HOST_DIR, "-s", "libthalhost.so"])
        H = C.CDLL(HOST_SO)
        H.thal_host_open.restype = C.c_void_p
        H.thal_host_open.argtypes = [C.c_char_p] + [C.c_double] * 4
        H.thal_host_close.argtypes = [C.c_void_p]
        H.thal_host_batch.restype = None
        H.thal_host_batch.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_double),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        _host["lib"] = H
    return _host["lib"]


def host_values(pairs, env, cutoff_wins=None):
    """[(hex, end1, end2)] from the host build of thal.hpp with the product's loader and environment arithmetic.
    cutoff_wins: a list that receives, per pair, how many entropy cut-off candidates won."""
    H = host_lib()
    h = H.thal_host_open(O.PRIMER3_CONFIG.encode(), env["mv"], env["dv"], env["dntp"], env["dna_conc"])
    assert h, "thal_host_open failed"
    try:
        n = len(pairs)
        off = (C.c_uint64 * (2 * n + 1))()
        parts = []
        pos = 0
        for k, (a, b) in enumerate(pairs):
            ea, eb = a.encode("latin-1"), b.encode("latin-1")
            parts += [ea, eb]
            off[2 * k] = pos
            off[2 * k + 1] = pos + len(ea)
            pos += len(ea) + len(eb)
        off[2 * n] = pos
        t = (C.c_double * max(1, n))()
        e1 = (C.c_int32 * max(1, n))()
        e2 = (C.c_int32 * max(1, n))()
        cw = (C.c_uint64 * max(1, n))()
        H.thal_host_batch(h, b"".join(parts), off, n, t, e1, e2, cw)
        if cutoff_wins is not None:
            cutoff_wins.extend(cw[i] for i in range(n))
        return [(hexd(t[i]), e1[i], e2[i]) for i in range(n)]
    finally:
        H.thal_host_close(h)


def mismatches(got, want):
    """indices where a computed (hex, end1, end2) differs from the reference's (hex, end1, end2, ok); ends only where ok"""
    assert len(got) == len(want)
    return [i for i, (g, w) in enumerate(zip(got, want)) if g[0] != w[0] or (w[3] and (g[1], g[2]) != (w[1], w[2]))]


_expected = {}


def expected(group, env_name="default"):
    """reference values of a corpus group (or of the environment pairs: group "env"), computed once per session"""
    key = (group, env_name)
    if key not in _expected:
        pairs = TC.env_pairs() if group == "env" else TC.groups()[group]
        _expected[key] = ref_values(pairs, TC.ENVS[env_name])
    return _expected[key]
