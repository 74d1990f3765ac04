"""What tests/test_batch_plan_host.py builds on: the host build of ftk_amd/csrc/batch_plan.hpp (tests/hostcheck/batch_plan.cpp, a g++ shared
object), the header's enums by name, slice facts and plans as Python values."""
import collections
import ctypes as C
import os
import struct
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "batch_plan.cpp")
U64 = C.c_ulonglong

Facts = collections.namedtuple("Facts", "has_M has_U sparse mask_factor mask_big u_rows max_known maxabs")
NO_MASKS = Facts(False, False, False, 0, False, 1, False, 0.0)
Job = collections.namedtuple("Job", "slice factor rule_on big")
Sub = collections.namedtuple("Sub", "job_off step_base jobs steps")
Run = collections.namedtuple("Run", "first nsteps cull fan form")
Plan = collections.namedtuple("Plan", "status refused subs tile_steps runs fields_off tile_base nfields bytes facts")
Request = collections.namedtuple("Request", "mode s0 s1 factor")      # mode by name; s1 = -1: ordinal sweep only

_lib = None


def host():
    """the shared object, built once per process; the enums' values are checked to be distinct and are turned into names"""
    global _lib
    if _lib is None:
        so = os.path.join(tempfile.mkdtemp(prefix="hostcheck_batch"), "libhostcheck_batch.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SRC])
        L = C.CDLL(so)
        P64 = C.POINTER(U64)
        L.hc_batch_names.argtypes = [C.POINTER(C.c_longlong)]; L.hc_batch_names.restype = None
        L.hc_overflow_free.argtypes = [C.c_int, C.c_double, U64]
        L.hc_big_threshold.argtypes = [C.c_int, U64]; L.hc_big_threshold.restype = C.c_double
        L.hc_pow2_factor.argtypes = [U64]
        L.hc_masks_valid.argtypes = [C.c_int, P64, U64, C.c_int, C.c_int]
        L.hc_job_big.argtypes = [C.c_int, P64, U64, C.POINTER(C.c_int)]; L.hc_job_big.restype = C.c_double
        L.hc_request_mode.argtypes = [C.c_int, U64, C.c_int, C.c_int, C.c_int]
        L.hc_sparse_slice_refuses.argtypes = [C.c_int]
        L.hc_tile_form.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int]
        L.hc_plan_batch.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int), P64, C.c_int, P64, C.c_int, C.c_int, P64, C.c_longlong]; L.hc_plan_batch.restype = C.c_longlong
        L.hc_key_bits.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_int]
        L.hc_overflow_verdict.argtypes = [P64, P64, C.c_int, U64, C.c_int, P64]
        L.hc_cull_verdict.argtypes = [U64, U64, U64, U64, C.c_int, P64]
        v = (C.c_longlong * 15)()
        L.hc_batch_names(v)
        v = list(v)
        L.mode = dict(zip(v[0:3], ("tile", "fast", "tile_cull")))
        L.status = dict(zip(v[3:6], ("ok", "sparse_cannot_serve", "too_many")))
        L.verdict = dict(zip(v[6:10], ("done", "replay_dense", "grow", "give_up")))
        assert len(L.mode) == 3 and len(L.status) == 3 and len(L.verdict) == 4
        L.mode_value = {name: value for value, name in L.mode.items()}
        L.sizeof_mask_job, L.sizeof_fields, L.step_bits, L.tag_reference, L.tag_work_index = v[10:15]
        _lib = L
    return _lib


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _double(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _words(f):
    return [int(f.has_M), int(f.has_U), int(f.sparse), f.mask_factor, int(f.mask_big), f.u_rows, int(f.max_known), _bits(f.maxabs)]


def _facts(w):
    return Facts(bool(w[0]), bool(w[1]), bool(w[2]), w[3], bool(w[4]), w[5], bool(w[6]), _double(w[7]))


def overflow_free(nd, maxabs, factor):
    return bool(host().hc_overflow_free(nd, maxabs, factor))


def big_threshold(nd, factor):
    return host().hc_big_threshold(nd, factor)


def pow2_factor(factor):
    return bool(host().hc_pow2_factor(factor))


def masks_valid(nd, facts, factor, two_level, u_rows):
    return bool(host().hc_masks_valid(nd, (U64 * 8)(*_words(facts)), factor, int(two_level), u_rows))


def job_big(nd, facts, factor):
    """-> (big, rule_on)"""
    on = C.c_int(0)
    big = host().hc_job_big(nd, (U64 * 8)(*_words(facts)), factor, C.byref(on))
    return big, bool(on.value)


def request_mode(exact_only, factor, nd, robust, dense_collects):
    L = host()
    return L.mode[L.hc_request_mode(int(exact_only), factor, nd, int(robust), dense_collects)]


def sparse_slice_refuses(mode):
    L = host()
    return bool(L.hc_sparse_slice_refuses(L.mode_value[mode]))


def tile_form(nd, robust, bound, fan):
    return host().hc_tile_form(nd, int(robust), float(bound), fan)


def plan_batch(nd, robust, two_level, u_rows, requests, slices, tile_walk=True, tile_fan=2):
    L = host()
    nreq, nsl = len(requests), len(slices)
    req = (C.c_int * (3 * nreq + 1))()
    fac = (U64 * (nreq + 1))()
    for i, r in enumerate(requests):
        req[3 * i], req[3 * i + 1], req[3 * i + 2], fac[i] = L.mode_value[r.mode], r.s0, r.s1, r.factor
    fw = (U64 * (8 * nsl + 1))()
    for i, f in enumerate(slices):
        fw[8 * i:8 * i + 8] = _words(f)
    cap = 64 + 16 * (nreq + nsl)
    out = (U64 * cap)()
    n = L.hc_plan_batch(nd, int(robust), int(two_level), u_rows, nreq, req, fac, nsl, fw, int(tile_walk), tile_fan, out, cap)
    assert n > 0, "the wrapper's buffer was too small, or plan_batch changed its input (0)"
    w = out[:n]
    signed = lambda x: x - (1 << 64) if x >> 63 else x
    status, refused, nsubs, nruns, ntile, fields_off, tile_base, nfields, nbytes = w[:9]
    at, subs = 9, []
    for _ in range(nsubs):
        job_off, step_base, njobs, nsteps = w[at:at + 4]
        at += 4
        jobs = [Job(w[at + 4 * k], w[at + 4 * k + 1], bool(w[at + 4 * k + 2]), _double(w[at + 4 * k + 3])) for k in range(njobs)]
        at += 4 * njobs
        subs.append(Sub(job_off, step_base, jobs, list(w[at:at + nsteps])))
        at += nsteps
    tile_steps = list(w[at:at + ntile])
    at += ntile
    runs = [Run(w[at + 5 * k], w[at + 5 * k + 1], w[at + 5 * k + 2], signed(w[at + 5 * k + 3]), signed(w[at + 5 * k + 4])) for k in range(nruns)]
    at += 5 * nruns
    facts = [_facts(w[at + 8 * k:at + 8 * k + 8]) for k in range(nsl)]
    assert at + 8 * nsl == n
    return Plan(L.status[status], signed(refused), subs, tile_steps, runs, fields_off, tile_base, nfields, nbytes, facts)


def key_bits(tag_mode, nd, core_sz, dom_sz, t_max):
    a, b = (C.c_longlong * 3)(*core_sz), (C.c_longlong * 3)(*dom_sz)
    return host().hc_key_bits(tag_mode, nd, a, b, t_max)


def overflow_verdict(n, cap, any_fast, fast_cells, attempt):
    """n, cap, and the wanted capacities returned: (hits, listed, refined, fragile)"""
    L = host()
    want = (U64 * 4)()
    what = L.hc_overflow_verdict((U64 * 4)(*n), (U64 * 4)(*cap), int(any_fast), fast_cells, attempt, want)
    return L.verdict[what], tuple(want)


def cull_verdict(listed, refined, list_cap, refine_cap, attempt):
    """-> verdict, (listed, refined) wanted"""
    L = host()
    want = (U64 * 2)()
    what = L.hc_cull_verdict(listed, refined, list_cap, refine_cap, attempt, want)
    return L.verdict[what], tuple(want)
