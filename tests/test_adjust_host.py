"""ftk_amd/csrc/adjust_steps.hpp WITHOUT a GPU, through tests/hostcheck/adjust_host.cpp: Philox4x32-10 against its known answers, the uniform's
ends, AS 241 against Python's statistics.NormalDist.inv_cdf (an independent implementation over libm's log) and the header's own log against
math.log, the clamp against the reference's (tests/golden/adjust/clamp.npz), the plan of a launch driven lane by lane (every element written
exactly once, nothing outside the array, the value the scalar function of (seed, t, e)), the noise's statistics, and the same file as a
program of its own under AddressSanitizer + UBSan."""
import math
import os
import statistics
import subprocess

import numpy as np
import pytest

import adjust_cases as AC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["ftkx_set_perturbation", "ftkx_set_clamp", "ftkx_adjust", "ftkx_adjust_f32", "ftkx_debug_adjust_relaunch", "ftkx_debug_adjust_counts", "ftkx_tracker_set_perturbation",
       "ftkx_tracker_set_clamp"]


def _runtime(name):
    p = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    return AC.host(tmp_path_factory.mktemp("hostcheck"))


def philox(hc, ctr, key):
    c, k, o = np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    hc.hc_philox(c.ctypes.data, k.ctypes.data, o.ctypes.data)
    return ["%08x" % v for v in o]


def test_philox_known_answers(hc):
    assert philox(hc, [0] * 4, [0] * 2) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8".split()
    assert philox(hc, [0xffffffff] * 4, [0xffffffff] * 2) == "408f276d 41c83b0e a20bc7c6 6d5451fd".split()
    assert philox(hc, [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == "d16cfe09 94fdcceb 5001e420 24126ea1".split()


def test_uniform_ends_are_inside_the_interval_and_exact(hc):
    lo, hi = hc.hc_uniform(0, 0), hc.hc_uniform(0xffffffff, 0xffffffff)
    assert lo == 2.0 ** -53 and hi == 1.0 - 2.0 ** -53
    # u - 0.5 is exact: (k + 0.5) * 2^-52 - 0.5 = (2k + 1 - 2^52) * 2^-53, an odd integer below 2^53 times a power of two
    rng = np.random.default_rng(3)
    for w_hi, w_lo in [(0, 0), (0xffffffff, 0xffffffff), (0x80000000, 0), (0x7fffffff, 0xffffffff)] + [tuple(int(v) for v in rng.integers(0, 2 ** 32, 2)) for _ in range(200)]:
        k = (w_hi << 20) | (w_lo >> 12)
        u = hc.hc_uniform(w_hi, w_lo)
        assert u == (2 * k + 1) / 2.0 ** 53 and 0.0 < u < 1.0                               # (2k + 1 < 2^53: the division is exact)
        assert u - 0.5 == (2 * k + 1 - 2 ** 52) / 2.0 ** 53


def quantile_inputs():
    """4096 values: both ends, 0.075 and 0.925 (|q| = 0.425, the border between the central and the tail branch) and exp(-25) (r = 5, the
    border between the two tail branches) with 8 neighbours on either side each, the rest uniform in (0, 1) and log-uniform towards both ends"""
    named = [2.0 ** -53, 1.0 - 2.0 ** -53]
    for c in (0.075, 0.925, math.exp(-25.0), 1.0 - math.exp(-25.0)):
        lo = hi = c
        named.append(c)
        for _ in range(8):
            lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, 1.0)
            named += [lo, hi]
    rng = np.random.default_rng(5)
    n = 4096 - len(named)
    small = np.exp(rng.uniform(math.log(2.0 ** -53), math.log(0.075), n // 4))
    u = np.concatenate([named, rng.uniform(0.0, 1.0, n - 2 * (n // 4)), small, 1.0 - small])
    u = np.clip(u, 2.0 ** -53, 1.0 - 2.0 ** -53)
    assert u.size == 4096
    return np.ascontiguousarray(u)


def test_quantile_against_an_independent_as241(hc):
    """the two differ by the rounding of log alone, which sqrt and well-conditioned polynomials hand on at a few 1e-16; a wrong coefficient shows
    orders above 1e-13"""
    u = quantile_inputs()
    z = np.empty_like(u)
    hc.hc_ppnd16(u.ctypes.data, z.ctypes.data, u.size)
    nd = statistics.NormalDist()
    ref = np.array([nd.inv_cdf(float(v)) for v in u])
    rel = np.abs(z - ref) / np.abs(ref)
    print("PPND16 against statistics.NormalDist.inv_cdf: largest relative difference %.3e at u = %r" % (rel.max(), float(u[rel.argmax()])))
    assert rel.max() <= 1e-13
    assert np.array_equal(np.sign(z), np.sign(u - 0.5))
    assert z[0] == -z[1] and 8.0 < z[1] < 8.3                                                  # the ends: +-8.21 sigma


def test_own_log_against_libm(hc):
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.uniform(0.0, 1.0, 2000), np.exp(rng.uniform(math.log(2.0 ** -53), 0.0, 1500)), np.exp(rng.uniform(-700.0, 700.0, 580)),
                        [2.0 ** -53, 0.5, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 2.0, math.sqrt(2.0), np.nextafter(math.sqrt(2.0), 0.0), math.sqrt(0.5), 0.075,
                         math.exp(-25.0), 2.2250738585072014e-308, 1.7976931348623157e308, 1.5, 0.75, 3.0, 10.0]])
    x = np.ascontiguousarray(x[x >= 2.2250738585072014e-308])
    assert x.size >= 4090
    y = np.empty_like(x)
    hc.hc_log(x.ctypes.data, y.ctypes.data, x.size)
    ref = np.array([math.log(float(v)) for v in x])
    rel = np.abs(y - ref) / np.abs(ref)
    print("adjust_log against math.log: largest relative difference %.3e at x = %r" % (rel.max(), float(x[rel.argmax()])))
    assert rel.max() <= 1e-13
    one = np.array([1.0]); out = np.array([7.0])
    hc.hc_log(one.ctypes.data, out.ctypes.data, 1)
    assert out[0] == 0.0


def test_clamp_is_the_references_bit_for_bit(hc):
    d = np.load(os.path.join(HERE, "golden", "adjust", "clamp.npz"))
    v, bounds, outputs = d["values"], d["bounds"].view(np.float64), d["outputs"]
    assert v.size == 64 and bounds.shape == (5, 2) and outputs.shape == (5, 64)
    x = v.view(np.float64)
    assert np.isnan(x).sum() >= 4 and np.signbit(x[np.isnan(x)]).any() and not np.signbit(x[np.isnan(x)]).all()
    for (lo, hi), exp in zip(bounds, outputs):
        out = np.zeros(v.size, dtype=np.uint64)
        hc.hc_clamp(v.ctypes.data, v.size, float(lo), float(hi), out.ctypes.data)
        assert np.array_equal(out, exp), (lo, hi)
        # ... and through the whole element function, for double and (where the value is a float) float sources
        assert np.array_equal(AC.host_adjust(x, clamp=(float(lo), float(hi))).view(np.uint64), exp), (lo, hi)
    # the corner cases by name
    assert AC.host_adjust(np.array([np.nan]), clamp=(-1.0, 1.0)).view(np.uint64)[0] == np.array([-1.0]).view(np.uint64)[0]
    assert AC.host_adjust(np.array([np.nan]), clamp=(1.0, -1.0)).view(np.uint64)[0] == np.array([-1.0]).view(np.uint64)[0]
    assert AC.host_adjust(np.array([-0.0]), clamp=(0.0, 0.0)).view(np.uint64)[0] == 0
    assert AC.host_adjust(np.array([-0.0]), clamp=(-0.0, 0.0)).view(np.uint64)[0] == 1 << 63
    assert np.all(AC.host_adjust(np.array([-3.0, 0.0, 3.0, np.inf]), clamp=(1.0, -1.0)) == -1.0)


@pytest.mark.parametrize("mode", sorted(AC.MODES))
@pytest.mark.parametrize("count", AC.COUNTS)
def test_every_element_once_and_nothing_else(hc, count, mode):
    perturb, clamp = AC.MODES[mode]
    big = count > 2000
    for src_off in range(4):
        for dst_off in range(2):
            if big and (src_off, dst_off) not in ((0, 0), (1, 1)):          # (the large counts: the aligned and one unaligned variant)
                continue
            seed = 100 * count + 10 * src_off + dst_off
            args = (int(perturb), AC.SIGMA, AC.SEED, AC.T, int(clamp), AC.LO, AC.HI)
            clamp_arg = (AC.LO, AC.HI) if clamp else None
            x = AC.values(count, seed, np.float64)
            xf = AC.values(count, seed, np.float32)
            out = np.full(max(1, count), 777.0)
            exp = AC.host_adjust(x, AC.SIGMA if perturb else 0.0, AC.SEED, AC.T, clamp_arg)
            assert hc.hc_plan_f64(x.ctypes.data, count, src_off & 1, dst_off, 0, *args, out.ctypes.data) == 0, (count, src_off, dst_off)
            assert AC.same_bits(out[:count], exp)
            out[:] = 777.0
            assert hc.hc_plan_f64(x.ctypes.data, count, 0, dst_off, 1, *args, out.ctypes.data) == 0, (count, "in place", dst_off)
            assert AC.same_bits(out[:count], exp)
            out[:] = 777.0
            assert hc.hc_plan_f32(xf.ctypes.data, count, src_off, dst_off, 0, *args, out.ctypes.data) == 0, (count, src_off, dst_off)
            assert AC.same_bits(out[:count], AC.host_adjust(xf, AC.SIGMA if perturb else 0.0, AC.SEED, AC.T, clamp_arg))


def test_noise_is_a_function_of_seed_snapshot_and_element_alone(hc):
    """an array taken apart anywhere -- odd starts included, where an element's Philox call is shared with one outside the piece -- gets the noise
    of the whole; perturbing is x + sigma * z with z the sigma = 1 noise of a zero array"""
    x = AC.values(1001, 9, np.float64)
    whole = AC.host_adjust(x, 0.5, 77, 3)
    for a, b in ((0, 1), (1, 2), (1, 500), (499, 1001), (1000, 1001)):
        assert AC.same_bits(AC.host_adjust(x[a:b], 0.5, 77, 3, e0=a), whole[a:b])
    z = AC.host_adjust(np.zeros(1001), 1.0, 77, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        exp = x + 0.5 * z
    ok = ~np.isnan(exp)
    assert np.array_equal(np.isnan(whole), np.isnan(exp)) and AC.same_bits(whole[ok], exp[ok])
    assert not np.array_equal(z, AC.host_adjust(np.zeros(1001), 1.0, 77, 4)) and not np.array_equal(z, AC.host_adjust(np.zeros(1001), 1.0, 78, 3))
    assert not np.array_equal(z, AC.host_adjust(np.zeros(1001), 1.0, 77 + (1 << 32), 3))            # the seed's high word is part of the key
    # element indices past 2^32 reach the counter's second word
    far = AC.host_adjust(np.zeros(4), 1.0, 77, 3, e0=1 << 33)
    assert not np.array_equal(far, z[:4]) and len(set(far.tolist())) == 4


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float(np.dot(a, b) / math.sqrt(np.dot(a, a) * np.dot(b, b)))


def test_noise_statistics(hc):
    """conditions a sample of independent N(0, 1) values of this size meets but for a chance of a few in 10^5 each; the sample is fixed by
    (seed, t), so the test cannot flicker"""
    n = 1 << 16
    z = AC.host_adjust(np.zeros(n), 1.0, 12345, 7)
    rn = math.sqrt(n)
    nd = statistics.NormalDist()
    s = np.sort(z)
    cdf = np.array([nd.cdf(float(v)) for v in s])
    i = np.arange(1, n + 1)
    D = max(float(np.max(i / n - cdf)), float(np.max(cdf - (i - 1) / n)))
    figures = {"mean": abs(z.mean()) * rn, "var": abs(z.var() - 1.0) * math.sqrt(n / 2.0), "ks": D * rn, "lag1": abs(_corr(z[:-1], z[1:])) * rn,
               "t7_t8": abs(_corr(z, AC.host_adjust(np.zeros(n), 1.0, 12345, 8))) * rn, "seeds": abs(_corr(z, AC.host_adjust(np.zeros(n), 1.0, 12346, 7))) * rn}
    print("noise statistics:", {k: round(v, 3) for k, v in figures.items()})
    assert figures["mean"] < 4 and figures["var"] < 4 and figures["ks"] < 1.95 and figures["lag1"] < 4 and figures["t7_t8"] < 4 and figures["seeds"] < 4, figures


def test_steps_are_clean_under_asan_ubsan(tmp_path):
    """(no skip where the runtimes are missing: the bounds of the arrays are then unchecked, which is a failure)"""
    assert _runtime("libasan.so") and _runtime("libubsan.so"), "g++ finds no libasan / libubsan: the sanitizer run of adjust_steps.hpp cannot be made"
    exe = str(tmp_path / "adjust_host_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DADJUST_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", exe, AC.SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "adjust_host run complete" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])


# ---- the entries, without a GPU --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ftk_amd import build, _lib
    build.build()
    return _lib.load()


def test_entries_are_declared_exported_and_bound(lib):
    from ftk_amd import _lib
    import ftk_amd
    hdr = open(os.path.join(ROOT, "include", "ftkx.h")).read() + open(os.path.join(ROOT, "include", "ftkx_tracker.hh")).read()
    for name in NEW:
        assert name + "(" in hdr and hasattr(lib, name) and name in _lib.EXPORTS, name
    for cls, names in ((ftk_amd.Context, ("set_perturbation", "set_clamp", "adjust", "adjust_counts", "debug_adjust_relaunch")),):
        for n in names:
            assert callable(getattr(cls, n)), n
    assert "adjust_kernels.hip" in [os.path.basename(s) for s in build_sources()]


def build_sources():
    from ftk_amd import build
    return build.SRC


def test_null_context_is_refused(lib):
    from ftk_amd import _lib
    E = _lib.E_INVALID
    assert lib.ftkx_set_perturbation(None, 1.0, 1) == E and lib.ftkx_set_clamp(None, 1, 0.0, 1.0) == E
    assert lib.ftkx_adjust(None, None, 8, 1.0, 1, 0, 0, 0.0, 0.0, None) == E and lib.ftkx_adjust_f32(None, None, 8, 1.0, 1, 0, 0, 0.0, 0.0, None) == E
    assert lib.ftkx_debug_adjust_counts(None, None, None, None) == E
    assert lib.ftkx_debug_adjust_relaunch(None, None, 0, 8, 1.0, 1, 0, 0, 0.0, 0.0, None, 1, None) == E
