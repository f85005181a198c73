"""The exact-FMA forms of the two 1-D Winograd F(4x4) transforms (tdnet_amd/csrc/td_wino.h td_wino4_bt_t / td_wino4_at_t) against the plain
expressions they replace, bit for bit.

`y + k * x` with contraction off rounds twice, fma(k, x, y) once -- but for k = +-2, +-4, +-8 the product is exact (no overflow below
8.5e37, and a subnormal times a power of two is exact too), so both round the same real number.  The reference below is a VERBATIM copy of
the expressions before the rewrite, compiled with -ffp-contract=off like the library; the new code is the header itself, compiled for the
host the way the emulator compiles it.  float, f32x2 and the four-channel form (reference: f32x4; header: f32x2p, two packed halves)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"          # the emulator's compiler (tests/emu/build_emu.py)

HARNESS = r"""
#include "td_wino.h"
// ---- verbatim: td_wino.h before the exact-FMA rewrite -------------------------------------------------------------------------
template <typename T>
static void ref_bt(const T (&d)[6], T (&t)[6]) {
    const T a = d[4] - 4.f * d[2], b = d[3] - 4.f * d[1], c = d[4] - d[2], e = 2.f * (d[3] - d[1]);
    t[0] = 4.f * d[0] - 5.f * d[2] + d[4];
    t[1] = a + b;
    t[2] = a - b;
    t[3] = c + e;
    t[4] = c - e;
    t[5] = 4.f * d[1] - 5.f * d[3] + d[5];
}
template <typename T>
static void ref_at(const T (&m)[6], T (&y)[4]) {
    const T p = m[1] + m[2], q = m[1] - m[2], r = m[3] + m[4], s = m[3] - m[4];
    y[0] = m[0] + p + r;
    y[1] = q + 2.f * s;
    y[2] = p + 4.f * r;
    y[3] = q + 8.f * s + m[5];
}
// -------------------------------------------------------------------------------------------------------------------------------
template <typename T> static T ldv(const float* p);
template <> float ldv<float>(const float* p) { return p[0]; }
template <> f32x2 ldv<f32x2>(const float* p) { return f32x2{p[0], p[1]}; }
template <> f32x4 ldv<f32x4>(const float* p) { return f32x4{p[0], p[1], p[2], p[3]}; }
template <> f32x2p ldv<f32x2p>(const float* p) { return td_w_split(f32x4{p[0], p[1], p[2], p[3]}); }
static void stv(float* p, float v) { p[0] = v; }
static void stv(float* p, f32x2 v) { p[0] = v[0]; p[1] = v[1]; }
static void stv(float* p, f32x4 v) { for (int i = 0; i < 4; ++i) p[i] = v[i]; }
static void stv(float* p, f32x2p v) { stv(p, td_w_join(v)); }

// in: [n][6][L]; bt: [n][6][L]; at: [n][4][L]
template <typename TN, typename TR, int L>
static void run(long n, const float* in, float* bt_new, float* bt_ref, float* at_new, float* at_ref) {
    for (long i = 0; i < n; ++i) {
        TN dn[6], tn[6], yn[4];
        TR dr[6], tr[6], yr[4];
        for (int k = 0; k < 6; ++k) { dn[k] = ldv<TN>(in + (i * 6 + k) * L); dr[k] = ldv<TR>(in + (i * 6 + k) * L); }
        td_wino4_bt_t(dn, tn); ref_bt(dr, tr);
        td_wino4_at_t(dn, yn); ref_at(dr, yr);
        for (int k = 0; k < 6; ++k) { stv(bt_new + (i * 6 + k) * L, tn[k]); stv(bt_ref + (i * 6 + k) * L, tr[k]); }
        for (int k = 0; k < 4; ++k) { stv(at_new + (i * 4 + k) * L, yn[k]); stv(at_ref + (i * 4 + k) * L, yr[k]); }
    }
}
extern "C" void wino_exact_run(int lanes, long n, const float* in, float* bt_new, float* bt_ref, float* at_new, float* at_ref) {
    if (lanes == 1) run<float, float, 1>(n, in, bt_new, bt_ref, at_new, at_ref);
    else if (lanes == 2) run<f32x2, f32x2, 2>(n, in, bt_new, bt_ref, at_new, at_ref);
    else run<f32x2p, f32x4, 4>(n, in, bt_new, bt_ref, at_new, at_ref);
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no host clang++ (the emulator's compiler)")
    d = tmp_path_factory.mktemp("wino_exact")
    src, out = str(d / "harness.cpp"), str(d / "libwino_exact.so")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.run([CXX, "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value", "-ffp-contract=off", "-Wno-psabi", "-Wno-unused-function",
                    "-include", os.path.join(ROOT, "tests", "emu", "td_device.h"), "-I", os.path.join(ROOT, "tdnet_amd", "csrc"), src, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.wino_exact_run.argtypes = [ctypes.c_int, ctypes.c_long] + [ctypes.c_void_p] * 5
    lib.wino_exact_run.restype = None
    return lib


def _inputs(kind, count, rng):
    if kind == "unit":
        return rng.uniform(-1, 1, count).astype(np.float32)
    if kind == "normal":
        return rng.standard_normal(count).astype(np.float32)
    if kind == "subnormal":                       # the subnormal range and its neighbourhood, both signs
        bits = rng.integers(0, 0x01800000, count, dtype=np.uint32) | (rng.integers(0, 2, count, dtype=np.uint32) << 31)
        return bits.view(np.float32)
    if kind == "large":                           # up to 1e37: 4 a + 5 b + c stays finite
        return (rng.uniform(-1, 1, count) * 10.0 ** rng.uniform(30, 37, count)).astype(np.float32)
    if kind == "bits":                            # arbitrary finite bit patterns below 1e37
        bits = rng.integers(0, 0x7C700000, count, dtype=np.uint32) | (rng.integers(0, 2, count, dtype=np.uint32) << 31)
        return bits.view(np.float32)
    if kind == "mixed":                           # neighbouring operands many binades apart: every rounding case of the sums
        return (rng.standard_normal(count) * 2.0 ** rng.integers(-40, 40, count)).astype(np.float32)
    if kind == "zeros":                           # signed zeros among small integers: exact cancellations, the sign of a zero result
        v = rng.integers(-2, 3, count).astype(np.float32)
        v[(v == 0) & (rng.integers(0, 2, count) == 1)] = -0.0
        return v
    raise ValueError(kind)


@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("kind", ["unit", "normal", "subnormal", "large", "bits", "mixed", "zeros"])
def test_exact_fma_forms_are_bit_identical(harness, lanes, kind):
    rng = np.random.default_rng(1000 * lanes + len(kind))
    n = 200000
    x = np.ascontiguousarray(_inputs(kind, n * 6 * lanes, rng))
    assert np.isfinite(x).all() and np.abs(x).max() < 1e37
    if kind == "zeros":
        assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
    bt_new, bt_ref = np.empty(n * 6 * lanes, np.float32), np.empty(n * 6 * lanes, np.float32)
    at_new, at_ref = np.empty(n * 4 * lanes, np.float32), np.empty(n * 4 * lanes, np.float32)
    harness.wino_exact_run(lanes, n, x.ctypes.data, bt_new.ctypes.data, bt_ref.ctypes.data, at_new.ctypes.data, at_ref.ctypes.data)
    for name, a, b in (("B^T", bt_new, bt_ref), ("A^T", at_new, at_ref)):
        bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
        print("%s, %d lanes, %s: %d values, %d mismatches" % (name, lanes, kind, a.size, bad.size))
        assert bad.size == 0, (name, bad[:5], a[bad[:5]], b[bad[:5]])
