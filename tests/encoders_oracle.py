"""Restatements of the frequency and spherical-harmonics encoders (csrc/encoders.hip), written from the definitions in
include/morpheus_hip.h -- numpy on the CPU, test infrastructure.

Frequency.  out = [x | sin(2^0 x) | cos(2^0 x) | sin(2^1 x) | ...], blocks of D columns, the bands f >= n_keep zero.  The argument
2^f x is exact in fp32 (a power-of-two scaling), so freq_ref(float64) -- numpy's sine and cosine of the float64 image of that fp32
argument -- is the true value of what the kernel is asked for, and freq_ref(float32) what a correctly working fp32 routine gives.
freq_ref_reference_formula is the reference's own wording (cosine as the sine of arg + fp32(pi/2), all in fp32): kept for the
record of what its argument rounding costs, not as a yardstick.

Frequency backward: grad_x[d] = grad[d] + sum_{f < n_keep} 2^f (g_sin cos - g_cos sin).  freq_bwd_count(n_keep) bounds the kernel's
error in units of 2^-24 times the sum of the ABSOLUTE terms |grad[d]| + sum 2^f (|g_sin cos| + |g_cos sin|)  (f64_judge.judge_sum):
    n_keep additions into the running sum and n_keep differences: each rounds a partial sum that the absolute sum bounds   2 n_keep
    the first term grad[d] is taken as it is; one more for the final value against the float64 sum rounded to fp32         1
    one rounded product per term                                                                                             1
    sine / cosine from sincosf: taken as within 2 ulp, a relative error of 4 x 2^-24 on its term (twice the 1 ulp that the
    forward test's gate -- 4 x 2^-24 absolute on values up to 1 -- allows at the top binade)                                 4
The scaling by 2^f is exact.  -> 2 n_keep + 6.

Spherical harmonics.  sh_def64 evaluates the definition directly in float64: Legendre derivatives (numpy.polynomial.legendre)
times the real or imaginary part of (x + iy)^|m| by complex powers; it does not touch the generated table.  sh_walk / sh_grad_walk
run the generated straight-line program (tools/make_sh_table.py: COMMON + FORWARD / BACKWARD lists of (target, operation,
operands)) in its own order in the requested dtype; in float32 every operator rounds on its own, which is what the kernel --
compiled from the same statements without contraction -- must reproduce bit for bit.

Roundings on the longest chain of the generated program (sh_chain_count): the depth of a target is 1 + the largest depth of its
operands for mul / add / sub, the same depth for set / neg (exact); x, y, z have depth 0 and a coefficient depth 1 (it is rounded
to fp32 once).  Derived over the program, not assumed:
    shared terms   c_m, s_m: 2 (m - 1)                       (two products and a sum per step of the recurrence; c_7: 12)
                   q_l_m: Horner in z2 (depth 1): one product and one sum per further coefficient, one product for an odd power
    forward        y = q c_m or q s_m: 1 + max(depth q, depth c_m)   -> 13 at degree 8 (column 49 / 63: q_7_7 is a constant, c_7 12)
    backward       dx / dy = (q m) c_(m-1): 1 + max(1 + depth q, depth c_(m-1));  dz = qz c_m
sh_chain_count(degree, kind) returns the figure for the columns below degree^2; the tests use it as the floor of the judgement
against sh_def64, in units of 2^-24 of the absolute-term value (sh_abs_walk: the same program over |x|, |y|, |z| with every
coefficient's magnitude and every difference taken as a sum -- the size the first-order rounding analysis is relative to).
The backward sums of the kernel add degree^2 rounded products in ascending column order from +0: sh_bwd_contract restates that order;
its judge_sum count is degree^2 additions + 1 product + the chain count of the derivative.
"""
from __future__ import annotations

import functools
import importlib.util
import math
import os

import numpy as np
from numpy.polynomial import legendre as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SINCOS_ULP = 2          # see the module docstring


@functools.lru_cache(maxsize=None)
def table_module():
    spec = importlib.util.spec_from_file_location("make_sh_table", os.path.join(ROOT, "tools", "make_sh_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def program():
    """-> (COMMON, FORWARD, BACKWARD) of tools/make_sh_table.py"""
    return table_module().program()


# ------------------------------------------------------------------------------------------------ frequency
def freq_width(D, degree):
    return D + 2 * D * degree


def freq_ref(x, degree, n_keep, dtype):
    """x [B,D] fp32 -> [B, D + 2 D degree] in `dtype` (np.float32 / np.float64): sine and cosine of the exactly scaled argument"""
    x = np.asarray(x, dtype=np.float32)
    B, D = x.shape
    out = np.zeros((B, freq_width(D, degree)), dtype=dtype)
    out[:, :D] = x
    for f in range(n_keep):
        arg = np.ldexp(x, f).astype(dtype)          # exact in fp32, then (exactly) widened
        assert np.array_equal(arg.astype(np.float64), x.astype(np.float64) * 2.0 ** f)
        out[:, D + 2 * f * D: D + (2 * f + 1) * D] = np.sin(arg)
        out[:, D + (2 * f + 1) * D: D + (2 * f + 2) * D] = np.cos(arg)
    return out


def freq_ref_reference_formula(x, degree):
    """the reference's fp32 wording (freqencoder.cu:52-56): the cosine is sin(arg + fp32(pi/2)), the sum rounded to fp32"""
    x = np.asarray(x, dtype=np.float32)
    B, D = x.shape
    out = np.zeros((B, freq_width(D, degree)), dtype=np.float32)
    out[:, :D] = x
    half_pi = np.float32(np.float32(3.141592653589793) / np.float32(2))
    for f in range(degree):
        arg = np.ldexp(x, f)
        out[:, D + 2 * f * D: D + (2 * f + 1) * D] = np.sin(arg)
        out[:, D + (2 * f + 1) * D: D + (2 * f + 2) * D] = np.sin((arg + half_pi).astype(np.float32))
    return out


def freq_bwd_ref(x, grad, degree, n_keep):
    """-> (grad_x in float64, the float64 sum of the absolute terms), both [B,D]"""
    x64, g = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(grad, dtype=np.float32).astype(np.float64)
    B, D = x64.shape
    out, ab = g[:, :D].copy(), np.abs(g[:, :D])
    for f in range(n_keep):
        arg = x64 * 2.0 ** f
        gs, gc = g[:, D + 2 * f * D: D + (2 * f + 1) * D], g[:, D + (2 * f + 1) * D: D + (2 * f + 2) * D]
        out += 2.0 ** f * (gs * np.cos(arg) - gc * np.sin(arg))
        ab += 2.0 ** f * (np.abs(gs * np.cos(arg)) + np.abs(gc * np.sin(arg)))
    return out, ab


def freq_bwd_count(n_keep):
    return 2 * n_keep + 1 + 1 + 2 * SINCOS_ULP


# ------------------------------------------------------------------------------------------------ spherical harmonics
def sh_def64(x, degree):
    """the definition in float64 at the fp32 points x [B,3] -> [B, degree^2]"""
    return sh_def64_at(np.asarray(x, dtype=np.float32).astype(np.float64), degree)


def sh_def64_at(p, degree):
    """the definition at float64 points (the central differences of the host test step off the fp32 lattice)"""
    xs, ys, zs = p[:, 0], p[:, 1], p[:, 2]
    w = xs + 1j * ys
    out = np.zeros((p.shape[0], degree * degree))
    for l in range(degree):
        for m in range(-l, l + 1):
            a = abs(m)
            k = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - a) / math.factorial(l + a))
            t = L.Legendre.basis(l).deriv(a)(zs) if a else L.Legendre.basis(l)(zs)
            if m == 0:
                v = k * t
            else:
                wm = w ** a
                v = (-1) ** a * math.sqrt(2.0) * k * t * (wm.real if m > 0 else wm.imag)
            out[:, l * l + l + m] = v
    return out


_OPS = {"set": lambda a: a, "neg": lambda a: -a, "mul": lambda a, b: a * b, "add": lambda a, b: a + b, "sub": lambda a, b: a - b}


def _walk(x, steps, dtype, absolute=False):
    p = np.asarray(x, dtype=np.float32).astype(dtype)
    if absolute:
        p = np.abs(p)
    env = {"x": p[:, 0].copy(), "y": p[:, 1].copy(), "z": p[:, 2].copy()}
    ops = dict(_OPS, sub=_OPS["add"], neg=_OPS["set"]) if absolute else _OPS
    for tgt, op, args in steps:
        vals = [env[a] if isinstance(a, str) else dtype(np.float32(abs(a) if absolute else a)) if dtype is np.float32
                else dtype(abs(a) if absolute else a) for a in args]
        r = ops[op](*vals)
        env[tgt] = np.broadcast_to(np.asarray(r, dtype=dtype), p.shape[:1]).astype(dtype)
    return env


def _columns(env, prefix, degree, n, dtype):
    out = np.zeros((n, degree * degree), dtype=dtype)
    for c in range(degree * degree):
        if f"{prefix}{c}" in env:
            out[:, c] = env[f"{prefix}{c}"]
    return out


def sh_walk(x, degree, dtype=np.float32, absolute=False):
    """the generated program in its own order -> [B, degree^2] in `dtype`"""
    common, fwd, _ = program()
    return _columns(_walk(x, common + fwd, dtype, absolute), "y", degree, len(x), dtype)


def sh_grad_walk(x, degree, dtype=np.float32, absolute=False):
    """-> (dY/dx, dY/dy, dY/dz), each [B, degree^2] in `dtype`; the columns whose derivative is identically zero hold 0"""
    common, _, bwd = program()
    env = _walk(x, common + bwd, dtype, absolute)
    return tuple(_columns(env, k, degree, len(x), dtype) for k in ("dx", "dy", "dz"))


def sh_abs_walk(x, degree):
    return sh_walk(x, degree, np.float64, absolute=True)


def sh_present(degree):
    """-> three boolean [degree^2] masks: the columns that have a dx / dy / dz term in the program"""
    names = {t for t, _, _ in program()[2]}
    return tuple(np.array([f"{k}{c}" in names for c in range(degree * degree)]) for k in ("dx", "dy", "dz"))


def sh_bwd_contract(x, grad, degree):
    """the kernel's sums in fp32, in its order: from +0, columns ascending, product rounded, then added; absent terms skipped"""
    g = np.asarray(grad, dtype=np.float32)
    out = np.zeros((len(g), 3), dtype=np.float32)
    for a, (d, present) in enumerate(zip(sh_grad_walk(x, degree, np.float32), sh_present(degree))):
        acc = np.zeros(len(g), dtype=np.float32)
        for c in np.nonzero(present)[0]:
            acc = (acc + (g[:, c] * d[:, c]).astype(np.float32)).astype(np.float32)
        out[:, a] = acc
    return out


def sh_bwd_ref64(x, grad, degree):
    """-> (grad_x [B,3] in float64 by the float64 walk, the float64 sum of the absolute terms |grad| x absolute-term derivative)"""
    g = np.asarray(grad, dtype=np.float32).astype(np.float64)
    d = sh_grad_walk(x, degree, np.float64)
    da = sh_grad_walk(x, degree, np.float64, absolute=True)
    return np.stack([(g * k).sum(1) for k in d], 1), np.stack([(np.abs(g) * k).sum(1) for k in da], 1)


@functools.lru_cache(maxsize=None)
def sh_chain_count(degree, kind="y"):
    """roundings on the longest chain that ends in a `kind` ('y', or 'd' for dx / dy / dz) target of a column below degree^2"""
    common, fwd, bwd = program()
    depth = {"x": 0, "y": 0, "z": 0}
    for tgt, op, args in common + fwd + bwd:
        d = max(depth[a] if isinstance(a, str) else 1 for a in args)
        depth[tgt] = d + (0 if op in ("set", "neg") else 1)
    prefixes = ("y",) if kind == "y" else ("dx", "dy", "dz")
    return max([depth[f"{p}{c}"] for p in prefixes for c in range(degree * degree) if f"{p}{c}" in depth] + [1])


def sh_bwd_count(degree):
    return degree * degree + 1 + sh_chain_count(degree, "d")


def sh_points(seed=0):
    """512 unit vectors, 512 points of [-1, 1]^3 and the 26 axis / diagonal directions, fp32 [1050, 3]"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((512, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    box = rng.uniform(-1.0, 1.0, (512, 3))
    dirs = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], dtype=np.float64)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return np.concatenate([u, box, dirs]).astype(np.float32)
