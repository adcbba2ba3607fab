"""Derive the real spherical harmonics of degree < 8 and their partial derivatives, as ONE straight-line program, and write it
as morpheus_amd/csrc/sh_table.inc (the text csrc/encoders.hip compiles).

    python tools/make_sh_table.py [--out morpheus_amd/csrc/sh_table.inc] [--verify]

Definition (include/morpheus_hip.h, mh_sh_encode_fwd): column c = l^2 + l + m, 0 <= l < 8, -l <= m <= l,
    m = 0:  K(l,0) P_l(z)
    m > 0:  (-1)^m sqrt(2) K(l,m) T(l,m)(z) Re (x + iy)^m
    m < 0:  (-1)^m sqrt(2) K(l,|m|) T(l,|m|)(z) Im (x + iy)^|m|
K(l,m) = sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!), T(l,m) = d^m P_l / dz^m, P_l the Legendre polynomial: polynomials in (x, y, z) that
are evaluated as they stand for any input.  Nothing here is read from another implementation's table: sympy differentiates P_l.

The program (program(), and the lists COMMON / FORWARD / BACKWARD it returns) is a list of (target, operation, operands):
    ("z2", "mul", ("z", "z"))      operations: set (one operand), neg, mul, add, sub; an operand is a name or a Python float
A float operand is the coefficient correctly rounded to float64; a walk in fp32 rounds it once more to fp32, which is the
literal the .inc holds.  Shared terms:
    z2 = z z;   c_m + i s_m = (x + iy)^m by c_m = c_(m-1) x - s_(m-1) y,  s_m = s_(m-1) x + c_(m-1) y   (c_1 = x, s_1 = y)
    q_l_m  = N(l,m) T(l,m)(z),  N the constant in front, by Horner's rule in z2 (times z where l - m is odd)
    qz_l_m = N(l,m) T(l,m+1)(z) the same way: d q_l_m / dz
    qm_l_m = q_l_m m
    Y(l,0) = q_l_0          Y(l,m) = q_l_m c_m             Y(l,-m) = q_l_m s_m
    dz:      qz_l_0                  qz_l_m c_m                      qz_l_m s_m
    dx:      0                       qm_l_m c_(m-1)                  qm_l_m s_(m-1)
    dy:      0                       -(qm_l_m s_(m-1))               qm_l_m c_(m-1)           (c_0 = 1, s_0 = 0: those products
                                                                                               are not formed, zero terms are absent)
Targets y<c> are the 64 columns, dx<c> / dy<c> / dz<c> the partial derivatives that are not identically zero.  verify() runs
the program over sympy expressions with exact coefficients and compares every target with the definition and its sympy
derivatives.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import sympy as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(ROOT, "morpheus_amd", "csrc", "sh_table.inc")
MAX_DEGREE = 8
_Z = sp.Symbol("z")


def constant(l: int, m: int):
    """N(l,m), exact"""
    k = sp.sqrt(sp.Rational(2 * l + 1, 4) / sp.pi * sp.Rational(sp.factorial(l - m), sp.factorial(l + m)))
    return k if m == 0 else (-1) ** m * sp.sqrt(2) * k


def t_poly(l: int, m: int):
    """T(l,m)(z) as a sympy polynomial in z"""
    return sp.Poly(sp.diff(sp.legendre(l, _Z), _Z, m), _Z)


def _real_parts(a: int):
    x, y = sp.symbols("x y", real=True)
    w = sp.expand((x + sp.I * y) ** a)
    return sp.re(w), sp.im(w)


def program(exact: bool = False):
    """-> (COMMON, FORWARD, BACKWARD): lists of (target, operation, operands); with `exact` the coefficients stay sympy numbers"""
    common, fwd, bwd = [], [], []
    num = (lambda v: v) if exact else (lambda v: float(sp.N(v, 40)))

    def horner(dst, name, l, m, order):
        """name = N(l,m) T(l,order)(z): Horner in z2 from the highest coefficient down, then z where the polynomial is odd"""
        coeffs = t_poly(l, order).all_coeffs()[::-1]          # ascending powers of z
        odd = (l - order) % 2
        a = [num(constant(l, m) * c) for c in coeffs[odd::2]]
        steps = [("set", (a[-1],))]
        for c in a[-2::-1]:
            steps += [("mul", (None, "z2")), ("add", (None, c))]
        if odd:
            steps.append(("mul", (None, "z")))
        if len(steps) >= 2 and steps[0][0] == "set" and steps[1][0] == "mul":      # (constant) times (name): one product
            steps = [("mul", (steps[1][1][1], steps[0][1][0]))] + steps[2:]
        for k, (op, args) in enumerate(steps):
            tgt = name if k == len(steps) - 1 else f"{name}_h{k}"
            prev = f"{name}_h{k - 1}"
            dst.append((tgt, op, tuple(prev if a_ is None else a_ for a_ in args)))

    common.append(("z2", "mul", ("z", "z")))
    c, s = {1: "x"}, {1: "y"}
    for m in range(2, MAX_DEGREE):
        common += [(f"c{m}_a", "mul", (c[m - 1], "x")), (f"c{m}_b", "mul", (s[m - 1], "y")), (f"c{m}", "sub", (f"c{m}_a", f"c{m}_b")),
                   (f"s{m}_a", "mul", (s[m - 1], "x")), (f"s{m}_b", "mul", (c[m - 1], "y")), (f"s{m}", "add", (f"s{m}_a", f"s{m}_b"))]
        c[m], s[m] = f"c{m}", f"s{m}"
    for l in range(MAX_DEGREE):
        for m in range(l + 1):
            horner(common, f"q_{l}_{m}", l, m, m)
    for l in range(MAX_DEGREE):
        base = l * l + l
        for m in range(-l, l + 1):
            a, q = abs(m), f"q_{l}_{abs(m)}"
            if m == 0:
                fwd.append((f"y{base}", "set", (q,)))
            else:
                fwd.append((f"y{base + m}", "mul", (q, c[a] if m > 0 else s[a])))
    for l in range(MAX_DEGREE):          # per l: the shared factors first, then the columns in ascending order (the kernel's sums
        base = l * l + l                 # take their terms in the order of these statements)
        for a in range(l + 1):
            if a < l:
                horner(bwd, f"qz_{l}_{a}", l, a, a + 1)
            if a >= 2:
                bwd.append((f"qm_{l}_{a}", "mul", (f"q_{l}_{a}", float(a) if not exact else sp.Integer(a))))
        for m in range(-l, l + 1):
            a, col = abs(m), base + m
            qz, qm = f"qz_{l}_{a}", (f"q_{l}_{a}" if a == 1 else f"qm_{l}_{a}")
            if a == 0:
                if l > 0:
                    bwd.append((f"dz{col}", "set", (qz,)))
                continue
            if a == 1:
                bwd.append((f"dx{col}" if m > 0 else f"dy{col}", "set", (qm,)))
            else:
                bwd.append((f"dx{col}", "mul", (qm, c[a - 1] if m > 0 else s[a - 1])))
                if m > 0:
                    bwd += [(f"dy{col}_n", "mul", (qm, s[a - 1])), (f"dy{col}", "neg", (f"dy{col}_n",))]
                else:
                    bwd.append((f"dy{col}", "mul", (qm, c[a - 1])))
            if a < l:
                bwd.append((f"dz{col}", "mul", (qz, c[a] if m > 0 else s[a])))
    return common, fwd, bwd


_OPS = {"set": lambda a: a, "neg": lambda a: -a, "mul": lambda a, b: a * b, "add": lambda a, b: a + b, "sub": lambda a, b: a - b}


def verify():
    """the program over sympy expressions with exact coefficients against the definition and its derivatives -> targets checked"""
    x, y, z = sp.symbols("x y z")
    common, fwd, bwd = program(exact=True)
    env = {"x": x, "y": y, "z": z}
    for tgt, op, args in common + fwd + bwd:
        env[tgt] = _OPS[op](*[env[a] if isinstance(a, str) else a for a in args])
    n = 0
    for l in range(MAX_DEGREE):
        for m in range(-l, l + 1):
            col = l * l + l + m
            a = abs(m)
            re_, im_ = _real_parts(a)
            xr, yr = sp.symbols("x y", real=True)
            part = sp.Integer(1) if m == 0 else (re_ if m > 0 else im_).subs({xr: x, yr: y})
            want = constant(l, a) * t_poly(l, a).as_expr().subs(_Z, z) * part
            assert sp.expand(env[f"y{col}"] - want) == 0, f"column {col}"
            n += 1
            for name, var in (("dx", x), ("dy", y), ("dz", z)):
                d = sp.expand(sp.diff(want, var))
                if f"{name}{col}" in env:
                    assert sp.expand(env[f"{name}{col}"] - d) == 0, f"{name} of column {col}"
                else:
                    assert d == 0, f"{name} of column {col} is absent but not zero"
                n += 1
    return n


def _lit(v) -> str:
    """operand as C text: a name, or the fp32 literal of a coefficient"""
    if isinstance(v, str):
        return v
    r = repr(float(np.float32(v)))          # the float64 spelling of the fp32 value parses back to that fp32 value
    assert np.float32(float(r)) == np.float32(v)
    return r + "f"


def _statement(tgt, op, args) -> str:
    a = [_lit(v) for v in args]
    rhs = {"set": "{0}", "neg": "-{0}", "mul": "{0} * {1}", "add": "{0} + {1}", "sub": "{0} - {1}"}[op].format(*a)
    for kind, macro in (("dx", "SH_DX"), ("dy", "SH_DY"), ("dz", "SH_DZ"), ("y", "SH_Y")):
        if tgt.startswith(kind) and tgt[len(kind):].isdigit():
            return f"const float {tgt} = {rhs}; {macro}({tgt[len(kind):]}, {tgt});"
    return f"const float {tgt} = {rhs};"


def text() -> str:
    common, fwd, bwd = program()
    lines = ["// Generated by tools/make_sh_table.py -- do not edit; regenerate with `python tools/make_sh_table.py`.",
             "// The real spherical harmonics of degree < 8 (column c = l*l + l + m) and their partial derivatives as straight-line fp32",
             "// statements over shared terms, in ONE fixed order (the order tests/encoders_oracle.py walks in numpy).  The including",
             "// function provides `const float x, y, z` and the macros SH_Y(c, v), SH_DX(c, v), SH_DY(c, v), SH_DZ(c, v); it defines",
             "// SH_TABLE_FORWARD and / or SH_TABLE_BACKWARD.  Build with -ffp-contract=off: every operator is rounded on its own.",
             f"// {len(common)} shared statements, {len(fwd)} forward, {len(bwd)} backward."]
    lines += [_statement(*st) for st in common]
    lines.append("#ifdef SH_TABLE_FORWARD")
    lines += [_statement(*st) for st in fwd]
    lines.append("#endif")
    lines.append("#ifdef SH_TABLE_BACKWARD")
    lines += [_statement(*st) for st in bwd]
    lines.append("#endif")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--verify", action="store_true", help="check every target symbolically against the definition first")
    a = ap.parse_args()
    if a.verify:
        print(f"verified {verify()} polynomials against the definition")
    with open(a.out, "w") as fh:
        fh.write(text())
    print(a.out)


if __name__ == "__main__":
    main()
