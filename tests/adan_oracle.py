"""Float64 yardstick and fp32 restatement of the Adan step (csrc/adan.hip, optim.FlatAdan) -- test infrastructure, plain numpy on
the CPU, in the form of tests/step_f64_oracle.py:adam: the rule written ONCE, dtype-generic, element by element with per-ELEMENT
segment values, every operator rounded on its own in the order of the reference's single-tensor path (models/optimizer.py:221-256).

    clip        c = min(max_grad_norm / (sqrt(sum g g over the elements that have a gradient) + eps), 1);  1 when max_grad_norm == 0;
                summed and formed in float64, rounded once to the step's precision
    per group   t = the group's step;  ss = lr / (1 - b1^t);  sd = lr b2 / (1 - b2^t);  bc3s = sqrt(1 - b3^t);
                decay = 1 - lr wd (no_prox) or 1 + lr wd -- formed in double; rounded to fp32 for the fp32 run, as mh_adan_step does
    first gradient of the parameter, or t == 1:   q = g (-c)
    g' = g c;  q = q + g';  m = m b1 + (1 - b1) g';  d = d b2 + (1 - b2) q;  q = q b2 + g';  n = n b3 + ((1 - b3) q) q
    den = sqrt(n) / bc3s + eps
    no_prox:    p = p decay;  p = p - (ss m) / den;  p = p - (sd d) / den
    otherwise:  p = p - (ss m) / den;  p = p - (sd d) / den;  p = p / decay
    q = -g'
    an element without a gradient keeps p, g, m, n, d, q

Run in float64 on the fp32 inputs this is the yardstick; run in fp32 it is the measure of what fp32 can keep where no recorded
result of the reference exists.  tests/test_adan_host.py pins both against tests/golden/adan.npz (tools/make_adan_golden.py: the
reference's own class in fp32 and, one step at a time from the same fp32 state, in float64).

Natural scales of one step (`scales`), all from the float64 state BEFORE it, g' = g c in float64, skipped elements 0 (exact):
    p    |p| + ss + sd            (the rounding of p itself dominates a move of ss + sd)
    g'   |g'|
    m    b1 |m| + (1 - b1) |g'|
    d    b2 |d| + (1 - b2) D,     D = |q| + |g'|, the two terms of the gradient difference; D = 0 on a first gradient, where the
                                  difference is g c - g c = 0 in every precision
    n    b3 n + (1 - b3) Q^2,     Q = b2 D + |g'|, the two terms of the q that is squared
    q    |g'|
"""
import math
import os

import numpy as np

from tests.f64_judge import U  # noqa: F401  (re-exported for the tests)

BETAS = (0.98, 0.92, 0.99)
MAX_SEGS = 160
SKIP, FIRST = 1, 2          # flag bits of a segment at the C ABI


def seg_params(lrs, steps, wd, no_prox, betas=BETAS, round32=True):
    """per segment (ss, sd, bc3s, decay) from its learning rate and its GROUP's step, in double; round32: rounded to fp32"""
    b1, b2, b3 = betas
    out = []
    for lr, t in zip(lrs, steps):
        t = max(int(t), 1)
        out.append((lr / (1.0 - b1 ** t), lr * b2 / (1.0 - b2 ** t), math.sqrt(1.0 - b3 ** t),
                    1.0 - lr * wd if no_prox else 1.0 + lr * wd))
    a = np.array(out, np.float64).reshape(-1, 4)
    if round32:
        a = a.astype(np.float32).astype(np.float64)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


def sum_squares(g, on):
    """sum of g g over the elements that have a gradient, in float64 whatever the step's precision (as csrc/adan.hip sums)"""
    g = np.asarray(g, np.float64)[np.asarray(on, bool)]
    return float(np.sum(g * g))


def clip_factor(g, on, max_grad_norm, eps, dtype):
    """c from the float64 sum, formed in float64 and rounded ONCE to `dtype` (csrc/adan.hip; the reference's fp32 class rounds the
    sum, the root and the quotient)"""
    if max_grad_norm == 0:
        return dtype(1.0)
    with np.errstate(all="ignore"):
        c = float(max_grad_norm) / (math.sqrt(sum_squares(g, on)) + float(eps))
    return dtype(1.0) if c > 1.0 else dtype(c)


def adan(p, g, m, n, d, q, ss, sd, bc3s, decay, on, first, c, dtype, betas=BETAS, eps=1e-8, no_prox=False):
    """one step element by element in `dtype`.  ss, sd, bc3s, decay: per-ELEMENT group values; on: the element has a gradient;
    first: its parameter's first gradient or group step 1; c: the clip factor.  -> p, g', m, n, d, q"""
    p, g, m, n, d, q, ss, sd, bc3s, decay = (np.asarray(a).astype(dtype) for a in (p, g, m, n, d, q, ss, sd, bc3s, decay))
    on, first = np.asarray(on, bool), np.asarray(first, bool)
    b1, b2, b3 = (dtype(b) for b in betas)
    omb1, omb2, omb3 = (dtype(1.0 - b) for b in betas)
    eps, c = dtype(eps), dtype(c)
    with np.errstate(all="ignore"):
        q0 = np.where(first, g * (-c), q)
        gp = g * c
        q1 = q0 + gp
        m2 = m * b1 + omb1 * gp
        d2 = d * b2 + omb2 * q1
        q2 = q1 * b2 + gp
        n2 = n * b3 + (omb3 * q2) * q2
        den = np.sqrt(n2) / bc3s + eps
        if no_prox:
            p2 = p * decay
            p2 = p2 - (ss * m2) / den
            p2 = p2 - (sd * d2) / den
        else:
            p2 = p - (ss * m2) / den
            p2 = p2 - (sd * d2) / den
            p2 = p2 / decay
        q3 = -gp
    out = tuple(np.where(on, new, old) for new, old in ((p2, p), (gp, g), (m2, m), (n2, n), (d2, d), (q3, q)))
    assert all(a.dtype == dtype for a in out)
    return out


def scales(p, g, m, n, d, q, ss, sd, on, first, c, betas=BETAS):
    """the natural scales of the module docstring -> (p, g', m, n, d, q), float64"""
    p, g, m, n, d, q, ss, sd = (np.asarray(a, np.float64) for a in (p, g, m, n, d, q, ss, sd))
    on, first = np.asarray(on, bool), np.asarray(first, bool)
    b1, b2, b3 = betas
    gp = np.abs(g * float(c))
    D = np.where(first, 0.0, np.abs(q) + gp)
    Q = b2 * D + gp
    z = lambda a: np.where(on, a, 0.0)
    return (z(np.abs(p) + ss + sd), z(gp), z(b1 * np.abs(m) + (1.0 - b1) * gp), z(b3 * n + (1.0 - b3) * Q * Q),
            z(b2 * np.abs(d) + (1.0 - b2) * D), z(gp))


def seg_of(ends, n):
    """the segment of every element: the first whose end lies beyond it"""
    return np.searchsorted(np.asarray(ends, np.int64), np.arange(n), side="right")


# ------------------------------------------------------------------------------------------- a small case for the oracle's own test
def state(n, seed=71):
    """p ~ 0.1 N(0, 1); per element a gradient scale 10^U(-6, 1), live m, d, q of that scale and n of its square; element i with
    i % 7 == 0: all four states zero"""
    rng = np.random.RandomState(seed + n)
    scale = 10.0 ** (rng.rand(n) * 7.0 - 6.0)
    f = lambda a: a.astype(np.float32)
    p, m, d, q = f(rng.randn(n) * 0.1), f(rng.randn(n) * 0.3 * scale), f(rng.randn(n) * 0.2 * scale), f(rng.randn(n) * scale)
    nn = f((rng.rand(n) + 0.5) * scale * scale)
    z = np.arange(n) % 7 == 0
    m[z], nn[z], d[z], q[z] = 0.0, 0.0, 0.0, 0.0
    return dict(p=p, m=m, n=nn, d=d, q=q, scale=scale, size=n)


def grad(st, it, mult=1.0):
    """the gradient of iteration `it`: the element's scale x a factor in +-[0.5, 2) x mult; exact zeros at i % 7 == 1"""
    n = st["size"]
    rng = np.random.RandomState(1201 + 37 * it + n)
    g = (st["scale"] * mult * (0.5 + 1.5 * rng.rand(n)) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    g[np.arange(n) % 7 == 1] = 0.0
    return g


# ------------------------------------------------------------------------------------------- tests/golden/adan.npz, step by step
KEYS = ("exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad")
NAMES = ("p", "g") + KEYS           # the order of adan()'s and scales()'s results
_GOLDEN = {}


def golden():
    """the arrays of tests/golden/adan.npz (tools/make_adan_golden.py describes them), loaded once"""
    if not _GOLDEN:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adan.npz")) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    return _GOLDEN


def golden_step(run, step, round32):
    """step `step` (0-based) of run `run`: the recorded arrays of that step plus, per element of the concatenated tensors, the
    group values of seg_params (rounded to fp32 or not), `on`, `first`, and the run's constants"""
    G = golden()
    out = {k: v[run, step] for k, v in G.items() if v.ndim >= 2 and v.shape[:2] == G["c32"].shape}
    el = np.repeat(np.arange(len(G["sizes"])), G["sizes"])
    grp = G["group_of"][el]
    no_prox, wd = bool(G["no_prox"][run]), float(G["weight_decay"][run])
    ss, sd, bc3s, decay = (a[grp] for a in seg_params(out["lrs"], out["steps_after"], wd, no_prox, tuple(G["betas"]), round32))
    out.update(ss=ss, sd=sd, bc3s=bc3s, decay=decay, on=out["has_grad"][el], first=(~out["seen_before"])[el] | (out["steps_after"][grp] == 1),
               no_prox=no_prox, weight_decay=wd, betas=tuple(float(b) for b in G["betas"]), eps=float(G["eps"]),
               max_grad_norm=float(G["max_grad_norm"]), element_tensor=el)
    return out


def golden_state_dict(run, step, when="before"):
    """the state_dict the reference's class had before (or after) that step, rebuilt from the recorded arrays in its format: state
    only for the parameters that have had a gradient, `step` in the groups once a step was made, every default key"""
    import torch
    G = golden()
    s = golden_step(run, step, False)
    seen, steps = s["seen_" + when], s["steps_" + when]
    ends = np.cumsum(G["sizes"])
    state = {}
    for i, (e, k) in enumerate(zip(ends, G["sizes"])):
        if seen[i]:
            src = "before_" if when == "before" else "after32_"
            state[i] = {key: torch.from_numpy(s[src + key][e - k:e].copy()) for key in KEYS}
    groups = []
    for gi, name in enumerate("ab"):
        lr = float(s["lrs"][gi])
        g = dict(name=name, lr=lr, betas=s["betas"], eps=s["eps"], weight_decay=s["weight_decay"], max_grad_norm=s["max_grad_norm"],
                 no_prox=s["no_prox"], foreach=False, params=[i for i, x in enumerate(G["group_of"]) if x == gi])
        if steps[gi] > 0:
            g["step"] = int(steps[gi])
        groups.append(g)
    return {"state": state, "param_groups": groups}
