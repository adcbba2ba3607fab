"""Record tests/golden/adan.npz from the reference's own Adan class (build container only: needs the reference tree).

    python tools/make_adan_golden.py <reference tree>

The class (models/optimizer.py) is loaded by file path and run with foreach=False, as morpheus.py:146-150 builds it.  Four runs of
six steps over two groups ("a": tensors of 3, 5 and 2 elements, "b": 7, 1 and 257) with different learning rates,
max_grad_norm = 5:
    run 0   no_prox False, weight_decay 2e-5, unit-scale gradients: clipping never bites (c == 1, asserted)
    run 1   no_prox True,  weight_decay 2e-2, gradients x 100: clipping bites at every step (asserted)
    run 2   no_prox False, weight_decay 2e-2, gradients x 100
    run 3   no_prox True,  weight_decay 2e-5, unit-scale gradients
Per element the gradient scale is 10^U(-4, 0).  Tensor 1 has a gradient on step 2 only, tensor 4 from step 4 on; group "b"'s
learning rate is halved by name after step 3.

For every step: the fp32 state before it (p and the four states; zeros where the class has no state yet, `seen_before` tells), the
gradients, the fp32 class's state after it (`after32_*`; `g` is the gradient as the class left it, scaled in place), and the result of
ONE float64 step of the class seeded from that same fp32 state (`after64_*`) -- errors do not compound across steps, a comparison
measures one step's arithmetic.  Also the clip factor of both (`c32`, `c64`; the float64 step runs with float64 as torch's
default dtype, so that the class forms its norm in float64 too), the group steps and learning rates, and which
parameters have state afterwards.  Numeric arrays only; tensors are concatenated in group order without pads.
Finally the float64 restatement tests/adan_oracle.py is checked against the float64 results: within 64 double round-offs of the
oracle's scales.
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import adan_oracle as A  # noqa: E402

SIZES = (3, 5, 2, 7, 1, 257)
GROUP_OF = (0, 0, 0, 1, 1, 1)
LRS = (5e-3, 1e-3)
RUNS = ((False, 2e-5, 1.0), (True, 2e-2, 100.0), (False, 2e-2, 100.0), (True, 2e-5, 1.0))      # no_prox, weight_decay, gradient x
STEPS = 6
EPS, MAX_GRAD_NORM = 1e-8, 5.0
KEYS = ("exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad")


def load_class(ref):
    spec = importlib.util.spec_from_file_location("reference_optimizer", os.path.join(ref, "models", "optimizer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Adan


def has_grad(i, step):          # step: 1-based
    return step == 2 if i == 1 else step >= 4 if i == 4 else True


def make(Adan, params, no_prox, wd):
    groups = [{"name": name, "params": [p for p, g in zip(params, GROUP_OF) if g == gi], "lr": LRS[gi]} for gi, name in enumerate("ab")]
    return Adan(groups, eps=EPS, weight_decay=wd, max_grad_norm=MAX_GRAD_NORM, no_prox=no_prox, foreach=False)


def stepped(opt):
    """opt.step() -> the clip factor it used (the one torch.clamp of the class)"""
    seen, clamp = [], torch.clamp

    def spy(*a, **k):
        out = clamp(*a, **k)
        seen.append(out.clone())
        return out
    torch.clamp = spy
    try:
        opt.step()
    finally:
        torch.clamp = clamp
    assert len(seen) == 1
    return float(seen[0])


def flat(opt, params, what):
    """p, the gradients or one state key of every tensor, concatenated (zeros where there is none)"""
    out = []
    for p in params:
        t = p.data if what == "p" else p.grad if what == "g" else opt.state[p].get(what) if p in opt.state else None
        out.append(np.zeros(p.numel(), p.detach().numpy().dtype) if t is None else t.detach().reshape(-1).numpy().copy())
    return np.concatenate(out)


def main(ref):
    Adan = load_class(ref)
    rec = {}
    put = lambda k, v: rec.setdefault(k, []).append(v)
    worst = 0.0
    for run, (no_prox, wd, mult) in enumerate(RUNS):
        rng = np.random.RandomState(4100 + run)
        p32 = [torch.nn.Parameter(torch.from_numpy((rng.randn(k) * 0.1).astype(np.float32))) for k in SIZES]
        o32 = make(Adan, p32, no_prox, wd)
        scale = [10.0 ** (rng.rand(k) * 4.0 - 4.0) * mult for k in SIZES]
        for step in range(1, STEPS + 1):
            if step == 4:
                for g in o32.param_groups:
                    if g["name"] == "b":
                        g["lr"] = g["lr"] * 0.5
            grads = [torch.from_numpy((s * rng.randn(k)).astype(np.float32)) if has_grad(i, step) else None
                     for i, (k, s) in enumerate(zip(SIZES, scale))]
            # the float64 twin: the fp32 state of this moment, one step
            p64 = [torch.nn.Parameter(p.detach().double().clone()) for p in p32]
            o64 = make(Adan, p64, no_prox, wd)
            o64.load_state_dict(copy.deepcopy(o32.state_dict()))
            for name, v in (("p", flat(o32, p32, "p")),) + tuple((k, flat(o32, p32, k)) for k in KEYS):
                put("before_" + name, v)
            put("seen_before", np.array(["neg_pre_grad" in o32.state.get(p, {}) for p in p32]))
            put("steps_before", np.array([g.get("step", 0) for g in o32.param_groups], np.int64))
            put("lrs", np.array([g["lr"] for g in o32.param_groups], np.float64))
            put("has_grad", np.array([g is not None for g in grads]))
            put("grads", np.concatenate([np.zeros(k, np.float32) if g is None else g.numpy() for k, g in zip(SIZES, grads)]))
            for params, opt, tag, dt in ((p32, o32, "32", torch.float32), (p64, o64, "64", torch.float64)):
                for p, g in zip(params, grads):
                    p.grad = None if g is None else g.clone().to(dt)
                # the class makes its norm accumulator and max_grad_norm with torch's DEFAULT dtype: float64 for the float64 step
                torch.set_default_dtype(dt)
                try:
                    put("c" + tag, stepped(opt))
                finally:
                    torch.set_default_dtype(torch.float32)
                for name in ("p", "g") + KEYS:
                    put(f"after{tag}_{name}", flat(opt, params, name))
            put("steps_after", np.array([g["step"] for g in o32.param_groups], np.int64))
            put("seen_after", np.array(["neg_pre_grad" in o32.state.get(p, {}) for p in p32]))
            assert [g["step"] for g in o64.param_groups] == [g["step"] for g in o32.param_groups]
            # the float64 restatement against the float64 class, from this step's record
            last = lambda k: rec[k][-1]
            el = np.repeat(np.arange(len(SIZES)), SIZES)
            grp = np.asarray(GROUP_OF)[el]
            ss, sd, bc3s, decay = (a[grp] for a in A.seg_params(last("lrs"), last("steps_after"), wd, no_prox, round32=False))
            on = last("has_grad")[el]
            first = (~last("seen_before"))[el] | (last("steps_after")[grp] == 1)
            c = A.clip_factor(last("grads"), on, MAX_GRAD_NORM, EPS, np.float64)
            assert abs(c - last("c64")) <= 8 * 2.0 ** -53 * c, (c, last("c64"))
            before = [last("before_" + k) for k in ("p",) + KEYS]
            got = A.adan(before[0], last("grads"), *before[1:], ss, sd, bc3s, decay, on, first, c, np.float64, eps=EPS, no_prox=no_prox)
            sc = A.scales(before[0], last("grads"), *before[1:], ss, sd, on, first, c)
            for name, x, s in zip(("p", "g") + KEYS, got, sc):
                r = last("after64_" + name)
                assert np.array_equal(x[s == 0], r[s == 0]), (run, step, name)
                if (s > 0).any():
                    worst = max(worst, float((np.abs(x - r)[s > 0] / s[s > 0]).max()) / 2.0 ** -53)
        c32 = rec["c32"][-STEPS:]
        assert all(c == 1.0 for c in c32) if mult == 1.0 else all(c < 1.0 for c in c32), (run, c32)
        print(f"run {run}: no_prox {no_prox}, wd {wd}, gradients x {mult:g}: c =", " ".join(f"{c:.4f}" for c in c32))
    print(f"float64 restatement vs the float64 class: worst {worst:.2f} double round-offs of the scale")
    assert worst <= 64.0
    shape = lambda a: a.reshape((len(RUNS), STEPS) + a.shape[1:])
    out = {k: shape(np.stack([np.asarray(x) for x in v])) for k, v in rec.items()}
    out.update(sizes=np.array(SIZES, np.int64), group_of=np.array(GROUP_OF, np.int64), betas=np.array(A.BETAS, np.float64),
               eps=np.float64(EPS), max_grad_norm=np.float64(MAX_GRAD_NORM), no_prox=np.array([r[0] for r in RUNS]),
               weight_decay=np.array([r[1] for r in RUNS], np.float64))
    path = os.path.join(ROOT, "tests", "golden", "adan.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
