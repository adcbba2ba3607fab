"""Is the b3 mode's worst sample of d(loss)/d(encoder.embeddings) in the `full` real-view step of tests/golden/round7.npz (3.2 x the
reference's own fp32 error on the fixture's 64 strided samples; f32 mode 0.55 x) ARITHMETIC (every row a little off) or a DISCRETE event
(a finite-difference tap point whose canonical position moved by an ulp sits in another grid cell at some level: a few rows far off,
the rest at round-off)?  The step of tests/test_gpu_render.py:real_view_f64_errors in the b3 and in the f32 mode, both cases; the
full table gradients compared row by row, and the strided samples placed among them."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from morpheus_amd import harness
import tests.test_gpu_render as T
from tests.util import load_golden

g = load_golden("round7.npz")
built = []
_build = harness.build_model


def capture(*a, **kw):
    m = _build(*a, **kw)
    built.append(m)
    return m


harness.build_model = capture
for case in ("plain", "full"):
    grads = {}
    for mode in ("b3", "f32", "b3"):
        T.real_view_f64_errors(case, None if mode == "b3" else mode)
        grads.setdefault(mode, []).append({k: p.grad.detach().double().cpu().reshape(-1) for k, p in built[-1].named_parameters()
                                           if p.grad is not None and "embeddings" in k})
    for k in ("encoder.embeddings", "encoder_c.embeddings"):
        a, b, a2 = grads["b3"][0][k], grads["f32"][0][k], grads["b3"][1][k]
        scale = float(b.abs().max())
        touched = (a != 0) | (b != 0)
        d = (a - b).abs() / scale
        dt = d[touched]
        idx = torch.linspace(0, a.numel() - 1, 64).long()
        s64 = torch.from_numpy(g[f"{case}|f64|grad|{k}|samples"]).double()
        sc64 = float(s64.abs().max())
        e_b3, e_f32 = (a[idx] - s64).abs() / sc64, (b[idx] - s64).abs() / sc64
        w = int(torch.argmax(e_b3))
        print(f"{case} {k}: b3 run twice equal {torch.equal(a, a2)}; {int(touched.sum())} touched rows x channels; b3 vs f32 |diff| / max: "
              f"median {float(dt.median()):.1e}, > 1e-4: {int((dt > 1e-4).sum())}, > 1e-3: {int((dt > 1e-3).sum())}, max {float(dt.max()):.1e}")
        print(f"    strided samples vs f64: b3 worst {float(e_b3[w]):.2e} at sample {w} (element {int(idx[w])}), there f32 "
              f"{float(e_f32[w]):.2e} and b3 - f32 {float(d[idx[w]]):.2e}; b3 2nd {float(e_b3.sort(descending=True).values[1]):.2e}, f32 worst "
              f"{float(e_f32.max()):.2e}; rank of that element's b3 - f32 difference among the touched entries: "
              f"{int((dt > float(d[idx[w]])).sum())}")
