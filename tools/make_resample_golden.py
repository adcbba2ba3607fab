"""Record tests/golden/sample_pdf.npz from the reference's own utils.sample_pdf (build container only: needs the reference tree).

    python tools/make_resample_golden.py <reference tree>

utils.py is loaded by file path with a stub `cv2` module (it imports cv2 at the top and sample_pdf does not use it); no bytecode
is written beside it.  For every case of tests/resample_oracle.cases() -- T in {2, 3, 64, 65, 66, 129, 200} with each kind of
weights (Laplace at beta = 0.02, uniform, all zero, 80 % exact zeros, 2^-20 .. 1), n and B cycling through {1, 63, 64, 65, 128}
and {1, 4, 5, 9} -- the inputs of resample_oracle.make_case are run through sample_pdf(bins, weights, n, det=False) with
torch.rand patched for the call so that the draws are the recorded u.  Recorded per case, numeric arrays only:

    <case>_bins [B,T] fp32, <case>_weights [B,T-1] fp32, <case>_u [B,n] fp32   the inputs
    <case>_s32  [B,n] fp32      the reference's result on them
    <case>_s64  [B,n] float64   the same function on the same inputs converted to float64
and det_n<n> [n] fp32: the u grid of det=True (recovered by running det=True on bins = cdf = [0, 1]: the sample is u itself).
Finally tests/resample_oracle.py is checked against all of it.
"""
import importlib.util
import os
import sys
import types
from unittest import mock

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import resample_oracle as ro  # noqa: E402


def load_utils(ref):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("reference_utils", os.path.join(ref, "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(mod, bins, weights, u, dtype):
    b, w, uu = (torch.from_numpy(np.ascontiguousarray(a)).to(dtype) for a in (bins, weights, u))
    with mock.patch.object(torch, "rand", lambda *a, **k: uu.clone()):
        return mod.sample_pdf(b, w, u.shape[-1], det=False).numpy()


def main(ref):
    mod = load_utils(ref)
    out = {}
    for ci, (name, T, n, B, kind) in enumerate(ro.cases()):
        bins, w, u = ro.make_case(T, n, B, kind, seed=1000 + ci)
        s32, s64 = run(mod, bins, w, u, torch.float32), run(mod, bins, w, u, torch.float64)
        assert s32.dtype == np.float32 and s64.dtype == np.float64 and s32.shape == (B, n)
        out.update({f"{name}_bins": bins, f"{name}_weights": w, f"{name}_u": u, f"{name}_s32": s32, f"{name}_s64": s64})
        o64 = ro.sample_pdf_np(bins, w, u, np.float64)
        o32 = ro.sample_pdf_np(bins, w, u, np.float32)
        e_ref, e_o32 = ro.score_dense(s32, s64, u, bins, w), ro.score_dense(o32, s64, u, bins, w)
        print(f"{name:16s} B {B} n {n:3d}: |oracle64 - ref64| {np.abs(o64 - s64).max():.2e}; worst e of the reference's fp32 "
              f"{e_ref / ro.U:.2f} U, of the fp32 oracle {e_o32 / ro.U:.2f} U")
    for n in ro.N_SET:
        # bins = [0, 1], one weight: cdf = [0, 1] exactly, denom = 1, so the sample IS u: the det grid with the reference's bits
        grid = mod.sample_pdf(torch.tensor([[0.0, 1.0]]), torch.ones(1, 1), n, det=True).numpy()[0]
        assert grid.dtype == np.float32 and np.array_equal(grid, torch.linspace(0. + 0.5 / n, 1. - 0.5 / n, steps=n).numpy())
        out[f"det_n{n}"] = grid
    path = os.path.join(ROOT, "tests", "golden", "sample_pdf.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
