"""Share of ALL-ZERO parked lines in the hidden rows of the MLPs, measured on the CPU (no GPU, no library).

A parked row of the MLP kernels is [feature][32 points] fp32: one 128-byte line per feature and tile, and the 32 points of a
tile are consecutive samples of one ray.  A ReLU unit that is off tends to stay off along a ray, so whole lines are zero -- the
b3 warp kernels record them in line words and the weight-gradient kernels do not fetch them (csrc/mlp_b3.hip:
b3_park_line_word, csrc/mlp.hip: wg_line_ptr).  This tool restates the nets in torch (fp32) at the
benchmark's geometry -- a synthetic frame's rays, uniform samples clipped to the box -- and reports, per hidden layer,

    zero      share of zero elements
    line32    share of tiles x features whose 32 values are all zero   (what the kernels skip)
    line16    the same for 16-point half lines

for the warp nets (deform / topo, H1..H5) and, report only, for the sdf / colour nets' hidden rows (their hash-feature inputs
are high-frequency; the field kernels do not skip).

    python tools/parked_line_zeros.py [--state b] [--frame 0] [--rays 2048] [--res 128] [--samples 128]

`ray_points` and `warp_hidden` are what tests/test_gpu_warp_zero_lines.py feeds the kernels with.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from morpheus_amd import synth  # noqa: E402
from oracle import field as of  # noqa: E402
from oracle import hashgrid_np  # noqa: E402

BOUND = 1.01


def ray_points(state, frame: int, n_rays: int, res: int = 128, samples: int = 128, first_ray=None):
    """-> x [n_rays * samples, 3] (ray-major, t-ordered sample mid-points), t (the frame's time), hit share.
    The rays are `n_rays` consecutive pixels of the frame's res x res image from `first_ray` on (default: centred rows)."""
    o, d, t, rid = synth.frame_rays(frame, res, res)
    o, d = of.pose_optimisation(state["pose_array.data"], o[0], d[0], rid[0])
    n_all = o.shape[0]
    if first_ray is None:
        first_ray = max(0, (n_all - n_rays) // 2 // res * res)
    idx = (first_ray + torch.arange(n_rays)) % n_all
    o, d = o[idx], d[idx]
    jit = synth.ray_jitter(n_all)[idx]
    ri, ts, te = of.uniform_samples(o, d, jit, samples, BOUND)
    x = o[ri] + d[ri] * (0.5 * (ts + te))[:, None]
    hit = float(((te - ts) > 0).float().mean())
    return x.contiguous(), float(t[0, 0, 0]), hit


def warp_params(state, prefix: str):
    """-> (weights W0 [128, 87] .. W5, biases b0 .. b5) with the weight norm applied"""
    W = [of.wn_weight(state[f"{prefix}.net.{l}.weight_g"], state[f"{prefix}.net.{l}.weight_v"]) for l in range(6)]
    b = [state[f"{prefix}.net.{l}.bias"] for l in range(6)]
    return W, b


def warp_hidden(x, W, b, bias0=None, code=None):
    """H1..H5 [M, 128] of one warp net.  bias0 [128]: the first layer's per-frame bias W0[:, 39:] code + b0 (then W[0] is used
    through its 39 encoding columns only), else `code` [48] is concatenated as the reference does."""
    enc = of.freq_encode(x, 6, None)
    if bias0 is None:
        h = torch.nn.functional.linear(torch.cat([enc, code[None].expand(x.shape[0], -1)], -1), W[0], b[0])
    else:
        h = torch.nn.functional.linear(enc, W[0][:, :39]) + bias0
    hs = [torch.relu(h)]
    for l in range(1, 5):
        hs.append(torch.relu(torch.nn.functional.linear(hs[-1], W[l], b[l])))
    return hs


def shares(h: torch.Tensor, tile: int = 32):
    """h [M, F] -> (zero elements, all-zero `tile`-point lines, all-zero half lines); a ragged last tile is dropped"""
    m = h.shape[0] // tile * tile
    z = (h[:m] == 0).view(-1, tile, h.shape[1])
    half = z.view(-1, 2, tile // 2, h.shape[1])
    return float(z.float().mean()), float(z.all(1).float().mean()), float(half.all(2).float().mean())


def field_hidden(state, x, topo):
    """hidden rows of sdf_net (S1, S2) and color_net (C1, C2) at the warped points"""
    offs = state["encoder.offsets"].numpy()
    L = len(offs) - 1
    res_tab = of.level_resolutions(L, 2.0 ** 0.2, 16)
    u = ((x + BOUND) / (2 * BOUND)).numpy().astype(np.float32)
    grid = lambda which: torch.from_numpy(hashgrid_np.forward(u, state[f"{which}.embeddings"].numpy(), offs, res_tab, L))
    feat = torch.cat([of.freq_encode(x, 6, None), grid("encoder"), topo], -1)
    lin = torch.nn.functional.linear
    s1 = torch.relu(lin(feat, state["sdf_net.net.0.weight"], state["sdf_net.net.0.bias"]))
    s2 = torch.relu(lin(s1, state["sdf_net.net.1.weight"], state["sdf_net.net.1.bias"]))
    geo = lin(s2, state["sdf_net.net.2.weight"], state["sdf_net.net.2.bias"])[:, 1:]
    Wc = [of.wn_weight(state[f"color_net.net.{l}.weight_g"], state[f"color_net.net.{l}.weight_v"]) for l in range(3)]
    c1 = torch.relu(lin(torch.cat([grid("encoder_c"), geo], -1), Wc[0], state["color_net.net.0.bias"]))
    c2 = torch.relu(lin(c1, Wc[1], state["color_net.net.1.bias"]))
    return {"sdf S1": s1, "sdf S2": s2, "colour C1": c1, "colour C2": c2}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--state", default="b", choices=["a", "b"])
    ap.add_argument("--frame", type=int, default=0)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--no-field", action="store_true", help="skip the sdf / colour nets (their hash grid is slow in numpy)")
    a = ap.parse_args()
    torch.manual_seed(0)
    state = synth.make_state(a.state)
    with torch.no_grad():
        x, t, hit = ray_points(state, a.frame, a.rays, a.res, a.samples)
        code = of.multicode_sample([state[f"deform_code.volumes.{k}"] for k in range(3)], torch.tensor([t]))[0]
        print(f"# state {a.state}, frame {a.frame} (t = {t:.4f}), {a.rays} of the {a.res}^2 rays, {a.samples} uniform samples clipped to "
              f"the box: {x.shape[0]} points, {100 * hit:.1f} % of them on rays that hit the box")
        print(f"# {'rows':<12} {'zero':>6} {'line32':>7} {'line16':>7}")
        outs = {}
        for prefix in ("deform_net", "topo_net"):
            W, b = warp_params(state, prefix)
            hs = warp_hidden(x, W, b, code=code)
            for l, h in enumerate(hs):
                z, l32, l16 = shares(h)
                print(f"  {prefix[:-4] + ' H' + str(l + 1):<12} {z:6.3f} {l32:7.3f} {l16:7.3f}")
            outs[prefix] = torch.nn.functional.linear(hs[-1], W[5], b[5])
        if not a.no_field:
            print("# field nets (report only: their kernels do not skip)")
            xc = (x + outs["deform_net"]).clamp(-BOUND, BOUND)
            for name, h in field_hidden(state, xc, outs["topo_net"]).items():
                z, l32, l16 = shares(h)
                print(f"  {name:<12} {z:6.3f} {l32:7.3f} {l16:7.3f}")


if __name__ == "__main__":
    main()
