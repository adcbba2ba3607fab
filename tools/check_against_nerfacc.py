"""One command from "unpinned" to "pinned": this build's occupancy marcher and compositor against nerfacc itself.

nerfacc is third-party, un-vendored and version un-pinned in the reference (docs/INSTALL.md:21) and is NOT in this image, so
`morpheus_amd.occgrid.OccupancyGrid` (interval placement, packed layout, the 'estimator' checkpoint buffers) and
`mh_composite_fwd` (nerfacc.render_weight_from_density + accumulate_along_rays) follow nerfacc's published 0.5.x behaviour as
recalled (occgrid.py:1-15, csrc/composite.hip:1-6) -- the parity tests compare them with this build's own oracle.  On a box WITH
nerfacc and an MI355X, this script feeds both the closed-form rays of `morpheus_amd.synth` through the reference's own call
sites and prints the differences:

    python tools/check_against_nerfacc.py            # exit code 0: intervals identical / within 1e-6, weights within 1e-5

  1. sampling -- morpheus.py:629-638: `OccGridEstimator(roi_aabb, resolution=128).sampling(rays_o, rays_d, sigma_fn=None,
     render_step_size=step, alpha_thre=0, stratified=False, cone_angle=0.0, early_stop_eps=0)` on a closed-form binary grid (a
     sphere of radius 0.6 and an off-centre box) against `OccupancyGrid.sampling` with the jitter pinned at 0: per-ray sample
     counts, ray indices, t_starts / t_ends.  (stratified=True draws nerfacc's own random offsets; pinning them needs the same
     generator, so the comparison is made un-jittered; the jitter is one per-ray shift of the same lattice in both.)
  2. compositing -- morpheus.py:675-685: `render_weight_from_density(t_starts, t_ends, sigmas, ray_indices=, n_rays=)` and
     `accumulate_along_rays(weights, values, ray_indices, n_rays)` against `ops.composite` on the SAME packed samples (nerfacc's)
     with a closed-form density and colour: weights, opacity, depth, colour.
  3. the estimator's state_dict keys / shapes / dtypes against `OccupancyGrid.state_dict()` (checkpoint entry 'estimator',
     morpheus.py:341,355).

  4. visibility pruning -- `sampling(sigma_fn=..., alpha_thre=..., early_stop_eps=...)` with one closed-form density through
     both: the difference of the kept sets (csrc/visibility.hip restates nerfacc's rule from recall).

  5. the volume-rendering functions under their own names -- `morpheus_amd.volrend` against nerfacc function by function on
     nerfacc's samples: pack_info, render_transmittance / render_weight _from_density / _from_alpha, accumulate_along_rays
     (values None, 1, 3 and 48 channels), render_visibility_from_density, rendering(), and the gradients to sigmas, alphas and
     values of one mixed loss.  At alpha == 1 nerfacc's alpha gradient is expected to be inf / NaN and this build's finite
     (volrend.py): that row is printed and not counted.

It cannot run in the build container (no nerfacc, no GPU); tests/test_host.py only checks that it imports and fails with its own
message there.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def closed_form_binary(R: int, bound: float):
    """occupied cells: a sphere of radius 0.6 around the origin or a box [0.3, 0.8] x [-0.2, 0.4] x [-0.9, -0.5] (cell centres)"""
    import torch
    c = (torch.arange(R, dtype=torch.float32) + 0.5) / R * (2 * bound) - bound
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    sphere = (x * x + y * y + z * z) < 0.36
    box = (x > 0.3) & (x < 0.8) & (y > -0.2) & (y < 0.4) & (z > -0.9) & (z < -0.5)
    return sphere | box


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=64, help="the view is res x res rays of synth frame 25")
    ap.add_argument("--step", type=float, default=0.01)
    args = ap.parse_args(argv)
    try:
        import nerfacc
    except ImportError:
        print("check_against_nerfacc: nerfacc is not installed here -- run this on a box with the reference's environment "
              "(docs/INSTALL.md:21) and an MI355X", file=sys.stderr)
        return 2
    import torch
    from morpheus_amd import ops, synth
    from morpheus_amd.occgrid import OccupancyGrid
    if not torch.cuda.is_available():
        print("check_against_nerfacc: needs the GPU (the HIP path has no CPU fallback)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    bound, R = 1.01, 128
    aabb = [-bound] * 3 + [bound] * 3
    o, d, _, _ = synth.frame_rays(25, args.res, args.res)
    o, d = o[0].to(dev), d[0].to(dev)
    N = o.shape[0]
    binary = closed_form_binary(R, bound).to(dev)
    ok = True

    # ---- 1. sampling (morpheus.py:196-202, 629-638)
    est = nerfacc.OccGridEstimator(roi_aabb=aabb, resolution=R).to(dev)
    est.binaries.copy_(binary.view_as(est.binaries))
    est.occs.copy_(binary.reshape(-1).float())
    ri_n, ts_n, te_n = est.sampling(o, d, sigma_fn=None, render_step_size=args.step, alpha_thre=0, stratified=False, cone_angle=0.0,
                                    early_stop_eps=0)
    grid = OccupancyGrid(aabb, R).to(dev)
    grid.set_binary(binary)
    grid.fixed_jitter = 0.0
    ri_h, ts_h, te_h = grid.sampling(o, d, sigma_fn=None, render_step_size=args.step, alpha_thre=0, stratified=False, cone_angle=0.0,
                                     early_stop_eps=0)
    cnt_n = torch.bincount(ri_n.long(), minlength=N)
    cnt_h = torch.bincount(ri_h.long(), minlength=N)
    print(f"sampling: {N} rays, nerfacc {ri_n.numel()} samples, this build {ri_h.numel()}; rays whose count differs: "
          f"{int((cnt_n != cnt_h).sum())} (max |difference| {int((cnt_n - cnt_h).abs().max())})")
    if ri_n.numel() == ri_h.numel() and torch.equal(ri_n.long(), ri_h.long()):
        e0, e1 = float((ts_n - ts_h).abs().max()), float((te_n - te_h).abs().max())
        print(f"          same packed layout; max |t_starts difference| {e0:.3e}, max |t_ends difference| {e1:.3e}")
        ok &= e0 <= 1e-6 and e1 <= 1e-6
    else:
        # different counts: say WHERE the lattices differ -- first interval of the first differing ray
        bad = int(torch.nonzero(cnt_n != cnt_h)[0]) if bool((cnt_n != cnt_h).any()) else 0
        sn, sh = ts_n[ri_n.long() == bad][:4].tolist(), ts_h[ri_h.long() == bad][:4].tolist()
        print(f"          ray {bad}: nerfacc t_starts {sn} ..., this build {sh} ...   (interval placement differs: occgrid.py:11-13)")
        ok = False

    # ---- 2. compositing on nerfacc's own samples (morpheus.py:675-685)
    tm = 0.5 * (ts_n + te_n)
    x = o[ri_n.long()] + d[ri_n.long()] * tm[:, None]
    sig = 40.0 * torch.exp(-8.0 * (x.norm(dim=-1) - 0.55).abs())             # a shell of density around the sphere's surface
    rgb = 0.5 + 0.5 * torch.sin(3.0 * x + torch.tensor([0.0, 1.0, 2.0], device=dev))
    w_n, _, _ = nerfacc.render_weight_from_density(ts_n, te_n, sig, ray_indices=ri_n, n_rays=N)
    op_n = nerfacc.accumulate_along_rays(w_n, values=None, ray_indices=ri_n, n_rays=N)
    dp_n = nerfacc.accumulate_along_rays(w_n, values=tm[:, None], ray_indices=ri_n, n_rays=N)
    cl_n = nerfacc.accumulate_along_rays(w_n, values=rgb, ray_indices=ri_n, n_rays=N)
    start, cnt = ops.packed_info(ri_n.long(), N)
    w_h, op_h, dp_h, cl_h = ops.composite(sig.contiguous(), ts_n.contiguous(), te_n.contiguous(), rgb.contiguous(), start, cnt)
    for name, a, b in (("weights", w_h, w_n), ("opacity", op_h, op_n.reshape(-1)), ("depth", dp_h, dp_n.reshape(-1)), ("colour", cl_h, cl_n)):
        err = float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
        print(f"compositing: {name:8s} max |difference| / max |nerfacc| = {err:.3e}")
        ok &= err <= 1e-5

    # ---- 3. the checkpoint entry 'estimator' (morpheus.py:341,355)
    sd_n, sd_h = est.state_dict(), grid.state_dict()
    for k in sorted(set(sd_n) | set(sd_h)):
        a, b = sd_n.get(k), sd_h.get(k)
        same = a is not None and b is not None and tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype
        print(f"state_dict: {k:12s} nerfacc {None if a is None else (tuple(a.shape), a.dtype)}  this build "
              f"{None if b is None else (tuple(b.shape), b.dtype)}  {'ok' if same else 'DIFFERS'}")
        ok &= same

    # ---- 4. visibility pruning: the same closed-form density through both `sampling(sigma_fn=...)` (include/morpheus_hip.h,
    # "visibility pruning": T >= early_stop_eps and alpha >= min(alpha_thre, mean(occs)), recalled -- this case pins it)
    def sigma_fn(t_starts, t_ends, ray_indices):
        xm = o[ray_indices.long()] + d[ray_indices.long()] * (0.5 * (t_starts + t_ends))[:, None]
        return 40.0 * torch.exp(-8.0 * (xm.norm(dim=-1) - 0.55).abs())

    grid.occs.copy_(binary.reshape(-1).float())
    for a_thre, eps in ((0.0, 1e-4), (1e-2, 0.0), (1e-2, 1e-4)):
        ri_p, ts_p, _ = est.sampling(o, d, sigma_fn=sigma_fn, render_step_size=args.step, alpha_thre=a_thre, stratified=False,
                                     cone_angle=0.0, early_stop_eps=eps)
        ri_q, ts_q, _ = grid.sampling(o, d, sigma_fn=sigma_fn, render_step_size=args.step, alpha_thre=a_thre, stratified=False,
                                      cone_angle=0.0, early_stop_eps=eps)
        # a sample is (ray, position in the un-pruned lattice): the un-pruned sets of case 1 agree, so compare by (ray, t_start)
        key = lambda ri, ts: set(zip(ri.tolist(), [round(v, 5) for v in ts.tolist()]))
        kn, kh = key(ri_p, ts_p), key(ri_q, ts_q)
        print(f"pruning: alpha_thre {a_thre:g} early_stop_eps {eps:g}: nerfacc keeps {len(kn)} of {ri_n.numel()}, this build "
              f"{len(kh)} of {ri_h.numel()}; only nerfacc {len(kn - kh)}, only this build {len(kh - kn)}")
        # samples within rounding of a threshold may fall either way (tests/test_gpu_visibility.py caps them at 0.1 %)
        ok &= len(kn ^ kh) <= max(1, ri_n.numel() // 1000)
    # ---- 5. morpheus_amd.volrend, function by function (signatures, shapes and numbers; recalled, this case pins them)
    from morpheus_amd import volrend

    def rel(a, b):
        return float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp(min=1e-30))

    def row(name, a, b, tol=1e-5, count=True):
        nonlocal ok
        same_shape = tuple(a.shape) == tuple(b.shape)
        err = rel(a, b) if same_shape and a.numel() else (0.0 if same_shape else float("inf"))
        print(f"volrend: {name:44s} shape {tuple(a.shape)} vs nerfacc {tuple(b.shape)}; max |difference| / max |nerfacc| = {err:.3e}")
        if count:
            ok &= same_shape and err <= tol

    row("pack_info", volrend.pack_info(ri_n, N), nerfacc.pack_info(ri_n, N), tol=0.0)
    packed = dict(ray_indices=ri_n, n_rays=N)
    sg_h, sg_n = sig.clone().requires_grad_(True), sig.clone().requires_grad_(True)
    rgb_h, rgb_n = rgb.clone().requires_grad_(True), rgb.clone().requires_grad_(True)
    probe = torch.sin(torch.arange(ri_n.numel(), device=dev) * 0.37)
    losses = []
    for mod, sg, cl in ((volrend, sg_h, rgb_h), (nerfacc, sg_n, rgb_n)):
        w, T, al = mod.render_weight_from_density(ts_n, te_n, sg, **packed)
        acc = [mod.accumulate_along_rays(w, values=v, **packed) for v in (None, tm[:, None], cl, cl.repeat(1, 16))]
        losses.append((w, T, al, acc, (w * probe).sum() + (T * probe).sum() + (al * probe).sum() + sum((x * x).sum() for x in acc)))
    for name, a, b in zip(("render_weight_from_density: weights", "render_weight_from_density: trans", "render_weight_from_density: alphas"),
                          losses[0][:3], losses[1][:3]):
        row(name, a.detach(), b.detach())
    for name, a, b in zip(("accumulate_along_rays(values=None)", "accumulate_along_rays, 1 channel", "accumulate_along_rays, 3 channels",
                           "accumulate_along_rays, 48 channels"), losses[0][3], losses[1][3]):
        row(name, a.detach(), b.detach())
    losses[0][4].backward()
    losses[1][4].backward()
    row("d loss / d sigmas", sg_h.grad, sg_n.grad, tol=1e-4)
    row("d loss / d values", rgb_h.grad, rgb_n.grad, tol=1e-4)
    T_h, a_h = volrend.render_transmittance_from_density(ts_n, te_n, sig, **packed)
    T_n, a_n = nerfacc.render_transmittance_from_density(ts_n, te_n, sig, **packed)
    row("render_transmittance_from_density: trans", T_h, T_n)
    row("render_transmittance_from_density: alphas", a_h, a_n)
    alphas = a_n.detach().clamp(max=0.999)
    al_h, al_n = alphas.clone().requires_grad_(True), alphas.clone().requires_grad_(True)
    for mod, al in ((volrend, al_h), (nerfacc, al_n)):
        w, T = mod.render_weight_from_alpha(al, **packed)
        ((w * probe).sum() + (T * probe).sum()).backward()
        if mod is volrend:
            w_a, T_a = w.detach(), T.detach()
    row("render_weight_from_alpha: weights", w_a, w.detach())
    row("render_weight_from_alpha: trans", T_a, T.detach())
    row("render_transmittance_from_alpha", volrend.render_transmittance_from_alpha(alphas, **packed),
        nerfacc.render_transmittance_from_alpha(alphas, **packed))
    row("d loss / d alphas (alphas < 1)", al_h.grad, al_n.grad, tol=1e-4)
    opaque = alphas.clone()
    opaque[::97] = 1.0
    op_h, op_n = opaque.clone().requires_grad_(True), opaque.clone().requires_grad_(True)
    for mod, al in ((volrend, op_h), (nerfacc, op_n)):
        w, T = mod.render_weight_from_alpha(al, **packed)
        ((w * probe).sum() + (T * probe).sum()).backward()
    print(f"volrend: d loss / d alphas with alpha == 1 samples: non-finite elements this build {int((~torch.isfinite(op_h.grad)).sum())}, "
          f"nerfacc {int((~torch.isfinite(op_n.grad)).sum())} (expected: 0 and > 0; not counted)")
    vis_h = volrend.render_visibility_from_density(ts_n, te_n, sig, early_stop_eps=1e-4, alpha_thre=1e-2, **packed)
    vis_n = nerfacc.render_visibility_from_density(ts_n, te_n, sig, early_stop_eps=1e-4, alpha_thre=1e-2, **packed)
    differ = int((vis_h != vis_n).sum())
    print(f"volrend: render_visibility_from_density: {differ} of {vis_n.numel()} samples differ")
    ok &= vis_h.shape == vis_n.shape and differ <= max(1, vis_n.numel() // 1000)
    fn = lambda t0, t1, idx: (rgb, sig)
    bkgd = torch.tensor([1.0, 0.5, 0.25], device=dev)
    out_h = volrend.rendering(ts_n, te_n, ri_n, N, rgb_sigma_fn=fn, render_bkgd=bkgd)
    out_n = nerfacc.rendering(ts_n, te_n, ri_n, N, rgb_sigma_fn=fn, render_bkgd=bkgd)
    for name, a, b in zip(("rendering: colors", "rendering: opacities", "rendering: depths"), out_h[:3], out_n[:3]):
        row(name, a, b)
    print(f"volrend: rendering: extras keys this build {sorted(out_h[3])}, nerfacc {sorted(out_n[3])}")
    ok &= set(out_n[3]) <= set(out_h[3])
    print("PINNED: nerfacc and this build agree" if ok else "DIFFERENCES FOUND (see above)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
