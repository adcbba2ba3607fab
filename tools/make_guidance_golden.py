"""Record tests/golden/guidance.npz from the reference's own Zero123.train_step (build container only: needs the reference tree).

    python tools/make_guidance_golden.py <reference tree>

models/guidance/zero123_utils.py is loaded by file path, with empty stand-in modules for what it imports and never uses here
(omegaconf, diffusers, ldm.util, torchvision.utils).  The object is made with Zero123.__new__ + nn.Module.__init__; its `model` is
bench_support.guidance_stub.StubLDM and its scheduler guidance_stub.Scheduler.  train_step runs on the CPU with injected t and noise
for the cases of tests/guidance_oracle.py (CASES, VIEWS): once in fp32, and once in float64 from the same fp32 inputs and weights
(torch's default dtype float64 -- the class builds its view tensors with it -- and Tensor.float patched to .double for that run).

Recorded per case <name>_*: pred, noise, t; the stub's weights (w_*); the embeddings of both runs (cc32 / cc64, cat32 / cat64); and
for both runs latents, latents_noisy, noise_preds [R,2B,...], grad, loss, scale (the returned grad_scale), angles, T, ws -- the
quantities train_step does not return are taken from the calls it makes (F.interpolate, scheduler.add_noise, apply_model,
torch.nan_to_num, cc_projection's input) -- and dpred64 = d loss / d pred_rgb of the float64 run.  Numeric arrays only.
F.interpolate's own results for the resize cases are NOT recorded: the 72 -> 256 case alone exceeds the size a committed file may
have; the tests call F.interpolate on the CPU themselves.
Finally tests/guidance_oracle.py's float64 restatements are checked against the float64 records.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_support import guidance_stub as GS  # noqa: E402
from tests import guidance_oracle as G  # noqa: E402


def load_class(ref):
    for name, attrs in (("omegaconf", ("OmegaConf",)), ("diffusers", ("DDIMScheduler",)), ("ldm", ()), ("ldm.util", ("instantiate_from_config",)),
                        ("torchvision", ()), ("torchvision.utils", ("save_image",))):
        if name not in sys.modules:
            mod = types.ModuleType(name)
            for a in attrs:
                setattr(mod, a, None)
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_zero123_utils", os.path.join(ref, "models", "guidance", "zero123_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Zero123


def make_guidance(Zero123, model, dtype):
    g = Zero123.__new__(Zero123)
    nn.Module.__init__(g)
    g.device, g.fp16, g.model = torch.device("cpu"), False, model
    g.scheduler = GS.Scheduler()                                    # the table is fp32 whatever the run's precision, as diffusers' is
    g.scheduler.alphas_cumprod = g.scheduler.alphas_cumprod.to(dtype)
    g.num_train_timesteps, g.min_step, g.max_step = 1000, 20, 980
    g.alphas = g.scheduler.alphas_cumprod
    return g


class Spy:
    """keeps what the named calls return (or are given) during one train_step"""

    def __init__(self, g):
        self.g, self.seen = g, {}
        self.undo = []

    def wrap(self, owner, name, key):
        fn = getattr(owner, name)

        def spy(*a, **k):
            out = fn(*a, **k)
            self.seen.setdefault(key, []).append(out.detach().clone())
            return out
        setattr(owner, name, spy)
        self.undo.append((owner, name, fn))

    def close(self):
        for owner, name, fn in reversed(self.undo):
            setattr(owner, name, fn)


def run(Zero123, name, dtype):
    c, v = G.CASES[name], G.VIEWS[name]
    pred_np, noise_np, refs_np = G.case_inputs(name)
    f64 = dtype == torch.float64
    float_ = torch.Tensor.float
    torch.set_default_dtype(dtype)
    if f64:
        torch.Tensor.float = torch.Tensor.double
    try:
        model = GS.StubLDM(stride=c["stride"]).to(dtype)
        g = make_guidance(Zero123, model, dtype)
        cc, cat = g.get_img_embeds(torch.from_numpy(refs_np).to(dtype))
        emb = dict(c_crossattn=cc, c_concat=cat, ref_polars=list(v["ref_polars"]), ref_azimuths=list(v["ref_azimuths"]),
                   ref_radii=list(v["ref_radii"]), zero123_ws=list(v["zero123_ws"]))
        pred = torch.from_numpy(pred_np).to(dtype).requires_grad_(True)
        col = lambda k: torch.tensor(np.asarray(v[k], np.float32)).to(dtype)
        t = torch.tensor(c["t"], dtype=torch.long)
        spy = Spy(g)
        spy.wrap(g.scheduler, "add_noise", "latents_noisy")
        spy.wrap(model, "apply_model", "noise_preds")
        hook = model.cc_projection.register_forward_pre_hook(lambda m, a: spy.seen.setdefault("cc_in", []).append(a[0].detach().clone()))
        spy.wrap(torch, "nan_to_num", "grad")
        spy.wrap(g, "angle_between", "angles_rad")
        if c["as_latent"]:
            spy.wrap(torch.nn.functional, "interpolate", "interp")
        else:
            spy.wrap(g, "encode_imgs", "latents")
        try:
            loss, t_out, scale, noise_out = g.train_step(emb, pred, col("polar"), col("azimuth"), col("radius"),
                                                         guidance_scale=G.GUIDANCE_SCALE, as_latent=c["as_latent"],
                                                         grad_scale=G.GRAD_SCALE, t=t, noise=torch.from_numpy(noise_np).to(dtype))
        finally:
            spy.close()
            hook.remove()
        loss.backward()
        s = spy.seen
        latents = s["interp"][0] * 2 - 1 if c["as_latent"] else s["latents"][0]
        grad = s["grad"][0]
        nps = torch.stack(s["noise_preds"])
        # zero123_ws (:164-175) is not returned by any call: the same statements on the recorded angles, in the run's precision
        angles = torch.rad2deg(s["angles_rad"][0])
        R = len(v["ref_azimuths"])
        if R > 1:
            inv = 1 / angles
            inv[inv > 100] = 100
            inv /= inv.max(dim=-1, keepdim=True)[0]
            inv[inv < 0.1] = 0
        else:
            inv = torch.tensor([1.])
        ws = torch.tensor(emb["zero123_ws"])[None, :] * inv
        ws /= ws.max(dim=-1, keepdim=True)[0]
        ws[ws < 0.1] = 0
        T = torch.stack([x[:, 0, -4:] for x in s["cc_in"]])          # cc_projection is fed [B,1,E + 4]: the last four are the row of T
        out = dict(latents=latents, latents_noisy=s["latents_noisy"][0], noise_preds=nps, grad=grad, loss=loss.detach(), scale=scale,
                   angles=angles, T=T, ws=ws.expand(c["B"], R), dpred=pred.grad, cc=torch.stack(cc), cat=torch.stack(cat))
        assert bool((t_out == t).all()) and noise_out.dtype == dtype
        return {k: x.detach().numpy().copy() for k, x in out.items()}, model.weights()
    finally:
        torch.Tensor.float = float_
        torch.set_default_dtype(torch.float32)


def main(ref):
    Zero123 = load_class(ref)
    rec = {}
    alphas = GS.scaled_linear_alphas().numpy()
    rec["alphas"] = alphas
    for name in sorted(G.CASES):
        c, v = G.CASES[name], G.VIEWS[name]
        pred, noise, _ = G.case_inputs(name)
        r32, w = run(Zero123, name, torch.float32)
        r64, _ = run(Zero123, name, torch.float64)
        rec.update({f"{name}_pred": pred, f"{name}_noise": noise, f"{name}_t": np.asarray(c["t"], np.int64)})
        rec.update({f"{name}_w_{k}": a for k, a in w.items()})
        for k in r32:
            assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64, (name, k, r32[k].dtype, r64[k].dtype)
            if k != "dpred":
                rec[f"{name}_{k}32"] = r32[k]
            rec[f"{name}_{k}64"] = r64[k]
        # what the cases are there for
        ang, ws = r64["angles"], r64["ws"]
        assert ang.min() >= 5.0, (name, ang)
        margins = np.abs(ws[ws > 0] - 0.1).min()
        print(f"{name}: angles {np.round(ang, 2).tolist()}, ws {np.round(ws, 4).tolist()}, scale {r64['scale'].tolist()}, "
              f"loss {float(r64['loss']):.6g} (fp32 {float(r32['loss']):.6g})")
        assert margins > 1e-3
        if c["R"] == 3:
            assert (ws == 0).any() and (np.asarray(v["azimuth"])[None, :] + v["ref_azimuths"][0] - np.asarray(v["ref_azimuths"])[:, None] > 180).any()
        # the float64 restatements against the float64 records, in double round-offs of each quantity's size
        E = 2.0 ** -53
        T, a, s, w_ = G.view(v["polar"], v["azimuth"], v["radius"], v["ref_polars"], v["ref_azimuths"], v["ref_radii"], v["zero123_ws"],
                             G.GRAD_SCALE)
        for got, want, what in ((T, r64["T"], "T"), (a, r64["angles"], "angles"), (s, r64["scale"], "scale"), (w_, r64["ws"], "ws")):
            print(f"  {what}: {np.abs(got - want).max() / E:.1f} double round-offs")
        x = G.add_noise(r64["latents"], noise, c["t"], alphas)
        g_, l_ = G.grad_loss(r64["noise_preds"], r64["ws"], noise, c["t"], alphas, r64["scale"], G.GUIDANCE_SCALE)
        print(f"  latents_noisy: {np.abs(x[:c['B']] - r64['latents_noisy']).max() / E:.1f}, grad: "
              f"{np.abs(g_ - r64['grad']).max() / (E * np.abs(r64['grad']).max()):.1f}, loss: {abs(l_ - r64['loss']) / (E * l_):.1f} (relative)")
    path = os.path.join(ROOT, "tests", "golden", "guidance.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
