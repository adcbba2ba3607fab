"""GPU: the guidance shell (csrc/guidance.hip, morpheus_amd/guidance.py) against the reference's recorded runs
(tests/golden/guidance.npz) in the float64 judgement of tests/f64_judge: the kernel's worst scaled error against the float64 record
at most max(3 x the worst error of the reference's own fp32 record, 4 U)."""
import os

import numpy as np
import pytest
import torch

from tests import f64_judge as J
from tests import guidance_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guidance.npz")
FACTOR, FLOOR = 3, 4 * J.U
FLT_MAX = G.FLT_MAX


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _f(values):
    return torch.tensor(np.asarray(values, np.float32)).to(DEV)


def _judge(hip, ref32, f64, scale, what):
    f = J.figures_vs_f64(hip, ref32, f64, scale, what, FLOOR)
    print(f"{what}: worst {f['worst_hip'] / J.U:.2f} U vs float64; the fp32 reference's own {f['worst_ref'] / J.U:.2f} U")
    assert f["bad_hip"] == 0, what
    assert J.within(f["worst_hip"], f["worst_ref"], FACTOR, FLOOR), (what, f["worst_hip"] / J.U, f["worst_ref"] / J.U)


def _view_args(name):
    v = G.VIEWS[name]
    return [_f(v[k]) for k in ("polar", "azimuth", "radius", "ref_polars", "ref_azimuths", "ref_radii", "zero123_ws")]


# ------------------------------------------------------------------------------------------------------------------- mh_sds_view
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_sds_view_against_the_golden(golden, name):
    """angles, scale, T and weights of views at least 5 degrees from every reference; r3b2 holds the a > 180 wrap and a
    reference whose weight falls below 0.1.  Each quantity is scaled by its own size (an exact 0 must be 0)."""
    from morpheus_amd import guidance
    c = G.CASES[name]
    T, angles, scale, ws = guidance.sds_view(*_view_args(name), grad_scale=G.GRAD_SCALE)
    assert T.shape == (c["R"], c["B"], 4) and angles.shape == ws.shape == (c["B"], c["R"]) and scale.shape == (c["B"],)
    for got, key in ((T, "T"), (angles, "angles"), (scale, "scale"), (ws, "ws")):
        f64 = golden[f"{name}_{key}64"]
        _judge(got, golden[f"{name}_{key}32"], f64, torch.from_numpy(np.abs(f64)), f"{name} {key}")
    assert bool(((ws == 0).cpu() == torch.from_numpy(golden[f"{name}_ws64"] == 0)).all())


def test_sds_view_at_its_own_reference():
    """the view identical to its reference: a dot product 4 ulp short of 1 would give an arccos of 0.06 degrees; the scale must
    be finite, non-negative and below exp(0.1 / 180) - 1"""
    from morpheus_amd import guidance
    z = torch.zeros(1, device=DEV)
    for ref in ((77.3, 33.1, 3.2), (90.0, 0.0, 3.0), (12.7, -171.9, 1.37)):
        T, angles, scale, ws = guidance.sds_view(z, z, z, _f([ref[0]]), _f([ref[1]]), _f([ref[2]]), _f([1.0]), grad_scale=1.0)
        s = float(scale[0])
        assert np.isfinite(s) and 0.0 <= s < np.exp(0.1 / 180) - 1, (ref, s)
        assert float(ws[0, 0]) == 1.0 and bool(torch.isfinite(T).all()) and 0.0 <= float(angles[0, 0]) < 0.06
    # among three references: the weights stay finite, the identical one has weight 1
    T, angles, scale, ws = guidance.sds_view(z, z, z, _f([77.3, 60.0, 100.0]), _f([33.1, -20.0, 90.0]), _f([3.2, 3.0, 3.5]),
                                             _f([1.0, 1.0, 1.0]))
    assert bool(torch.isfinite(ws).all()) and float(ws[0, 0]) == 1.0 and 0.0 <= float(scale[0]) < np.exp(0.1 / 60) - 1


def test_sds_view_bank_picks_the_keyframe_on_the_device():
    from morpheus_amd import guidance
    kf = [0, 4, 8, 9]
    ref_p, ref_a, ref_r, w = [90.0, 80.0, 70.0, 100.0], [0.0, 120.0, -100.0, 45.0], [3.0, 3.5, 2.75, 3.25], [1.0, 1.0, 1.0, 1.0]
    polar, azimuth, radius = [10.0, -20.0], [100.0, -30.0], [0.5, -0.25]
    bank = [_t(np.asarray(kf, np.int64))] + [_f(a) for a in (ref_p, ref_a, ref_r, w)]
    # exact hit, midpoint ties (the lowest index), beyond the last keyframe, before the first
    for frame, want in ((4, 1), (2, 0), (6, 1), (40, 3), (9, 3), (-3, 0)):
        assert G.nearest_keyframe(frame, kf) == want
        rays_id = torch.full((1, 5, 1), frame, dtype=torch.int64, device=DEV)
        for target in (False, True):
            chosen, T, angles, scale, ws = guidance.sds_view_bank(_f(polar), _f(azimuth), _f(radius), rays_id, *bank, target, G.GRAD_SCALE)
            sel = 0 if target else want
            assert chosen.dtype == torch.int64 and int(chosen[0]) == sel
            p, a, r = G.retarget(polar, azimuth, radius, ref_p, ref_a, ref_r, want) if target else (polar, azimuth, radius)
            o64 = G.view(p, a, r, [ref_p[sel]], [ref_a[sel]], [ref_r[sel]], [w[sel]], G.GRAD_SCALE)
            o32 = G.view(p, a, r, [ref_p[sel]], [ref_a[sel]], [ref_r[sel]], [w[sel]], G.GRAD_SCALE, np.float32)
            for got, r32, r64, key in zip((T, angles, scale, ws), o32, o64, ("T", "angles", "scale", "ws")):
                _judge(got, r32, r64, torch.from_numpy(np.abs(r64)), f"bank frame {frame} target {target} {key}")


def test_angle_between():
    from morpheus_amd import guidance
    g = guidance.SDSGuidance(None, DEV)
    rng = np.random.RandomState(61)
    v = np.stack([rng.rand(5) + 2.5, np.deg2rad(rng.rand(5) * 60 + 45), np.deg2rad(rng.rand(5) * 360 - 180)], -1).astype(np.float32)
    got = g.angle_between(torch.from_numpy(v), torch.from_numpy(v[:3]))
    f64 = G.angles_rad(v.astype(np.float64), v[:3].astype(np.float64))
    off = ~np.eye(5, 3, dtype=bool)                                       # away from the diagonal, where arccos is ill-conditioned
    _judge(got.cpu()[torch.from_numpy(off)], G.angles_rad(v, v[:3])[off], f64[off], torch.from_numpy(f64[off]), "angle_between")
    assert bool((got.cpu()[torch.from_numpy(~off)] < 1e-3).all())


# -------------------------------------------------------------------------------------------------- mh_sds_noise and mh_sds_grad
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_sds_noise_against_the_golden(golden, name):
    """fed the recorded fp32 latents; t in {20, 980} (r3b2) and {500} (r1b1)"""
    from morpheus_amd import guidance
    c = G.CASES[name]
    lat, noise, t = golden[f"{name}_latents32"], golden[f"{name}_noise"], golden[f"{name}_t"]
    x_in = guidance.sds_noise(_t(lat), _t(noise), _t(t), _t(golden["alphas"]))
    assert x_in.shape == (2 * c["B"],) + lat.shape[1:] and torch.equal(x_in[:c["B"]], x_in[c["B"]:])
    a = golden["alphas"].astype(np.float64)[t].reshape(-1, 1, 1, 1)
    size = np.sqrt(a) * np.abs(lat) + np.sqrt(1 - a) * np.abs(noise)
    _judge(x_in[:c["B"]], golden[f"{name}_latents_noisy32"], golden[f"{name}_latents_noisy64"], torch.from_numpy(size), f"{name} latents_noisy")


def _grad_inputs(golden, name):
    return (_t(golden[f"{name}_noise_preds32"]), _t(golden[f"{name}_ws32"]), _t(golden[f"{name}_noise"]), _t(golden[f"{name}_t"]),
            _t(golden["alphas"]), _t(golden[f"{name}_scale32"]))


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_sds_grad_against_the_golden(golden, name):
    """fed the recorded fp32 noise_preds, weights and scale.  grad is scaled by the size of its terms, scale (1 - a_t) (sum_k w_k
    (|u_k| + s |c_k - u_k|) / sum_k w_k + |noise|); the loss by itself.  Two runs give the same loss bits."""
    from morpheus_amd import guidance
    c = G.CASES[name]
    args = _grad_inputs(golden, name)
    grad, loss = guidance.sds_grad(*args, G.GUIDANCE_SCALE)
    nps, ws, noise = (golden[f"{name}_{k}"].astype(np.float64) for k in ("noise_preds64", "ws64", "noise"))
    B = c["B"]
    wk = ws.T.reshape(c["R"], B, 1, 1, 1)
    terms = (wk * (np.abs(nps[:, :B]) + G.GUIDANCE_SCALE * np.abs(nps[:, B:] - nps[:, :B]))).sum(0) / ws.sum(-1).reshape(B, 1, 1, 1)
    w_t = 1 - golden["alphas"].astype(np.float64)[golden[f"{name}_t"]]
    size = (golden[f"{name}_scale64"] * w_t).reshape(B, 1, 1, 1) * (terms + np.abs(noise))
    _judge(grad, golden[f"{name}_grad32"], golden[f"{name}_grad64"], torch.from_numpy(size), f"{name} grad")
    l64 = float(golden[f"{name}_loss64"])
    _judge(loss.reshape(1), golden[f"{name}_loss32"].reshape(1), np.asarray([l64]), l64, f"{name} loss")
    # the loss is the sum over THIS grad: 0.5 sum g^2 / B in float64, to one fp32 rounding
    own = 0.5 * float((grad.double() ** 2).sum()) / B
    assert abs(float(loss) - own) <= 2 * J.U * own
    grad2, loss2 = guidance.sds_grad(*args, G.GUIDANCE_SCALE)
    assert torch.equal(grad, grad2) and loss.view(torch.int32).item() == loss2.view(torch.int32).item()


def test_sds_grad_nan_inf_and_zero_weights(golden):
    from morpheus_amd import guidance
    name = "r3b2"
    nps, ws, noise, t, alphas, scale = _grad_inputs(golden, name)
    clean, _ = guidance.sds_grad(nps, ws, noise, t, alphas, scale, G.GUIDANCE_SCALE)
    # view 1 weighs all three references: NaN -> 0, +-inf -> +-FLT_MAX
    bad = nps.clone()
    B = 2
    bad[0, 1, 0, 0, 0] = float("nan")
    bad[1, B + 1, 0, 0, 1] = float("inf")                               # in the conditional half: u + s (inf - u) = inf
    bad[2, B + 1, 0, 0, 2] = float("-inf")
    grad, loss = guidance.sds_grad(bad, ws, noise, t, alphas, scale, G.GUIDANCE_SCALE)
    assert float(grad[1, 0, 0, 0]) == 0.0 and float(grad[1, 0, 0, 1]) == FLT_MAX and float(grad[1, 0, 0, 2]) == -FLT_MAX
    keep = torch.ones_like(grad, dtype=torch.bool)
    keep[1, 0, 0, :3] = False
    assert torch.equal(grad[keep], clean[keep])
    # view 0 gives reference 2 the weight 0: the result is the run without that reference, grad and loss bits
    assert float(ws[0, 2]) == 0.0
    one = slice(0, 1)
    sub = torch.cat([nps[:, 0:1], nps[:, B:B + 1]], dim=1)               # view 0 alone: [R, 2, ...]
    with3 = guidance.sds_grad(sub.contiguous(), ws[one], noise[one], t[one], alphas, scale[one], G.GUIDANCE_SCALE)
    with2 = guidance.sds_grad(sub[:2].contiguous(), ws[one, :2].contiguous(), noise[one], t[one], alphas, scale[one], G.GUIDANCE_SCALE)
    assert torch.equal(with3[0], with2[0]) and torch.equal(with3[1], with2[1])
    assert torch.equal(with3[0], clean[one])


# ---------------------------------------------------------------------------------------------------------- the step on the device
def _stub(golden, name):
    from bench_support import guidance_stub as GS
    weights = {k[len(name) + 3:]: a for k, a in golden.items() if k.startswith(f"{name}_w_")}
    return GS.StubLDM(stride=G.CASES[name]["stride"]).load_weights(weights).to(DEV)


def _embeddings(golden, name):
    v = G.VIEWS[name]
    return dict(c_crossattn=list(_t(golden[f"{name}_cc32"])), c_concat=list(_t(golden[f"{name}_cat32"])),
                **{k: list(v[k]) for k in ("ref_polars", "ref_azimuths", "ref_radii", "zero123_ws")})


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_train_step_against_the_golden(golden, name):
    """SDSGuidance.train_step with the stub on the device: loss and d loss / d pred_rgb against the reference's float64 run.  The
    yardstick is the plain-torch chain (guidance_oracle.train_step_torch) on the same GPU in fp32 with the same stub, so the
    rounding of the stub's convolutions is part of the yardstick.  The gradient image is scaled by its largest element."""
    from morpheus_amd import guidance
    c, v = G.CASES[name], G.VIEWS[name]
    model, emb = _stub(golden, name), _embeddings(golden, name)
    g = guidance.SDSGuidance(model, DEV)
    assert torch.equal(g.alphas.cpu(), torch.from_numpy(golden["alphas"]))
    polar, azimuth, radius = _f(v["polar"]), _f(v["azimuth"]), _f(v["radius"])
    t, noise = _t(golden[f"{name}_t"]), _t(golden[f"{name}_noise"])
    kw = dict(guidance_scale=G.GUIDANCE_SCALE, as_latent=c["as_latent"], grad_scale=G.GRAD_SCALE)
    pred = _t(golden[f"{name}_pred"]).requires_grad_(True)
    loss, t_out, scale, noise_out = g.train_step(emb, pred, polar, azimuth, radius, t=t, noise=noise, **kw)
    loss.backward()
    assert t_out is t and noise_out is noise and loss.dim() == 0
    ref_pred = _t(golden[f"{name}_pred"]).requires_grad_(True)
    ref = G.train_step_torch(model, g.alphas, emb, ref_pred, polar, azimuth, radius, G.GUIDANCE_SCALE, c["as_latent"], G.GRAD_SCALE, t, noise)
    ref["loss"].backward()
    d64, l64 = golden[f"{name}_dpred64"], float(golden[f"{name}_loss64"])
    _judge(loss.detach().reshape(1), ref["loss"].detach().reshape(1), np.asarray([l64]), l64, f"{name} train_step loss")
    _judge(pred.grad, ref_pred.grad, d64, float(np.abs(d64).max()), f"{name} train_step d loss / d pred_rgb")
    _judge(scale, golden[f"{name}_scale32"], golden[f"{name}_scale64"], torch.from_numpy(golden[f"{name}_scale64"]), f"{name} grad_scale")
    # the renderer's own layout gives the same bits
    nhwc = _t(golden[f"{name}_pred"]).permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    loss2 = g.train_step(emb, nhwc, polar, azimuth, radius, t=t, noise=noise, layout="nhwc", **kw)[0]
    loss2.backward()
    assert torch.equal(loss2, loss)
    if c["as_latent"]:                                                   # (no convolution between the loss and the image)
        assert torch.equal(nhwc.grad.permute(0, 3, 1, 2), pred.grad)
    else:
        assert float((nhwc.grad.permute(0, 3, 1, 2) - pred.grad).abs().max()) <= 16 * J.U * float(pred.grad.abs().max())
    # t and noise drawn inside
    loss3, t3, _, noise3 = g.train_step(emb, pred.detach(), polar, azimuth, radius, **kw)
    assert t3.dtype == torch.int64 and t3.shape == (c["B"],) and noise3.shape == noise.shape and bool(torch.isfinite(loss3))


def _bank(golden, device_frames=(0, 7)):
    """two keyframes from the recorded r3b2 embeddings (references 0 and 1 as keyframes 0 and 7)"""
    from morpheus_amd import guidance
    v = G.VIEWS["r3b2"]
    emb = {f: dict(c_crossattn=[_t(golden["r3b2_cc32"][i])], c_concat=[_t(golden["r3b2_cat32"][i])], zero123_ws=[1],
                   ref_polars=[v["ref_polars"][i]], ref_azimuths=[v["ref_azimuths"][i]], ref_radii=[v["ref_radii"][i]])
           for i, f in enumerate(device_frames)}
    return emb, guidance.EmbeddingBank.from_embeddings(emb, torch.tensor(device_frames), device=DEV)


def test_the_step_reads_nothing_from_the_device(golden):
    """with t and noise injected, train_step (forward and backward) and virtual_view_loss complete under
    torch.cuda.set_sync_debug_mode("error"); virtual_view_loss equals train_step on the embeddings the reference would pick"""
    from morpheus_amd import guidance
    name = "r3b2"
    c, v = G.CASES[name], G.VIEWS[name]
    model, emb = _stub(golden, name), _embeddings(golden, name)
    g = guidance.SDSGuidance(model, DEV)
    polar, azimuth, radius = _f(v["polar"]), _f(v["azimuth"]), _f(v["radius"])
    t, noise = _t(golden[f"{name}_t"]), _t(golden[f"{name}_noise"])
    kf_emb, bank = _bank(golden)
    rays_id = torch.full((1, 9, 1), 5, dtype=torch.int64, device=DEV)               # nearest keyframe: 7 (index 1)
    kw = dict(guidance_scale=G.GUIDANCE_SCALE, grad_scale=G.GRAD_SCALE, t=t, noise=noise)

    class Coin:
        def __init__(self, values):
            self.values = list(values)

        def random(self):
            return self.values.pop(0)

    pred0 = _t(golden[f"{name}_pred"])

    def both():
        pred = pred0.clone().requires_grad_(True)
        loss = g.train_step(emb, pred, polar, azimuth, radius, **kw)[0]
        loss.backward()
        coin = Coin([0.75, 0.25])                                                   # the current keyframe, then keyframe 0
        cur = guidance.virtual_view_loss(g, bank, pred.detach(), polar, azimuth, radius, rays_id, coin, **kw)
        one = guidance.virtual_view_loss(g, bank, pred.detach(), polar, azimuth, radius, rays_id, coin, **kw)
        return loss, pred.grad, cur, one

    warm = both()                                                                   # caches, scratch and the convolutions' plans
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, dpred, cur, one = both()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(loss, warm[0]) and torch.equal(dpred, warm[1]) and bool(torch.isfinite(dpred).all())
    pred = pred0
    want_cur = g.train_step(kf_emb[7], pred, polar, azimuth, radius, **kw)[0]
    assert torch.equal(cur, want_cur)
    # keyframe 0 as the target: the view re-expressed as morpheus.py:1059-1070 does, on the host here
    p = polar + v["ref_polars"][1] - v["ref_polars"][0]
    a = azimuth + v["ref_azimuths"][1] - v["ref_azimuths"][0]
    a = torch.where(a > 180, a - 360, a)
    r = radius + v["ref_radii"][1] - v["ref_radii"][0]
    want_one = g.train_step(kf_emb[0], pred, p, a, r, **kw)[0]
    assert abs(float(one.detach()) - float(want_one.detach())) <= 1e-5 * float(want_one.detach())               # (the host's fp32 sums against the kernel's float64)


def test_virtual_view_train_step_takes_the_guidance(golden):
    """bench_support.trainstep.VirtualViewTrainStep(guidance=as_step_guidance(...)): one 24 x 24 step, finite gradients on the model"""
    from bench_support import trainstep
    from morpheus_amd import guidance, harness, synth
    from oracle import field as of
    name = "r1b1"
    model_ldm = _stub(golden, name)
    emb = _embeddings(golden, name)
    g = guidance.SDSGuidance(model_ldm, DEV)
    hw, S, frame = 24, 16, 25
    z = torch.zeros(1, device=DEV)
    step_guidance = guidance.as_step_guidance(g, emb, z + 15.0, z - 40.0, z + 0.25, hw, hw, guidance_scale=G.GUIDANCE_SCALE,
                                              t=torch.tensor([500], device=DEV))
    o, d = synth.camera_rays(hw, hw, synth.look_at_pose(70.0, 35.0, 1.5))
    N = o.shape[0]
    smp = of.uniform_samples(o, d, synth.ray_jitter(N), S, 1.01)
    model = harness.build_model("b", DEV, 0.75).train()
    rend = harness.make_renderer(model, S, samples=tuple(x.to(DEV) for x in smp))
    ts = trainstep.VirtualViewTrainStep(rend, res=hw, guidance=step_guidance)
    data = dict(H=hw, W=hw, rays_o=o[None].to(DEV), rays_d=d[None].to(DEV), rays_t=torch.full((1, N, 1), frame / 200, device=DEV),
                rays_id=torch.full((1, N, 1), frame, device=DEV, dtype=torch.int64))
    light = of.safe_normalize(o + torch.tensor([0.3, -0.2, 0.5])).to(DEV)
    loss = ts(data=data, shading="albedo", ambient_ratio=1.0, bg_color=None, light_d=light)
    loss.backward()
    assert ts.guidance is step_guidance and bool(torch.isfinite(loss))
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(x).all()) for x in grads) and any(float(x.abs().max()) > 0 for x in grads)
