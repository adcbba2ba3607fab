"""Restatements of the guidance shell (csrc/guidance.hip, morpheus_amd/guidance.py) -- the checker, not the product.

numpy, in a chosen dtype: view() (zero123_utils.py:107-119, :129-134, :164-175, :191-197), nearest_keyframe() and retarget()
(morpheus.py:1031-1070), add_noise() and grad_loss() (:180, :204-234).  train_step_torch() is the whole of Zero123.train_step as a
plain chain of torch operations on the tensors' own device and dtype: in float64 on the CPU it is compared with the golden, in fp32
on the GPU it is the yardstick of what fp32 keeps of the step (the stub's convolutions included).

The golden's cases (tools/make_guidance_golden.py records them, the tests read them) are listed in CASES.
"""
import numpy as np
import torch
import torch.nn.functional as F

FLT_MAX = float(np.finfo(np.float32).max)

# name: R references, B views, as_latent, render size, the stub's stride, t per view.  Every value the cases must cover appears:
# R in {1, 3}, B in {1, 2}, as_latent both ways, sizes 36 and 72, t in {20, 500, 980}.
CASES = {
    "r3b2": dict(R=3, B=2, as_latent=False, size=36, stride=16, t=(20, 980)),
    "r1b1": dict(R=1, B=1, as_latent=True, size=72, stride=8, t=(500,)),
}
# the views (deltas to reference 0) and reference views of each case; fp32-representable.  r3b2: view 0 is 25.5 degrees of azimuth
# from reference 0 and far from the others (reference 2's weight falls below 0.1 and is zeroed); view 1's azimuth relative to
# reference 1 is 200 - (-40) = 240 > 180: the wrap.  Every view is at least 5 degrees from every reference.
VIEWS = {
    "r3b2": dict(polar=(-12.5, 20.0), azimuth=(25.5, 200.0), radius=(0.25, -0.125),
                 ref_polars=(90.0, 75.0, 60.0), ref_azimuths=(0.0, -40.0, 150.0), ref_radii=(3.0, 3.5, 2.75), zero123_ws=(1.0, 0.75, 0.3125)),
    "r1b1": dict(polar=(15.0,), azimuth=(-60.25,), radius=(0.5,),
                 ref_polars=(80.0,), ref_azimuths=(10.0,), ref_radii=(3.25,), zero123_ws=(1.0,)),
}
GUIDANCE_SCALE, GRAD_SCALE = 3.0, 0.5


# ---- numpy ---------------------------------------------------------------------------------------------------------------------
def _unit(r, theta, phi):
    v = np.stack([r * np.sin(theta) * np.cos(phi), r * np.sin(theta) * np.sin(phi), r * np.cos(theta)], -1)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def angles_rad(v1, v2):
    """rows [r, theta, phi] (radians): [N1,3], [N2,3] -> [N1,N2] radians"""
    u1, u2 = _unit(v1[:, 0], v1[:, 1], v1[:, 2]), _unit(v2[:, 0], v2[:, 1], v2[:, 2])
    return np.arccos(np.clip(u1 @ u2.T, -1.0, 1.0))


def view(polar, azimuth, radius, ref_p, ref_a, ref_r, user_w, grad_scale, dtype=np.float64):
    """-> T [R,B,4], angles [B,R] (degrees), scale [B], ws [B,R]"""
    f = dtype
    polar, azimuth, radius, ref_p, ref_a, ref_r, user_w = (np.asarray(a, np.float32).astype(f) for a in
                                                           (polar, azimuth, radius, ref_p, ref_a, ref_r, user_w))
    R = ref_p.shape[0]
    v1 = np.stack([radius + ref_r[0], np.deg2rad(polar + ref_p[0]), np.deg2rad(azimuth + ref_a[0])], -1)
    v2 = np.stack([ref_r, np.deg2rad(ref_p), np.deg2rad(ref_a)], -1)
    angles = np.rad2deg(angles_rad(v1, v2)).astype(f)
    scale = (np.exp(angles.min(axis=1) / f(180.0 / R)) - 1) * f(grad_scale)
    if R > 1:
        with np.errstate(divide="ignore"):
            inv = 1 / angles
        inv[inv > 100] = 100
        inv = inv / inv.max(axis=-1, keepdims=True)
        inv[inv < 0.1] = 0
    else:
        inv = np.ones((polar.shape[0], 1), f)
    ws = user_w[None, :] * inv
    ws = ws / ws.max(axis=-1, keepdims=True)
    ws[ws < 0.1] = 0
    p = polar[None, :] + ref_p[0] - ref_p[:, None]
    a = azimuth[None, :] + ref_a[0] - ref_a[:, None]
    a = np.where(a > 180, a - 360, a)
    r = radius[None, :] + ref_r[0] - ref_r[:, None]
    T = np.stack([np.deg2rad(p), np.sin(np.deg2rad(a)), np.cos(np.deg2rad(a)), r], -1)
    return T.astype(f), angles, scale.astype(f), ws.astype(f)


def nearest_keyframe(frame_id, kf):
    """morpheus.py:1031-1042: the index of the keyframe nearest to frame_id, the lowest on a tie"""
    return int(np.argmin(np.abs(np.asarray(kf, np.int64) - int(frame_id))))


def retarget(polar, azimuth, radius, ref_p, ref_a, ref_r, near, dtype=np.float64):
    """morpheus.py:1059-1070: the view given relative to keyframe `near`, relative to keyframe 0"""
    f = dtype
    c = lambda a: np.asarray(a, np.float32).astype(f)
    p = c(polar) + c(ref_p)[near] - c(ref_p)[0]
    a = c(azimuth) + c(ref_a)[near] - c(ref_a)[0]
    r = c(radius) + c(ref_r)[near] - c(ref_r)[0]
    return p, np.where(a > 180, a - 360, a), r


def add_noise(latents, noise, t, alphas, dtype=np.float64):
    f = dtype
    a = np.asarray(alphas).astype(f)[np.asarray(t)].reshape((-1,) + (1,) * (np.ndim(latents) - 1))
    x = np.sqrt(a) * np.asarray(latents).astype(f) + np.sqrt(1 - a) * np.asarray(noise).astype(f)
    return np.concatenate([x, x], 0)


def grad_loss(noise_preds, ws, noise, t, alphas, scale, guidance_scale, dtype=np.float64):
    """noise_preds [R,2B,...] -> (grad [B,...], loss)"""
    f = dtype
    nps, ws, noise, scale = (np.asarray(a).astype(f) for a in (noise_preds, ws, noise, scale))
    B = noise.shape[0]
    tail = (1,) * (noise.ndim - 1)
    acc = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(nps.shape[0]):
            u, c = nps[k, :B], nps[k, B:]
            acc = acc + ws[:, k].reshape((B,) + tail) * (u + f(guidance_scale) * (c - u))
        e = acc / ws.sum(axis=-1).reshape((B,) + tail)
        w = 1 - np.asarray(alphas).astype(f)[np.asarray(t)]
        g = (scale * w).reshape((B,) + tail) * (e - noise)
    g = np.nan_to_num(g, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)
    return g, 0.5 * (g.astype(np.float64) ** 2).sum() / B


# ---- torch: the whole step ---------------------------------------------------------------------------------------------------
def _sph_unit_t(r, theta, phi):
    v = torch.stack([r * torch.sin(theta) * torch.cos(phi), r * torch.sin(theta) * torch.sin(phi), r * torch.cos(theta)], -1)
    return v / torch.linalg.norm(v, dim=-1, keepdim=True)


def train_step_torch(model, alphas, embeddings, pred_rgb, polar, azimuth, radius, guidance_scale, as_latent, grad_scale, t, noise):
    """Zero123.train_step (:138-236) with t and noise given, vectorised, in pred_rgb's dtype on its device
    -> dict(loss, grad, latents, latents_noisy, noise_preds [R,2B,...], T [R,B,4], angles, scale, ws)"""
    dt, dev = pred_rgb.dtype, pred_rgb.device
    c = lambda k: torch.tensor([float(v) for v in embeddings[k]], dtype=torch.float32).to(dt).to(dev)
    ref_p, ref_a, ref_r, user_w = c("ref_polars"), c("ref_azimuths"), c("ref_radii"), c("zero123_ws")
    R = ref_p.shape[0]
    u1 = _sph_unit_t(radius + ref_r[0], torch.deg2rad(polar + ref_p[0]), torch.deg2rad(azimuth + ref_a[0]))
    u2 = _sph_unit_t(ref_r, torch.deg2rad(ref_p), torch.deg2rad(ref_a))
    angles = torch.rad2deg(torch.arccos(torch.clip(u1 @ u2.T, -1.0, 1.0)))
    scale = (torch.exp(angles.min(dim=1)[0] / (180 / R)) - 1) * grad_scale
    if as_latent:
        latents = F.interpolate(pred_rgb, (32, 32), mode="bilinear", align_corners=False) * 2 - 1
    else:
        x = F.interpolate(pred_rgb, (256, 256), mode="bilinear", align_corners=False) * 2 - 1
        latents = torch.cat([model.get_first_stage_encoding(model.encode_first_stage(img.unsqueeze(0))) for img in x], dim=0)
    B = latents.shape[0]
    if R > 1:
        inv = (1 / angles).clamp(max=100)
        inv = inv / inv.max(dim=-1, keepdim=True)[0]
        inv = torch.where(inv < 0.1, torch.zeros_like(inv), inv)
    else:
        inv = torch.ones(1, dtype=dt, device=dev)
    ws = user_w[None, :] * inv
    ws = ws / ws.max(dim=-1, keepdim=True)[0]
    ws = torch.where(ws < 0.1, torch.zeros_like(ws), ws)
    with torch.no_grad():
        a_t = alphas.to(dt).to(dev)[t].reshape(B, 1, 1, 1)
        noisy = a_t ** 0.5 * latents + (1 - a_t) ** 0.5 * noise
        x_in, t_in = torch.cat([noisy] * 2), torch.cat([t] * 2)
        preds, rows, acc = [], [], 0
        for k in range(R):
            p = polar + ref_p[0] - ref_p[k]
            a = azimuth + ref_a[0] - ref_a[k]
            a = torch.where(a > 180, a - 360, a)
            r = radius + ref_r[0] - ref_r[k]
            T = torch.stack([torch.deg2rad(p), torch.sin(torch.deg2rad(a)), torch.cos(torch.deg2rad(a)), r], dim=-1)
            rows.append(T)
            cc, ccat = embeddings["c_crossattn"][k], embeddings["c_concat"][k]
            clip_emb = model.cc_projection(torch.cat([cc.repeat(B, 1, 1), T[:, None, :]], dim=-1))
            cond = {"c_crossattn": [torch.cat([torch.zeros_like(clip_emb), clip_emb], dim=0)],
                    "c_concat": [torch.cat([torch.zeros_like(ccat).repeat(B, 1, 1, 1), ccat.repeat(B, 1, 1, 1)], dim=0)]}
            pred = model.apply_model(x_in, t_in, cond)
            preds.append(pred)
            u, cnd = pred.chunk(2)
            acc = acc + ws[:, k].reshape(B, 1, 1, 1) * (u + guidance_scale * (cnd - u))
        e = acc / ws.sum(dim=-1).reshape(B, 1, 1, 1)
        grad = torch.nan_to_num((scale * (1 - alphas.to(dt).to(dev)[t])).reshape(B, 1, 1, 1) * (e - noise))
    loss = 0.5 * F.mse_loss(latents, (latents - grad).detach(), reduction="sum") / B
    return dict(loss=loss, grad=grad, latents=latents, latents_noisy=noisy, noise_preds=torch.stack(preds), T=torch.stack(rows),
                angles=angles, scale=scale, ws=ws)


# ---- the cases' inputs -------------------------------------------------------------------------------------------------------
def case_inputs(name):
    """pred_rgb [B,C,size,size] in [0,1) (C = 4 with as_latent: a latent render), noise [B,4,h,h], the reference images
    [R,3,256,256] -- fp32 numpy, from the case's own seed"""
    c = CASES[name]
    rng = np.random.RandomState(9300 + sorted(CASES).index(name))
    h = 32 if c["as_latent"] else 256 // c["stride"]
    pred = rng.rand(c["B"], 4 if c["as_latent"] else 3, c["size"], c["size"]).astype(np.float32)
    noise = rng.randn(c["B"], 4, h, h).astype(np.float32)
    refs = rng.rand(c["R"], 3, 256, 256).astype(np.float32)
    return pred, noise, refs
