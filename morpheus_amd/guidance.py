"""The Zero-1-to-3 SDS guidance with everything around its three networks on HIP kernels (csrc/guidance.hip, csrc/imageops.hip).

SDSGuidance stands where models/guidance/zero123_utils.py:Zero123 stands: the same methods and results, driven by the CALLER's
`ldm` model object (encode_first_stage, get_first_stage_encoding, get_learned_conditioning, cc_projection, apply_model -- called
exactly as :199-202 and :289 call them).  The UNet, the VAE and CLIP stay on stock PyTorch; the resize of the render, the view
arithmetic, add_noise, the classifier-free combination, the weights, nan_to_num and the loss are five launches (the resize's
backward is a sixth), and the host reads nothing from the device (the reference's `a[a > 180] -= 360`, its Python angle loop and
`rays_id[0,0,0].cpu()` all do).

EmbeddingBank / virtual_view_loss are get_embeddings' dict and get_virtual_view_loss ('cur_or_one', morpheus.py:1044-1088) with
the keyframe chosen on the device; as_step_guidance adapts the whole to bench_support.trainstep.VirtualViewTrainStep(guidance=...).
"""
from __future__ import annotations

import torch

from . import _lib, imageops
from ._lib import launch, ptr, require_gpu

MAX_REFS = 8          # mh_sds_max_refs()


def scaled_linear_alphas(num_train_timesteps: int, linear_start: float, linear_end: float):
    """alphas_cumprod of diffusers' `scaled_linear` schedule as recalled: betas = linspace(sqrt(start), sqrt(end), T) ** 2"""
    betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def _f32(x, device, n=None):
    t = torch.as_tensor(x, dtype=torch.float32).reshape(-1).to(device)
    if n is not None and t.numel() != n:
        raise ValueError(f"{n} values expected, got {t.numel()}")
    return t.contiguous()


def _views(polar, azimuth, radius):
    if not (polar.dim() == 1 and polar.shape == azimuth.shape == radius.shape):
        raise ValueError(f"polar, azimuth and radius [B] expected, got {tuple(polar.shape)}, {tuple(azimuth.shape)}, {tuple(radius.shape)}")
    return tuple(v.detach().float().contiguous() for v in (polar, azimuth, radius))


# ---- the three kernels ---------------------------------------------------------------------------------------------------------
@torch.no_grad()
def sds_view(polar, azimuth, radius, ref_polars, ref_azimuths, ref_radii, user_ws, grad_scale: float = 1.0):
    """mh_sds_view: the view deltas [B] (degrees, degrees, radius) against R reference views ->
    (T [R,B,4], angles [B,R] in degrees, scale [B], zero123_ws [B,R])"""
    polar, azimuth, radius = _views(polar, azimuth, radius)
    R = ref_polars.numel()
    if not 1 <= R <= MAX_REFS or not (ref_azimuths.numel() == ref_radii.numel() == user_ws.numel() == R):
        raise ValueError(f"sds_view: 1 to {MAX_REFS} reference views with one polar, azimuth, radius and weight each expected, got "
                         f"{R}, {ref_azimuths.numel()}, {ref_radii.numel()}, {user_ws.numel()}")
    require_gpu(polar, azimuth, radius, ref_polars, ref_azimuths, ref_radii, user_ws)
    B, dev = polar.shape[0], polar.device
    T, angles = torch.empty(R, B, 4, device=dev), torch.empty(B, R, device=dev)
    scale, ws = torch.empty(B, device=dev), torch.empty(B, R, device=dev)
    launch("mh_sds_view", ptr(polar), ptr(azimuth), ptr(radius), B, ptr(ref_polars), ptr(ref_azimuths), ptr(ref_radii), ptr(user_ws),
           R, float(grad_scale), ptr(T), ptr(angles), ptr(scale), ptr(ws))
    return T, angles, scale, ws


@torch.no_grad()
def sds_view_bank(polar, azimuth, radius, frame_id, kf_index, ref_polars, ref_azimuths, ref_radii, user_ws, target: bool,
                  grad_scale: float = 1.0):
    """mh_sds_view_bank: frame_id int64 (device, its first element is read) against the bank's keyframes kf_index int64 [K] ->
    (chosen int64 [1], T [1,B,4], angles [B,1], scale [B], zero123_ws [B,1])"""
    polar, azimuth, radius = _views(polar, azimuth, radius)
    K = kf_index.numel()
    if K < 1 or kf_index.dtype != torch.int64 or frame_id.dtype != torch.int64 or frame_id.numel() < 1 or \
            not (ref_polars.numel() == ref_azimuths.numel() == ref_radii.numel() == user_ws.numel() == K):
        raise ValueError(f"sds_view_bank: int64 frame_id and kf_index [K >= 1] with one view and weight per keyframe expected, got "
                         f"{frame_id.dtype}, {kf_index.dtype} [{K}], {ref_polars.numel()} views")
    require_gpu(polar, azimuth, radius, frame_id, kf_index, ref_polars, ref_azimuths, ref_radii, user_ws)
    B, dev = polar.shape[0], polar.device
    chosen = torch.empty(1, dtype=torch.int64, device=dev)
    T, angles = torch.empty(1, B, 4, device=dev), torch.empty(B, 1, device=dev)
    scale, ws = torch.empty(B, device=dev), torch.empty(B, 1, device=dev)
    # frame_id: the address of its first element (rays_id [1,N,1] need not be contiguous for that)
    launch("mh_sds_view_bank", ptr(polar), ptr(azimuth), ptr(radius), B, frame_id.data_ptr(), ptr(kf_index), K, ptr(ref_polars),
           ptr(ref_azimuths), ptr(ref_radii), ptr(user_ws), int(bool(target)), float(grad_scale), ptr(chosen), ptr(T), ptr(angles),
           ptr(scale), ptr(ws))
    return chosen, T, angles, scale, ws


def _latent_rows(latents, noise, t):
    if latents.dim() < 2 or latents.shape != noise.shape or latents.dtype != torch.float32 or noise.dtype != torch.float32:
        raise ValueError(f"float32 latents and noise of one shape [B, ...] expected, got {latents.dtype} {tuple(latents.shape)}, "
                         f"{noise.dtype} {tuple(noise.shape)}")
    B = latents.shape[0]
    if t.dtype != torch.int64 or tuple(t.shape) != (B,):
        raise ValueError(f"t: int64 [{B}] expected, got {t.dtype} {tuple(t.shape)}")
    return B, latents[0].numel()


@torch.no_grad()
def sds_noise(latents, noise, t, alphas_cumprod):
    """mh_sds_noise: -> x_in [2B, ...] = sqrt(a_t) latents + sqrt(1 - a_t) noise, twice (the two halves the UNet is fed)"""
    B, n = _latent_rows(latents, noise, t)
    require_gpu(latents, noise, t, alphas_cumprod)
    lat, noi = latents.detach().contiguous(), noise.contiguous()
    x_in = torch.empty((2 * B,) + tuple(latents.shape[1:]), device=latents.device)
    launch("mh_sds_noise", ptr(lat), ptr(noi), ptr(t.contiguous()), ptr(alphas_cumprod), alphas_cumprod.numel(), B, n, ptr(x_in))
    return x_in


_SCRATCH = {}


def _grad_scratch(device):
    """per device: the float64 partials and the zeroed ticket of mh_sds_grad (every call leaves the ticket at zero)"""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _SCRATCH:
        _SCRATCH[key] = (torch.empty(int(_lib.load().mh_sds_grad_blocks()), dtype=torch.float64, device=device),
                         torch.zeros(1, dtype=torch.int32, device=device))
    return _SCRATCH[key]


@torch.no_grad()
def sds_grad(noise_preds, ws, noise, t, alphas_cumprod, scale, guidance_scale: float):
    """mh_sds_grad: noise_preds [R,2B,...] (unconditional half first), ws [B,R], noise [B,...], scale [B] ->
    (grad [B,...], loss 0-dim = 0.5 sum grad^2 / B)"""
    B, n = _latent_rows(noise, noise, t)
    if noise_preds.dim() < 3 or noise_preds.dtype != torch.float32 or tuple(noise_preds.shape[1:]) != (2 * B,) + tuple(noise.shape[1:]):
        raise ValueError(f"sds_grad: float32 noise_preds [R,{2 * B},...] beside noise {tuple(noise.shape)} expected, got "
                         f"{noise_preds.dtype} {tuple(noise_preds.shape)}")
    R = noise_preds.shape[0]
    if not 1 <= R <= MAX_REFS or tuple(ws.shape) != (B, R) or tuple(scale.shape) != (B,):
        raise ValueError(f"sds_grad: 1 to {MAX_REFS} references, ws [{B},{R}] and scale [{B}] expected, got {R}, {tuple(ws.shape)}, "
                         f"{tuple(scale.shape)}")
    require_gpu(noise_preds, ws, noise, t, alphas_cumprod, scale)
    grad = torch.empty_like(noise, memory_format=torch.contiguous_format)
    loss = torch.empty(1, device=noise.device)
    partials, ticket = _grad_scratch(noise.device)
    launch("mh_sds_grad", ptr(noise_preds.contiguous()), ptr(ws.float().contiguous()), ptr(noise.contiguous()), ptr(t.contiguous()),
           ptr(alphas_cumprod), alphas_cumprod.numel(), ptr(scale.float().contiguous()), float(guidance_scale), R, B, n, ptr(grad),
           ptr(partials), ptr(ticket), ptr(loss))
    return grad, loss[0]


class _SDSLoss(torch.autograd.Function):
    """loss = 0.5 sum grad^2 / B as a function of the latents with d loss / d latents = grad / B: in exact arithmetic the
    reference's 0.5 * mse(latents, (latents - grad).detach(), 'sum') / B (:233-234)"""

    @staticmethod
    def forward(ctx, latents, grad, loss):
        ctx.save_for_backward(grad)
        ctx.B = latents.shape[0]
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return grad * (g / ctx.B), None, None


# ---- the class -----------------------------------------------------------------------------------------------------------------
class SDSGuidance(torch.nn.Module):
    """models/guidance/zero123_utils.py:Zero123 around the caller's `model`"""

    def __init__(self, model, device, fp16: bool = False, t_range=(0.02, 0.98), num_train_timesteps: int = 1000,
                 linear_start: float = 0.00085, linear_end: float = 0.0120):
        super().__init__()
        if fp16:
            raise NotImplementedError("SDSGuidance: fp16=True is not served (the reference itself runs the guidance in fp32)")
        self.device, self.fp16 = torch.device(device), False
        self.__dict__["model"] = model          # the caller's object, not registered: its parameters are not this module's
        self.num_train_timesteps = int(num_train_timesteps)
        self.update_t_range(list(t_range))
        self.alphas = scaled_linear_alphas(self.num_train_timesteps, linear_start, linear_end).to(self.device)
        self._refs = {}

    def update_t_range(self, t_range):
        self.t_range = t_range
        self.min_step = int(self.num_train_timesteps * t_range[0])
        self.max_step = int(self.num_train_timesteps * t_range[1])

    @torch.no_grad()
    def get_img_embeds(self, x):
        x = x * 2 - 1
        c = [self.model.get_learned_conditioning(xx.unsqueeze(0)) for xx in x]
        v = [self.model.encode_first_stage(xx.unsqueeze(0)).mode() for xx in x]
        return c, v

    def encode_imgs(self, imgs):
        return self._encode(imgs * 2 - 1)

    def _encode(self, imgs):
        """the latents of images already in [-1, 1] (:289)"""
        return torch.cat([self.model.get_first_stage_encoding(self.model.encode_first_stage(img.unsqueeze(0))) for img in imgs], dim=0)

    @torch.no_grad()
    def angle_between(self, sph_v1, sph_v2):
        """rows [r, theta, phi] in radians, [N1,3] and [N2,3] -> the angles [N1,N2] in radians (:102-120), on the device"""
        v1 = torch.as_tensor(sph_v1, dtype=torch.float32).to(self.device).reshape(-1, 3).contiguous()
        v2 = torch.as_tensor(sph_v2, dtype=torch.float32).to(self.device).reshape(-1, 3).contiguous()
        require_gpu(v1, v2)
        out = torch.empty(v1.shape[0], v2.shape[0], device=self.device)
        launch("mh_sds_angles", ptr(v1), v1.shape[0], ptr(v2), v2.shape[0], ptr(out))
        return out

    def _ref_views(self, embeddings):
        """the reference views and user weights of an embeddings dict on the device, moved once"""
        key = id(embeddings)
        hit = self._refs.get(key)
        if hit is None or hit[0] is not embeddings:
            R = len(embeddings["ref_azimuths"])
            if not 1 <= R <= MAX_REFS:
                raise ValueError(f"SDSGuidance: 1 to {MAX_REFS} reference views expected, got {R}")
            as_list = lambda k: [float(v) for v in embeddings[k]]
            hit = (embeddings,) + tuple(_f32(as_list(k), self.device, R) for k in ("ref_polars", "ref_azimuths", "ref_radii", "zero123_ws"))
            self._refs[key] = hit
        return hit[1:]

    @torch.no_grad()
    def get_angle_scale(self, embeddings, polar, azimuth, radius, grad_scale=1):
        return sds_view(polar, azimuth, radius, *self._ref_views(embeddings), grad_scale=grad_scale)[2]

    def train_step(self, embeddings, pred_rgb, polar, azimuth, radius, guidance_scale=3, as_latent=False, grad_scale=1,
                   save_guidance_path=None, t=None, last_grad_scale=None, noise=None, layout: str = "nchw"):
        """Zero123.train_step (:138-236) -> (loss, t, grad_scale, noise).  pred_rgb [B,3,H,W] in [0,1], or with layout="nhwc" the
        renderer's [B,H,W,3] (the permute of get_pred_from_outputs is then part of the resize)."""
        if save_guidance_path:
            raise NotImplementedError("SDSGuidance.train_step: save_guidance_path (the decoded debug images) is not served")
        view = sds_view(polar, azimuth, radius, *self._ref_views(embeddings), grad_scale=grad_scale)
        return self._step(view, embeddings["c_crossattn"], embeddings["c_concat"], pred_rgb, guidance_scale, as_latent, t, noise, layout)

    def _step(self, view, c_crossattn, c_concat, pred_rgb, guidance_scale, as_latent, t, noise, layout):
        T, _, scale, ws = view
        if as_latent:
            latents = imageops.resize_bilinear(pred_rgb, (32, 32), layout, mul=2.0, add=-1.0)
        else:
            latents = self._encode(imageops.resize_bilinear(pred_rgb, (256, 256), layout, mul=2.0, add=-1.0))
        B = latents.shape[0]
        if t is None:
            t = torch.randint(self.min_step, self.max_step + 1, (B,), dtype=torch.long, device=self.device)
        with torch.no_grad():
            if noise is None:
                noise = torch.randn_like(latents)
            lat = latents.detach().float()
            x_in = sds_noise(lat, noise, t, self.alphas)
            t_in = torch.cat([t] * 2)
            noise_preds = []
            for k, (cc, ccat) in enumerate(zip(c_crossattn, c_concat)):
                Tk = T[k][:, None, :]
                cond = {}
                clip_emb = self.model.cc_projection(torch.cat([cc.repeat(B, 1, 1), Tk], dim=-1))
                cond["c_crossattn"] = [torch.cat([torch.zeros_like(clip_emb), clip_emb], dim=0)]
                cond["c_concat"] = [torch.cat([torch.zeros_like(ccat).repeat(B, 1, 1, 1), ccat.repeat(B, 1, 1, 1)], dim=0)]
                noise_preds.append(self.model.apply_model(x_in, t_in, cond))
            stacked = noise_preds[0][None] if len(noise_preds) == 1 else torch.stack(noise_preds)
            grad, loss = sds_grad(stacked.float(), ws, noise, t, self.alphas, scale, guidance_scale)
        return _SDSLoss.apply(latents, grad, loss), t, scale, noise


# ---- the keyframe bank and the virtual-view loss ------------------------------------------------------------------------------
def get_kf(num_frames: int, kf_every: int):
    """morpheus.py:204-216: every kf_every-th frame and the last one"""
    frame_idx = torch.arange(0, num_frames, kf_every).long()
    if (num_frames - 1) not in frame_idx:
        frame_idx = torch.cat([frame_idx, torch.tensor([num_frames - 1])])
    return frame_idx


def prepare_embedding_image(image, mask):
    """morpheus.py:254-260: the frame [H,W,3] on white through its thresholded mask [H,W], area-resized -> [1,3,256,256]"""
    return imageops.masked_area_resize(image, mask, (256, 256))


class EmbeddingBank:
    """get_embeddings' dict {frame: embedding dict with ONE reference view} stacked along the keyframes, on the device:
    kf_index int64 [K], c_crossattn [K,...], c_concat [K,...], ref_polars / ref_azimuths / ref_radii / zero123_ws fp32 [K]"""

    def __init__(self, kf_index, c_crossattn, c_concat, ref_polars, ref_azimuths, ref_radii, zero123_ws):
        self.kf_index, self.c_crossattn, self.c_concat = kf_index, c_crossattn, c_concat
        self.ref_polars, self.ref_azimuths, self.ref_radii, self.zero123_ws = ref_polars, ref_azimuths, ref_radii, zero123_ws

    @classmethod
    def from_embeddings(cls, embeddings, embedding_idx, device=None):
        frames = [int(i) for i in embedding_idx]
        if not frames:
            raise ValueError("EmbeddingBank: no keyframes")
        for f in frames:
            if len(embeddings[f]["ref_azimuths"]) != 1:
                raise ValueError(f"EmbeddingBank: one reference view per keyframe expected, frame {f} has {len(embeddings[f]['ref_azimuths'])}")
        device = torch.device(device) if device is not None else embeddings[frames[0]]["c_crossattn"][0].device
        col = lambda k: _f32([float(embeddings[f][k][0]) for f in frames], device)
        return cls(torch.tensor(frames, dtype=torch.int64, device=device),
                   torch.stack([embeddings[f]["c_crossattn"][0] for f in frames]).to(device),
                   torch.stack([embeddings[f]["c_concat"][0] for f in frames]).to(device),
                   col("ref_polars"), col("ref_azimuths"), col("ref_radii"), col("zero123_ws"))


def virtual_view_loss(guidance: SDSGuidance, bank: EmbeddingBank, pred, polar, azimuth, radius, rays_id, rng, guidance_scale=3,
                      grad_scale=1, t=None, noise=None, layout: str = "nchw", as_latent: bool = False):
    """get_nearest_frame + get_virtual_view_loss with 'cur_or_one' (morpheus.py:1031-1088): the coin from the host `rng.random()`
    as in the reference; the frame id is read from rays_id ON the device (its first element), the nearest keyframe is chosen
    there and its embeddings are index_select-ed.  -> the loss"""
    target = not rng.random() > 0.5
    chosen, *view = sds_view_bank(polar, azimuth, radius, rays_id, bank.kf_index, bank.ref_polars, bank.ref_azimuths, bank.ref_radii,
                                  bank.zero123_ws, target, grad_scale)
    cc = bank.c_crossattn.index_select(0, chosen)[0]
    ccat = bank.c_concat.index_select(0, chosen)[0]
    return guidance._step(tuple(view), [cc], [ccat], pred, guidance_scale, as_latent, t, noise, layout)[0]


class _StepGuidance:
    """pred_rgb [1,3,H,W] -> loss, with the H / W attributes VirtualViewTrainStep asks its guidance for"""

    def __init__(self, fn, H, W):
        self.fn, self.H, self.W = fn, int(H), int(W)

    def __call__(self, pred_rgb):
        return self.fn(pred_rgb)


def as_step_guidance(guidance: SDSGuidance, embeddings, polar, azimuth, radius, H: int, W: int, guidance_scale=3, grad_scale=1,
                     t=None, noise=None, rays_id=None, rng=None):
    """A callable pred_rgb -> loss for bench_support.trainstep.VirtualViewTrainStep(guidance=...): train_step on an embeddings
    dict, or virtual_view_loss on an EmbeddingBank (then rays_id and rng are required)"""
    if isinstance(embeddings, EmbeddingBank):
        if rays_id is None or rng is None:
            raise ValueError("as_step_guidance: an EmbeddingBank needs rays_id and rng")
        return _StepGuidance(lambda pred: virtual_view_loss(guidance, embeddings, pred, polar, azimuth, radius, rays_id, rng,
                                                            guidance_scale, grad_scale, t, noise), H, W)
    return _StepGuidance(lambda pred: guidance.train_step(embeddings, pred, polar, azimuth, radius, guidance_scale=guidance_scale,
                                                          grad_scale=grad_scale, t=t, noise=noise)[0], H, W)
