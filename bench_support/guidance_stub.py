"""A small deterministic stand-in for the `ldm` model that Zero-1-to-3's guidance drives (harness code, like the rest of
bench_support/): the five methods models/guidance/zero123_utils.py calls, on a few convolutions and linear layers, so that the
guidance shell -- everything AROUND the three networks -- can run, be recorded and be tested without the checkpoint.

    encode_first_stage(x [1,3,256,256])    -> a posterior with .mode(): one strided convolution, [1,4,256/stride,256/stride]
    get_first_stage_encoding(posterior)    -> scale_factor * posterior.mode()
    get_learned_conditioning(x)            -> [1,1,E]: 4 x 4 average pool, one linear layer
    cc_projection([.., E + 4])             -> [.., E]: the linear layer over (embedding, T)
    apply_model(x_in, t_in, cond)          -> the noise prediction: conv3x3(x_in | c_concat) + per-channel terms from c_crossattn
                                              and t, tanh, conv3x3

Nothing here reads from the device.  The weights are plain arrays (weights(), load_weights()); Scheduler is the piece of a DDIM
scheduler the guidance uses (alphas_cumprod, add_noise).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

EMBED = 16
HIDDEN = 8
LATENT = 4
SCALE_FACTOR = 0.18215


def scaled_linear_alphas(num_train_timesteps=1000, linear_start=0.00085, linear_end=0.0120, dtype=torch.float32):
    """alphas_cumprod of the `scaled_linear` beta schedule: betas = linspace(sqrt(start), sqrt(end), T) ** 2"""
    betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, num_train_timesteps, dtype=dtype) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


class Scheduler:
    """alphas_cumprod and add_noise, as the guidance uses its scheduler (zero123_utils.py:87, :180)"""

    def __init__(self, num_train_timesteps=1000, linear_start=0.00085, linear_end=0.0120, dtype=torch.float32):
        self.alphas_cumprod = scaled_linear_alphas(num_train_timesteps, linear_start, linear_end, dtype)

    def add_noise(self, original_samples, noise, timesteps):
        a = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)[timesteps]
        sa, s1 = (a ** 0.5).flatten(), ((1 - a) ** 0.5).flatten()
        while sa.dim() < original_samples.dim():
            sa, s1 = sa.unsqueeze(-1), s1.unsqueeze(-1)
        return sa * original_samples + s1 * noise


class _Posterior:
    def __init__(self, mean):
        self.mean = mean

    def mode(self):
        return self.mean

    def sample(self):
        return self.mean


class StubLDM(nn.Module):
    def __init__(self, stride: int = 8, seed: int = 7100):
        super().__init__()
        self.stride = int(stride)
        self.enc = nn.Conv2d(3, LATENT, self.stride, stride=self.stride)
        self.clip = nn.Linear(3 * 16, EMBED)
        self.cc_projection = nn.Linear(EMBED + 4, EMBED)
        self.conv_in = nn.Conv2d(2 * LATENT, HIDDEN, 3, padding=1)
        self.ctx = nn.Linear(EMBED, HIDDEN)
        self.time = nn.Linear(2, HIDDEN)
        self.conv_out = nn.Conv2d(HIDDEN, LATENT, 3, padding=1)
        rng = np.random.RandomState(seed)
        # weights: N(0, 1 / fan_in); biases: N(0, 0.1^2)
        self.load_weights({k: (rng.randn(*v.shape) * (float(np.prod(v.shape[1:])) ** -0.5 if v.dim() > 1 else 0.1)).astype(np.float32)
                           for k, v in self.state_dict().items()})
        self.eval()

    def weights(self):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.state_dict().items()}

    def load_weights(self, arrays):
        own = self.state_dict()
        self.load_state_dict({k: torch.as_tensor(np.asarray(arrays[k])).to(own[k]) for k in own})
        return self

    # ---- the five methods ------------------------------------------------------------------------------------------------
    def encode_first_stage(self, x):
        return _Posterior(self.enc(x))

    def get_first_stage_encoding(self, posterior):
        return SCALE_FACTOR * posterior.mode()

    def get_learned_conditioning(self, x):
        return self.clip(F.adaptive_avg_pool2d(x, 4).flatten(1))[:, None, :]

    def apply_model(self, x_noisy, t, cond):
        ctx, cat = cond["c_crossattn"][0], cond["c_concat"][0]
        h = self.conv_in(torch.cat([x_noisy, cat], dim=1))
        tt = t.to(x_noisy.dtype) / 1000.0
        bias = self.ctx(ctx[:, 0, :]) + self.time(torch.stack([torch.sin(6.0 * tt), torch.cos(6.0 * tt)], dim=-1))
        return self.conv_out(torch.tanh(h + bias[:, :, None, None]))
