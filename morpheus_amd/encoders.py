"""The reference's encoder factory (models/encodings.py:59-91) over this package's kernels.

`get_encoder` hands out, under the reference's names and with its defaults, the frequency encoding ('frequency': csrc/encoders.hip;
'frequency_torch': plain torch), the real spherical harmonics ('sphere_harmonics': csrc/encoders.hip) and the multiresolution grid
('hashgrid' / 'tiledgrid': model.GridEncoder), so that a head built on the reference's factory moves over by changing one import.
The HIP encoders have no CPU path: a CPU tensor raises MorpheusHipError.  `FreqEncoderTorch` works wherever torch does.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops


class FreqEncoder(nn.Module):
    """external/encoders/freqencoder/freq.py:55-77 on mh_freq_encode_*: [..., input_dim] -> [..., input_dim + 2 input_dim degree].
    `max_level` is FreqEncoder_torch's progressive mask (encodings.py:35-57), which the reference's CUDA encoder ignores: None
    keeps every band, otherwise the first int(max_level * degree) bands are computed and the rest is zero."""

    def __init__(self, input_dim=3, degree=4):
        super().__init__()
        self.input_dim = input_dim
        self.degree = degree
        self.output_dim = input_dim + input_dim * 2 * degree

    def __repr__(self):
        return f"FreqEncoder: input_dim={self.input_dim} degree={self.degree} output_dim={self.output_dim}"

    def forward(self, inputs, max_level=None, **kwargs):
        n_keep = self.degree if max_level is None else max(0, min(self.degree, int(max_level * self.degree)))
        prefix_shape = list(inputs.shape[:-1])
        outputs = ops.freq_encode(inputs.reshape(-1, self.input_dim), self.degree, n_keep)
        return outputs.reshape(prefix_shape + [self.output_dim])


class SHEncoder(nn.Module):
    """external/encoders/shencoder/sphere_harmonics.py:61-87 on mh_sh_encode_*: [..., 3] -> [..., degree^2]."""

    def __init__(self, input_dim=3, degree=4):
        super().__init__()
        self.input_dim = input_dim
        self.degree = degree
        self.output_dim = degree ** 2
        assert self.input_dim == 3, "SH encoder only support input dim == 3"
        assert self.degree > 0 and self.degree <= 8, "SH encoder only supports degree in [1, 8]"

    def __repr__(self):
        return f"SHEncoder: input_dim={self.input_dim} degree={self.degree}"

    def forward(self, inputs, size=1):
        inputs = inputs / size
        prefix_shape = list(inputs.shape[:-1])
        outputs = ops.sh_encode(inputs.reshape(-1, self.input_dim), self.degree)
        return outputs.reshape(prefix_shape + [self.output_dim])


class FreqEncoderTorch(nn.Module):
    """FreqEncoder_torch (encodings.py:10-57) in plain torch, constructor and all; what 'frequency_torch' returns."""

    def __init__(self, input_dim, max_freq_log2, N_freqs, log_sampling=True, include_input=True,
                 periodic_fns=(torch.sin, torch.cos)):
        super().__init__()
        self.input_dim = input_dim
        self.include_input = include_input
        self.periodic_fns = periodic_fns
        self.N_freqs = N_freqs
        self.output_dim = (self.input_dim if include_input else 0) + self.input_dim * N_freqs * len(periodic_fns)
        if log_sampling:
            bands = 2 ** torch.linspace(0, max_freq_log2, N_freqs)
        else:
            bands = torch.linspace(2 ** 0, 2 ** max_freq_log2, N_freqs)
        self.freq_bands = bands.numpy().tolist()

    def forward(self, input, max_level=None, **kwargs):
        keep = self.N_freqs if max_level is None else int(max_level * self.N_freqs)
        out = [input] if self.include_input else []
        for freq in self.freq_bands[:keep]:
            out += [fn(input * freq) for fn in self.periodic_fns]
        if self.N_freqs - keep > 0:
            out.append(input.new_zeros(*input.shape[:-1], (self.N_freqs - keep) * len(self.periodic_fns) * input.shape[-1]))
        return torch.cat(out, dim=-1)


def get_encoder(encoding, input_dim=3, multires=6, degree=4, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                desired_resolution=2048, align_corners=False, interpolation='linear', **kwargs):
    """-> (encoder, output_dim), the reference's factory with its names and defaults (encodings.py:59-91).  The grid names pass
    every geometry argument explicitly: model.GridEncoder's own defaults are this project's scene geometry, not the factory's."""
    if encoding == 'None':
        return lambda x, **kwargs: x, input_dim
    elif encoding == 'frequency_torch':
        encoder = FreqEncoderTorch(input_dim=input_dim, max_freq_log2=multires - 1, N_freqs=multires, log_sampling=True)
    elif encoding == 'frequency':
        encoder = FreqEncoder(input_dim=input_dim, degree=multires)
    elif encoding == 'sphere_harmonics':
        encoder = SHEncoder(input_dim=input_dim, degree=degree)
    elif encoding in ('hashgrid', 'tiledgrid'):
        from .model import GridEncoder
        encoder = GridEncoder(input_dim=input_dim, num_levels=num_levels, level_dim=level_dim, base_resolution=base_resolution,
                              log2_hashmap_size=log2_hashmap_size, desired_resolution=desired_resolution, per_level_scale=None,
                              gridtype='hash' if encoding == 'hashgrid' else 'tiled', align_corners=align_corners,
                              interpolation=interpolation)
    else:
        raise NotImplementedError('Unknown encoding mode, choose from [None, frequency, sphere_harmonics, hashgrid, tiledgrid]')
    return encoder, encoder.output_dim
