"""Host: what the renderer and its samplers agree on without a GPU -- the PackedSamples record's field order, the one
`sample_packed` every packed sampler shares, the record staying out of `state_dict()`, `HotPathRenderer._prune_args` and the
frame layout of a render_rays call, case by case."""
import pytest
import torch

from morpheus_amd.estimator import OccGridEstimator
from morpheus_amd.occgrid import OccupancyGrid, PackedSamples, PackedSampling
from morpheus_amd.render import HotPathRenderer, PresetSampler, UniformSampler, frame_layout

BOX = [-1.01] * 3 + [1.01] * 3


def test_record_begins_with_the_sampling_tuple():
    assert PackedSamples._fields == ("ray_indices", "t_starts", "t_ends", "ray_start", "ray_cnt", "n_valid", "src_index", "xyz")
    ri, ts, te, rs, rc = (torch.full((2,), float(k)) for k in range(5))
    rec = PackedSamples(ri, ts, te, rs, rc)
    assert rec[:3] == (ri, ts, te) and rec[3] is rs and rec[4] is rc
    assert rec.n_valid is None and rec.src_index is None and rec.xyz is None
    assert isinstance(rec, tuple) and not isinstance(rec, torch.nn.Module)


def test_every_packed_sampler_has_the_one_sample_packed():
    """UniformSampler and the two grids run PackedSampling.sample_packed itself: no class has a copy of the jitter choice or the
    pruning step (its argument errors are tests/test_visibility_host.py::test_sampling_argument_rules)."""
    for cls in (UniformSampler, OccupancyGrid, OccGridEstimator):
        assert issubclass(cls, PackedSampling) and cls.sample_packed is PackedSampling.sample_packed, cls
        assert "sample_packed" not in vars(cls) and "_marcher" in vars(cls), cls
    smp = UniformSampler(8, 1.01)
    assert smp.last is None and smp.packed is None and smp.src_index is None and smp.n_valid is None
    assert smp.sample_capacity is None and smp.overflow is None and smp.fixed_jitter is None and not hasattr(smp, "xyz")
    j = torch.rand(5)
    assert UniformSampler(8, 1.01, j).fixed_jitter is j
    # the shared path checks the arguments before anything is marched: a CPU call gets as far as the class's own rules
    with pytest.raises(ValueError, match="density function is required"):
        smp.sample_packed(torch.zeros(2, 3), torch.ones(2, 3), early_stop_eps=1e-4)
    assert smp.last is None


def test_attributes_mirror_the_last_record_and_state_dict_does_not_carry_it():
    rec = PackedSamples(*(torch.zeros(3) for _ in range(5)), n_valid=torch.tensor(3), src_index=torch.arange(3))
    for grid in (OccupancyGrid(BOX, 4), OccGridEstimator(BOX, 4)):
        keys = set(grid.state_dict())
        assert keys == {"resolution", "aabbs", "occs", "binaries"}
        grid.last = rec
        assert grid.packed[0] is rec.ray_start and grid.packed[1] is rec.ray_cnt
        assert grid.src_index is rec.src_index and grid.n_valid is rec.n_valid
        assert set(grid.state_dict()) == keys and not list(grid.named_parameters()) and len(list(grid.named_buffers())) == 4
        with pytest.raises(AttributeError):
            grid.n_valid = None                     # not set piecemeal: they read `last`


def test_preset_sampler_record():
    ri = torch.tensor([0, 0, 2], dtype=torch.int32)
    ts, te = torch.tensor([0.1, 0.2, 0.3]), torch.tensor([0.2, 0.3, 0.4])
    smp = PresetSampler(ri, ts, te)
    rec = smp.sample_packed(torch.zeros(4, 3), torch.ones(4, 3), stratified=True)
    assert rec[0] is ri and rec[1] is ts and rec[2] is te and smp.sampling(None, None) == (ri, ts, te)
    assert rec.ray_start.tolist() == [0, 2, 2, 3] and rec.ray_cnt.tolist() == [2, 0, 1, 0]
    assert rec.ray_start.dtype == rec.ray_cnt.dtype == torch.int32 and rec.n_valid is None and rec.xyz is None


def test_prune_args():
    rend = HotPathRenderer(None, {}, None, 1)
    assert rend._prune_args() is None
    rend.prune = {}
    assert rend._prune_args() is None
    rend.prune = dict(early_stop_eps=1e-3)
    assert rend._prune_args() == dict(alpha_thre=0.0, early_stop_eps=1e-3)
    rend.prune = dict(alpha_thre=1, early_stop_eps=0)
    args = rend._prune_args()
    assert args == dict(alpha_thre=1.0, early_stop_eps=0.0) and all(isinstance(v, float) for v in args.values())
    rend.prune = dict(early_stop_eps=1e-3, alpha=0.1, thre=2)
    with pytest.raises(ValueError) as e:
        rend._prune_args()
    assert str(e.value) == "HotPathRenderer.prune: unknown keys ['alpha', 'thre'] (alpha_thre, early_stop_eps)"


N_ = 5
B_ = 3
#          prefix     cano   frame_batched   single_frame  per-row slots  one_t
LAYOUTS = [((1, N_),  False, True,           True,         False,         True),
           ((1, N_),  True,  True,           False,        False,         True),      # one_t ignores cano: the smoothness loss warps always
           ((1, N_),  False, False,          False,        False,         False),
           ((1, N_),  True,  False,          False,        False,         False),
           ((B_, N_), False, True,           False,        True,          False),
           ((B_, N_), True,  True,           False,        False,         False),     # a canonical render reads no frame's deform code
           ((B_, N_), False, False,          False,        False,         False),
           ((B_, N_), True,  False,          False,        False,         False),
           ((N_,),    False, True,           False,        False,         False),
           ((N_,),    True,  True,           False,        False,         False),
           ((N_,),    False, False,          False,        False,         False),
           ((N_,),    True,  False,          False,        False,         False)]


@pytest.mark.parametrize("prefix,cano,frame_batched,single_frame,slots,one_t", LAYOUTS)
def test_frame_layout(prefix, cano, frame_batched, single_frame, slots, one_t):
    n = 1
    for p in prefix:
        n *= p
    rays_t = (torch.arange(n, dtype=torch.float32) // prefix[-1] * 0.25 + 0.125).view(-1, 1)      # one time per batch row
    lay = frame_layout(torch.Size(prefix), frame_batched, cano, rays_t)
    assert (lay.single_frame, lay.ray_slots is not None, lay.one_t) == (single_frame, slots, one_t)
    assert type(lay.single_frame) is bool and type(lay.one_t) is bool
    if slots:
        t_rows, slot_ray = lay.ray_slots
        assert t_rows.tolist() == [0.125, 0.375, 0.625] and t_rows.is_contiguous()
        assert slot_ray.dtype == torch.int32 and slot_ray.tolist() == [0] * N_ + [1] * N_ + [2] * N_
