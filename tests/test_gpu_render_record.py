"""GPU: the PackedSamples record between the samplers and HotPathRenderer -- `sample_packed` against `sampling` and the
attributes that mirror the record for every packed sampler, a sampler that has nothing but `.sampling` (int64 indices) against
PresetSampler and against the grid its samples came from, and a renderer that leaves its sampler as `sampling()` left it.

Shapes: 2 frames of 35 rays (70: no multiple of the 4 rays of a marcher block, nor of 64; two frames take the per-row slots)
or one frame of 67 rays; a 16^3 grid with about 40 % of its cells occupied from a fixed seed at step 0.05 -- up to about 70
steps a ray, more than one 64-lane trip."""
import pytest
import torch

from morpheus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOX = [-1.01] * 3 + [1.01] * 3
STEP = 0.05


def _rays(frames, hw):
    """[B, n, .] rays of `frames`, n = hw[0] * hw[1] per frame (hw[2] where given: the first so many)"""
    rows = [synth.frame_rays(f, hw[0], hw[1]) for f in frames]
    n = hw[2] if len(hw) == 3 else hw[0] * hw[1]
    return tuple(torch.cat([r[k][:, :n] for r in rows], 0).contiguous().to(DEV) for k in range(4))


def _binary():
    return torch.rand(16, 16, 16, generator=torch.Generator().manual_seed(16)) < 0.4


def _grid(cls=None, **attrs):
    from morpheus_amd.occgrid import OccupancyGrid
    grid = (cls or OccupancyGrid)(BOX, 16).to(DEV)
    grid.set_binary(_binary().to(DEV))
    grid.occs.copy_(_binary().reshape(-1).float())
    grid.fixed_jitter = 0.25
    for k, v in attrs.items():
        setattr(grid, k, v)
    return grid


def _dense(t_starts, t_ends, ray_indices):
    return torch.full_like(t_starts, 8.0)            # T = exp(-0.4 k): under early_stop_eps = 0.05 from a ray's 9th sample on, at steps of 0.05


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and torch.equal(a, b), what


SAMPLERS = ("grid", "grid-capacity-above", "grid-capacity-below", "grid-sigma_fn", "estimator-lattice", "estimator-dda", "uniform",
            "uniform-pruned")


@pytest.fixture(scope="module")
def marched():
    """the ragged total of the fixture grid on the 70 rays, which the two capacities are set around"""
    o, d = (x.view(-1, 3) for x in _rays((25, 90), (7, 5))[:2])
    total = int(_grid().sample_packed(o, d, render_step_size=STEP).ray_cnt.sum())
    assert total > 70 * 4
    return total


@pytest.mark.parametrize("name", SAMPLERS)
def test_record_and_attributes_agree(name, marched):
    """sample_packed(...) and a following sampling(...) with the same pinned jitter: the same three tensors, and `packed`,
    `src_index`, `n_valid` are the record's own fields after either call."""
    from morpheus_amd import ops
    from morpheus_amd.estimator import OccGridEstimator
    from morpheus_amd.render import UniformSampler
    o, d = (x.view(-1, 3) for x in _rays((25, 90), (7, 5))[:2])
    N = o.shape[0]
    kw = dict(render_step_size=STEP, stratified=True)
    pruned = name in ("grid-sigma_fn", "uniform-pruned")
    if pruned:
        kw.update(sigma_fn=_dense, early_stop_eps=0.05)
    capacity = dict([("grid-capacity-above", marched + 37), ("grid-capacity-below", marched - 37)]).get(name)
    if name.startswith("grid"):
        smp = _grid(sample_capacity=capacity)
    elif name.startswith("estimator"):
        smp = _grid(OccGridEstimator, traversal=name.split("-")[1])
    else:
        smp = UniformSampler(16, 1.01, synth.ray_jitter(N).to(DEV))
    rec = smp.sample_packed(o, d, **kw)
    assert smp.last is rec and smp.packed[0] is rec.ray_start and smp.packed[1] is rec.ray_cnt
    assert smp.src_index is rec.src_index and smp.n_valid is rec.n_valid
    # the record in itself
    assert rec.ray_indices.dtype == rec.ray_start.dtype == rec.ray_cnt.dtype == torch.int32
    assert rec.ray_start.shape == rec.ray_cnt.shape == (N,) and rec.t_starts.shape == rec.t_ends.shape == rec.ray_indices.shape
    total = int(rec.ray_cnt.sum())
    if capacity is None:
        assert rec.n_valid is None and rec.ray_indices.shape[0] == total and smp.overflow is None
        assert torch.equal(rec.ray_start, (torch.cumsum(rec.ray_cnt, 0) - rec.ray_cnt).to(torch.int32))
        assert torch.equal(rec.ray_indices, torch.repeat_interleave(torch.arange(N, device=DEV), rec.ray_cnt.long()).to(torch.int32))
    else:
        assert rec.ray_indices.shape[0] == capacity and rec.n_valid.dtype == torch.int32 and rec.n_valid.dim() == 0
        assert int(rec.n_valid) == min(marched, capacity) and int(smp.overflow) == (1 if capacity < marched else 0)
    assert (rec.src_index is not None) == pruned
    if pruned:
        assert rec.src_index.dtype == torch.int32 and rec.src_index.shape == rec.ray_indices.shape
        assert 0 < total < (marched if name.startswith("grid") else 16 * N)
        if name.startswith("grid"):      # steps of 0.05 at sigma = 8: the 9th sample of a ray is behind T = exp(-3.2) < 0.05
            assert int(rec.ray_cnt.max()) == 8
    assert (rec.xyz is not None) == name.startswith("uniform")
    if rec.xyz is not None:          # the kernel's own midpoints, after pruning the survivors': o + d (ts + te) / 2
        want = ops.sample_positions_nograd(o, d, rec.ray_indices, rec.t_starts, rec.t_ends)
        print(f"{name}: max |xyz - sample_positions| = {float((rec.xyz - want).abs().max()):.3g}")
        assert torch.equal(rec.xyz, want)
    # sampling() is the same call's first three fields, and leaves the same record behind
    got = smp.sampling(o, d, **kw)
    assert isinstance(got, tuple) and len(got) == 3 and smp.last is not rec
    for a, b, what in zip(got, rec[:3], ("ray_indices", "t_starts", "t_ends")):
        _same(a, b, what)
        assert a is getattr(smp.last, what)
    for what in ("ray_start", "ray_cnt", "n_valid", "src_index", "xyz"):
        _same(getattr(smp.last, what), getattr(rec, what), what)
    assert smp.packed[0] is smp.last.ray_start and smp.src_index is smp.last.src_index and smp.n_valid is smp.last.n_valid


class _OnlySampling:
    """a sampler from elsewhere: nothing but nerfacc's call, int64 indices"""

    def __init__(self, ray_indices, t_starts, t_ends):
        self._out = (ray_indices.long(), t_starts, t_ends)

    def sampling(self, rays_o, rays_d, **kw):
        return self._out


def _training_render(model, sampler, rays, hw):
    from morpheus_amd.render import HotPathRenderer
    o, d, t, rid = rays
    torch.manual_seed(11)
    model.zero_grad(set_to_none=True)
    res = HotPathRenderer(model, model.config, sampler, 200).render_rays(
        o, d, t, rid, hw[0], hw[1], ambient_ratio=1.0, shading="albedo_normal", real_view=False, cano=False)
    terms = [v for k, v in sorted(res.items()) if k != "loss_code" and (k.startswith("loss_") or k == "normal_reg")]
    assert len(terms) == 4 and "loss_code" in res and "normal_image" in res, sorted(res)
    ((res["image"] ** 2).mean() + res["normal_image"].mean() + (res["depth"] ** 2).mean() + sum(terms)).backward()
    return res, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


# the first layers behind the per-frame code bias: with several frames in a batch their gradients are float32 sums by atomics
FRAME_BIAS_GRADS = tuple(f"{net}.net.0.{w}" for net in ("deform_net", "topo_net") for w in ("bias", "weight_g", "weight_v")) + \
    tuple(f"deform_code.volumes.{k}" for k in range(3))


@pytest.mark.parametrize("frames,hw", [((25, 90), (7, 5)), ((25,), (9, 8, 67))], ids=["2x35", "1x67"])
def test_foreign_sampler_renders_as_preset_and_as_the_grid(frames, hw):
    """A training render (shading="albedo_normal", the regularisers of the shipped config and the two others that read the frame
    slots and the ranges: deform_smooth, normal_smooth_2d) through an object that has only `.sampling` and returns int64
    indices: every output torch.equal to PresetSampler on the same samples and to the OccupancyGrid render the samples were
    taken from, and the parameter gradients too.

    What keeps bitwise comparison honest, each measured on the parent commit as on this one by running ONE renderer twice:
      * no depth supervision here: sdf_loss / fs_loss are sums by one atomic per workgroup (csrc/normal.hip) and two identical
        runs give different last bits;
      * loss_code is compared as a value and left out of the backward: its three code samples meet in the same cells of
        deform_code.volumes by atomics (one run in two differed by 9.3e-10 on gradients of 4.2e-3);
      * deform_smooth_t / topo_smooth_t stay off: they warp at a random time per sample, a code gradient of thousands of atomics;
      * with two frames in the batch the nine FRAME_BIAS_GRADS are atomic sums as well (two identical runs: up to 3.3e-7 on
        gradients of 0.77, 8.9e-8 on 0.30): there the check is tests/test_gpu_render.py's for sums in another order, a relative
        norm of 1e-4, and torch.equal for the 48 other gradients; one frame: torch.equal for all."""
    from morpheus_amd import harness
    from morpheus_amd.render import PresetSampler
    rays = _rays(frames, hw)
    B, n = rays[0].shape[:2]
    assert (B, n) == (len(frames), 35 if B == 2 else 67)
    model = harness.build_model("b", DEV).train()
    model.config["render"]["step_size"] = STEP
    model.config["train"].update(deform_smooth=0.1, normal_smooth_2d=0.1)
    grid = _grid()
    res_g, g_g = _training_render(model, grid, rays, hw)
    ri, ts, te = (x.clone() for x in grid.last[:3])
    assert ri.dtype == torch.int32 and res_g["sdf"].shape[0] == ri.shape[0] > 4 * B * n
    res_p, g_p = _training_render(model, PresetSampler(ri, ts, te), rays, hw)
    foreign = _OnlySampling(ri, ts, te)
    res_f, g_f = _training_render(model, foreign, rays, hw)
    assert set(vars(foreign)) == {"_out"}
    assert len(g_g) >= 50 and set(FRAME_BIAS_GRADS) <= set(g_g)
    for tag, res, grads in (("preset", res_p, g_p), ("grid", res_g, g_g)):
        assert set(res) == set(res_f) and set(grads) == set(g_f), tag
        for k in res_f:
            assert torch.equal(res_f[k], res[k]), (tag, k)
        for k in g_f:
            if B > 1 and k in FRAME_BIAS_GRADS:
                rel = float((g_f[k] - grads[k]).norm() / grads[k].norm().clamp_min(1e-30))
                print(f"{tag} {k}: relative norm of the difference {rel:.3g}")
                assert rel <= 1e-4, (tag, k, rel)
            else:
                assert torch.equal(g_f[k], grads[k]), (tag, k)


def test_renderer_leaves_its_sampler_alone():
    """After a render through UniformSampler the sampler holds what its own sample_packed left -- nothing removed, nothing
    written by the renderer -- and a second render with the same jitter is the first one's bytes."""
    from morpheus_amd import harness
    from morpheus_amd.render import HotPathRenderer, UniformSampler
    o, d, t, rid = _rays((25,), (9, 8, 67))
    model = harness.build_model("b", DEV).eval()
    smp = UniformSampler(16, model.bound, synth.ray_jitter(67).to(DEV))
    smp.sampling(o[0], d[0])
    left = dict(vars(smp))
    assert left["last"].xyz is not None and left["last"].xyz.shape == (67 * 16, 3)
    rend = HotPathRenderer(model, model.config, smp, 200)
    with torch.no_grad():
        a = rend.render_rays(o, d, t, rid, 9, 8, shading="albedo")
        after = dict(vars(smp))
        assert set(after) == set(left)
        for k in left:
            if k != "last":
                assert after[k] is left[k], k
        assert type(after["last"]) is type(left["last"])
        for x, y, what in zip(after["last"], left["last"], left["last"]._fields):
            _same(x, y, what)
        xyz = after["last"].xyz.clone()
        b = rend.render_rays(o, d, t, rid, 9, 8, shading="albedo")
    assert torch.equal(smp.last.xyz, xyz) and a["sdf"].shape[0] == 67 * 16
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
