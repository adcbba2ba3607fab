"""The guidance shell without a GPU: the float64 restatements (tests/guidance_oracle.py) against the reference's recorded float64 run
(tests/golden/guidance.npz, tools/make_guidance_golden.py), the keyframe rules, the refusals of the Python layer, the build tables."""
import os
import re

import numpy as np
import pytest
import torch

from tests import guidance_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "guidance.npz")
E = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_golden_holds_every_case(golden):
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    assert {c["R"] for c in G.CASES.values()} == {1, 3} and {c["B"] for c in G.CASES.values()} == {1, 2}
    assert {c["as_latent"] for c in G.CASES.values()} == {False, True} and {c["size"] for c in G.CASES.values()} == {36, 72}
    assert {t for c in G.CASES.values() for t in c["t"]} == {20, 500, 980}
    for name, c in G.CASES.items():
        pred, noise, _ = G.case_inputs(name)
        assert np.array_equal(golden[f"{name}_pred"], pred) and np.array_equal(golden[f"{name}_noise"], noise)
        assert golden[f"{name}_t"].tolist() == list(c["t"])
        h = noise.shape[-1]
        assert golden[f"{name}_noise_preds32"].shape == (c["R"], 2 * c["B"], 4, h, h)
        assert golden[f"{name}_dpred64"].shape == pred.shape and golden[f"{name}_dpred64"].dtype == np.float64
        for k in ("latents", "latents_noisy", "grad", "loss", "scale", "angles", "T", "ws"):
            assert golden[f"{name}_{k}32"].dtype == np.float32 and golden[f"{name}_{k}64"].dtype == np.float64, (name, k)
        assert golden[f"{name}_angles64"].min() >= 5.0
    r3 = golden["r3b2_ws64"]
    assert bool((r3 == 0).any())                                        # a reference whose weight fell below 0.1
    v = G.VIEWS["r3b2"]
    assert max(a + v["ref_azimuths"][0] - r for a in v["azimuth"] for r in v["ref_azimuths"]) > 180      # the wrap


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_reproduces_the_float64_records(golden, name):
    """the numpy chain in float64 against the reference's float64 run: the same statements, so a few double round-offs of each
    quantity's size; the angles pass through an arccos of condition 1 / sin(angle) <= 12 at 5 degrees, in degrees: 2^10 of them"""
    c, v = G.CASES[name], G.VIEWS[name]
    g = lambda k: golden[f"{name}_{k}64"]
    T, ang, scale, ws = G.view(v["polar"], v["azimuth"], v["radius"], v["ref_polars"], v["ref_azimuths"], v["ref_radii"],
                               v["zero123_ws"], G.GRAD_SCALE)
    assert np.abs(T - g("T")).max() <= 8 * E * max(1.0, np.abs(g("T")).max())
    assert np.abs(ang - g("angles")).max() <= 1024 * E * 180
    assert np.abs(scale - g("scale")).max() <= 1024 * E * max(1.0, g("scale").max())
    assert np.abs(ws - g("ws")).max() <= 64 * E
    noise, alphas = golden[f"{name}_noise"], golden["alphas"]
    x = G.add_noise(g("latents"), noise, c["t"], alphas)
    assert x.shape[0] == 2 * c["B"] and np.array_equal(x[:c["B"]], x[c["B"]:])
    assert np.abs(x[:c["B"]] - g("latents_noisy")).max() <= 8 * E * np.abs(g("latents_noisy")).max()
    grad, loss = G.grad_loss(g("noise_preds"), g("ws"), noise, c["t"], alphas, g("scale"), G.GUIDANCE_SCALE)
    assert np.abs(grad - g("grad")).max() <= 64 * E * np.abs(g("grad")).max()
    # the reference's loss is 0.5 sum (latents - (latents - grad))^2 / B: each term carries the rounding of latents - grad
    lat = np.abs(g("latents")).max()
    assert abs(loss - float(g("loss"))) <= 8 * E * (lat + np.abs(grad).max()) * np.abs(grad).sum() / c["B"]


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_torch_chain_reproduces_the_float64_records(golden, name):
    """train_step_torch in float64 on the CPU with the stub rebuilt from the recorded weights: loss and d loss / d pred_rgb"""
    from bench_support import guidance_stub as GS
    c, v = G.CASES[name], G.VIEWS[name]
    model = GS.StubLDM(stride=c["stride"]).load_weights({k[len(name) + 3:]: a for k, a in golden.items() if k.startswith(f"{name}_w_")}).double()
    emb = dict(c_crossattn=list(torch.from_numpy(golden[f"{name}_cc64"])), c_concat=list(torch.from_numpy(golden[f"{name}_cat64"])),
               **{k: list(v[k]) for k in ("ref_polars", "ref_azimuths", "ref_radii", "zero123_ws")})
    pred = torch.from_numpy(golden[f"{name}_pred"]).double().requires_grad_(True)
    col = lambda k: torch.tensor(np.asarray(v[k], np.float32)).double()
    out = G.train_step_torch(model, torch.from_numpy(golden["alphas"]), emb, pred, col("polar"), col("azimuth"), col("radius"),
                             G.GUIDANCE_SCALE, c["as_latent"], G.GRAD_SCALE, torch.tensor(c["t"]), torch.from_numpy(golden[f"{name}_noise"]).double())
    out["loss"].backward()
    want = float(golden[f"{name}_loss64"])
    assert abs(float(out["loss"].detach()) - want) <= 1e-12 * want
    d = golden[f"{name}_dpred64"]
    assert np.abs(pred.grad.numpy() - d).max() <= 1e-12 * np.abs(d).max()
    assert np.abs(out["noise_preds"].numpy() - golden[f"{name}_noise_preds64"]).max() <= 1e-12 * np.abs(golden[f"{name}_noise_preds64"]).max()


def test_keyframes():
    from morpheus_amd import guidance
    assert guidance.get_kf(10, 3).tolist() == [0, 3, 6, 9] and guidance.get_kf(10, 4).tolist() == [0, 4, 8, 9]
    assert guidance.get_kf(1, 2).tolist() == [0] and guidance.get_kf(5, 2).dtype == torch.int64
    kf = [0, 4, 8, 9]
    assert G.nearest_keyframe(4, kf) == 1 and G.nearest_keyframe(2, kf) == 0 and G.nearest_keyframe(6, kf) == 1      # hit, two ties
    assert G.nearest_keyframe(40, kf) == 3 and G.nearest_keyframe(5, kf) == 1
    p, a, r = G.retarget([10.0], [100.0], [0.5], [90.0, 80.0], [0.0, 120.0], [3.0, 3.5], 1)
    assert p.tolist() == [0.0] and a.tolist() == [-140.0] and r.tolist() == [1.0]


def test_alphas_schedule():
    from morpheus_amd import guidance
    a = guidance.scaled_linear_alphas(1000, 0.00085, 0.0120)
    assert a.dtype == torch.float32 and a.shape == (1000,) and bool((a[1:] < a[:-1]).all())
    assert abs(float(a[0]) - (1 - 0.00085)) < 1e-6 and 0.004 < float(a[-1]) < 0.005
    with np.load(GOLDEN) as z:
        assert np.array_equal(a.numpy(), z["alphas"])


def test_argument_checks_need_no_device():
    from morpheus_amd import guidance
    from morpheus_amd._lib import MorpheusHipError
    v = torch.zeros(2)
    r = lambda n: torch.ones(n)
    with pytest.raises(ValueError, match="polar, azimuth and radius"):
        guidance.sds_view(v, torch.zeros(3), v, r(1), r(1), r(1), r(1))
    with pytest.raises(ValueError, match="reference views"):
        guidance.sds_view(v, v, v, r(9), r(9), r(9), r(9))
    with pytest.raises(ValueError, match="reference views"):
        guidance.sds_view(v, v, v, r(2), r(2), r(1), r(2))
    with pytest.raises(ValueError, match="int64"):
        guidance.sds_view_bank(v, v, v, torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), r(2), r(2), r(2), r(2), False)
    lat, t = torch.zeros(2, 4, 8, 8), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="one shape"):
        guidance.sds_noise(lat, torch.zeros(2, 4, 8, 7), t, r(10))
    with pytest.raises(ValueError, match="int64"):
        guidance.sds_noise(lat, lat, t.int(), r(10))
    with pytest.raises(ValueError, match="noise_preds"):
        guidance.sds_grad(torch.zeros(1, 2, 4, 8, 8), r(2).reshape(2, 1), lat, t, r(10), r(2), 3.0)
    with pytest.raises(ValueError, match="ws"):
        guidance.sds_grad(torch.zeros(1, 4, 4, 8, 8), r(2).reshape(1, 2), lat, t, r(10), r(2), 3.0)
    with pytest.raises(NotImplementedError, match="fp16"):
        guidance.SDSGuidance(None, "cpu", fp16=True)
    g = guidance.SDSGuidance(None, "cpu")
    assert (g.min_step, g.max_step) == (20, 980)
    g.update_t_range([0.2, 0.5])
    assert (g.min_step, g.max_step) == (200, 500)
    emb = dict(ref_polars=[90.0], ref_azimuths=[0.0], ref_radii=[3.0], zero123_ws=[1], c_crossattn=[None], c_concat=[None])
    with pytest.raises(NotImplementedError, match="save_guidance_path"):
        g.train_step(emb, torch.zeros(1, 3, 8, 8), v[:1], v[:1], v[:1], save_guidance_path="x.png")
    with pytest.raises(ValueError, match="reference views"):
        g.train_step(dict(emb, ref_azimuths=[0.0] * 9), torch.zeros(1, 3, 8, 8), v[:1], v[:1], v[:1])
    with pytest.raises(ValueError, match="one reference view"):
        guidance.EmbeddingBank.from_embeddings({0: dict(emb, ref_azimuths=[0.0, 1.0])}, [0], device="cpu")
    with pytest.raises(ValueError, match="rays_id and rng"):
        guidance.as_step_guidance(g, guidance.EmbeddingBank(*[None] * 7), v, v, v, 8, 8)
    with pytest.raises(MorpheusHipError, match="MI355X"):             # valid arguments: the next thing asked for is the GPU
        guidance.sds_view(v, v, v, r(1), r(1), r(1), r(1))


def test_sources_and_entry_points():
    from morpheus_amd import _lib, build
    assert "guidance.hip" in build.SOURCES and "guidance.hip" not in build.FILE_FLAGS          # its own pragma, like sampler.hip
    src = open(os.path.join(build.CSRC, "guidance.hip")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "wave.h"' in src and "wave_sum(" in src
    hdr = open(os.path.join(ROOT, "include", "morpheus_hip.h")).read()
    for name in ("mh_sds_view", "mh_sds_view_bank", "mh_sds_angles", "mh_sds_noise", "mh_sds_grad", "mh_sds_max_refs", "mh_sds_grad_blocks"):
        assert len(re.findall(r"\b%s\s*\(" % name, hdr)) == 1 and name in _lib.EXPORTS, name
    lib = _lib.load()
    assert lib.mh_sds_max_refs() == 8 and lib.mh_sds_grad_blocks() == 256
    assert lib.mh_sds_view(*[None] * 3, 0, *[None] * 4, 1, 1.0, *[None] * 4, None) == 0          # no views: nothing to do
    assert lib.mh_sds_view(*[None] * 3, 2, *[None] * 4, 1, 1.0, *[None] * 4, None) == 1
    assert lib.mh_sds_noise(None, None, None, None, 10, 2, 16, None, None) == 1
    assert lib.mh_sds_grad(*[None] * 5, 10, None, 3.0, 9, 1, 16, *[None] * 4, None) == 1
