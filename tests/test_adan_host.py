"""Host side of the Adan step (no GPU): the float64 restatement tests/adan_oracle.py against the reference class's recorded results
(tests/golden/adan.npz), optim.FlatAdan's layout, checkpoint format and loud failures, FlatEMA over it, make_optimizer, and the
C ABI's declarations."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import adan_oracle as A
from tests import step_f64_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS, STEPS = 4, 6


def _oracle(s, dtype, c):
    return A.adan(s["before_p"], s["grads"], *(s["before_" + k] for k in A.KEYS), s["ss"], s["sd"], s["bc3s"], s["decay"], s["on"],
                  s["first"], c, dtype, betas=s["betas"], eps=s["eps"], no_prox=s["no_prox"])


def _scales(s):
    return A.scales(s["before_p"], s["grads"], *(s["before_" + k] for k in A.KEYS), s["ss"], s["sd"], s["on"], s["first"], s["c64"],
                    betas=s["betas"])


def test_golden_is_the_layout_the_issue_describes():
    G = A.golden()
    assert list(G["sizes"]) == [3, 5, 2, 7, 1, 257] and list(G["group_of"]) == [0, 0, 0, 1, 1, 1] and G["c32"].shape == (RUNS, STEPS)
    assert sorted(zip(G["no_prox"].tolist(), (G["c32"].max(1) < 1.0).tolist())) == [(False, False), (False, True), (True, False), (True, True)]
    for run in range(RUNS):
        c = G["c32"][run]
        assert bool((c == 1.0).all()) or bool((c < 0.5).all())                         # clipping never bites, or at every step
        assert [list(x) for x in G["steps_after"][run]] == [[t, t] for t in range(1, 7)]
        assert G["has_grad"][run, :, 1].tolist() == [False, True, False, False, False, False]      # tensor 1: step 2 only
        assert G["has_grad"][run, :, 4].tolist() == [False, False, False, True, True, True]        # tensor 4: from step 4 on
        assert G["seen_after"][run, :, 4].tolist() == [False, False, False, True, True, True]
        assert G["lrs"][run, 2, 1] == 1e-3 and G["lrs"][run, 3, 1] == 5e-4 and G["lrs"][run, 3, 0] == 5e-3
        g = np.abs(G["grads"][run][G["grads"][run] != 0])
        assert g.max() / g.min() > 1e4                                                  # gradient scales over several decades
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "adan.npz")) < 1 << 20


def test_float64_restatement_is_the_reference_class_in_float64():
    """the rule in float64 against ONE float64 step of the reference's class from the same fp32 state: within 64 double round-offs
    of the scales (the chain has fewer than 32 rounded operations); elements without a gradient exactly as they were"""
    worst = 0.0
    for run in range(RUNS):
        for step in range(STEPS):
            s = A.golden_step(run, step, round32=False)
            c = A.clip_factor(s["grads"], s["on"], s["max_grad_norm"], s["eps"], np.float64)
            assert abs(c - s["c64"]) <= 8 * 2.0 ** -53 * c
            for name, x, sc in zip(A.NAMES, _oracle(s, np.float64, c), _scales(s)):
                r = s["after64_" + name]
                assert np.array_equal(x[sc == 0], r[sc == 0]), (run, step, name)
                worst = max(worst, float((np.abs(x - r)[sc > 0] / sc[sc > 0]).max(initial=0.0)))      # (step 1: exp_avg_diff is all exact)
    print(f"float64 restatement: worst {worst / 2.0 ** -53:.2f} double round-offs")
    assert worst <= 64 * 2.0 ** -53


def test_fp32_restatement_is_as_close_to_float64_as_the_reference_class():
    """the rule in fp32 (every operator rounded, group values rounded as mh_adan_step rounds them) and the reference's own fp32
    step, both against the float64 step: the judgement the kernel faces (step_f64_oracle.judge)"""
    for run in range(RUNS):
        pool = {}
        for step in range(STEPS):
            s = A.golden_step(run, step, round32=True)
            c = A.clip_factor(s["grads"], s["on"], s["max_grad_norm"], s["eps"], np.float32)
            assert abs(float(c) - s["c64"]) <= A.U * s["c64"]                # one rounding
            for name, x, sc in zip(A.NAMES, _oracle(s, np.float32, c), _scales(s)):
                h, r32, r64, ss = pool.setdefault(name, ([], [], [], []))
                h.append(x), r32.append(s["after32_" + name]), r64.append(s["after64_" + name]), ss.append(sc)
        for name, v in pool.items():
            S.judge(*(torch.from_numpy(np.concatenate(a)) for a in v), f"Adan restatement in fp32, run {run}: {name}")


def test_oracle_leaves_skipped_elements_and_first_gradients_as_defined():
    n = 12
    st = A.state(n)
    g = A.grad(st, 0)
    on = np.arange(n) % 2 == 0
    first = np.arange(n) % 3 == 0
    ones = np.ones(n)
    out = A.adan(st["p"], g, st["m"], st["n"], st["d"], st["q"], 1e-2 * ones, 5e-3 * ones, 0.5 * ones, ones, on, first, 0.25, np.float32)
    before = (st["p"], g, st["m"], st["n"], st["d"], st["q"])
    for x, b in zip(out, before):
        assert np.array_equal(x[~on].view(np.int32), b[~on].view(np.int32))
    assert np.array_equal(out[1][on], g[on] * np.float32(0.25)) and np.array_equal(out[5][on], -out[1][on])
    f = on & first                                                                  # a first gradient: the difference is exactly 0
    assert np.array_equal(out[4][f], st["d"][f] * np.float32(A.BETAS[1]))
    sc = A.scales(*before, 1e-2 * ones, 5e-3 * ones, on, first, 0.25)
    live = on & (g != 0)
    for name, x in zip(A.NAMES, sc):            # (exp_avg_diff on a first gradient: only b2 |d|, the difference being exactly 0)
        assert bool((x[~on] == 0).all()) and bool((x[live & ~first] > 0).all()), name
        assert name == "exp_avg_diff" or bool((x[live] > 0).all()), name
    assert np.array_equal(sc[4][live & first], A.BETAS[1] * np.abs(st["d"][live & first].astype(np.float64)))


# --------------------------------------------------------------------------------------------------------------- optim.FlatAdan
def _params():
    G = A.golden()
    return [torch.nn.Parameter(torch.zeros(int(k))) for k in G["sizes"]]


def _groups(ps):
    return [{"name": "a", "params": ps[:3], "lr": 5e-3}, {"name": "b", "params": ps[3:], "lr": 1e-3}]


def test_flat_adan_layout_and_group_names():
    from morpheus_amd.optim import FlatAdan
    ps = _params()
    opt = FlatAdan(_groups(ps), eps=1e-8, weight_decay=2e-5, max_grad_norm=5.0, foreach=False)
    assert opt._seg_end == [12, 280] and opt.n == 280
    assert opt._kseg_end == [3, 8, 10, 12, 19, 20, 277, 280] and opt._kseg_param == [0, 1, 2, -1, 3, 4, 5, -1]
    assert [g["name"] for g in opt.param_groups] == ["a", "b"]
    assert ps[3].data_ptr() == opt.flat_p[12:].data_ptr() and ps[0].grad.data_ptr() == opt.bucket.flat.data_ptr()
    for buf in (opt.exp_avg, opt.exp_avg_sq, opt.exp_avg_diff, opt.neg_pre_grad):
        assert buf.shape == opt.flat_p.shape and float(buf.abs().max()) == 0.0
    sd = opt.state_dict()
    assert sd["state"] == {} and all("step" not in g for g in sd["param_groups"])     # lazily made state, no step before the first
    for g in sd["param_groups"]:
        assert g["betas"] == (0.98, 0.92, 0.99) and g["eps"] == 1e-8 and g["weight_decay"] == 2e-5 and g["max_grad_norm"] == 5.0
        assert g["no_prox"] is False and g["foreach"] is False
    assert float(opt.last_clip) == 1.0
    for g in opt.param_groups:                                                      # learning rates are mutated by group name
        if g["name"] == "b":
            g["lr"] = 7e-4
    assert opt.state_dict()["param_groups"][1]["lr"] == 7e-4


@pytest.mark.parametrize("run,step", [(0, 0), (1, 2), (2, 4), (3, 5)])
def test_state_dict_in_the_reference_format_loads_and_round_trips(run, step):
    """a state_dict built from the golden's arrays in the reference class's format: unseen parameters absent, `step` in the groups,
    every default key; loaded into the flat buffers and given back unchanged"""
    from morpheus_amd.optim import FlatAdan
    s = A.golden_step(run, step, False)
    sd = A.golden_state_dict(run, step)
    opt = FlatAdan(_groups(_params()), lr=1.0)
    opt.load_state_dict(sd)
    assert opt._seen == s["seen_before"].tolist()
    assert [g.get("step", 0) for g in opt.param_groups] == s["steps_before"].tolist()
    assert [g["lr"] for g in opt.param_groups] == s["lrs"].tolist() and opt.param_groups[0]["no_prox"] == s["no_prox"]
    el = s["element_tensor"]
    for key in A.KEYS:
        flat = torch.cat([getattr(opt, key)[o:o + k] for _, o, k in opt._views]).numpy()
        assert np.array_equal(flat.view(np.int32), s["before_" + key].view(np.int32)), key
        assert float(np.abs(flat[~s["seen_before"][el]]).max(initial=0.0)) == 0.0
    back = opt.state_dict()
    assert sorted(back["state"]) == sorted(sd["state"]) == [i for i in range(6) if s["seen_before"][i]]
    for i, st in sd["state"].items():
        assert sorted(back["state"][i]) == sorted(A.KEYS)
        assert all(torch.equal(back["state"][i][k], st[k]) for k in A.KEYS)
    for g, h in zip(back["param_groups"], sd["param_groups"]):
        assert g == h and (("step" in g) == (step > 0))
    opt.restart_opt()
    assert [g["step"] for g in opt.param_groups] == [0, 0]
    assert all(float(b.abs().max()) == 0.0 for b in (opt.exp_avg, opt.exp_avg_sq, opt.exp_avg_diff))


def test_flat_adan_fails_loudly():
    from morpheus_amd._lib import MorpheusHipError
    from morpheus_amd.optim import FlatAdan
    opt = FlatAdan(_groups(_params()))
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        opt.step()
    with pytest.raises(NotImplementedError, match="closure"):
        opt.step(lambda: 0.0)
    with pytest.raises(NotImplementedError, match="shared by all groups"):
        FlatAdan([{"params": [torch.nn.Parameter(torch.zeros(2))], "betas": (0.5, 0.9, 0.9)},
                  {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(NotImplementedError, match="shared by all groups"):
        FlatAdan([{"params": [torch.nn.Parameter(torch.zeros(2))], "no_prox": True}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(NotImplementedError, match="fp32"):
        FlatAdan([torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))])
    with pytest.raises(ValueError):
        FlatAdan([torch.nn.Parameter(torch.zeros(2))], max_grad_norm=-1.0)
    with pytest.raises(NotImplementedError, match="160 segments"):
        FlatAdan([torch.nn.Parameter(torch.zeros(1)) for _ in range(161)])


def test_flat_ema_over_flat_adan():
    from morpheus_amd.optim import FlatAdan, FlatEMA
    ps = _params()
    opt = FlatAdan(_groups(ps))
    ema = FlatEMA(opt, decay=0.9, parameters=[ps[5]] + ps[:5])
    with torch.no_grad():
        opt.flat_p.add_(1.0)
    ema.update()                                    # decay_1 = min(0.9, 2 / 11): shadow moves by 1 - 2 / 11 of the difference
    assert torch.allclose(ema.shadow[:3], torch.full((3,), 1.0 - 2.0 / 11.0))
    sd = ema.state_dict()
    assert [tuple(t.shape) for t in sd["shadow_params"]] == [(257,), (3,), (5,), (2,), (7,), (1,)]
    ema.store(), ema.copy_to()
    assert torch.equal(ps[0].detach(), ema.shadow[:3])
    ema.restore()
    assert float(ps[0].detach().min()) == 1.0


def test_make_optimizer_restates_get_optimizer():
    from morpheus_amd import harness
    from morpheus_amd.optim import FlatAdam, FlatAdan, FlatEMA, make_optimizer
    model = harness.build_model("b", "cpu")
    lr = model.config["train"]["lr"]
    cfg = {"train": dict(model.config["train"], optim="adan", ema_decay=0.95)}
    opt, ema = make_optimizer(cfg, model)
    assert type(opt) is FlatAdan and type(ema) is FlatEMA and ema.decay == 0.95
    names = [g["name"] for g in model.get_params_all(1.0)]
    assert [g["name"] for g in opt.param_groups] == names
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in model.get_params_all(5 * lr)]      # "Adan usually requires a larger LR"
    for g in opt.param_groups:
        assert (g["betas"], g["eps"], g["weight_decay"], g["max_grad_norm"], g["no_prox"], g["foreach"]) == \
            ((0.98, 0.92, 0.99), 1e-8, 2e-5, 5.0, False, False)
    assert [tuple(t.shape) for t in ema.state_dict()["shadow_params"]] == [tuple(p.shape) for p in model.parameters()]
    model = harness.build_model("b", "cpu")
    opt, ema = make_optimizer({"train": dict(model.config["train"], optim="adam", ema_decay=0.0)}, model)
    assert type(opt) is FlatAdam and ema is None
    assert opt.param_groups[0]["betas"] == (0.9, 0.99) and opt.param_groups[0]["eps"] == 1e-15
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in model.get_params_all(lr)]


# --------------------------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_adan_entry_points():
    from morpheus_amd import _lib, build
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "morpheus_hip.h")).read()
    raw = ctypes.CDLL(_lib.SO)
    for name in ("mh_adan_workspace_bytes", "mh_adan_step", "mh_adan_step_dev"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(raw, name), name
    assert lib.mh_abi_version() == 10
    assert "adan.hip" in build.SOURCES and build.FILE_FLAGS["adan.hip"] == ["-ffp-contract=off"]
    P, I32, I64, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert lib.mh_adan_workspace_bytes.restype is I64 and list(lib.mh_adan_workspace_bytes.argtypes) == []
    assert list(lib.mh_adan_step.argtypes) == [P] * 6 + [I64, I32] + [P] * 4 + [D] * 6 + [I32, P, P]
    assert list(lib.mh_adan_step_dev.argtypes) == [P] * 6 + [I64, I32] + [P] * 5 + [D] * 6 + [I32, P, P]
    # c, the sum of squares, the norm; a table of 160 segments (end, four floats, a flag); 512 double partial sums
    assert lib.mh_adan_workspace_bytes() == 16 + 160 * (8 + 4 * 4 + 4) + 512 * 8
    # host-validated arguments: no device, no launch
    assert lib.mh_adan_step(*([None] * 6), 0, 0, *([None] * 4), 0.98, 0.92, 0.99, 1e-8, 0.0, 0.0, 0, None, None) == 0      # empty bucket
    assert lib.mh_adan_step(*([None] * 6), 8, 1, *([None] * 4), 0.98, 0.92, 0.99, 1e-8, 0.0, 0.0, 0, None, None) == 1
    assert lib.mh_adan_step_dev(*([None] * 6), 8, 1, *([None] * 5), 0.98, 0.92, 0.99, 1e-8, 0.0, 0.0, 0, None, None) == 1
