"""tests/glue_f64_oracle.py on the CPU: the conditions tests/test_gpu_glue_f64.py relies on.  Every case builder is run here and
shown to populate the branches it names, to hit its ties exactly in fp32, and to take the same decisions in fp32 and float64;
the oracle's expressions are checked against the project's restatements of the reference (oracle/field.py)."""
import pytest
import torch

from oracle import field as of
from tests import glue_f64_oracle as G

F32, F64 = torch.float32, torch.float64
SDF_SIZES = [1, 255, 256, 257, 32768, 33069]


def _d(t):
    return None if t is None else t.double()


# ---------------------------------------------------------------------------------------------------------------- taps
@pytest.mark.parametrize("eps", G.EPS_CASES)
def test_taps_case_places_the_clamp_edges(eps):
    c = G.taps_case(257, 2, eps)
    x, b = c["x"], torch.tensor(c["bound"], dtype=F32)
    v = x[:, None] + G.tap_offsets(eps)
    inside = G.taps_decisions(x, eps, c["bound"])
    assert c["n_placed"] == 42
    for sign in (1.0, -1.0):
        on = v == b * sign                                             # exact ties: the mask is decided AT the bound
        assert int((on[:, 0::2] if sign > 0 else on[:, 1::2]).any(-1).any(-1).sum()) >= 4
        assert bool(inside[on].all())                                  # the clamp passes its gradient at the bound itself
        for a in range(3):
            assert int(on[:, 2 * a + (0 if sign > 0 else 1), a].sum()) >= 1, "a +-eps tap lands exactly on the bound, per axis"
            assert int((x[:, a] == b * sign).sum()) >= 1, "a point exactly on the bound, per axis"
        ulp_out = v == torch.nextafter(b * sign, torch.tensor(float("inf") * sign))
        ulp_in = v == torch.nextafter(b * sign, torch.tensor(0.0))
        assert int(ulp_out.sum()) >= 4 and int(ulp_in.sum()) >= 4 and not bool(inside[ulp_out].any()) and bool(inside[ulp_in].all())
    assert int((~inside).any(-1).any(-1).sum()) >= 12 and int(inside.all(-1).all(-1).sum()) >= 100
    for a in range(3):                                                 # all six taps clamped on an axis: d/dx must be exactly 0 there
        assert int((~inside[:, :, a]).all(-1).sum()) >= 2
    # the decisions are the ones torch's own clamp takes in fp32: same taps, same gradient, bit for bit
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    t_plain, _ = G.taps(xa, None, eps, c["bound"])
    t_dec, _ = G.taps(xb, None, eps, c["bound"], inside)
    (t_plain * c["g_taps"]).sum().backward()
    (t_dec * c["g_taps"]).sum().backward()
    assert torch.equal(t_plain, t_dec) and torch.equal(xa.grad, xb.grad)
    # and they are NOT the ones a float64 evaluation would take: the reason the oracle takes them from fp32
    v64 = x.double()[:, None] + G.tap_offsets(eps).double()
    assert bool((((v64 >= -float(b)) & (v64 <= float(b))) != inside).any())


@pytest.mark.parametrize("M", [1, 42, 43, 255, 256, 257])
def test_taps_case_sizes(M):
    c = G.taps_case(M, 5, 2e-3)
    assert c["x"].shape == (M, 3) and c["topo"].shape == (M, 5) and c["g_taps"].shape == (6 * M, 3) and c["n_placed"] == min(M, 42)
    assert G.taps_case(M, None, 2e-3)["topo"] is None


# -------------------------------------------------------------------------------------------------------------- normal
@pytest.mark.parametrize("eps", G.EPS_CASES)
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_normal_case_straddles_the_clamp_without_a_flip(M, eps):
    c = G.normal_case(M, eps)
    s6, kind = c["s6"], c["kind"]
    clamped = G.normal_decisions(s6, eps)
    _, raw64 = G.normal(s6.double(), eps)
    ss64 = (raw64 * raw64).sum(-1)
    assert torch.equal(clamped, ss64 < G.f32_scalar(1e-20)), "the 1e-20 decision flips between fp32 and float64"
    assert bool(((ss64 / 1e-20 - 1).abs() > 0.5).all())               # nothing within rounding of the threshold
    _, raw32 = G.normal(s6, eps)
    assert torch.equal((raw32 * raw32).sum(-1) < 1e-20, clamped)      # torch's own fp32 chain decides alike
    if M >= 255:
        for k in range(7):
            assert int((kind == k).sum()) >= 4
        assert bool(clamped[(kind >= 1) & (kind <= 3)].all()) and not bool(clamped[(kind == 0) | (kind >= 4)].any())
        assert bool((raw64[kind == 1] == 0).all())                     # exactly flat
        assert bool((ss64[kind == 6].sqrt() > 30).all()) and float(ss64[kind == 6].sqrt().max()) > 900
        for k, sc in ((2, 0.25), (3, 0.5), (4, 2.0), (5, 4.0)):
            # |raw| = 1e-10 x scale x |u|, |u| in (1e-3, 1]
            assert float(ss64[kind == k].sqrt().max()) <= 1.001e-10 * sc and float(ss64[kind == k].sqrt().median()) > 0.9e-10 * sc
    # filter cap: finite in fp32 -> finite in float64, and (backward cases) nothing to filter at all
    s64 = s6.double().requires_grad_(True)
    n64, r64 = G.normal(s64, eps, clamped)
    ((n64 * c["g_n"].double()).sum() + (r64 * c["g_r"].double()).sum()).backward()
    s32 = s6.clone().requires_grad_(True)
    n32, r32 = G.normal(s32, eps)
    ((n32 * c["g_n"]).sum() + (r32 * c["g_r"]).sum()).backward()
    fin32 = torch.isfinite(s32.grad).all(-1)
    assert bool(torch.isfinite(s64.grad)[fin32].all())
    assert int((~fin32).sum()) * 64 <= M


def test_normal_nonfinite_case_has_every_kind():
    c = G.normal_nonfinite_case()
    s = c["s6"]
    assert int(torch.isnan(s).any(-1).sum()) == 6 and int((s == float("inf")).any(-1).sum()) == 6
    assert int((s == float("-inf")).any(-1).sum()) == 6 and int((~torch.isfinite(s)).any(-1).sum()) == 18
    n, _ = G.normal(s, c["eps"])
    assert bool(torch.isfinite(n).all())                               # nan_to_num: 0 or +-FLT_MAX only where it acted


# ----------------------------------------------------------------------------------------------------- sample positions
def test_positions_case_reaches_every_trip_count():
    c = G.positions_case()
    assert c["N"] == 13 and c["cnt"].tolist() == G.RAY_COUNTS and int(c["cnt"][0]) == 0 and int(c["cnt"][-1]) == 0
    assert c["N"] % 4 == 1                                             # the last block holds one ray and three idle waves
    trips = (c["cnt"] + 63) // 64
    assert sorted(set(trips.tolist())) == [0, 1, 2, 3, 4]
    assert torch.equal(torch.repeat_interleave(torch.arange(13), c["cnt"].long()).int(), c["ri"])
    assert bool((c["g"] > 0).any()) and bool((c["g"] < 0).any())
    # the one-line break `i += 128`: a lane then skips every second trip; rays above 64 samples lose terms of either sign
    g = c["g"].double()
    for r in range(13):
        n, s = int(c["cnt"][r]), int(c["start"][r])
        if n > 64:
            i = torch.arange(n)
            kept = (i // 64) % 2 == 0
            bound = ((n + 63) // 64 + 6) * G.U * g[s:s + n].abs().sum(0)          # what the GPU test allows the segment sum
            assert bool((g[s:s + n][~kept].sum(0).abs() > 10 * bound).all())


# ------------------------------------------------------------------------------------------------------------ MultiCode
@pytest.mark.parametrize("sizes", [(2, 3, 200), (25, 50, 200)])
def test_multicode_case_and_restatement(sizes):
    c = G.multicode_case(sizes, 16, 600)
    t = c["t"]
    one_below = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
    for s in sizes:
        for k in range(s):
            assert bool((t == torch.tensor(k / (s - 1), dtype=F64).to(F32)).any())
    for v in (0.0, 1.0, float(one_below), -0.2, 1.3):
        assert bool((t == torch.tensor(v, dtype=F32)).any())
    i0, _, _ = G.code_taps_f32(t, max(sizes))
    assert int(torch.bincount(i0).max()) >= 200                        # the hot address
    # the oracle is the project's restatement of deform_code.py:20-38 (zero padding there: t is clamped, nothing is padded)
    assert torch.equal(G.multicode(t, c["vols"]), of.multicode_sample(c["vols"], t))
    assert torch.equal(G.multicode(t, c["vols"], "zeros"), G.multicode(t, c["vols"]))
    # the kernel's index arithmetic, evaluated in fp32 torch, is that function too
    want = G.multicode(t.double(), [v.double() for v in c["vols"]])
    got = []
    for vol in c["vols"]:
        a, b, fr = G.code_taps_f32(t, vol.shape[2])
        v = vol[0, :, :, 0]
        got.append((v[:, a] * (1 - fr) + v[:, b] * fr).t())
    assert float((torch.cat(got, -1).double() - want).abs().max()) <= 4 * max(sizes) * G.U
    # the one-line break `i1 = i0 + 1`: the rows at t >= 1 (and only they) index one past the table -- shown here, never run
    for s in sizes:
        _, i1, _ = G.code_taps_f32(t, s, clamp_i1=False)
        assert int((i1 >= s).sum()) >= 2 and torch.equal(i1 >= s, t >= 1.0)
    for F, C in ((1, 16), (5, 16), (6, 16), (85, 1), (86, 1)):
        assert G.multicode_case(sizes, C, F)["t"].shape == (F,)
    assert 5 * 3 * 16 < 256 < 6 * 3 * 16 and 85 * 3 < 256 < 86 * 3


# ----------------------------------------------------------------------------------------------------------- sdf losses
def test_zero_ties_of_the_free_space_term_under_torch_autograd():
    """utils.py:109 at a predicted sdf of exactly 0, by torch autograd on the CPU -- fixes what the kernel has to return
    independently of the kernel: clamp(min=0) passes its gradient AT 0, max() splits a tie in halves."""
    for dtype in (F32, F64):
        for bnd, want in ((0.5, -5.0), (0.0, 0.5 * (-5.0 + 1.0))):
            p = torch.zeros(1, dtype=dtype, requires_grad=True)
            front = torch.ones(1, dtype=torch.bool)
            n = front.sum(-1).to(dtype) + 1e-8
            fs = (torch.max(torch.exp(-5.0 * p) - 1.0, p - bnd).clamp(min=0.0) * front).sum(-1) / n
            fs.backward()
            assert float(fs) == 0.0
            assert abs(float(p.grad) - want / float(n)) <= 1e-6, (bnd, float(p.grad))


@pytest.mark.parametrize("M", SDF_SIZES)
def test_sdf_case_branches_ties_and_no_flip(M):
    c = G.sdf_case(M)
    h = G.SDF_STEP
    for k in ("ts", "te"):
        assert bool((c[k].double() / h == (c[k].double() / h).round()).all())      # the dyadic grid
    assert bool((c["depth"].double() / h == (c["depth"].double() / h).round()).all()) and c["trunc"] == 0.125
    assert int(c["ri"].max()) < c["depth"].shape[0] and bool((c["ri"][1:] >= c["ri"][:-1]).all())
    for use_mask in (True, False):
        mask = c["mask"] if use_mask else None
        d32 = G.sdf_decisions(c["ts"], c["te"], c["depth"], mask, c["ri"], c["trunc"])
        # the same comparisons on the float64 values of the same inputs: no flip
        z = (c["ts"].double() + c["te"].double()) / 2
        tgt = c["depth"].double().reshape(-1)[c["ri"].long()]
        assert torch.equal(z, d32["z"].double()) and torch.equal(torch.where(tgt < 0, torch.full_like(z, 10.0), tgt - z), d32["bnd"].double())
        front = (z < tgt - c["trunc"]) | ((tgt < 0) & (z < 3.5))
        smask = (d32["bnd"].double().abs() <= c["trunc"]) & (tgt > 0)
        if use_mask:
            smask &= c["mask"].double().reshape(-1)[c["ri"].long()] > 0.5
        assert torch.equal(front, d32["front"]) and torch.equal(smask, d32["smask"])
        assert not bool((front & smask).any())
        # max(a, b) and clamp(min=0): an exact tie or a margin no rounding crosses, in fp32 and float64 alike
        for p in (c["pred"], c["pred"].double()):
            a, b = torch.exp(-5.0 * p) - 1.0, p - d32["bnd"].to(p.dtype)
            mx = torch.max(a, b)
            assert bool((((a - b).abs() > 1e-3) | (a == b))[front].all()) and bool(((mx.abs() > 1e-3) | (mx == 0))[front].all())
        br = G.sdf_branches(c, use_mask)
        if M >= 255:
            for name, rows in br.items():
                if name == "masked out in the band" and not use_mask:
                    assert int(rows.sum()) == 0
                    continue
                assert int(rows.sum()) >= 4, (name, int(rows.sum()))
        # restatement: the oracle in fp32 == oracle/field.py (utils.py:91-113 restated) on the same inputs, gradient included
        ri = c["ri"].long()
        pa, pb = c["pred"].clone().requires_grad_(True), c["pred"].clone().requires_grad_(True)
        fs_a, sl_a = G.sdf_losses(pa, c["ts"], c["te"], c["depth"], mask, c["ri"], c["trunc"])
        fs_b, sl_b = of.sdf_losses(((c["ts"] + c["te"]) / 2)[:, None], c["depth"][ri], pb, c["trunc"], None if mask is None else mask[ri])
        (2.0 * fs_a + 3.0 * sl_a).backward()
        (2.0 * fs_b + 3.0 * sl_b).backward()
        assert torch.equal(fs_a, fs_b) and torch.equal(sl_a, sl_b) and torch.equal(pa.grad, pb.grad)
        # ... and with the decisions handed in
        pc = c["pred"].clone().requires_grad_(True)
        fs_c, sl_c = G.sdf_losses(pc, c["ts"], c["te"], c["depth"], mask, c["ri"], c["trunc"], d32)
        (2.0 * fs_c + 3.0 * sl_c).backward()
        assert torch.equal(fs_a, fs_c) and torch.equal(sl_a, sl_c) and torch.equal(pa.grad, pc.grad)
        # filter cap: every finite fp32 row is finite in float64; nothing is filtered
        pd = c["pred"].double().requires_grad_(True)
        fs_d, sl_d = G.sdf_losses(pd, _d(c["ts"]), _d(c["te"]), _d(c["depth"]), _d(mask), c["ri"], c["trunc"], d32)
        (2.0 * fs_d + 3.0 * sl_d).backward()
        fin = torch.isfinite(pa.grad)
        assert bool(torch.isfinite(pd.grad)[fin].all()) and int((~fin).sum()) * 64 <= M
        if M >= 255 and bool(torch.isfinite(fs_a)):
            nd = float(d32["nz"].sum())
            t1, t2 = br["zero tie: p == 0 in free space"], br["zero tie: p == 0 on the surface"]
            # tie 1 is live in the loss: -5 / n per unit of fs; tie 2 lies outside free space (z == target is never `front`), so the
            # free-space term contributes nothing there and |p - bnd| has slope 0 at 0
            assert torch.allclose(pd.grad[t1], torch.full_like(pd.grad[t1], 2.0 * -5.0 / (1 + 1e-8) / nd), rtol=1e-12, atol=0)
            assert bool((pd.grad[t2] == 0).all()) and bool((pa.grad[t2] == 0).all())
            assert torch.allclose(pa.grad[t1].double(), pd.grad[t1], rtol=1e-6, atol=0)


def test_sdf_sizes_reach_the_stride_loop():
    assert G.loss_rounding_count(32768) == 1 + 6 + 3 + 128 and G.loss_rounding_count(33069) == 2 + 6 + 3 + 128
    assert G.loss_rounding_count(257) == 1 + 6 + 3 + 2
    # 33 069 = 128 workgroups x 256 threads + 301: threads 0..300 take a second trip, thread 301 onwards does not
    assert 33069 - 128 * 256 == 301 and 301 % 64 != 0 and 301 % 256 != 0


# -------------------------------------------------------------------------------------------------------- the judgement
def test_judge_rules():
    f64 = torch.linspace(1, 2, 1000, dtype=F64)
    chain = f64 * (1 + 1e-7 * torch.sin(torch.arange(1000.0, dtype=F64)))
    G.judge(chain, chain, f64, f64.abs(), 2, "same error")
    with pytest.raises(AssertionError):
        G.judge(f64 * (1 + 4e-7), chain, f64, f64.abs(), 2, "4 x")
    with pytest.raises(AssertionError):
        G.judge(f64 * (1 + 2.5e-7), chain, f64, f64.abs(), 2, "every element above the chain's 99.9th percentile")
    G.judge(f64 + 1.5 * G.U, f64, f64, 1.0, 2, "exact chain: the rounding-count floor")
    with pytest.raises(AssertionError):
        G.judge(f64 + 2.5 * G.U, f64, f64, 1.0, 2, "exact chain, above the floor")
    one = torch.tensor([1.0, 0.0], dtype=F64)
    G.judge_sum(torch.tensor([1.0 + 3 * G.U, 0.0], dtype=F64), one, one, 3, "sum")
    with pytest.raises(AssertionError):
        G.judge_sum(torch.tensor([1.0 + 4 * G.U, 0.0], dtype=F64), one, one, 3, "sum")
    with pytest.raises(AssertionError):
        G.judge_sum(torch.tensor([1.0, 1e-30], dtype=F64), one, one, 3, "empty sum")
