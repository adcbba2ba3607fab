"""Float64 yardstick and case builders for the field-query glue kernels (csrc/normal.hip) -- test infrastructure, plain torch,
any device, like tests/visibility_oracle.py.

The reference expressions are written ONCE, dtype-generic, and differentiated by torch autograd (no hand-written gradient):
    taps             models/model.py:367-376     clamp(x +- eps e_k, -bound, bound)
    normal           models/model.py:377-398, utils.py:70-71
    sample assembly  morpheus.py:644-647
    sdf losses       utils.py:91-113
    MultiCode        models/deform_code.py:20-38  (F.grid_sample itself, align_corners=True)
Called on fp32 tensors they ARE the fp32 torch chain the kernels restate; called on the same values in float64 they are the
yardstick.  A float64 run must not differ from the kernel by a flipped comparison, so every discrete decision (the clamp masks of
the taps, the 1e-20 clamp of the normal, the loss masks) can be handed in, taken from the fp32 inputs as the kernel sees them
(`*_decisions`); the float64 values then follow the fp32 branch.

Case builders (`*_case`) place the rows at which the kernels branch; tests/test_glue_oracle_host.py asserts on the CPU that they
really do (branch population, exact ties, no fp32 / float64 decision flip), tests/test_gpu_glue_f64.py runs them on the GPU.
"""
import math

import torch

from morpheus_amd import synth
from tests.f64_judge import F32, F64, U, judge_sum, judge_vs_f64      # noqa: F401  (judge_sum: the suites call it from here)


def f32_scalar(v) -> float:
    """the python scalar as the kernel receives it (a float argument)"""
    return float(torch.tensor(float(v), dtype=F32))


# ---------------------------------------------------------------------------------------------------------------- taps
def tap_offsets(eps, device=None):
    """[1, 6, 3] fp32: +x, -x, +y, -y, +z, -z (the kernel's point-major tap order)."""
    off = torch.zeros(1, 6, 3, dtype=F32, device=device)
    for k in range(3):
        off[0, 2 * k, k], off[0, 2 * k + 1, k] = eps, -eps
    return off


def taps_decisions(x32, eps, bound):
    """[M, 6, 3] bool: the tap component lies inside [-bound, bound] -- decided on the fp32 sum x + off, as the kernel does."""
    x32 = x32.detach().to(F32)
    v = x32[:, None] + tap_offsets(eps, x32.device)
    b = torch.tensor(bound, dtype=F32, device=x32.device)
    return (v >= -b) & (v <= b)


def taps(x, topo, eps, bound, inside=None):
    """-> taps [6M, 3], topo6 [6M, C] or None.  inside=None: the reference expression as written (clamp decides on its own
    input, in x's dtype); inside given: where it is False the tap is the constant fp32 clamp value."""
    M = x.shape[0]
    v = x[:, None] + tap_offsets(eps, x.device).to(x.dtype)          # fp32(eps) exactly, in either dtype
    if inside is None:
        t = v.clamp(-bound, bound)
    else:
        b = f32_scalar(bound)
        t = torch.where(inside, v, v.detach().clamp(-b, b))
    topo6 = None if topo is None else topo[:, None].expand(M, 6, topo.shape[1]).reshape(6 * M, topo.shape[1])
    return t.reshape(6 * M, 3), topo6


# -------------------------------------------------------------------------------------------------------------- normal
def normal_decisions(s6_32, eps):
    """[M] bool: |raw|^2 < 1e-20 in the kernel's own fp32 operation order ((r0^2 + r1^2) + r2^2, r = (0.5 (a - b)) * (1 / eps))."""
    s = s6_32.detach().to(F32)
    inv = torch.tensor(1.0, dtype=F32, device=s.device) / torch.tensor(eps, dtype=F32, device=s.device)
    r = (0.5 * (s[:, 0::2] - s[:, 1::2])) * inv
    ss = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    return ~(ss >= torch.tensor(1e-20, dtype=F32, device=s.device))


def normal(s6, eps, clamped=None):
    """s6 [M, 6] -> (normal, raw).  clamped=None: nan_to_num(safe_normalize(raw)) as written; clamped given (finite rows
    only): the squared length of those rows is the constant fp32(1e-20)."""
    raw = torch.stack([0.5 * (s6[:, 0] - s6[:, 1]) / eps, 0.5 * (s6[:, 2] - s6[:, 3]) / eps, 0.5 * (s6[:, 4] - s6[:, 5]) / eps], -1)
    ss = torch.sum(raw * raw, -1, keepdim=True)
    if clamped is None:
        return torch.nan_to_num(raw / torch.sqrt(torch.clamp(ss, min=1e-20))), raw
    return raw / torch.sqrt(torch.where(clamped[:, None], torch.full_like(ss, f32_scalar(1e-20)), ss)), raw


# ----------------------------------------------------------------------------------------------------- sample positions
def positions(rays_o, rays_d, ri, ts, te):
    ri = ri.long()
    return rays_o[ri] + rays_d[ri] * ((ts[:, None] + te[:, None]) / 2.0)


# ------------------------------------------------------------------------------------------------------------ MultiCode
def multicode(t, volumes, padding_mode="border"):
    """t [F] -> [F, 3 C]; volumes [1, C, size, 1] each."""
    t = torch.clamp(t.reshape(-1, 1), 0, 1)
    t = t * 2 - 1
    t = t[None, :, None, :]
    grid = torch.cat([torch.zeros_like(t), t], dim=-1)                # (x = 0, y = t): [1, F, 1, 2]
    feat = []
    for vol in volumes:
        s = torch.nn.functional.grid_sample(vol, grid, mode="bilinear", padding_mode=padding_mode, align_corners=True)
        feat.append(s[0, :, :, 0].permute(1, 0))
    return torch.cat(feat, dim=-1)


def code_taps_f32(t32, size, clamp_i1=True):
    """The kernel's index arithmetic (code_taps) in fp32 torch -> (i0, i1, fr).  clamp_i1=False is the broken form
    `i1 = i0 + 1`, kept here so that the host test can show which rows tell the two apart without running it on a GPU."""
    t = t32.detach().to(F32).reshape(-1).clamp(0.0, 1.0)
    r = (((t * 2.0 - 1.0) + 1.0) / 2.0) * float(size - 1)
    r0 = torch.floor(r)
    i0 = r0.long().clamp(0, size - 1)
    i1 = (i0 + 1).clamp(max=size - 1) if clamp_i1 else i0 + 1
    return i0, i1, r - r0


# ----------------------------------------------------------------------------------------------------------- sdf losses
def sdf_decisions(ts32, te32, depth32, mask32, ri, trunc):
    """The loss masks from the fp32 z = (ts + te) / 2 and bnd = target - z, as the kernel forms them."""
    ri = ri.long()
    z = (ts32.detach().to(F32) + te32.detach().to(F32)) / 2.0
    tgt = depth32.detach().to(F32).reshape(-1)[ri]
    tr = torch.tensor(trunc, dtype=F32, device=z.device)
    neg = tgt < 0.0
    front = (z < (tgt - tr)) | (neg & (z < 3.5))
    bnd = torch.where(neg, torch.full_like(z, 10.0), tgt - z)
    smask = (bnd.abs() <= tr) & (tgt > 0.0)
    if mask32 is not None:
        smask = smask & (mask32.detach().to(F32).reshape(-1)[ri] > 0.5)
    return dict(front=front, smask=smask, neg=neg, nz=tgt != 0.0, z=z, bnd=bnd, tgt=tgt)


def sdf_losses(pred, ts, te, depth, mask, ri, trunc, dec=None, terms=False):
    """utils.py:91-113 on packed samples with per-ray depth / mask read through ri.  dec=None: as written; dec given: its
    masks replace the comparisons.  -> (fs_loss, sdf_loss[, per-sample fs terms, per-sample sdf terms, count])."""
    ri = ri.long()
    z_vals = ((ts + te) / 2.0)[:, None]
    target_d = depth.reshape(-1)[ri][:, None]
    p = pred[..., None]
    if dec is None:
        depth_mask = target_d > 0.0
        front = (z_vals < (target_d - trunc)) | ((target_d < 0.0) & (z_vals < 3.5))
        bnd = target_d - z_vals
        bnd = torch.where((target_d[:, 0] < 0.0)[:, None], torch.full_like(bnd, 10.0), bnd)
        smask = (bnd.abs() <= trunc) & depth_mask
        if mask is not None:
            smask = smask & (mask.reshape(-1)[ri][:, None] > 0.5)
        nd = torch.count_nonzero(target_d)
    else:
        front, smask = dec["front"][:, None], dec["smask"][:, None]
        bnd = torch.where(dec["neg"][:, None], torch.full_like(z_vals, 10.0), target_d - z_vals)
        nd = dec["nz"].sum()
    n = (front.sum(-1) + smask.sum(-1)).to(p.dtype) + 1e-8
    fs_t = (torch.max(torch.exp(-5.0 * p) - 1.0, p - bnd).clamp(min=0.0) * front).sum(-1) / n
    sl_t = (torch.abs(p - bnd) * smask).sum(-1) / n
    fs, sl = fs_t.sum() / nd, sl_t.sum() / nd
    return (fs, sl, fs_t, sl_t, nd) if terms else (fs, sl)


# -------------------------------------------------------------------------------------------------------- the judgement
def judge(hip, chain, f64, scale, count, what):
    """The rule for everything with a division, sqrt, expf or lerp: errors are |x - f64| / scale (scale: same shape or scalar,
    the element's own magnitude as the caller defines it; where it is 0 the value must be exactly the yardstick's).  The fp32
    torch chain's own error is the measure: the worst HIP element within 3 x the chain's worst, and at most 3 x as many (+ 2)
    elements above the chain's 99.9th percentile.  Where the chain is exact the floor is `count` roundings (count * 2^-24).
    -> the record the report keeps; raises AssertionError (f64_judge.judge_vs_f64)."""
    floor = count * U
    f = judge_vs_f64(hip, chain, f64, scale, what, 3.0, floor, 2, percentile=True)
    if f["n"] == 0:      # nothing live: with count == 0 the ratio below would be 0 / 0
        return dict(worst_hip=0.0, worst_chain=0.0, ratio=0.0, n_above=0)
    return dict(worst_hip=f["worst_hip"], worst_chain=f["worst_ref"], ratio=f["worst_hip"] / max(f["worst_ref"], floor),
                n_above=f["n_hip"])


# --------------------------------------------------------------------------------------------------------------- cases
BOUND = 1.01
EPS_CASES = (2e-3, 5e-3)      # the model's default (no config overrides it: configs/snoopy.yaml resolves to 2e-3 as well) and
#                               train.smoothness_std of that config, the other finite-difference step a run uses
RAY_COUNTS = [0, 1, 63, 64, 65, 0, 127, 128, 129, 200, 2, 64, 0]


def positions_case():
    """13 rays = three blocks of four waves and one block with three idle waves; counts around every multiple of the wave
    (one, two, three and four trips of the i += 64 loop), a zero count first and last."""
    cnt = torch.tensor(RAY_COUNTS, dtype=torch.int32)
    N, M = cnt.numel(), int(cnt.sum())
    ri = torch.repeat_interleave(torch.arange(N), cnt.long()).int()
    start = (torch.cumsum(cnt, 0) - cnt).int()
    ts = synth.hash_tensor((M,), 1709, 1.0, 1.5)
    return dict(cnt=cnt, start=start, ri=ri, N=N, M=M, o=synth.hash_tensor((N, 3), 1707, 1.0), d=synth.hash_tensor((N, 3), 1708, 1.0),
                ts=ts, te=ts + synth.hash_tensor((M,), 1711, 0.004, 0.01), g=synth.hash_tensor((M, 3), 1710, 1.0))


def _tie_below_bound(eps, bound, sign):
    """fp32 x with fl(x + sign * eps) == sign * bound exactly (the clamp's gradient mask is decided AT the bound).  x, eps and
    bound share a binade, so stepping x by one ulp steps the rounded sum by one ulp: a solution is next to fl(bound - eps)."""
    b, e = torch.tensor(bound, dtype=F32), torch.tensor(eps, dtype=F32)
    x = (b - e) * sign
    for _ in range(8):
        v = x + e * sign
        if float(v) == float(b) * sign:
            return x
        x = torch.nextafter(x, torch.tensor(float("inf") if (float(v) < float(b) * sign) else float("-inf")))
    raise AssertionError("no fp32 x reaches the bound exactly")


def taps_case(M, C, eps, bound=BOUND):
    """x [M, 3] with the placed rows first (as many as fit): per axis and sign the point at exactly +-bound, the point whose
    +-eps tap lands exactly on +-bound, each with its two fp32 neighbours (36 rows), then per axis and sign a point beyond
    bound + eps, whose six taps are all clamped on that axis (6 rows); hashed points, a few outside the box, fill the rest."""
    x = synth.hash_tensor((M, 3), 1700 + M, 1.02).to(F32)
    rows = []
    for a in range(3):
        for sign in (1.0, -1.0):
            for centre in (torch.tensor(bound, dtype=F32) * sign, _tie_below_bound(eps, bound, sign)):
                for to in (None, float("inf"), float("-inf")):
                    rows.append((a, centre if to is None else torch.nextafter(centre, torch.tensor(to))))
    for a in range(3):
        for sign in (1.0, -1.0):
            rows.append((a, torch.tensor(1.5 * sign, dtype=F32)))
    for i, (a, v) in enumerate(rows[:M]):
        x[i] = x[i].clamp(-0.9, 0.9)                                  # the other two axes well inside
        x[i, a] = v
    topo = None if C is None else synth.hash_tensor((M, C), 1701 + M, 0.3).to(F32)
    g_taps = synth.hash_tensor((6 * M, 3), 1702 + M, 1.0).to(F32)
    g_topo6 = None if C is None else synth.hash_tensor((6 * M, C), 1703 + M, 1.0).to(F32)
    return dict(x=x, topo=topo, g_taps=g_taps, g_topo6=g_topo6, eps=eps, bound=bound, n_placed=min(M, len(rows)))


NORMAL_KINDS = ("ordinary", "flat", "below_x0.25", "below_x0.5", "above_x2", "above_x4", "large", "ordinary")


def normal_case(M, eps):
    """s6 [M, 6], row i of kind NORMAL_KINDS[i % 8]: exactly flat; |raw| = 1e-10 x {0.25, 0.5, 2, 4} (|raw|^2 on both sides of the
    1e-20 clamp: tap differences of 2 eps 1e-10 x scale, taps of that size so that fp32 holds them); ordinary; |raw| ~ 1e3."""
    s6 = synth.hash_tensor((M, 6), 1720 + M, 0.5).double()
    u = synth.hash_tensor((M, 3), 1721 + M, 1.0).double()
    u = u / u.norm(dim=-1, keepdim=True).clamp(min=1e-3)
    kind = torch.arange(M) % 8
    s6[kind == 1] = 0.25
    for k, scale in ((2, 0.25), (3, 0.5), (4, 2.0), (5, 4.0)):
        half = eps * 1e-10 * scale * u                               # raw = 0.5 (2 half) / eps = 1e-10 scale u
        rows = torch.stack([half[:, 0], -half[:, 0], half[:, 1], -half[:, 1], half[:, 2], -half[:, 2]], -1)
        s6[kind == k] = rows[kind == k]
    half = eps * 1e3 * u
    rows = 0.3 + torch.stack([half[:, 0], -half[:, 0], half[:, 1], -half[:, 1], half[:, 2], -half[:, 2]], -1)
    s6[kind == 6] = rows[kind == 6]
    return dict(s6=s6.to(F32), kind=kind, eps=eps, g_n=synth.hash_tensor((M, 3), 1722 + M, 1.0).to(F32),
                g_r=synth.hash_tensor((M, 3), 1723 + M, 1.0).to(F32))


def normal_nonfinite_case(eps=2e-3):
    """forward only: every row carries one NaN, +inf, -inf or overflowing tap, in each of the six positions."""
    bad = [float("nan"), float("inf"), float("-inf"), 3.0e38]
    s6 = synth.hash_tensor((6 * len(bad), 6), 1730, 0.5).to(F32)
    for i in range(s6.shape[0]):
        s6[i, i % 6] = bad[i // 6]
    s6[-6:, 1] = -3.0e38                                              # a - b overflows
    return dict(s6=s6, eps=eps)


def multicode_case(sizes, C, F):
    """tables [1, C, size, 1] and times [F].  F == 600 is the atomics batch: every knot of every level, 0, 1, the fp32 below
    1, -0.2, 1.3, 200 times inside ONE cell of the finest level (a hot address), hashed times in [-0.1, 1.1] for the rest."""
    vols = [synth.hash_tensor((1, C, s, 1), 1740 + i, 1.0).to(F32) for i, s in enumerate(sizes)]
    fill = (synth.hash_tensor((max(F, 8),), 1743 + F, 0.6, 0.5)).to(F32)
    special = torch.tensor([0.123456, 0.0, 1.0, 1.3, -0.2, 0.5], dtype=F32)
    if F != 600:
        t = torch.cat([special, fill])[:F]
    else:
        knots = torch.cat([(torch.arange(s, dtype=F64) / (s - 1)).to(F32) for s in sizes])
        one = torch.tensor(1.0, dtype=F32)
        cell = ((60.0 + 0.01 + (torch.arange(200, dtype=F64) + 0.5) / 200.0 * 0.98) / (max(sizes) - 1)).to(F32)   # rows 60.01 .. 60.99
        t = torch.cat([knots, special, torch.nextafter(one, torch.tensor(0.0))[None], cell, fill])[:F]
        assert t.numel() == F
    return dict(vols=vols, t=t, sizes=list(sizes), C=C, g=synth.hash_tensor((F, 3 * C), 1744 + F, 1.0).to(F32))


SDF_TRUNC = 0.125
SDF_STEP = 2.0 ** -10


def _sdf_table():
    """The fixed ray table on the dyadic grid (depths, ts, te multiples of 2^-10, trunc = 1/8: z and bnd are exact in fp32 and
    the equalities are hit exactly).  -> per-ray (depth, mask), per-sample (ray, z, pred), ray-major."""
    h, tr = SDF_STEP, SDF_TRUNC
    P4 = [-0.375, -0.0625, 0.25, 1.25]      # exp(-5p) - 1 > 0 > p - bnd | both below 0 | p - bnd > 0 > exp(-5p) - 1 (bnd <= 1)
    rays, samples = [], []

    def ray(depth, mask):
        rays.append((depth, mask))
        return len(rays) - 1

    def add(r, z, preds):
        samples.extend((r, z, p) for p in preds)

    r = ray(-1.0, 1.0)                                                # no depth: free space in front of 3.5
    for z in (3.5 - h, 3.5, 3.5 + h, 1.0):
        add(r, z, P4)
    r = ray(0.0, 1.0)                                                 # zero depth: no loss, not counted
    add(r, 1.0, P4)
    for depth, mask in ((1.5, 1.0), (1.5, 0.0), (1.5, 0.5), (2.0, 1.0)):
        r = ray(depth, mask)
        add(r, 0.5, P4)                                               # deep in free space, bnd = depth - 0.5
        for z0 in (depth - tr, depth + tr):                           # z == target - trunc / |bnd| == trunc, a step either side
            for z in (z0 - h, z0, z0 + h):
                add(r, z, P4)
        add(r, depth, P4)                                             # on the surface
        add(r, depth - 8 * h, [8 * h, 8 * h - 0.25, 8 * h + 0.25, 8 * h])   # in the band: p == bnd twice, either side once
        add(r, 0.25, [0.0, 0.0])                                      # ZERO TIE 1: p == 0 in free space (bnd > 0): mx == 0, a > b
        add(r, 0.75, [0.0])
        add(r, depth, [0.0, 0.0])                                     # ZERO TIE 2: p == 0 on the surface (bnd == 0): a == b == 0
    return rays, samples


def sdf_case(M):
    """The table tiled to M samples; every tile brings its own rays, so ray_idx stays ray-major."""
    rays, samples = _sdf_table()
    T, R = len(samples), len(rays)
    tiles = (M + T - 1) // T
    m = torch.arange(M)
    sr = torch.tensor([s[0] for s in samples])
    sz = torch.tensor([s[1] for s in samples], dtype=F64)
    sp = torch.tensor([s[2] for s in samples], dtype=F64)
    ri = (sr[m % T] + (m // T) * R).int()
    z = sz[m % T]
    half = (1 + (m % 5)).double() * SDF_STEP                          # sample lengths 2..10 grid steps, z stays the midpoint
    depth = torch.tensor([r[0] for r in rays], dtype=F64).repeat(tiles)
    mask = torch.tensor([r[1] for r in rays], dtype=F64).repeat(tiles)
    return dict(M=M, T=T, ts=(z - half).to(F32), te=(z + half).to(F32), pred=sp[m % T].to(F32), ri=ri, depth=depth.to(F32)[:, None],
                mask=mask.to(F32)[:, None], trunc=SDF_TRUNC)


def sdf_branches(case, use_mask=True):
    """name -> [M] bool, from the fp32 inputs: the rows the GPU test relies on."""
    d = sdf_decisions(case["ts"], case["te"], case["depth"], case["mask"] if use_mask else None, case["ri"], case["trunc"])
    z, bnd, tgt, p = d["z"], d["bnd"], d["tgt"], case["pred"]
    tr = torch.tensor(case["trunc"], dtype=F32)
    a, b = torch.exp(-5.0 * p) - 1.0, p - bnd
    mx = torch.max(a, b)
    pos = tgt > 0
    return {
        "no depth, z < 3.5": d["neg"] & (z < 3.5), "no depth, z == 3.5": d["neg"] & (z == 3.5), "no depth, z > 3.5": d["neg"] & (z > 3.5),
        "zero depth": tgt == 0,
        "z < target - trunc by a step": pos & (z == tgt - tr - SDF_STEP), "z == target - trunc": pos & (z == tgt - tr),
        "z > target - trunc by a step": pos & (z == tgt - tr + SDF_STEP),
        "bnd == -trunc": pos & (bnd == -tr), "bnd == -trunc - step": pos & (bnd == -tr - SDF_STEP),
        "bnd == -trunc + step": pos & (bnd == -tr + SDF_STEP),
        "masked out in the band": pos & (bnd.abs() <= tr) & ~d["smask"],
        "front, a > b, mx > 0": d["front"] & (a > b) & (mx > 0), "front, a < b, mx > 0": d["front"] & (a < b) & (mx > 0),
        "front, mx < 0": d["front"] & (mx < 0),
        "zero tie: p == 0 in free space": d["front"] & (p == 0) & (bnd > 0) & (mx == 0) & (a > b),
        "zero tie: p == 0 on the surface": (p == 0) & (bnd == 0) & (a == b),
        "band, p > bnd": d["smask"] & (b > 0), "band, p < bnd": d["smask"] & (b < 0), "band, p == bnd": d["smask"] & (b == 0),
    }


def loss_rounding_count(M):
    """roundings on the way of one term into a loss total: grid-stride trips + 6 shuffle steps + 3 (two levels of the LDS
    combination, the division by the count) + one atomic per workgroup."""
    groups = min((M + 255) // 256, 128)
    return math.ceil(M / 32768) + 6 + 3 + groups
