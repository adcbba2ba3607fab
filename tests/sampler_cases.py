"""Case builders and float32 restatements for the ray samplers (csrc/sampler.hip) -- test infrastructure, numpy / torch on
the CPU, no GPU, like tests/glue_f64_oracle.py.

The definition the kernels are held to is oracle/field.py's (uniform_samples, march_samples: fp32, one rounding per operation,
the kernel's operation order).  This file adds
  * what a fixed-length slot row of mh_march_slots holds, derived from the oracle's packed result (`slot_expect`),
  * a plain restatement of the pinhole rays for any intrinsics and pose (`pixel_rays`),
  * a float64 evaluation of the same formulas with a rounding-count bound (`march_f64`, `uniform_f64`),
  * the cases: each a small dict of rays, jitter, grid, step, bound, cap and `reaches`, what it is meant to reach.
tests/test_sampler_cases_host.py asserts on the CPU that every case reaches what it names; tests/test_gpu_sampler_cases.py
runs them on the GPU, bit for bit.

A MISS: the clipped segment is empty, one of the six slab quotients is NaN, or the clipped
t_near / t_far is not finite.  Zero-width samples at t = 0 in the uniform sampler, no samples in the marcher.
"""
import math

import numpy as np
import torch

from morpheus_amd import synth
from oracle import field as of
from tests.f64_judge import U

F = np.float32
BELOW_ONE = float(np.nextafter(F(1), F(0)))        # the largest float below 1: the largest jitter a [0,1) draw can give
JITTERS = (None, 0.0, BELOW_ONE)                   # None = the NULL pointer of the C ABI (no jitter)
SENTINEL = -12345.0                                # fills slot buffers: no sample has a negative t
CNT_SENTINEL = -7

STEP, BOUND = 0.0075, 1.01                         # the marcher cases: 2.02 / 0.0075 = 269 steps on an axis chord
CAPS = (1, 21, 63, 64, 65, 128, 129)               # below a wave, one off / on / one past 64 and 128
COUNTS = tuple(sorted({c + e for c in CAPS for e in (-1, 0, 1)}))      # step counts cap - 1, cap, cap + 1 of every cap
WAVE = 64


def walked(cap: int) -> int:
    """steps the marcher's loop can visit with a slot row of `cap`: whole trips of 64 while k0 < cap"""
    return -(-cap // WAVE) * WAVE


def guard_len(cap: int) -> int:
    """floats behind the last slot row that a kernel without its `pos < cap` guard can still reach: its positions stay under
    walked(cap) + 1 <= cap + 64, so a guard of max(cap, 64) + 1 keeps every surplus write of that mutant inside the allocation"""
    return max(cap, WAVE) + 1


def _t(a, dtype=F):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype)))


# ------------------------------------------------------------------------------------------------------------------ rays
def count_ray(n: int, u: float, where: str, step: float = STEP, bound: float = BOUND, xy=(0.5, -0.5)):
    """An axis-aligned ray (+z) with exactly n steps at jitter u: the walked chord is (n - 0.5 + u) * step, so the last step
    starts half a step before t_far and the next one half a step behind it -- rounding cannot move the count, in fp32 or
    float64.  where: 'inside' (t_near = 0, unit direction), 'face' (origin on the -z face) or 'outside' (origin one unit in
    front of it); the latter two cross the whole box with a direction scaled to the chord.  n = 0: a ray pointing away."""
    b = float(F(bound))
    if n == 0:
        return (xy[0], xy[1], {"inside": 2.0, "face": b + 0.5, "outside": 3.0}[where]), (0.0, 0.0, 1.0)
    T = (n - 0.5 + u) * step
    if where == "inside":
        return (xy[0], xy[1], b - T), (0.0, 0.0, 1.0)
    L = 2.0 * b / T
    return (xy[0], xy[1], -b if where == "face" else -b - 1.0), (0.0, 0.0, L)


def clamp_live_z(bound: float = BOUND) -> float:
    """z just inside the +z face whose cell coordinate (z + b) / (2 b) rounds to exactly 1 in fp32: floor(u * R) = R, one past
    the last cell -- the sample that only the kernel's `R - 1` clamp keeps inside the grid"""
    b = F(bound)
    z = np.nextafter(b, F(0))
    assert z < b and (z + b) / (F(2) * b) == F(1), "this bound has no such z next to the face: pick a bound with an even mantissa"
    return float(z)


def finite_specials(bound: float = BOUND):
    """-> (o [n,3], d [n,3], names): finite rays at the edges of the slab clip.  The long diagonal is LAST: with a short slot
    row its surplus lands in the guard row."""
    b = float(F(bound))
    zc = clamp_live_z(bound)
    rows = [
        ("signed_zero_dir", (0.2, 0.1, 2.0), (0.0, -0.0, -1.0)),            # +0.0 and -0.0: quotients of both infinities
        ("points_away", (0.0, 0.0, 2.0), (0.0, 0.0, 1.0)),
        ("passes_beside", (3.0, 3.0, 3.0), (1.0, 0.0, 0.0)),
        ("edge_touch", (-2.0 * b, 0.0, 0.3), (1.0, 1.0, 0.0)),              # t_near == t_far exactly on the x/y edge: a miss
        ("edge_thin", (-2.0 * b, -0.01, 0.3), (1.0, 1.0, 0.0)),             # the same edge, 0.01 inside: a chord of 0.01
        ("face_graze_in", (-2.0, 0.25, zc), (1.0, 0.0, 0.0)),               # along the +z face, one ulp inside: cell index R
        ("inside_oblique", (0.1, -0.2, 0.3), (0.3, 0.5, -0.8)),
        ("on_face_entering", (b, 0.0, 0.0), (-1.0, 0.2, 0.1)),              # t_near = -0.0 before the clamp
        ("on_face_leaving", (-b, 0.0, 0.0), (-1.0, 0.0, 0.0)),
    ]
    g = synth.hash_tensor((4, 6), 6101, 1.0).numpy().astype(np.float64)
    for i in range(4):                                                       # oblique rays from a shell towards the middle
        o = g[i, :3] / np.linalg.norm(g[i, :3]) * 2.5
        rows.append((f"oblique{i}", tuple(o), tuple(0.4 * g[i, 3:] - o)))
    rows.append(("long_diagonal", (-2.0, -2.0, -2.0), (1.0, 1.0, 1.0)))
    return _t([r[1] for r in rows]), _t([r[2] for r in rows]), [r[0] for r in rows]


def nonfinite_rows(bound: float = BOUND):
    """-> (o [8,3], d [8,3], names, miss [8] bool): the rows of the miss rule, with two ordinary hits among them.  Eight rays:
    a marcher that still walked one of them to the end of its slot row would stay small."""
    b = float(F(bound))
    n, inf = float("nan"), float("inf")
    rows = [
        ("nan_dir_x", (0.0, 0.0, 2.0), (n, 0.0, -1.0), True),               # fmaxf / fminf would march [0.99, 3.01]
        ("all_nan", (n, n, n), (n, n, n), True),                            # ... and here [0, inf)
        ("zero_dir_inside", (0.1, 0.2, 0.3), (0.0, 0.0, 0.0), True),        # t_far = inf: no NaN anywhere
        ("plain_hit", (0.0, 0.0, 2.0), (0.0, 0.0, -1.0), False),
        ("inf_dir", (-2.0, 0.0, 0.0), (inf, 0.0, 0.0), True),               # quotients +-0: an empty clip
        ("nan_origin", (n, 0.0, 0.0), (1.0, 0.0, 0.0), True),
        ("in_face_plane", (-2.0, -b, 0.0), (1.0, 0.0, 0.0), True),          # 0/0 on the y face: a NaN quotient of finite inputs
        ("oblique_hit", (1.5, 1.8, -2.0), (-0.6, -0.7, 0.9), False),
    ]
    return _t([r[1] for r in rows]), _t([r[2] for r in rows]), [r[0] for r in rows], np.array([r[3] for r in rows])


def jitter_tensor(u, n: int):
    return None if u is None else torch.full((n,), float(u), dtype=torch.float32)


def marcher_rays(u):
    """The marcher's finite ray set at jitter u (None counts as 0): for every count in COUNTS an inside, an on-face and an
    outside ray, then the finite specials.  -> dict(o, d, names, want_steps [N] (-1 = not prescribed))"""
    uu = 0.0 if u is None else float(u)
    o, d, names, want = [], [], [], []
    for n in COUNTS:
        for where in ("inside", "face", "outside"):
            ro, rd = count_ray(n, uu, where)
            o.append(ro), d.append(rd), names.append(f"count{n}_{where}"), want.append(n)
    so, sd, sn = finite_specials()
    return dict(o=torch.cat([_t(o), so]), d=torch.cat([_t(d), sd]), names=names + sn,
                want_steps=np.array(want + [-1] * len(sn)))


# ----------------------------------------------------------------------------------------------------------------- grids
def grids():
    """name -> uint8 [R,R,R].  R = 1, 2, 3, 5 and 128 all occur; the random grids are asymmetric in their three indices and the
    single cell (2, 0, 1) of the R = 3 grid is the one the count rays (x = 0.5, y = -0.5) cross: a transposed index reads (0, 2, 1)."""
    one = torch.zeros(3, 3, 3, dtype=torch.uint8)
    one[2, 0, 1] = 1
    return {
        "full_R1": torch.ones(1, 1, 1, dtype=torch.uint8),
        "empty_R2": torch.zeros(2, 2, 2, dtype=torch.uint8),
        "random_R128": (synth.hash_tensor((128, 128, 128), 4242, 0.5, 0.5) > 0.6).to(torch.uint8).contiguous(),
        "random_R5": (synth.hash_tensor((5, 5, 5), 4243, 0.5, 0.5) > 0.5).to(torch.uint8).contiguous(),
        "single_R3": one,
    }


# ------------------------------------------------------------------------------------------------- marcher restatements
def march_full(o, d, jit, step, bound, grid):
    """the oracle's packed samples plus per-ray step counts and per-sample interval numbers, as one dict"""
    ri, ts, te, n_steps, k = of.march_samples(o, d, jit, step, bound, grid, return_steps=True)
    N = o.shape[0]
    cnt = torch.bincount(ri, minlength=N) if ri.numel() else torch.zeros(N, dtype=torch.int64)
    return dict(ri=ri, ts=ts, te=te, n_steps=n_steps, k=k, cnt=cnt, N=N)


def slot_expect(m, cap: int):
    """What mh_march_slots leaves for a slot row of `cap` in buffers pre-filled with SENTINEL / CNT_SENTINEL, from march_full's
    result: -> (ray_cnt [N] int32, rows_ts [N, cap], rows_te [N, cap], flag 0/1).
    The loop visits the steps k < walked(cap); n = the occupied ones among them; ray_cnt = min(n, cap) and the row holds the
    first ray_cnt of them; the flag is set when n > cap or when step walked(cap) still lies inside the ray."""
    N, W = m["N"], walked(cap)
    rows_s = torch.full((N, cap), SENTINEL)
    rows_e = torch.full((N, cap), SENTINEL)
    cnt = torch.zeros(N, dtype=torch.int32)
    flag = 0
    for r in range(N):
        sel = (m["ri"] == r) & (m["k"] < W)
        n = int(sel.sum())
        c = min(n, cap)
        rows_s[r, :c], rows_e[r, :c] = m["ts"][sel][:c], m["te"][sel][:c]
        cnt[r] = c
        if n > cap or int(m["n_steps"][r]) > W:
            flag = 1
    return cnt, rows_s, rows_e, flag


def overflow_halves(m, cap: int):
    """-> (rays with n > cap, rays with unwalked steps): the two halves of the kernel's overflow condition, per ray"""
    W = walked(cap)
    n = torch.stack([((m["ri"] == r) & (m["k"] < W)).sum() for r in range(m["N"])]) if m["N"] else torch.zeros(0, dtype=torch.int64)
    return n > cap, m["n_steps"] > W


def trips(n_steps: int, cap: int) -> int:
    """trips of the marcher's 64-step loop in which a lane is inside the ray"""
    return min(-(-cap // WAVE), -(-int(n_steps) // WAVE))


def steps_f64(o, d, jit, step, bound):
    """per-ray step counts of the same definition evaluated in float64 on the fp32 inputs (finite rays only)"""
    o64, d64 = o.numpy().astype(np.float64), d.numpy().astype(np.float64)
    b, st = float(F(bound)), float(F(step))
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-b - o64) / d64, (b - o64) / d64
    tmin = np.maximum(np.minimum(ta, tb).max(-1), 0.0)
    tmax = np.maximum(ta, tb).min(-1)
    hit = tmax > tmin
    u = np.zeros(o.shape[0]) if jit is None else jit.numpy().astype(np.float64)
    out = np.zeros(o.shape[0], np.int64)
    for r in np.nonzero(hit)[0]:
        k = 0
        while tmin[r] + u[r] * st + k * st < tmax[r]:
            k += 1
        out[r] = k
    return out


def _slab64(o, d, bound):
    o64, d64 = o.numpy().astype(np.float64), d.numpy().astype(np.float64)
    b = float(F(bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-b - o64) / d64, (b - o64) / d64
    return np.maximum(np.minimum(ta, tb).max(-1), 0.0), np.maximum(ta, tb).min(-1)


def march_f64(o, d, jit, step, bound, m):
    """Float64 evaluation of the kept samples of march_full's result m (the fp32 decisions -- which steps exist, which are
    kept -- are taken from m) -> (ts64, te64, bound_abs).
    The bound counts the fp32 roundings on the longest path to a value: the slab quotient (a subtraction and a division: 2),
    u * step (1), its sum with t_near (1), k * step (1), the sum ts (1), ts + step (1) = 7 roundings, each at most U times a
    partial result; every term on the path is non-negative, so every partial result is at most A = t_near + u step + k step +
    step, or t_far where te is clipped to it (2 roundings).  min() is exact and 1-Lipschitz.  Hence |fp32 - float64| <=
    7 U A (1 + 7 U)."""
    tmin, tmax = _slab64(o, d, bound)
    st = float(F(step))
    ri, k = m["ri"].numpy(), m["k"].numpy().astype(np.float64)
    u = np.zeros(o.shape[0]) if jit is None else jit.numpy().astype(np.float64)
    ts = tmin[ri] + u[ri] * st + k * st
    te = np.minimum(ts + st, tmax[ri])
    A = np.maximum(ts + st, tmax[ri])
    return ts, te, 7 * U * A * (1 + 7 * U)


def uniform_f64(o, d, jit, S, bound):
    """Float64 evaluation of uniform_samples for rays that hit -> (ts64 [N,S], te64 [N,S], bound_abs [N,S], hit [N]).
    Roundings on the path: the two quotients (2 each), t_far - t_near (1), the division by S + 1 (1), i + u or (i + 1) + u (1;
    i + 1 is exact), the product (1), the sum (1) = 7.  t_far - t_near cancels, so the magnitude the roundings act on is
    A = t_near + (i + 1 + u) (t_far + t_near) / (S + 1) >= every partial result.  |fp32 - float64| <= 7 U A (1 + 7 U)."""
    tmin, tmax = _slab64(o, d, bound)
    hit = (tmax > tmin) & np.isfinite(tmax)
    tmin, tmax = np.where(hit, tmin, 0.0), np.where(hit, tmax, 0.0)
    u = jit.numpy().astype(np.float64)[:, None]
    i = np.arange(S, dtype=np.float64)[None, :]
    dt = ((tmax - tmin) / (S + 1))[:, None]
    ts, te = tmin[:, None] + (i + u) * dt, tmin[:, None] + (i + 1.0 + u) * dt
    A = tmin[:, None] + (i + 1.0 + u) * ((tmax + tmin) / (S + 1))[:, None]
    return ts, te, 7 * U * A * (1 + 7 * U), hit


# -------------------------------------------------------------------------------------------------------- marcher cases
def marcher_cases():
    """One case per (jitter, grid): the finite ray set marched once by the oracle; every cap in CAPS is compared against the
    same result (slot_expect).  N = 58 rays."""
    out = []
    for u in JITTERS:
        rays = marcher_rays(u)
        for gname, grid in grids().items():
            out.append(dict(name=f"u={u}-{gname}", o=rays["o"], d=rays["d"], names=rays["names"], want_steps=rays["want_steps"],
                            jitter=jitter_tensor(u, rays["o"].shape[0]), u=u, grid=grid, gname=gname, step=STEP, bound=BOUND,
                            caps=CAPS, reaches="cap - 1 / cap / cap + 1 steps from inside, a face and outside; slab-clip edges; "
                                               "1-3 loop trips; both overflow halves; surplus into the next row and the guard"))
    return out


def small_n_cases():
    """N = 1, 3, 4, 5 (four rays per workgroup): the last workgroup partly filled, and exactly filled.  The rays are the long
    diagonal first (so that N = 1 overflows a short row into the guard) and count rays."""
    so, sd, sn = finite_specials()
    rays = marcher_rays(0.0)
    pick = [rays["names"].index(n) for n in ("count65_outside", "count21_inside", "count129_face", "count64_outside")]
    o = torch.cat([so[-1:], rays["o"][pick]])
    d = torch.cat([sd[-1:], rays["d"][pick]])
    g = grids()
    return [dict(name=f"N={N}", o=o[:N].contiguous(), d=d[:N].contiguous(), jitter=jitter_tensor(0.0, N), grid=g["random_R128"],
                 step=STEP, bound=BOUND, caps=(21, 64, 129), reaches="grid = (N + 3) / 4 workgroups") for N in (1, 3, 4, 5)]


def nonfinite_cases():
    """The rows of the miss rule at N = 8, on the full and the random grid, with and without jitter."""
    o, d, names, miss = nonfinite_rows()
    g = grids()
    return [dict(name=f"nonfinite-u={u}-{gn}", o=o, d=d, names=names, miss=miss, jitter=jitter_tensor(u, 8), u=u, grid=g[gn],
                 step=STEP, bound=BOUND, caps=(21, 129), reaches="the miss rule: NaN quotient, non-finite t_far")
            for u in (None, BELOW_ONE) for gn in ("full_R1", "random_R128")]


# ---------------------------------------------------------------------------------------------------------- retry cases
RETRY_STEP, RETRY_BOUND, RETRY_CAP = 0.2, 1.0, 21       # mh_march_cap(0.2, 1.0) = int(2 sqrt(3) / 0.2) + 4 = 21


def retry_cases():
    """Seven rays through march_rays at the real mh_march_cap = 21; ray 3 has its direction scaled down, so it takes 30 (1/3) or
    100 (1/10) steps.  Full grid: n > cap, the first half of the overflow condition, 1 / 3 doublings.  Empty grid: nothing is
    kept, so only the second half can fire -- it does for the 100-step ray (steps beyond the 64 walked: 2 doublings) and must NOT
    for the 30-step ray, whose every step was walked in the first trip."""
    g = synth.hash_tensor((7, 6), 6202, 1.0).numpy().astype(np.float64)
    o = np.array([gi[:3] / np.linalg.norm(gi[:3]) * 2.0 for gi in g])
    d = np.array([0.3 * gi[3:] - oi for gi, oi in zip(g, o)])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[3], d[3] = (0.1, -0.2, -2.0), (0.0, 0.0, 1.0)
    out = []
    for scale, tag in ((1.0 / 3.0, "third"), (0.1, "tenth")):
        dd = d.copy()
        dd[3] *= scale
        for gname, grid in (("full", torch.ones(2, 2, 2, dtype=torch.uint8)), ("empty", torch.zeros(2, 2, 2, dtype=torch.uint8))):
            caps = [RETRY_CAP]
            m = march_full(_t(o), _t(dd), jitter_tensor(0.25, 7), RETRY_STEP, RETRY_BOUND, grid)
            while slot_expect(m, caps[-1])[3]:
                caps.append(caps[-1] * 2)
            out.append(dict(name=f"retry-{tag}-{gname}", o=_t(o), d=_t(dd), jitter=jitter_tensor(0.25, 7), grid=grid,
                            step=RETRY_STEP, bound=RETRY_BOUND, caps_visited=caps, scaled_ray=3, oracle=m,
                            reaches="march_rays' retry: cap *= 2 and a new march into new slot rows"))
    return out


# ----------------------------------------------------------------------------------------------------------- pack cases
PACK_COUNTS = (65, 0, 1, 0, 63, 0, 64, 0, 129, 0, 0)


def pack_case():
    """Per-ray counts 65, 1, 63, 64, 129 with empty rays between and behind them, on the full grid: march_pack's loop runs 0, 1,
    2 and 3 trips, and every capacity of march_rays_capped below falls where it is named."""
    o, d = zip(*[count_ray(n, 0.0, "inside") for n in PACK_COUNTS])
    total = sum(PACK_COUNTS)
    caps = {"total": total, "total-1": total - 1, "mid-ray": 65 + 1 + 30, "ray-boundary": 65 + 1 + 63,
            "ray-boundary-before-empty": 65, "below-first-ray": 30, "one": 1}
    return dict(name="pack", o=_t(o), d=_t(d), jitter=jitter_tensor(0.0, len(PACK_COUNTS)), grid=torch.ones(1, 1, 1, dtype=torch.uint8),
                step=STEP, bound=BOUND, counts=PACK_COUNTS, total=total, capacities=caps,
                reaches="pack trips 0-3; capacities at, one below, inside a ray, at a ray boundary, below the first ray, 1")


def capped_expect(cnt, capacity: int):
    """(start, cnt_c, n_valid, overflow) of march_rays_capped from the ragged counts (no slot-row overflow)"""
    cnt = cnt.to(torch.int64)
    start = (torch.cumsum(cnt, 0) - cnt).clamp(max=capacity)
    cnt_c = torch.minimum(cnt, capacity - start)
    total = int(cnt.sum())
    return start, cnt_c, min(total, capacity), int(total > capacity)


# -------------------------------------------------------------------------------------------------------- pinhole rays
def pose(rx=0.4, ry=-0.7, rz=0.25, t=(0.6, -0.9, 2.4)):
    """a rotated, translated camera-to-world matrix [4,4] fp32 (no axis of the camera is a world axis)"""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = Rz @ Ry @ Rx, t
    return m.astype(F)


def pixel_rays(fx, fy, cx, cy, c2w, H, W, pix=None):
    """Pinhole rays of pixels pix (None: all H*W, row-major idx = j*W + i), fp32, one rounding per operation:
    camera direction ((i + .5 - cx) / fx, -((j + .5 - cy) / fy), -1), d = (d0 R[a,0] + d1 R[a,1]) + d2 R[a,2], o = translation.
    -> rays_o, rays_d [n, 3] torch fp32"""
    idx = np.arange(H * W, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64)
    j = idx // W
    i = idx - j * W
    fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
    c2w = np.asarray(c2w, dtype=F).reshape(4, 4)
    d0 = ((i.astype(F) + F(0.5)) - cx) / fx
    d1 = -(((j.astype(F) + F(0.5)) - cy) / fy)
    d2 = F(-1.0)
    d = np.stack([(d0 * c2w[a, 0] + d1 * c2w[a, 1]) + d2 * c2w[a, 2] for a in range(3)], -1).astype(F)
    o = np.broadcast_to(c2w[:3, 3], d.shape).astype(F)
    return _t(o), _t(d)


RAYGEN_SHAPES = ((17, 15), (16, 16), (257, 1))           # H x W: H*W = 255, 256, 257 around one 256-thread block


def raygen_cases():
    return [dict(name=f"{H}x{W}", H=H, W=W, fx=21.5, fy=17.25, cx=W * 0.5 + 1.75, cy=H * 0.5 - 2.5, c2w=pose(),
                 reaches="fx != fy, off-centre principal point, rotated pose; a block one short, full, one over") for H, W in RAYGEN_SHAPES]


# ------------------------------------------------------------------------------------------------- uniform sampler cases
UNIFORM_S = (1, 2, 7, 255, 256, 257)
UNIFORM_JITTERS = (0.0, BELOW_ONE)


def uniform_ray_sets():
    """name -> (o, d): the marcher's special rays (finite ones; the eight rows of the miss rule), and N = 1 / N = 3 slices of
    hits so that N * S straddles one 256-thread block (S = 255 .. 257) and three of them"""
    so, sd, _ = finite_specials()
    no, nd, _, _ = nonfinite_rows()
    hits = [6, 9, 13]                                    # inside_oblique, oblique0, long_diagonal
    return {"finite": (so, sd), "nonfinite": (no, nd), "N1": (so[hits[:1]].contiguous(), sd[hits[:1]].contiguous()),
            "N3": (so[hits].contiguous(), sd[hits].contiguous())}


def uniform_expect(o, d, jit, S, bound):
    """the oracle's samples plus everything else the kernel writes: -> ri int32, ts, te, xyz [N*S,3], ray_start, ray_cnt int32"""
    ri, ts, te = of.uniform_samples(o, d, jit, S, bound)
    tm = (ts + te) / 2.0
    xyz = o[ri] + d[ri] * tm[:, None]
    N = o.shape[0]
    return (ri.to(torch.int32), ts, te, xyz, (torch.arange(N, dtype=torch.int64) * S).to(torch.int32),
            torch.full((N,), S, dtype=torch.int32))


def fused_cases():
    """pixel sets for the fused ray generation + sampler: repeated indices and the last pixel; one-row and one-column images"""
    out = []
    for H, W in ((6, 9), (1, 7), (7, 1)):
        last = H * W - 1
        pix = [last, 0, last, 3 % (last + 1), 3 % (last + 1), last // 2, 0, last]
        out.append(dict(name=f"{H}x{W}", H=H, W=W, fx=7.5, fy=5.25, cx=W * 0.5 + 0.75, cy=H * 0.5 - 0.5, c2w=pose(),
                        pix=np.array(pix, dtype=np.int32), reaches="repeated pixels, pixel H*W - 1, H = 1, W = 1"))
    return out


def same_values(a, b) -> bool:
    """torch.equal with NaN == NaN (a missed ray with a NaN / infinite direction has xyz = o + d * 0 = NaN in both)"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a),
                                                                      torch.where(nb, torch.zeros_like(b), b))
