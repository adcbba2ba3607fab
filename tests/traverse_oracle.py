"""Float32 restatement of mh_est_traverse_slots (csrc/estimator.hip, `OccGridEstimator(traversal="dda")`), its float64 judge and
its cases -- test infrastructure, numpy on the CPU, scalar per ray, no GPU.  One rounding per operation, the kernel's operation
order; the kernel is held to it bit for bit.

The definition (include/morpheus_hip.h, mh_est_traverse_slots):
  1. clip, miss rule, planes and per-ray limits: points 1 - 3 of estimator_oracle.march, then t_near = t_near + u * step;
  2. level segments: (a_l, b_l) = clip against level l's box, coarse to fine, a_l = min(max(a_l, a_{l+1}), b_{l+1}),
     b_l = max(min(b_l, b_{l+1}), a_l), a miss a_l = b_l = b_{l+1}; a_{L-1}, b_{L-1} = t_near, t_far.  With the boundaries
     T = (a_{L-1}, ..., a_0, b_0, ..., b_{L-1}) segment j is [T_j, T_{j+1}] at level |L - 1 - j|; e <= s is skipped;
  3. cell spans: start cell clamp(floor(((o + d s) - lo) / (hi - lo) * R), 0, R - 1); plane k = lo + ((float)k / (float)R) * (hi - lo);
     exit of axis a = (plane(c_a + (d_a > 0)) - o_a) / d_a, +inf when d_a == 0; a span ends at x = max(min(min(min(tx, ty), tz), e),
     start); x >= e ends the segment, else the first axis (x, y, z) whose exit is the minimum is stepped and an index outside
     [0, R - 1] ends the segment; at most Rx + Ry + Rz + 3 spans a segment;
  4. runs: spans with end <= start are ignored; a run is a maximal sequence of consecutive occupied spans, [A, B];
  5. samples: A' = max(A, te of the ray's last sample); cone_angle == 0: ts_k = A' + (float)k * step, te_k = A' + (float)(k + 1) *
     step; cone_angle > 0: ts_0 = A', dt_k = min(max(ts_k * cone_angle, step), 1e10f), te_k = ts_k + dt_k, ts_{k+1} = te_k; kept
     while (ts_k + te_k) / 2 < B; te is not clamped.
The rule is this build's statement of nerfacc 0.5.x's traverse_grids as recalled, agreement unverified; point 5's max(A, last te)
is a deliberate departure (the recalled rule restarts at the cell entry and lets two samples overlap over a short gap).
"""
import numpy as np
import torch

from morpheus_amd import synth
from tests import estimator_oracle as eo
from tests import sampler_cases as sc
from tests.estimator_oracle import F, _np, _t, clip, level_aabbs

INF = F(np.inf)


# ----------------------------------------------------------------------------------------------------------- the definition
def ray_limits(o, d, jitter, step, aabbs, near_plane, far_plane, t_min, t_max):
    """points 1 and 2, every ray at once -> T fp32 [N, 2 L]: the segment boundaries of every ray"""
    L, N, st = aabbs.shape[0], o.shape[0], F(step)
    tn, tf = clip(o, d, aabbs[L - 1])
    tn = np.where(F(near_plane) > tn, F(near_plane), tn)
    if t_min is not None:
        v = _np(t_min)
        tn = np.where(v > tn, v, tn)
    tf = np.where(F(far_plane) < tf, F(far_plane), tf)
    if t_max is not None:
        v = _np(t_max)
        tf = np.where(v < tf, v, tf)
    u = np.zeros(N, F) if jitter is None else _np(jitter)
    tn = (tn + u * st).astype(F)
    a, b = [None] * L, [None] * L
    a[L - 1], b[L - 1] = tn, tf.astype(F)
    for l in range(L - 2, -1, -1):
        ca, cb = clip(o, d, aabbs[l])
        miss = cb == 0                                                  # a hit has t_far > t_near >= 0
        al = np.minimum(np.maximum(ca, a[l + 1]), b[l + 1])
        bl = np.maximum(np.minimum(cb, b[l + 1]), al)
        a[l], b[l] = np.where(miss, b[l + 1], al).astype(F), np.where(miss, b[l + 1], bl).astype(F)
    return np.stack(a[::-1] + b, -1).astype(F)


def ray_spans(o, d, T, aabbs, res):
    """point 3 for one ray -> list of (start, end, level, (cx, cy, cz)): every span in order, the zero-width ones included"""
    L = aabbs.shape[0]
    R = [int(r) for r in res]
    out = []
    for j in range(2 * L - 1):
        l, s, e = abs(L - 1 - j), T[j], T[j + 1]
        if not (e > s):
            continue
        lo, hi = aabbs[l, :3], aabbs[l, 3:]
        ext = hi - lo
        c, t = [0] * 3, [INF] * 3

        def exit_of(ax):
            if d[ax] == 0:
                return INF
            k = c[ax] + (1 if d[ax] > 0 else 0)
            plane = lo[ax] + (F(k) / F(R[ax])) * ext[ax]
            return (plane - o[ax]) / d[ax]

        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for ax in range(3):
                x = o[ax] + d[ax] * s
                v = np.floor(((x - lo[ax]) / ext[ax]) * F(R[ax]))
                c[ax] = int(min(max(0.0 if np.isnan(v) else float(v), 0.0), R[ax] - 1.0))
                t[ax] = exit_of(ax)
            cur = s
            for _ in range(R[0] + R[1] + R[2] + 3):
                m = min(min(t[0], t[1]), t[2])
                x = max(min(m, e), cur)
                out.append((cur, x, l, tuple(c)))
                if x >= e:
                    break
                ax = 0 if t[0] == m else (1 if t[1] == m else 2)
                c[ax] += 1 if d[ax] > 0 else -1
                if c[ax] < 0 or c[ax] >= R[ax]:
                    break
                t[ax] = exit_of(ax)
                cur = x
    return out


def ray_runs(spans, bn):
    """point 4 -> list of (A, B, first span index, last span index)"""
    runs, cur = [], None
    for i, (s, e, l, c) in enumerate(spans):
        if not (e > s):
            continue
        if bn[l, c[0], c[1], c[2]] != 0:
            cur = [s, e, i, i] if cur is None else [cur[0], e, cur[2], i]
        elif cur is not None:
            runs.append(tuple(cur))
            cur = None
    if cur is not None:
        runs.append(tuple(cur))
    return runs


def run_samples(A, B, last_te, step, cone):
    """point 5 for one run -> (ts, te) fp32 arrays"""
    st = F(step)
    A1 = A if last_te is None else max(A, last_te)
    if cone > 0:
        ts_l, te_l, ts = [], [], A1
        while True:
            dt = min(max(ts * cone, st), F(1e10))
            te = ts + dt
            if not ((ts + te) / F(2) < B):
                break
            ts_l.append(ts), te_l.append(te)
            ts = te
        return np.asarray(ts_l, F), np.asarray(te_l, F)
    n = int(max(float(B) - float(A1), 0.0) / float(st)) + 4
    k = np.arange(n, dtype=F)
    ts, te = A1 + k * st, A1 + (k + F(1)) * st
    keep = (ts + te) / F(2) < B
    m = n if keep.all() else int(np.argmin(keep))
    assert m < n
    return ts[:m].astype(F), te[:m].astype(F)


def traverse(rays_o, rays_d, jitter, step, aabbs, binaries, cone_angle=0.0, near_plane=0.0, far_plane=1e10, t_min=None, t_max=None):
    """-> estimator_oracle.march's dict (ri, ts, te, n_steps, k, N, cnt; k = the sample's number inside its ray and n_steps = cnt,
    which is how sampler_cases.slot_expect reads a kernel that fills its slot row sample by sample), and for the host tests
    `spans` / `runs` (per ray, as ray_spans / ray_runs give them) and `run_of` [M]: the run of every sample."""
    o, d = _np(rays_o), _np(rays_d)
    aabbs, bn = _np(aabbs), _np(binaries, np.uint8)
    res, N, cone = bn.shape[1:], o.shape[0], F(cone_angle)
    T = ray_limits(o, d, jitter, step, aabbs, near_plane, far_plane, t_min, t_max)
    ri, ts_all, te_all, k_all, run_of, spans_all, runs_all = [], [], [], [], [], [], []
    for r in range(N):
        spans = ray_spans(o[r], d[r], T[r], aabbs, res)
        runs = ray_runs(spans, bn)
        last, n = None, 0
        for q, (A, B, _, _) in enumerate(runs):
            ts, te = run_samples(A, B, last, step, cone)
            if ts.size:
                last = te[-1]
                ri.append(np.full(ts.size, r, np.int64)), ts_all.append(ts), te_all.append(te)
                k_all.append(np.arange(n, n + ts.size, dtype=np.int64)), run_of.append(np.full(ts.size, q, np.int64))
                n += ts.size
        spans_all.append(spans), runs_all.append(runs)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    ri_t = torch.from_numpy(cat(ri, np.int64))
    cnt = torch.bincount(ri_t, minlength=N) if ri_t.numel() else torch.zeros(N, dtype=torch.int64)
    return dict(ri=ri_t, ts=torch.from_numpy(cat(ts_all, F)), te=torch.from_numpy(cat(te_all, F)), n_steps=cnt.clone(),
                k=torch.from_numpy(cat(k_all, np.int64)), N=N, cnt=cnt, spans=spans_all, runs=runs_all, run_of=cat(run_of, np.int64), T=T)


def recalled_samples(rays_o, rays_d, jitter, step, aabbs, binaries, **kw):
    """the RECALLED rule (every run restarts at its own A): only to show the overlap that point 5's max(A, last te) removes"""
    m = traverse(rays_o, rays_d, jitter, step, aabbs, binaries, **kw)
    out = []
    for runs in m["runs"]:
        ts = [run_samples(A, B, None, step, F(kw.get("cone_angle", 0.0))) for A, B, _, _ in runs]
        out.append((np.concatenate([t[0] for t in ts]) if ts else np.zeros(0, F), np.concatenate([t[1] for t in ts]) if ts else np.zeros(0, F)))
    return out


# ------------------------------------------------------------------------------------------------------- the float64 judge
def judge(m, rays_o, rays_d, aabbs, binaries, ulps=4):
    """Float64: the midpoint of every sample lies in an occupied cell of the finest level holding it (lo <= x < hi, none: the
    coarsest).  -> (outside, set_aside, total): samples whose midpoint is in an empty cell, and the samples not judged because
    their midpoint is within `ulps` ulp (of t, fp32) of a boundary of one of the ray's spans."""
    o, d = _np(rays_o).astype(np.float64), _np(rays_d).astype(np.float64)
    a64, bn = _np(aabbs).astype(np.float64), _np(binaries, np.uint8)
    L, res = bn.shape[0], np.asarray(bn.shape[1:], np.float64)
    ri, ts, te = m["ri"].numpy(), m["ts"].numpy(), m["te"].numpy()
    outside = aside = 0
    edges = [np.unique(np.asarray([v for s in sp for v in s[:2]], np.float64)) if sp else np.zeros(0) for sp in m["spans"]]
    for i in range(ri.size):
        r = ri[i]
        tm = (float(ts[i]) + float(te[i])) / 2.0
        if edges[r].size and np.abs(edges[r] - tm).min() <= ulps * float(np.spacing(F(tm))):
            aside += 1
            continue
        x = o[r] + d[r] * tm
        lvl = L - 1
        for l in range(L - 1):
            if (a64[l, :3] <= x).all() and (x < a64[l, 3:]).all():
                lvl = l
                break
        c = np.clip(np.floor((x - a64[lvl, :3]) / (a64[lvl, 3:] - a64[lvl, :3]) * res), 0, res - 1).astype(np.int64)
        outside += int(bn[lvl, c[0], c[1], c[2]] == 0)
    return outside, aside, int(ri.size)


def coverage(m, step, cone_angle, ulps=4):
    """Float64, per run -> (late starts, runs past dt_next / 2, runs past dt_last / 2, runs with samples).  A run's first sample
    must start at max(A, the previous te of the ray).  Behind its last sample the run goes on for at most half of the step the
    next sample would have had, dt_next = min(max(te_last * cone_angle, step), 1e10) -- its midpoint is the first not before B;
    with cone_angle == 0 that is dt_last (both up to `ulps` fp32 ulp of t).  `worst`: the largest (B - te_last) / dt_last."""
    ri, ts, te, run_of = m["ri"].numpy(), m["ts"].numpy().astype(np.float64), m["te"].numpy().astype(np.float64), m["run_of"]
    st, cone = float(F(step)), float(F(cone_angle))
    late = short = short_last = n = 0
    for r, runs in enumerate(m["runs"]):
        sel = np.nonzero(ri == r)[0]
        prev = None
        for q, (A, B, _, _) in enumerate(runs):
            idx = sel[run_of[sel] == q]
            if idx.size == 0:
                continue
            n += 1
            want = float(A) if prev is None else max(float(A), prev)
            late += int(ts[idx[0]] != want)
            t_last = te[idx[-1]]
            dt_last, dt_next = t_last - ts[idx[-1]], min(max(t_last * cone, st), 1e10)
            band = ulps * float(np.spacing(F(B)))
            short += int(float(B) - t_last > dt_next / 2.0 + band)
            short_last += int(float(B) - t_last > dt_last / 2.0 + band)
            prev = t_last
    return late, short, short_last, n


# --------------------------------------------------------------------------------------------------------------- the grids
BOX1 = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
BOX40 = (-0.3, 0.1, -0.6, 0.7, 0.9, 0.6)                     # estimator_oracle.UPD_ROOT: non-centred, not exact in fp32
STEP, U = 0.02, 0.37
SEED40 = 9100


def grid_full8():
    return _t(level_aabbs(BOX1, 1)), torch.ones(1, 8, 8, 8, dtype=torch.uint8)


def grid_rand40(seed=SEED40):
    return _t(level_aabbs(BOX40, 1)), (synth.hash_tensor((1, 40, 40, 40), seed, 0.5, 0.5) < 0.35).to(torch.uint8).contiguous()


def grid_levels3():
    aabbs, _ = eo.marcher_grid()
    return aabbs, (synth.hash_tensor((eo.LEVELS,) + eo.RES, 9200, 0.5, 0.5) < 0.35).to(torch.uint8).contiguous()


def grid_empty():
    aabbs, b = grid_levels3()
    return aabbs, torch.zeros_like(b)


GRIDS = {"full8": grid_full8, "rand40": grid_rand40, "levels3": grid_levels3, "empty": grid_empty}


def aimed_rays(n, box, seed, radius=3.0):
    """n rays from a sphere of `radius` box half-diagonals about the box centre, aimed at hashed points inside the box, unit length"""
    b = np.asarray(box, np.float64)
    c, h = (b[:3] + b[3:]) / 2, (b[3:] - b[:3]) / 2
    v = synth.hash_tensor((n, 3), seed, 1.0, 0.0).numpy().astype(np.float64)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    o = c + v * radius * np.linalg.norm(h)
    tgt = c + synth.hash_tensor((n, 3), seed + 1, 0.95, 0.0).numpy().astype(np.float64) * h
    d = tgt - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return [(f"aimed{i}", tuple(o[i].astype(F).tolist()), tuple(d[i].astype(F).tolist())) for i in range(n)]


def _case(name, grid, rays, reaches, **kw):
    c = eo._case(name, rays, reaches, **{"step": STEP, **kw})
    c["grid"] = grid
    return c


def diagonal_rays(box):
    """the four body diagonals of `box` in both directions, from outside the box, unit length: more than 64 cells of a 40^3 grid"""
    b = np.asarray(box, np.float64)
    c, h = (b[:3] + b[3:]) / 2, (b[3:] - b[:3]) / 2
    rows = []
    for i, sg in enumerate(((1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (-1, -1, -1), (-1, -1, 1), (-1, 1, -1), (-1, 1, 1))):
        s = np.asarray(sg, np.float64)
        # shifted off the exact diagonal, so that the three axes do not step at the same instant
        o = c - 1.25 * s * h + np.array([0.013, -0.007, 0.004]) * (i + 1)
        d = s * h / np.linalg.norm(h)
        rows.append((f"diag{i}", tuple(o.astype(F).tolist()), tuple(d.astype(F).tolist())))
    return rows


def levels3_rays():
    return [("inside_l0", (0.5, 0.25, 0.75), (0.6, 0.0, 0.8)),                      # starts at the centre of level 0
            ("inside_l0_neg", (0.45, 0.3, 0.8), (-0.48, -0.6, -0.64)),
            ("misses_l0", (-0.4, 1.4, -1.0), (0.0, 0.0, 1.0)),                      # y = 1.4: outside levels 0 and 1, inside level 2
            ("misses_l0_l1_oblique", (-0.45, -1.2, -1.2), (0.0, 0.6, 0.8)),
            ("through_all", (-1.5, 0.2, 0.7), (1.0, 0.0, 0.0)),
            ("through_l1", (-1.5, 0.8, 0.7), (1.0, 0.0, 0.0))] + aimed_rays(26, eo.ROOT, 9300, radius=4.0)


def degenerate_rays():
    a = level_aabbs(eo.ROOT, eo.LEVELS)
    return [("one_zero", (-1.0, 0.2, 0.7), (0.8, 0.6, 0.0)),
            ("one_zero_neg", (2.0, 1.0, 0.9), (-0.8, -0.6, 0.0)),
            ("two_zero_x", (-1.0, 0.3, 0.8), (1.0, 0.0, 0.0)),
            ("two_zero_y_neg", (0.6, 2.5, 1.1), (0.0, -1.0, 0.0)),
            ("two_zero_z", (0.3, 0.1, -2.0), (0.0, 0.0, 1.0)),
            ("in_face_plane", (-1.0, float(a[2, 4]), 0.75), (1.0, 0.0, 0.0)),         # y ON the coarsest hi face: the miss rule
            ("on_face_leaving", (-0.5, 0.25, 0.75), (-1.0, 0.0, 0.0)),
            ("through_edge", (-1.5, -2.25, 0.75), (1.0, 1.0, 0.0)),                   # meets the coarsest box at its edge x = -0.5, y = -1.25
            ("through_l0_edge", (-0.75, -1.125, 0.75), (1.0, 1.0, 0.0)),              # and level 0 at its edge x = 0.25, y = -0.125
            ("through_corner", (-1.5, -2.25, -2.25), (1.0, 1.0, 1.0)),
            ("all_negative", (1.4, 1.6, 2.6), (-0.48, -0.6, -0.64)),
            ("neg_x", (1.4, 0.3, 0.7), (-1.0, 0.0, 0.0)),
            ("neg_yz", (0.5, 1.7, 2.7), (0.0, -0.6, -0.8))]


def plane_rays():
    """the same +z ray through the middle of the root box under different limits; three jitters each (per ray)"""
    names = ["planes_only", "tmin_raises", "tmax_cuts", "tmax_lt_tmin"]
    big = 3.0e38
    tmin, tmax = [0.0, 1.93, 0.0, 2.2], [big, big, 2.31, 1.4]
    rows, lo, hi, js = [], [], [], []
    for u in (0.0, U, sc.BELOW_ONE):
        for nm, a, b in zip(names, tmin, tmax):
            rows.append((f"{nm}_u{u:.2f}", (0.5, 0.25, -1.75), (0.0, 0.0, 1.0)))
            rows.append((f"{nm}_oblique_u{u:.2f}", (-0.3, -0.9, -1.0), (0.36, 0.48, 0.8)))
            lo.extend([a, a]), hi.extend([b, b]), js.extend([u, u])
    return rows, _t(lo), _t(hi), _t(js)


def cases():
    pr, p_lo, p_hi, p_j = plane_rays()
    out = [
        _case("full8", "full8", [("corner", (-1.25, -1.25, -1.25), tuple([float(F(1) / np.sqrt(F(3)))] * 3)),
                                 ("corner_back", (1.2, 1.25, 1.3), tuple([-float(F(1) / np.sqrt(F(3)))] * 3))] + aimed_rays(6, BOX1, 9400),
              "one run a ray, more than 64 samples: the sample writer takes several rounds", jitter=U),
        _case("rand40", "rand40", diagonal_rays(BOX40) + aimed_rays(24, BOX40, 9500),
              "more than 64 cells a ray: a run open across spans 63 / 64 and an empty span exactly there", jitter=U),
        _case("levels3", "levels3", levels3_rays(), "runs across level changes, a start inside level 0, a miss of level 0", jitter=U),
        _case("degenerate", "levels3", degenerate_rays(), "zero components, a face plane, edges and corners, negative directions", jitter=U),
        _case("planes", "levels3", pr, "planes cutting a cell, t_min / t_max, t_max < t_min, jitters 0 / 0.37 / below one",
              near_plane=1.07, far_plane=3.13, t_min=p_lo, t_max=p_hi, jitter=p_j),
        _case("rand40-cone", "rand40", diagonal_rays(BOX40) + aimed_rays(24, BOX40, 9500), "rand40 with cone steps", jitter=U, cone_angle=0.01),
        _case("levels3-cone", "levels3", levels3_rays(), "levels3 with cone steps", jitter=U, cone_angle=0.01),
        _case("empty", "empty", levels3_rays()[:8], "no occupied cell: no sample", jitter=U),
    ]
    return out


def overflow_case():
    """a direction a third of unit length on the full 8^3 grid at step 0.05: mh_est_march_cap = int(sqrt(12) / 0.05) + 4 = 73, the
    scaled ray's chord is 6 in t: 120 samples, more than one slot row and fewer than two -> one doubling"""
    rows = [("scaled", (-1.5, 0.1, 0.2), (float(F(1) / F(3)), 0.0, 0.0)),
            ("unit", (-1.5, 0.1, 0.2), (1.0, 0.0, 0.0)),
            ("oblique", (-1.5, -1.2, -0.9), (0.6, 0.48, 0.64))]
    return _case("overflow", "full8", rows, "a slot row that overflows once and is retried", step=0.05, jitter=U, cap=73)


def run_case(c, grid=None):
    aabbs, binaries = GRIDS[c["grid"]]() if grid is None else grid
    return traverse(c["o"], c["d"], c["jitter"], c["step"], aabbs, binaries, c["cone_angle"], c["near_plane"], c["far_plane"],
                    c["t_min"], c["t_max"])
