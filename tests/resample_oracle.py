"""numpy restatements of importance resampling (csrc/resample.hip) -- test infrastructure, no GPU.

    sample_pdf_np       the reference's utils.sample_pdf (utils.py:17-42), statement by statement, in float64 or fp32
    resample_packed_np  the packed form: per ray, draws at u_k = (k + j_k) / n from the piecewise-constant pdf over the ray's own
                        intervals, each held inside its interval, and the coarse intervals cut at them (a merge by rank)
    score               the measure the suites judge samples by
    cases / make_case   the dense cases of the golden (tests/golden/sample_pdf.npz, tools/make_resample_golden.py)
    sphere_*            the analytic sphere with a Laplace density (the refinement property)

cdf="reference": weights + eps, a sum, a division and a running sum in the working precision, as torch executes them on the CPU
(its cumsum accumulates fp32 terms in float64 and rounds every output once; its sum is a pairwise fp32 sum, as numpy's).
cdf="kernel": what the kernel stores -- the sum and the running sum in float64, each rounded to fp32 once, then a running maximum.
"""
import numpy as np

U = 2.0 ** -24
EPS = 1e-5

T_SET = (2, 3, 64, 65, 66, 129, 200)
N_SET = (1, 63, 64, 65, 128)
B_SET = (1, 4, 5, 9)
KINDS = ("laplace", "uniform", "zero", "sparse", "span20")


# ---------------------------------------------------------------------------------------------------------------- dense form
def cdf_np(weights, eps, dtype, cdf="reference"):
    """[B, c] weights -> [B, c + 1] CDF with the leading 0"""
    w = np.asarray(weights, dtype=dtype) + dtype(eps)
    if cdf == "kernel":
        assert dtype == np.float32
        total = w.astype(np.float64).sum(-1, keepdims=True).astype(np.float32)
        pdf = w / total
        c = np.cumsum(pdf.astype(np.float64), -1).astype(np.float32)
        c = np.maximum.accumulate(np.maximum(c, np.float32(0)), -1)
    else:
        pdf = w / np.sum(w, -1, keepdims=True, dtype=dtype)
        # torch's CPU cumsum carries fp32 terms in a float64 accumulator and rounds each output once (a plain fp32 running
        # sum scores up to 28 U at T = 200 where the reference's own run scores 2.4 U)
        c = np.cumsum(pdf.astype(np.float64), -1).astype(dtype)
    return np.concatenate([np.zeros_like(c[..., :1]), c], -1)


def invert_np(cdf_row, u, lo_edge, hi_edge, dtype, hold=False):
    """the inverse-CDF statements for one row: cdf_row [T], u [n]; lo_edge(below), hi_edge(below, above) -> the bin's two ends.
    -> (samples [n], below [n]).  hold: the kernel's last statement, the sample held inside its bin."""
    T = cdf_row.shape[0]
    inds = np.searchsorted(cdf_row, u, side="right")
    below, above = np.maximum(inds - 1, 0), np.minimum(inds, T - 1)
    denom = cdf_row[above] - cdf_row[below]
    denom = np.where(denom < dtype(1e-5), dtype(1), denom)
    t = (u - cdf_row[below]) / denom
    b0, b1 = lo_edge(below), hi_edge(below, above)
    s = b0 + t * (b1 - b0)
    if hold:
        s = np.minimum(np.maximum(s, np.minimum(b0, b1)), np.maximum(b0, b1))
    return s.astype(dtype), below


def sample_pdf_np(bins, weights, u, dtype=np.float64, cdf="reference", hold=False):
    """utils.sample_pdf with the draws given: bins [B, T], weights [B, T - 1], u [B, n] -> samples [B, n]"""
    bins, u = np.asarray(bins, dtype=dtype), np.asarray(u, dtype=dtype)
    c = cdf_np(weights, EPS, dtype, cdf)
    out = np.empty(u.shape, dtype=dtype)
    for b in range(bins.shape[0]):
        row = bins[b]
        out[b], _ = invert_np(c[b], u[b], lambda lo: row[lo], lambda lo, hi: row[hi], dtype, hold)
    return out


# ---------------------------------------------------------------------------------------------------------------- the measure
def cdf64_range(ts, te, weights, s, eps=EPS):
    """The float64 piecewise-linear CDF of (weights + eps) over the intervals [ts_i, te_i] at the positions s -> (low, high):
    the CDF's value, or the two ends of its jump where s sits on zero-width intervals."""
    ts, te, s = (np.asarray(a, dtype=np.float64) for a in (ts, te, s))
    w = np.asarray(weights, dtype=np.float64) + eps
    pdf = w / w.sum()
    width = te - ts
    frac = np.clip((s[:, None] - ts[None]) / np.where(width > 0, width, 1.0)[None], 0.0, 1.0)
    flat = (width <= 0)[None]
    lo = np.where(flat, (s[:, None] > te[None]).astype(np.float64), frac)
    hi = np.where(flat, (s[:, None] >= ts[None]).astype(np.float64), frac)
    return (lo * pdf[None]).sum(-1), (hi * pdf[None]).sum(-1)


def score(s, s64, u, ts, te, weights, eps=EPS):
    """e = min(|s - s64| / (last edge - first edge), |CDF64(s) - u|) per sample of one row.  Sample position is ill-conditioned
    where the CDF is flat, CDF position where it is steep; a sample is judged by the better of the two.  A row of zero extent
    scores 0 where s == s64 and inf elsewhere."""
    s, s64, u = (np.asarray(a, dtype=np.float64) for a in (s, s64, u))
    span = float(np.max(te) - np.min(ts))
    with np.errstate(divide="ignore", invalid="ignore"):
        e_pos = np.where(s == s64, 0.0, np.abs(s - s64) / span if span > 0 else np.inf)
    lo, hi = cdf64_range(ts, te, weights, s, eps)
    e_cdf = np.where((lo <= u) & (u <= hi), 0.0, np.minimum(np.abs(lo - u), np.abs(hi - u)))
    return np.minimum(e_pos, e_cdf)


def score_dense(s, s64, u, bins, weights):
    """worst score over the rows of a dense case"""
    worst = 0.0
    for b in range(np.asarray(bins).shape[0]):
        worst = max(worst, float(score(s[b], s64[b], u[b], bins[b][:-1], bins[b][1:], weights[b]).max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------- packed form
def resample_packed_np(ray_start, ray_cnt, t_starts, t_ends, weights, n, jitter=None, eps=EPS, dtype=np.float32, cdf="reference"):
    """-> dict(ray_idx, t_starts, t_ends, ray_start, ray_cnt, draws): `draws` a list per ray of (u [n], s [n], interval [n]),
    None for an empty ray.  jitter [N, n] or None (0.5)."""
    rs, rc = np.asarray(ray_start, dtype=np.int64), np.asarray(ray_cnt, dtype=np.int64)
    N = rs.shape[0]
    new_cnt = np.where(rc > 0, rc + n, 0)
    new_start = np.cumsum(new_cnt) - new_cnt
    M_out = int(new_cnt.sum())
    o_ri = np.zeros(M_out, dtype=np.int32)
    o_ts, o_te = np.zeros(M_out, dtype=dtype), np.zeros(M_out, dtype=dtype)
    draws = []
    for r in range(N):
        c = int(rc[r])
        if c <= 0:
            draws.append(None)
            continue
        sl = slice(int(rs[r]), int(rs[r]) + c)
        ts, te = np.asarray(t_starts[sl], dtype=dtype), np.asarray(t_ends[sl], dtype=dtype)
        row = cdf_np(np.asarray(weights[sl])[None], eps, dtype, cdf)[0]
        # the draws are part of the definition and are formed in fp32 whatever the working precision: u_k = (k + j_k) / n
        j = np.full(n, 0.5, dtype=np.float32) if jitter is None else np.asarray(jitter[r], dtype=np.float32)
        u = ((np.arange(n, dtype=np.float32) + j) / np.float32(n)).astype(dtype)
        lo_edge = lambda lo: np.where(lo < c, ts[np.minimum(lo, c - 1)], te[c - 1])
        hi_edge = lambda lo, hi: np.where(hi == lo, lo_edge(lo), te[np.minimum(lo, c - 1)])
        s, below = invert_np(row, u, lo_edge, hi_edge, dtype, hold=True)
        iv = np.minimum(below, c - 1)
        draws.append((u, s, iv))
        ob = int(new_start[r])
        kk = np.arange(n)
        o_te[ob + iv + kk] = s
        o_ts[ob + iv + kk + 1] = s
        m = np.bincount(iv, minlength=c)
        lo = np.cumsum(m) - m
        i = np.arange(c)
        o_ts[ob + i + lo] = ts
        o_te[ob + i + lo + m] = te
        o_ri[ob:ob + c + n] = r
    return dict(ray_idx=o_ri, t_starts=o_ts, t_ends=o_te, ray_start=new_start.astype(np.int32), ray_cnt=new_cnt.astype(np.int32),
                draws=draws)


def draws_of(out_ts_row, coarse_ts):
    """the n drawn points of one ray's refined t_starts, in order: the row minus one occurrence of every coarse start (an
    AssertionError if a coarse start is missing).  A draw equal to a coarse start is indistinguishable from it -- and has its value."""
    rest = list(np.asarray(out_ts_row).tolist())
    for v in np.asarray(coarse_ts).tolist():
        assert v in rest, f"coarse start {v!r} is not among the refined starts"
        rest.remove(v)
    return np.sort(np.asarray(rest, dtype=np.asarray(out_ts_row).dtype))


def check_invariants(out, ray_start, ray_cnt, t_starts, t_ends, n):
    """The exact invariants of a refined set `out` (dict of numpy arrays: ray_idx, t_starts, t_ends, ray_start, ray_cnt) against
    the coarse one.  Everything is compared as values of the arrays' own type, nothing to a tolerance."""
    rs, rc = np.asarray(ray_start, dtype=np.int64), np.asarray(ray_cnt, dtype=np.int64)
    o_rs, o_rc = np.asarray(out["ray_start"], dtype=np.int64), np.asarray(out["ray_cnt"], dtype=np.int64)
    o_ts, o_te, o_ri = np.asarray(out["t_starts"]), np.asarray(out["t_ends"]), np.asarray(out["ray_idx"])
    assert np.array_equal(o_rc, np.where(rc > 0, rc + n, 0)), "per-ray counts are c + n, 0 for an empty ray"
    assert np.array_equal(o_rs, np.cumsum(o_rc) - o_rc), "ray_start is the exclusive scan of ray_cnt"
    total = int(o_rc.sum())
    assert o_ts.shape[0] >= total and o_te.shape[0] >= total and o_ri.shape[0] >= total
    assert np.array_equal(o_ri[:total], np.repeat(np.arange(rs.shape[0]), o_rc)), "ray_indices follow ray_start / ray_cnt"
    assert bool((np.diff(o_ri[:total]) >= 0).all())
    for r in range(rs.shape[0]):
        c = int(rc[r])
        if c <= 0:
            continue
        ts, te = np.asarray(t_starts[rs[r]:rs[r] + c]), np.asarray(t_ends[rs[r]:rs[r] + c])
        a, b = o_ts[o_rs[r]:o_rs[r] + c + n], o_te[o_rs[r]:o_rs[r] + c + n]
        assert bool((np.diff(a) >= 0).all()), (r, "t_starts non-decreasing")
        assert bool((b >= a).all()), (r, "t_ends >= t_starts")
        # walk the refined intervals through the coarse ones: inside coarse interval i the pieces start at ts_i, chain edge to
        # edge bit for bit, and end at te_i -- the widths telescope as edges; a piece that is not chained would sit in a gap
        # (a coarse interval ends at the first piece that ends at te_i and is followed by ts_{i+1}; where a zero-width piece
        # could belong to either neighbour the two readings have the same values; the last interval takes every piece left)
        last, p = c + n - 1, 0
        for i in range(c):
            assert p <= last and a[p] == ts[i], (r, i, p, "the coarse start is present unchanged")
            while True:
                assert ts[i] <= a[p] and b[p] <= te[i], (r, i, p, "no draw lies in a gap")
                if i == c - 1:
                    done = p == last
                else:
                    done = b[p] == te[i] and p < last and a[p + 1] == ts[i + 1]
                if done:
                    break
                assert p < last and a[p + 1] == b[p], (r, i, p, "pieces of one coarse interval share their cut points bit for bit")
                p += 1
            assert b[p] == te[i], (r, i, p, "the coarse end is present unchanged")
            p += 1
        assert p == c + n, (r, p, c + n)


# ---------------------------------------------------------------------------------------------------------------- dense cases
def cases():
    """(name, T, n, B, kind) of the golden: every T with every kind of weights, n and B cycling so that each is met"""
    out = []
    for ti, T in enumerate(T_SET):
        for ki, kind in enumerate(KINDS):
            i = ti * len(KINDS) + ki
            n, B = N_SET[(i + ti) % len(N_SET)], B_SET[(i + ki) % len(B_SET)]
            out.append((f"T{T}_{kind}", T, n, B, kind))
    return out


def laplace_weights(bins, depth, beta):
    """rendering weights of a Laplace-density surface at `depth` [B] on the intervals of bins [B, T] (float64)"""
    mid, dt = 0.5 * (bins[:, 1:] + bins[:, :-1]), np.diff(bins, axis=-1)
    sdf = depth[:, None] - mid
    sigma = np.where(sdf > 0, 0.5 * np.exp(-np.abs(sdf) / beta), 1.0 - 0.5 * np.exp(-np.abs(sdf) / beta)) / beta
    x = sigma * dt
    trans = np.exp(-(np.cumsum(x, -1) - x))
    return trans * (1.0 - np.exp(-x))


def make_case(T, n, B, kind, seed):
    """fp32 inputs of one dense case: equal-step bins with a per-ray offset (how a marcher makes them), weights of `kind`, draws
    with the first two forced to 0 and 1 - 2^-24"""
    rng = np.random.default_rng(seed)
    step = np.float32(2.0 / max(T - 1, 1) if T < 64 else 0.01)
    t0 = (0.5 + rng.random(B)).astype(np.float32)
    bins = (t0[:, None] + np.arange(T, dtype=np.float32)[None] * step).astype(np.float32)
    if kind == "laplace":
        depth = bins[:, 0].astype(np.float64) + rng.random(B) * (bins[:, -1] - bins[:, 0]).astype(np.float64)
        w = laplace_weights(bins.astype(np.float64), depth, 0.02)
    elif kind == "uniform":
        w = rng.random((B, T - 1))
    elif kind == "zero":
        w = np.zeros((B, T - 1))
    elif kind == "sparse":
        w = rng.random((B, T - 1)) * (rng.random((B, T - 1)) >= 0.8)
    else:
        w = 2.0 ** (-20.0 * rng.random((B, T - 1)))
    u = rng.random((B, n)).astype(np.float32)
    u = np.minimum(u, np.float32(1 - U))
    if n > 1:
        u[:, 0], u[:, 1] = 0.0, np.float32(1 - U)
    else:                                   # one draw a row: the two forced values go to the first two rows
        u[0, 0] = 0.0
        u[1:2, 0] = np.float32(1 - U)
    return bins, w.astype(np.float32), u


# ---------------------------------------------------------------------------------------------------------------- the sphere
def sphere_rays(n_rays=256, seed=0):
    """rays from z = -1.5 towards +z on a disc of radius 0.45 around the axis: origins [n, 3], unit directions [n, 3]"""
    rng = np.random.default_rng(seed)
    rad, ang = 0.45 * np.sqrt(rng.random(n_rays)), 2 * np.pi * rng.random(n_rays)
    o = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(n_rays, -1.5)], -1)
    d = np.tile(np.array([0.0, 0.0, 1.0]), (n_rays, 1))
    return o, d


def sphere_sigma(o, d, t, beta, radius=0.5):
    """Laplace density of the sphere's SDF at o + d t (t [n, S]), float64"""
    x = o[:, None, :] + d[:, None, :] * t[..., None]
    sdf = np.linalg.norm(x, axis=-1) - radius
    return np.where(sdf > 0, 0.5 * np.exp(-np.abs(sdf) / beta), 1.0 - 0.5 * np.exp(-np.abs(sdf) / beta)) / beta


def render_depth(ts, te, sigma):
    """midpoint-rule depth sum w_i (ts_i + te_i) / 2 and the weights, rows = rays, float64"""
    x = sigma * (te - ts)
    trans = np.exp(-(np.cumsum(x, -1) - x))
    w = trans * (1.0 - np.exp(-x))
    return (w * 0.5 * (ts + te)).sum(-1), w
