"""numpy restatement of visibility pruning, written from the text of include/morpheus_hip.h ("visibility pruning of packed
samples"), not from csrc/visibility.hip.

mask(..., f64=False) is the reading aid: float32 values, the sum of a ray taken sample after sample.  The kernel sums a ray
with a wave scan, i.e. in another order, so the fp32 form is not a bit-level pin; mask(..., f64=True) is what the GPU test
compares with, together with band(): the samples whose float64 transmittance / opacity lies so close to its threshold that
float32 arithmetic may decide either way.
"""
import numpy as np


def alpha_thre_eff(alpha_thre, occs):
    """min(alpha_thre, mean(occs)): the opacity threshold in force when a sigma_fn / alpha_fn is given"""
    return min(float(alpha_thre), float(np.mean(np.asarray(occs, dtype=np.float64))))


def mask(values, t_starts, t_ends, ray_start, ray_cnt, early_stop_eps, alpha_thre=0.0, alpha_form=False, f64=False):
    """-> dict(keep uint8 [M], kept_cnt int32 [N], T [M], alpha [M], S [M] exclusive sums, cnt_of [M] the owning ray's count).
    Entries no ray owns keep 0."""
    ft = np.float64 if f64 else np.float32
    v = np.asarray(values, dtype=np.float32).astype(ft)
    M, N = v.shape[0], len(ray_start)
    keep = np.zeros(M, np.uint8)
    T, A, S = np.zeros(M, ft), np.zeros(M, ft), np.zeros(M, ft)
    cnt_of = np.zeros(M, np.int64)
    kept = np.zeros(N, np.int32)
    eps, thre = ft(early_stop_eps), ft(alpha_thre)
    with np.errstate(all="ignore"):
        for r in range(N):
            s, c = int(ray_start[r]), int(ray_cnt[r])
            if c == 0:
                continue
            vv = v[s:s + c]
            if alpha_form:
                ok = ~np.isnan(vv)
                a = np.clip(np.where(ok, vv, 0), 0, 1).astype(ft)
                x = (-np.log1p(-a)).astype(ft)
            else:
                d = (np.asarray(t_ends[s:s + c], np.float32).astype(ft) - np.asarray(t_starts[s:s + c], np.float32).astype(ft)).astype(ft)
                x = (vv * d).astype(ft)
                ok = ~np.isnan(x)
                x = np.maximum(np.where(ok, x, 0), 0).astype(ft)
                a = (-np.expm1(-x)).astype(ft)
            x = np.where(ok, x, 0).astype(ft)                       # a dropped sample adds 0
            excl = np.concatenate([[ft(0)], np.cumsum(x, dtype=ft)[:-1]]).astype(ft)      # sequential, in order
            t = np.exp(-excl).astype(ft)
            k = ok & (t >= eps) & (a >= thre)
            keep[s:s + c], T[s:s + c], A[s:s + c], S[s:s + c], cnt_of[s:s + c] = k, t, a, excl, c
            kept[r] = int(k.sum())
    return dict(keep=keep, kept_cnt=kept, T=T, alpha=A, S=S, cnt_of=cnt_of)


def band(m64, early_stop_eps, alpha_thre):
    """bool [M]: samples whose float64 T / alpha (mask(..., f64=True)) lie inside the float32 error band of their threshold.
      T:     |T - eps| <= eps * (cnt_r + 4) * 2^-23 * max(S, 1)   -- the sum of cnt_r terms of <= 1 ulp each, summed with
             <= 1 ulp per addition, moves S by <= cnt_r * 2^-23 * S, which is the RELATIVE move of T = exp(-S); expf, the carry
             and the product sigma * D account for the 4 further ulps (of T, or of S where S > 1);
      alpha: |alpha - thre| <= 4 ulp(alpha): D (exact or 1/2 ulp), sigma * D (1/2 ulp), expm1f (<= 2 ulp)."""
    T, A, S, c = m64["T"], m64["alpha"], m64["S"], m64["cnt_of"]
    u = 2.0 ** -23
    with np.errstate(all="ignore"):
        Sf = np.where(np.isfinite(S), S, 0.0)                       # behind an opaque sample T is exactly 0 in any arithmetic
        bt = (early_stop_eps > 0) & (np.abs(T - early_stop_eps) <= early_stop_eps * (c + 4) * u * np.maximum(Sf, 1.0))
        ba = (alpha_thre > 0) & (np.abs(A - alpha_thre) <= 4 * np.spacing(A.astype(np.float32)).astype(np.float64))
    return (bt | ba) & (c > 0)


def pack(keep, t_starts, t_ends, ray_start, ray_cnt, capacity=None):
    """numpy's compaction of the packed samples by `keep` -> (ray_idx, t_starts, t_ends, ray_start, ray_cnt, src_index[, n_valid]);
    capacity: outputs of that length, the rest the marcher's padding (ray 0, t = 0; src_index 0)."""
    N = len(ray_start)
    src = []
    rc = np.zeros(N, np.int32)
    for r in range(N):
        s, c = int(ray_start[r]), int(ray_cnt[r])
        idx = s + np.nonzero(keep[s:s + c])[0]
        src.append(idx)
        rc[r] = len(idx)
    src = np.concatenate(src).astype(np.int32) if src else np.zeros(0, np.int32)
    rs = (np.cumsum(rc) - rc).astype(np.int32)
    ri = np.repeat(np.arange(N, dtype=np.int32), rc)
    ts, te = np.asarray(t_starts, np.float32)[src], np.asarray(t_ends, np.float32)[src]
    if capacity is None:
        return ri, ts, te, rs, rc, src
    pad = lambda a: np.concatenate([a, np.zeros(capacity - len(a), a.dtype)])
    return pad(ri), pad(ts), pad(te), rs, rc, pad(src), np.int32(len(src))


# ---- the fixture of the GPU mask test (tests/test_gpu_visibility.py), shared with the host test that holds it under its cap ----
EPS_CASES = (0.0, 1e-4, 1e-2)
THRE_CASES = (0.0, 1e-3, 1e-2)
BAND_CAP = 1e-3          # share of the samples that may disagree with the float64 oracle, all of them inside the band


def fixture(n_rays=2048, seed=7, alpha_form=False):
    """Ragged rays of 0 ... 350 samples of step 0.01: counts drawn uniformly, plus rays that end on a chunk boundary (64, 128,
    320), one past it (65, 129), an empty ray, a ray whose every sample is dropped (NaN) and one whose every sample is kept
    under every case (sigma = 2: alpha = 0.0198 > 1e-2, T >= exp(-2) > 1e-2).  Densities: a per-ray scale, log-uniform over
    [0.1, 300], times a log-normal per sample -- continuous, so that a float64 T or alpha within rounding of a threshold is an
    accident (a few in 10^5), not a property of the data; some negative and NaN values.  The alpha form feeds 1 - exp(-sigma D)
    of the same densities, kept strictly below 1.
    -> dict(values, t_starts, t_ends, ray_start, ray_cnt, all_dropped, all_kept) of numpy arrays / ray numbers."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 351, n_rays).astype(np.int32)
    special = {0: 0, 1: 64, 2: 128, 3: 320, 4: 65, 5: 129, 6: 350, 7: 1, 8: 100, 9: 100}
    for r, c in special.items():
        cnt[r] = c
    start = (np.cumsum(cnt) - cnt).astype(np.int32)
    M = int(cnt.sum())
    ray = np.repeat(np.arange(n_rays), cnt)
    k = np.arange(M) - start[ray]
    t0 = rng.uniform(0.2, 1.5, n_rays).astype(np.float32)
    ts = (t0[ray] + k.astype(np.float32) * np.float32(0.01)).astype(np.float32)
    te = (ts + np.float32(0.01)).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(0.1), np.log(300.0), n_rays))
    sigma = (scale[ray] * np.exp(rng.normal(0.0, 1.0, M))).astype(np.float32)
    sigma[rng.random(M) < 0.002] *= -1.0
    sigma[rng.random(M) < 0.001] = np.nan
    sigma[start[8]:start[8] + 100] = np.nan          # ray 8: every sample dropped
    sigma[start[9]:start[9] + 100] = 2.0             # ray 9: every sample kept
    values = sigma
    if alpha_form:
        with np.errstate(all="ignore"):
            a = -np.expm1(-np.maximum(sigma.astype(np.float64) * (te.astype(np.float64) - ts.astype(np.float64)), 0))
        values = np.minimum(a, 1 - 2.0 ** -20).astype(np.float32)
        values[np.isnan(sigma)] = np.nan
        values[sigma < 0] = -0.25                     # clamped to 0
    return dict(values=values, t_starts=ts, t_ends=te, ray_start=start, ray_cnt=cnt, all_dropped=8, all_kept=9)
