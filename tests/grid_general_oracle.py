"""The grid encoder in full, restated twice in numpy on the CPU -- test infrastructure, no test lives here.

The reference operator (external/encoders/gridencoder/src/gridencoder.cu) is CUDA-only and cannot run where these tests run, so no
golden can come from it (oracle/hashgrid.py says the same of its one configuration): what pins csrc/hashgrid_general.hip is
    * an fp32 restatement -- one rounding per operation, in the kernels' operation order -- of the cited lines, which on the default
      switches must equal the pinned C restatement oracle/hashgrid.c bit for bit (tests/test_grid_general_host.py), and
    * a float64 evaluation of the same definitions that takes its CELL decisions (in range or not, cell index) from the fp32
      restatement, as sampler_cases.march_f64 does, so that the two differ by round-off and never by a cell.

    smoothstep / derivative       gridencoder.cu:35-42     f^2 (3 - 2 f),  6 f (1 - f)
    index                         :61-79                   stride loop while stride <= T (uint32), hash iff gridtype 0 and stride > T, % T
    range, position, cell         :105-111, :143-151       u outside [0,1] -> nothing; align: pos = u (res-1), g = min(floor, res-2);
                                                            else pos = clamp(u res - 0.5, 0, res-1), g = floor; f = pos - g
    corners and weights           :171-184                 bit d of the corner -> (f_d, min(g_d+1, res-1)) else (1-f_d, g_d), on the
                                                            transformed f
    d/dx                          :205-247, :353-378       scale (res-1 | res) x weights of the other axes x (right - left) x derivative
                                                            factor; contracted with grad over levels and channels; x 1/(2 bound)
    table gradient                :313-348                 grad_emb[row] += w grad
    total variation               :526-631                 right neighbour always (unclamped), left iff g_d > 0; (weight/6) r / sqrt(q+1e-9)
    weight decay                  :671-703                 grad[i] += 2 weight emb[i] / rows(level)

`u res - 0.5` and the forward's `+= w value` are single-rounding fused multiply-adds (what nvcc -fmad=true makes of them; explicit
fmaf in oracle/hashgrid.c, csrc/hashgrid.hip and csrc/hashgrid_general.hip); every other operation rounds on its own.
"""
import numpy as np

F32, F64 = np.float32, np.float64
P1, P2 = 2654435761, 805459861
M32 = 0xFFFFFFFF
TV_EPS32 = np.float32(1e-9)
TV_CHAIN_ROUNDINGS = 16     # see tv_f64


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: the product is exact in float64; the float64 sum is made round-to-odd from its
    TwoSum error term (an inexact even result moves to its odd neighbour on the error's side), after which the rounding to the 24
    bits of float32 is the single rounding of the exact value."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p, c64 = a.astype(F64) * b.astype(F64), c.astype(F64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(F32)


class Level:
    """one level's geometry: get_grid_index's strides in its own uint32 arithmetic"""

    def __init__(self, offsets, res_tab, l, gridtype):
        self.l, self.off, self.T, self.res = l, int(offsets[l]), int(offsets[l + 1]) - int(offsets[l]), int(res_tab[l])
        stride, self.my, self.mz = self.res, 0, 0
        if stride <= self.T:
            self.my, stride = stride, (stride * self.res) & M32
            if stride <= self.T:
                self.mz, stride = stride, (stride * self.res) & M32
        self.hashed = gridtype == 0 and stride > self.T

    def rows(self, cx, cy, cz):
        cx, cy, cz = (np.asarray(c).astype(np.uint64) & np.uint64(M32) for c in (cx, cy, cz))
        if self.hashed:
            idx = cx ^ ((cy * np.uint64(P1)) & np.uint64(M32)) ^ ((cz * np.uint64(P2)) & np.uint64(M32))
        else:
            idx = (cx + cy * np.uint64(self.my) + cz * np.uint64(self.mz)) & np.uint64(M32)
        return (idx % np.uint64(self.T)).astype(np.int64)


def normalise32(x, bound, normalized=False):
    """u in fp32 (grid.py:157: one add, one correctly rounded division) and the in-range mask of gridencoder.cu:105-111"""
    x = np.asarray(x, F32).reshape(-1, 3)
    u = x if normalized else ((x + F32(bound)) / (F32(2.0) * F32(bound))).astype(F32)
    with np.errstate(invalid="ignore"):
        return u, np.all((u >= 0) & (u <= 1), axis=1)


def cell32(u, res, align):
    """fp32 position and cell of a level -> (g int64 [M,3], f float32 [M,3])"""
    with np.errstate(invalid="ignore"):
        if align:
            pos = (u * F32(res - 1)).astype(F32)
            g = np.minimum(np.floor(pos).astype(np.int64), res - 2)
        else:
            pos = np.minimum(np.maximum(fma32(u, F32(res), F32(-0.5)), F32(0)), F32(res - 1)).astype(F32)
            g = np.floor(pos).astype(np.int64)
    return g, (pos - g.astype(F32)).astype(F32)


def cell64(u64, res, align, g):
    """float64 position inside the cell g the fp32 restatement chose"""
    pos = u64 * (res - 1) if align else np.clip(u64 * res - 0.5, 0, res - 1)
    return pos - g


def smooth(f, interp, dtype):
    """(transformed f, derivative factor), gridencoder.cu:35-42, :153-159"""
    if not interp:
        return f, np.ones_like(f)
    one, two, three, six = (dtype(v) for v in (1, 2, 3, 6))
    return ((f * f) * (three - two * f)).astype(dtype), ((six * f) * (one - f)).astype(dtype)


def corners(g, f, lv, dtype):
    """rows [M,8] and weights [M,8] of the eight corners (gridencoder.cu:171-184): w = ((1 a) b) c in axis order"""
    hi = np.minimum(g + 1, lv.res - 1)
    rows, ws = [], []
    for c in range(8):
        w = np.ones(g.shape[0], dtype)
        cc = []
        for d in range(3):
            up = (c >> d) & 1
            w = (w * (f[:, d] if up else dtype(1) - f[:, d])).astype(dtype)
            cc.append(hi[:, d] if up else g[:, d])
        rows.append(lv.rows(*cc))
        ws.append(w)
    return np.stack(rows, 1), np.stack(ws, 1)


class Case:
    """One configuration and one set of points, evaluated in fp32 (the restatement) and in float64 (the yardstick)."""

    def __init__(self, x, emb, offsets, res_tab, bound, n_levels, C, gridtype=0, align=0, interp=0, normalized=False):
        self.x = np.asarray(x, F32).reshape(-1, 3)
        self.emb = np.asarray(emb, F32)
        self.offsets, self.res_tab = [int(o) for o in offsets], [int(r) for r in res_tab]
        self.L, self.C, self.n_levels, self.bound = len(self.res_tab), int(C), int(n_levels), float(bound)
        self.gridtype, self.align, self.interp = int(gridtype), int(align), int(interp)
        assert self.emb.shape == (self.offsets[-1], self.C)
        self.u32, self.inb = normalise32(self.x, bound, normalized)
        self.u64 = self.x.astype(F64) if normalized else (self.x.astype(F64) + self.bound) / (2 * self.bound)
        self.levels = [Level(self.offsets, self.res_tab, l, self.gridtype) for l in range(self.L)]
        self.M = self.x.shape[0]

    def _geom(self, lv, dtype):
        """(g, transformed f, derivative factor, rows [M,8], w [M,8]) of a level, for the in-range points, in `dtype`"""
        g, f32 = cell32(self.u32[self.inb], lv.res, self.align)
        f = f32 if dtype is F32 else cell64(self.u64[self.inb], lv.res, self.align, g)
        f, df = smooth(f, self.interp, dtype)
        rows, w = corners(g, f, lv, dtype)
        return g, f, df, rows, w

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def forward(self, dtype=F32):
        out = np.zeros((self.M, self.L, self.C), dtype)
        emb = self.emb.astype(dtype)
        for lv in self.levels[:self.n_levels]:
            _, _, _, rows, w = self._geom(lv, dtype)
            acc = np.zeros((rows.shape[0], self.C), dtype)
            for c in range(8):
                v = emb[lv.off + rows[:, c]]
                acc = fma32(w[:, c, None], v, acc) if dtype is F32 else acc + w[:, c, None] * v
            out[self.inb, lv.l] = acc
        return out.reshape(self.M, self.L * self.C)

    # ---- d/dx ---------------------------------------------------------------------------------------------------------------
    def grad_x(self, grad, dtype=F32):
        """kernel_grid's dy_dx contracted as kernel_input_backward contracts it (levels ascending, channels ascending, one
        running sum per axis), times 1 / (2 bound) as the kernels apply it: one multiplication by the fp32 reciprocal"""
        grad = np.asarray(grad, F32).reshape(self.M, self.L, self.C).astype(dtype)[self.inb]
        emb = self.emb.astype(dtype)
        res3 = np.zeros((grad.shape[0], 3), dtype)
        for lv in self.levels[:self.n_levels]:
            g, f, df, _, _ = self._geom(lv, dtype)
            hi = np.minimum(g + 1, lv.res - 1)
            scale = dtype(lv.res - 1 if self.align else lv.res)
            for gd in range(3):
                dy = np.zeros((g.shape[0], self.C), dtype)
                for idx in range(4):
                    w = np.full(g.shape[0], scale, dtype)
                    c = [None, None, None]
                    for nd in range(2):
                        d = nd + 1 if nd >= gd else nd
                        up = (idx >> nd) & 1
                        w = (w * (f[:, d] if up else dtype(1) - f[:, d])).astype(dtype)
                        c[d] = hi[:, d] if up else g[:, d]
                    c[gd] = g[:, gd]
                    left = emb[lv.off + lv.rows(*c)]
                    c[gd] = hi[:, gd]
                    right = emb[lv.off + lv.rows(*c)]
                    t = (w[:, None] * (right - left).astype(dtype)).astype(dtype)
                    dy = (dy + (t * df[:, gd, None]).astype(dtype)).astype(dtype)
                for ch in range(self.C):
                    res3[:, gd] = (res3[:, gd] + (grad[:, lv.l, ch] * dy[:, ch]).astype(dtype)).astype(dtype)
        out = np.zeros((self.M, 3), dtype)
        if dtype is F32:
            out[self.inb] = (res3 * (F32(1.0) / (F32(2.0) * F32(self.bound)))).astype(F32)
        else:
            out[self.inb] = res3 / (2 * self.bound)
        return out

    # ---- table gradient -----------------------------------------------------------------------------------------------------
    def grad_emb(self, grad, dtype=F32):
        """grad_emb[row] += w grad.  fp32: one product and one running sum per term, points ascending, corners ascending (the
        order oracle/hashgrid.c fixes; np.add.at adds element by element in that order).  float64: the same terms, exact
        products, float64 sums.  -> [rows, C]"""
        grad = np.asarray(grad, F32).reshape(self.M, self.L, self.C).astype(dtype)[self.inb]
        out = np.zeros((self.offsets[-1], self.C), dtype)
        for lv in self.levels[:self.n_levels]:
            _, _, _, rows, w = self._geom(lv, dtype)
            terms = (w[:, :, None] * grad[:, None, lv.l, :]).astype(dtype)                  # [m, 8, C]
            np.add.at(out, (lv.off + rows).reshape(-1), terms.reshape(-1, self.C))
        return out

    def term_counts(self):
        """int64 [rows]: (point, corner) terms of the table gradient landing on each row"""
        out = np.zeros(self.offsets[-1], np.int64)
        for lv in self.levels[:self.n_levels]:
            _, _, _, rows, _ = self._geom(lv, F32)
            out += np.bincount((lv.off + rows).reshape(-1), minlength=out.shape[0])
        return out

    # ---- total variation ----------------------------------------------------------------------------------------------------
    def tv(self, weight, dtype=F32):
        """-> (addend sums [rows, C], sums of the addends' ABSOLUTE terms float64 [rows, C], addend counts int64 [rows]).
        An addend is (weight / 6) r / sqrt(q + 1e-9); its absolute terms are (|weight| / 6) sum |v - v_nb| / sqrt(q + 1e-9) >= |addend|
        (r cancels, the bound of its rounding does not).  fp32: the kernel's chain per addend -- a difference, a running sum and a
        product-and-sum per neighbour, one add of 1e-9f, sqrt, weight / 6, a product, a quotient -- then a running fp32 sum per row.
        All L levels (kernel_grad_tv has no max_level)."""
        emb = self.emb.astype(dtype)
        w6 = (F32(weight) / F32(6)) if dtype is F32 else F64(F32(weight)) / 6
        eps = TV_EPS32 if dtype is F32 else F64(1e-9)
        out = np.zeros((self.offsets[-1], self.C), dtype)
        absum = np.zeros((self.offsets[-1], self.C), F64)
        cnt = np.zeros(self.offsets[-1], np.int64)
        for lv in self.levels:
            g, _ = cell32(self.u32[self.inb], lv.res, self.align)
            row = lv.off + lv.rows(g[:, 0], g[:, 1], g[:, 2])
            v = emb[row]
            r, q, a = np.zeros_like(v), np.zeros_like(v), np.zeros(v.shape, F64)
            for d in range(3):
                for step in (1, -1):
                    c = [g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy()]
                    c[d] = c[d] + step
                    live = np.ones(g.shape[0], bool) if step == 1 else g[:, d] > 0       # :595 always holds, :608
                    c[d] = np.where(live, c[d], 0)
                    gv = np.where(live[:, None], (v - emb[lv.off + lv.rows(*c)]).astype(dtype), dtype(0))
                    r = (r + gv).astype(dtype)
                    q = (q + (gv * gv).astype(dtype)).astype(dtype)
                    a += np.abs(gv.astype(F64))
            s = np.sqrt((q + eps).astype(dtype)).astype(dtype)
            addend = ((w6 * r).astype(dtype) / s).astype(dtype)
            np.add.at(out, row, addend)
            np.add.at(absum, row, np.abs(F64(w6)) * a / s.astype(F64))
            cnt += np.bincount(row, minlength=cnt.shape[0])
        return out, absum, cnt

    # ---- weight decay -------------------------------------------------------------------------------------------------------
    def wd(self, weight, dtype=F32):
        """the addend 2 weight emb[i] / rows(level of i): (2 weight) exact, one product, one quotient"""
        out = np.zeros((self.offsets[-1], self.C), dtype)
        two_w = dtype(F32(2) * F32(weight))
        for lv in self.levels:
            a, b = lv.off, lv.off + lv.T
            out[a:b] = ((two_w * self.emb[a:b].astype(dtype)).astype(dtype) / dtype(lv.T)).astype(dtype)
        return out


# ---- the bound of the total-variation comparison (judge_sum: count x 2^-24 x the sum of absolute terms) ------------------------------
# Per addend, relative to its absolute terms (|w6| sum|d| / sqrt(q + eps)), in units of 2^-24:
#   d = v - v_nb                                   1     (each difference, relative to |d|)
#   r: at most five inexact running additions      5     (each at most one rounding of a partial sum <= sum|d|)
#   q: d^2 carries 2 (from d) + 1 (the product), five running additions, the add of 1e-9f, 1e-9f against 1e-9:  3 + 5 + 1 + 1 = 10,
#      halved by the square root                   5
#   sqrt, weight / 6, w6 r, the quotient           4
# = 15, and one more for the single conversion of a row's exact fixed-point sum to fp32: TV_CHAIN_ROUNDINGS = 16.  The kernel's row
# sum itself is exact up to the fixed-point grid (tv_fixed_point_quantum per addend, passed to judge_sum as `extra`), so the count of
# a row with n addends is 16 + n only because the issue's rule counts the addends; the n is slack an fp32 running sum would need.
def tv_fixed_point_quantum(weight, M):
    """half a step of the grid an addend is rounded onto: 2^-(40 - shift) G / 2, G the power of two above |weight|, shift the
    headroom that keeps M addends inside 2^62 (csrc/hashgrid_general.hip, mh_grid_grad_tv)"""
    if weight == 0:
        return 0.0
    e = max(int(np.frexp(abs(float(F32(weight))))[1]), -60)
    shift = 0
    while shift < 40 and M > 2.0 ** (62 - 40 + shift):
        shift += 1
    return 2.0 ** (e - 40 + shift) / 2
