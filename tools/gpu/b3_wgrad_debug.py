import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morpheus_amd import ops
DEV = "cuda"
torch.manual_seed(7)
M = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
nets = []
for nout in (3, 2):
    W = [torch.randn(128, 39, device=DEV) * 0.15] + [torch.randn(128, 128, device=DEV) * 0.1 for _ in range(4)] + [torch.randn(nout, 128, device=DEV) * 0.15]
    b = [torch.randn(128, device=DEV) * 0.1 for _ in range(5)] + [torch.randn(nout, device=DEV) * 0.1]
    nets.append(W + b)
x = torch.rand(M, 3, device=DEV) * 2 - 1
b0 = [torch.randn(1, 128, device=DEV) * 0.3 for _ in range(2)]
wd_, wt_ = torch.randn(M, 3, device=DEV), torch.randn(M, 2, device=DEV)
# the b3 forward and backward-data park the tiles (every row: no eliding, dPre4 parked); both arithmetic forms of mh_warp_wgrad read them
from morpheus_amd.ops import ptr, stream, check
lib = ops._lib.load()
ops.set_mlp_mode("b3")
op = ops.prepare_warp_operands(nets[0], nets[1])
acts, dpre = torch.zeros(lib.mh_warp_acts_floats(M), device=DEV), torch.zeros(lib.mh_warp_dpre_floats(M), device=DEV)
d, t, g_x = torch.empty(M, 3, device=DEV), torch.empty(M, 2, device=DEV), torch.empty(M, 3, device=DEV)
check(lib.mh_warp_fwd(ptr(x), None, ptr(b0[0]), ptr(b0[1]), ptr(op.w3[0]), ptr(op.w3[1]), ptr(op.b[0]), ptr(op.b[1]), 6, ptr(d), ptr(t),
                      ptr(acts), M, 1, 0, stream()), "fwd")
check(lib.mh_warp_bwd_data(ptr(x), ptr(wd_), ptr(wt_), ptr(op.wT3[0]), ptr(op.wT3[1]), 6, ptr(acts), ptr(dpre), ptr(g_x), M, 1, 0, 0,
                           stream()), "bwd_data")
ws = torch.empty(max(lib.mh_warp_wgrad_workspace_floats(M), 1), device=DEV)
r32, r3 = torch.zeros(lib.mh_warp_raw_floats(), device=DEV), torch.zeros(lib.mh_warp_raw_floats(), device=DEV)
check(lib.mh_warp_wgrad(ptr(acts), ptr(dpre), None, None, None, None, 0, 0, 0, ptr(ws), ptr(r32), M, stream()), "wgrad f32")
check(lib.mh_warp_wgrad(ptr(acts), ptr(dpre), ptr(wd_), ptr(wt_), ptr(op.wT3[0]), ptr(op.wT3[1]), 1, 0, 0, ptr(ws), ptr(r3), M,
                        stream()), "wgrad b3")
torch.cuda.synchronize()
cap = {"acts": acts, "dpre": dpre}
print("acts finite", bool(torch.isfinite(cap["acts"].view(-1, 1384, 32)[:, :1344]).all()), "dpre finite", bool(torch.isfinite(cap["dpre"]).all()))
print("raw len", r3.numel(), "nan in b3:", int(torch.isnan(r3).sum()), "nan in f32:", int(torch.isnan(r32).sum()))
off = 0
geo = (None, None, [64, 128, 128, 128, 128, 128] * 2, [128, 128, 128, 128, 128, 32] * 2)    # padded in / out rows (csrc/mlp.hip: warp_wg_geometry)
assert sum(i * o + o for i, o in zip(geo[2], geo[3])) == r3.numel()
for l, (i, o) in enumerate(zip(geo[2], geo[3])):
    n = i * o
    a, b = r3[off:off + n], r32[off:off + n]
    print(f"layer {l}: in {i} out {o}: nan {int(torch.isnan(a).sum())}  max |b3-f32| {float((a - b).abs().nan_to_num(0).max()):.3e}  max|f32| {float(b.abs().max()):.3e}")
    off += n
print("---- error pattern of layer 1 (raw [out 128][in 128]) by 32 x 32 block, and of its bias gradient")
off = geo[2][0] * geo[3][0]
a = r3[off:off + 16384].view(128, 128); b = r32[off:off + 16384].view(128, 128)
for ot in range(4):
    print("out tile", ot, [f"{float((a[32*ot:32*ot+32, 32*it:32*it+32] - b[32*ot:32*ot+32, 32*it:32*it+32]).abs().max()):.2e}" for it in range(4)])
dw_total = sum(i * o for i, o in zip(geo[2], geo[3]))
db3, db32 = r3[dw_total:], r32[dw_total:]
print("db layer0..1 max err", float((db3[:256] - db32[:256]).abs().max()), "max", float(db32[:256].abs().max()))
# ratio test: is b3 a multiple of f32 somewhere?
ratio = (a / b)[b.abs() > 1.0]
print("ratio b3/f32 quantiles", [float(ratio.quantile(q)) for q in (0.01, 0.25, 0.5, 0.75, 0.99)])
