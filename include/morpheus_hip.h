/*
 * morpheus_hip.h -- C ABI of libmorpheus_hip.so (gfx950 / MI355X).
 *
 * Drop-in native boundary for the render_rays hot path of HengyiWang/MorpheuS.
 * Every entry point takes raw device pointers + sizes + an explicit hipStream_t
 * (passed as void*), returns an int status (0 = ok), never throws, never
 * allocates or frees, keeps no thread-local state and no global state that a
 * call's result depends on (forward and backward arrive on different host
 * threads; the only host statics are idempotent per-DEVICE caches -- a device's
 * CU count, "dynamic-LDS limit of kernel k raised on device d" -- indexed by
 * the current device, csrc/common.h), and launches only on the
 * stream it is given (the reference launched on the legacy default stream --
 * gridencoder.cu:386 -- a defect this ABI deliberately does not reproduce).
 * All buffers are caller-owned, contiguous, fp32 unless stated.
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   mh_grid_encode_fwd / _bwd   external/encoders/gridencoder/src/gridencoder.h:12-13,
 *                               bindings.cpp:5-10, python callers grid.py:61,91
 *   mh_composite_fwd / _bwd     nerfacc.render_weight_from_density + accumulate_along_rays,
 *                               call sites morpheus.py:675-685 (third-party, un-vendored)
 *   mh_sample_uniform           nerfacc OccGridEstimator.sampling call site morpheus.py:628-638
 *                               (benchmark sampler of SURVEY 8d; marcher is next-tier)
 *   mh_generate_rays            datasets/utils.py:28-65 + datasets/dataset.py:363-366
 *   mh_rays_sample_uniform      the two above + the pixel draw of datasets/dataset.py:412-423, one launch
 *   mh_warp_* / mh_field_*      models/model.py:412-437 (warp), :273-307 (get_sigma_albedo),
 *                               models/decoders.py:59-64, models/encodings.py:35-57,
 *                               models/density.py:22-31 -- plain PyTorch in the reference
 *   mh_warp_wgrad               the weight-gradient GEMMs autograd ran for the warp MLPs
 *   mh_adam_step / mh_adan_step torch.optim.Adam (morpheus.py:154-155) / models/optimizer.py:101-256 (Adan, morpheus.py:146-150)
 *   mh_freq_encode_fwd / _bwd   external/encoders/freqencoder/src/freqencoder.cu:28-94 (freq.py:15-52), and the progressive
 *                               max_level of FreqEncoder_torch, models/encodings.py:35-57
 *   mh_sh_encode_fwd / _bwd     external/encoders/shencoder/src/shencoder.cu:28-end (sphere_harmonics.py:14-58)
 * The warp / field entries run in two arithmetic forms behind ONE interface -- fp32 in, fp32 out, same parked tiles -- chosen by
 * their `arith` argument: native fp32 MFMA (MH_ARITH_F32) and exact three-way bf16 splits (MH_ARITH_B3: fp32-faithful, what the
 * Python side calls by default -- morpheus_amd/ops.py, MORPHEUS_MLP); mh_b3_slice cuts the weight operands of the latter.
 */
#ifndef MORPHEUS_HIP_H
#define MORPHEUS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_OK 0
#define MH_ERR_ARG 1     /* bad size / null pointer / unsupported configuration */
#define MH_ERR_LAUNCH 2  /* hipGetLastError() != hipSuccess after the launch */
#define MH_ERR_OVERFLOW 3 /* a result count does not fit the output's int32 indices (mh_mc_count) */

#define MH_ABI_VERSION 10   /* 10: one MLP entry point per pass with an `arith` argument (mh_warp_fwd, mh_warp_bwd_data, mh_warp_wgrad, mh_field_fwd, mh_field_bwd_fused; MH_ARITH_F32 / MH_ARITH_B3) and mh_warp_raw_floats; removed: mh_warp_fwd_b3, mh_warp_fwd_b3_elide, mh_warp_bwd_data_b3, mh_warp_bwd_data_b3_elide, mh_mlp_wgrad, mh_mlp_wgrad_b3, mh_mlp_wgrad_workspace_floats, mh_warp_wgrad_b3, mh_warp_wgrad_b3_elide, mh_field_fwd_b3, mh_field_bwd_fused_b3; 9: emb_acc of mh_grid_encode_bwd_binned (order-independent table gradient), later mh_subdiv_count / mh_subdiv_emit (additive: the number stays); 8: mh_smooth_points_*, mh_bg_blend_* (the last operator chains inside render_rays), live-row counts of mh_mlp_wgrad and mh_mlp_wgrad_b3, mh_warp_wgrad_b3 / mh_warp_regen_dpre4 and skip_dpre4 of mh_warp_bwd_data_b3; 7: the fp16 x 2 (_h2) entry points removed (not fp32-faithful; round-5 verdict item 8); 6: mh_grid_stage_min_points, mh_grid_encode_fwd_binned; 5: accumulate flags of mh_grid_encode_bwd_binned (d/dx) and mh_field_bwd_fused (raw; d(beta) is raw[24 928]); 4: mh_graph_*, mh_masked_mean_*, mh_ortho_perturb_*, mh_pose_apply_*, mh_render_loss_*; 3: round-3 prune (measured-loser entry points removed), n_valid in mh_sdf_losses_* */
#define MH_MAX_LEVELS 32
#define MH_TILE 32       /* sample points per wavefront tile in the MLP kernels */

int mh_abi_version(void);
const char *mh_status_string(int status);

/* ---- multiresolution hash grid (D=3, C=2, linear, align_corners=false, gridtype=hash) --------
 * x:        [M,3] world coordinates; u = (x + bound) / (2*bound) is formed in-kernel
 * emb:      [rows,2] table;  offsets_host: [L+1] HOST ints;  res_host: [L] HOST ints
 *           (res_l = (uint32)ceil(exp2f(l*S)*H) evaluated in float32 by the caller)
 * out:      [M, L*2] point-major, level-major/channel-minor inside a point (grid.py:64)
 * n_levels: levels >= n_levels are written as zero (grid.py:42,53)
 * Out-of-range points give zeros and zero gradients (gridencoder.cu:105-130, :279-284).
 * group:    performance hint, >= 1: every `group` consecutive points lie close together (6 = the finite-difference
 *           taps of one sample, models/model.py:367-385) and may share gathered corners; results do not depend on it. */
int mh_grid_encode_fwd(const float *x, const float *emb, const int32_t *offsets_host,
                       const int32_t *res_host, float *out, int64_t M, int32_t L, int32_t n_levels,
                       float bound, int32_t group, void *stream);
/* grad: [M, L*2]; grad_emb: [rows,2] ACCUMULATED into (caller zeroes it, as grid.py:84 does);
 * grad_x: NULL or [M,3], receives d/dx (the 1/(2*bound) chain factor included).  The slope uses
 * the kernel's dy_dx definition, which ignores the border clamp (gridencoder.cu:205-247). */
int mh_grid_encode_bwd(const float *grad, const float *x, const float *emb,
                       const int32_t *offsets_host, const int32_t *res_host, float *grad_emb,
                       float *grad_x, int64_t M, int32_t L, int32_t n_levels, float bound, void *stream);

/* Brick-binned backward (the fast path; same results as mh_grid_encode_bwd up to summation order).
 * mh_grid_bin_points counting-sorts the points into 16^3 spatial bricks of the box:
 *   workspace: int32[mh_grid_bin_workspace_ints()] scratch; perm: int32[M] point ids grouped by brick
 *   (out-of-box points last); brick_start: int32[mh_grid_bin_index_ints()] = offsets into perm followed
 *   by the work-item table (bricks holding more than 1024 points -- 2048 in calls of >= mh_grid_stage_min_points() points -- are
 *   split over several workgroups) and a
 *   few scratch words used by the backward (max |grad| for its fixed-point on-chip accumulation).
 * One binning serves every encoder evaluated at the same x (sdf and colour tables).
 * mh_grid_encode_bwd_binned: one workgroup per brick accumulates all levels in LDS in fixed point, then flushes the
 * touched vertices with one integer atomic each into emb_acc ([rows*2] DEVICE int64 scratch, zeroed by the call), which a last
 * pass adds to grad_emb: the table gradient is the same whatever order the workgroups run in (grad_emb is ADDED to: zero it,
 * or hand over the running sum of several queries of one table). L must be 16. grad_x (optional): accumulate_dx == 0 -> fully written; != 0 -> the points' d/dx is
 * added to what grad_x holds (the field nets' d/dx of the same points: saves the caller one pass and one launch).
 * gmax_bits: NULL, or a DEVICE word holding max |grad| as raw float bits (the producer of `grad` may compute it on
 * the fly, see mh_field_bwd_fused); NULL costs one extra pass over `grad`. */
int64_t mh_grid_bin_workspace_ints(void);
int32_t mh_grid_bin_bricks(void);
int32_t mh_grid_bin_index_ints(void);
int mh_grid_bin_points(const float *x, int64_t M, float bound, int32_t *workspace, int32_t *perm,
                       int32_t *brick_start, void *stream);
int mh_grid_encode_bwd_binned(const float *grad, const float *x, const float *emb,
                              const int32_t *offsets_host, const int32_t *res_host, const int32_t *perm,
                              const int32_t *brick_start, float *grad_emb, int64_t *emb_acc, float *grad_x, int32_t accumulate_dx,
                              int64_t M, int32_t L, int32_t n_levels, float bound, const uint32_t *gmax_bits, void *stream);
/* Brick-binned forward: mh_grid_encode_fwd's features (bit-identical), for points binned by mh_grid_bin_points BEFORE the
 * forward: a workgroup stages its brick's table rows in LDS once and its <= 1024 points read their corners there instead of
 * gathering 8 rows per (point, level) through the texture-address path (0.46 -> 0.2x ms per table at 2.1 M points).  The
 * same perm / brick_start then serve mh_grid_encode_bwd_binned.  L must be 16.  Points outside the box get zero rows.
 * (The host side takes it for every call of >= mh_grid_stage_min_points() points, the grouped finite-difference-tap calls included.) */
int mh_grid_encode_fwd_binned(const float *x, const float *emb, const int32_t *offsets_host, const int32_t *res_host,
                              const int32_t *perm, const int32_t *brick_start, float *out, int64_t M, int32_t L,
                              int32_t n_levels, float bound, void *stream);
/* Tuning knob (process-wide) of the d/dx forms of mh_grid_encode_bwd_binned: a call of at least this many points stages each
 * brick's table rows in LDS once per work item (one workgroup per CU) instead of gathering eight rows per (point, level) from
 * global memory; smaller calls (the ~0.1 ms calls of a training step) are faster gathering.  Results are bit-identical either
 * way.  set < 0: query only.  Returns the value in force (default 2^20). */
int64_t mh_grid_stage_min_points(int64_t set);
/* Host only: where the staged d/dx forms of mh_grid_encode_bwd_binned keep a brick's sums in LDS, for the resolutions res_host
 * [L] (L must be 16; a geometry the binned calls refuse returns MH_ERR_ARG).  cbase int32[3*16]: the 8-byte word k (sum x,
 * sum y, staged table row) of vertex li of level l is at byte cbase[16 k + l] + li * stride.  Where it fits, the layout is
 * COLUMNS: rows of 128 bytes = 16 words, stride 128, for every k the 16 levels on 16 different columns (byte / 8 mod 16),
 * so that the 16 levels of a point -- one lane group of an 8-byte LDS atomic -- never share a bank pair; *rows is the number of
 * 128-byte rows the accumulator takes.  A geometry whose columns would need more rows than the kernel's accumulator has gets the
 * LINEAR layout instead (stride 24, cbase = 8 (3 first_vertex(l) + k)), the same kernel and the same results.  Purely additive:
 * MH_ABI_VERSION is unchanged. */
int mh_grid_bwd_layout(const int32_t *res_host, int32_t L, int32_t *cbase, int32_t *stride, int32_t *rows);

/* ---- the grid encoder in full (csrc/hashgrid_general.hip) ------------------------------------
 * Every switch of the reference operator (gridencoder.cu:61-378): C = 1, 2, 4 or 8 channels per level, gridtype 0 hash /
 * 1 tiled, align_corners 0 / 1, interp 0 linear / 1 smoothstep; D = 3.  x [M,3] world units, emb [rows,C], offsets_host [L+1]
 * and res_host [L] HOST arrays as above, out / grad [M, L*C] level-major and channel-minor, levels >= n_levels zero.  A point
 * with any (x + bound) / (2 bound) outside [0,1] gets zero features, zero d/dx and adds nothing to the table gradient.
 * The plain path: one lane per point, one level per wave, no brick staging; the default configuration (C = 2, hash, linear,
 * not aligned) is served by mh_grid_encode_* above and gives the same cells here.
 * mh_grid_general_bwd: grad_emb [rows,C] is ADDED to (zero it, or hand over a running sum) through emb_acc, DEVICE int64
 * [rows*C + 1] scratch the call zeroes: terms are summed in 64-bit fixed point (one rounding each onto 2^-40 of the power of two
 * above max |grad|, found by the call), so the table gradient is identical from run to run.  grad_x [M,3] optional, fully
 * written; any L <= MH_MAX_LEVELS.
 * mh_grid_grad_tv (kernel_grad_tv, gridencoder.cu:526-631): per point inside the box and per level (ALL L levels) the cell's row
 * receives (weight / 6) r / sqrt(q + 1e-9) per channel, r / q the sums of the differences / squared differences to the right
 * neighbour on every axis and to the left one where the cell index is > 0.  normalized != 0: x holds u in [0,1] already (bound
 * unused).  Added to grad_emb IN PLACE through emb_acc (DEVICE int64 [rows*C], zeroed by the call; fixed point on the power of
 * two above |weight|: identical from run to run); entries no point reaches are not written.
 * mh_grid_grad_wd (kernel_grad_wd, :671-703): grad_emb[i] += 2 weight emb[i] / rows(level of i) over the whole table, in place.
 * grad_emb needs 4-byte alignment only (it may be a view into a flat gradient bucket); rows are read as C-wide vectors where emb
 * is aligned for it and element by element otherwise.
 * Bad arguments return MH_ERR_ARG before any launch; M == 0 returns MH_OK without one. */
int mh_grid_general_fwd(const float *x, const float *emb, const int32_t *offsets_host, const int32_t *res_host, float *out,
                        int64_t M, int32_t L, int32_t n_levels, int32_t C, int32_t gridtype, int32_t align_corners,
                        int32_t interp, float bound, void *stream);
int mh_grid_general_bwd(const float *grad, const float *x, const float *emb, const int32_t *offsets_host,
                        const int32_t *res_host, float *grad_emb, int64_t *emb_acc, float *grad_x, int64_t M, int32_t L,
                        int32_t n_levels, int32_t C, int32_t gridtype, int32_t align_corners, int32_t interp, float bound,
                        void *stream);
int mh_grid_grad_tv(const float *x, const float *emb, const int32_t *offsets_host, const int32_t *res_host, float *grad_emb,
                    int64_t *emb_acc, float weight, int64_t M, int32_t L, int32_t C, int32_t gridtype, int32_t align_corners,
                    int32_t normalized, float bound, void *stream);
int mh_grid_grad_wd(const float *emb, const int32_t *offsets_host, float *grad_emb, float weight, int32_t L, int32_t C,
                    void *stream);

/* ---- packed transmittance compositor -------------------------------------------------------
 * Samples of ray r are the contiguous range [ray_start[r], ray_start[r]+ray_cnt[r]) of the packed
 * arrays, ordered by t.  w_i = exp(-sum_{j<i} sigma_j dt_j) * (1 - exp(-sigma_i dt_i)).
 * weights [M]; opacity [N]; depth [N] = sum w * (ts+te)/2; color [N,3] = sum w * rgb. */
int mh_composite_fwd(const float *sigma, const float *t_starts, const float *t_ends, const float *rgb,
                     const int32_t *ray_start, const int32_t *ray_cnt, float *weights, float *opacity,
                     float *depth, float *color, int32_t N, void *stream);
/* g_weights may be NULL.  Outputs d_sigma [M], d_rgb [M,3]. */
int mh_composite_bwd(const float *sigma, const float *t_starts, const float *t_ends, const float *rgb,
                     const int32_t *ray_start, const int32_t *ray_cnt, const float *weights,
                     const float *g_weights, const float *g_opacity, const float *g_depth,
                     const float *g_color, float *d_sigma, float *d_rgb, int32_t N, void *stream);

/* ---- ray generation + uniform stratified sampler ------------------------------------------- */
/* K = fx,fy,cx,cy; c2w: [4,4] row-major HOST floats; rays_o/rays_d: [H*W,3] (OpenGL, un-normalised) */
int mh_generate_rays(float fx, float fy, float cx, float cy, const float *c2w_host, int32_t H, int32_t W,
                     float *rays_o, float *rays_d, void *stream);
/* AABB slab clip to [-bound,bound]^3, S bins of (t_far-t_near)/(S+1), comb shifted by jitter*dt.
 * A ray is a MISS -- S zero-width samples at t = 0 here, no samples in the marcher below -- when the clipped segment is empty
 * (t_far <= t_near, t_near >= 0), when any of its six slab quotients (+-bound - o[a]) / d[a] is NaN (a NaN origin or direction
 * component; 0/0: a ray lying in a face plane), or when the clipped t_near / t_far is not finite (d = 0 inside the box).  The
 * NaN is not dropped the way fmaxf / fminf alone would drop it.  Every finite ray that hits is clipped as before.
 * Outputs (length N*S, ray-major): ray_idx int32, t_starts, t_ends, xyz [N*S,3] = o + d*(ts+te)/2;
 * and ray_start/ray_cnt [N] int32. */
int mh_sample_uniform(const float *rays_o, const float *rays_d, const float *jitter, int32_t N, int32_t S,
                      float bound, int32_t *ray_idx, float *t_starts, float *t_ends, float *xyz,
                      int32_t *ray_start, int32_t *ray_cnt, void *stream);

/* The two above in one launch (BASELINE.json north_star "fused ray-generate + stratified sampler"): ray r looks
 * through pixel pix[r] (int32 [N] on the device; NULL = pixel r, N <= H*W) -- the per-iteration pixel draw of
 * datasets/dataset.py:412-423.  Writes rays_o/rays_d [N,3] and every mh_sample_uniform output, bit-identical to
 * mh_generate_rays + gather + mh_sample_uniform. */
int mh_rays_sample_uniform(float fx, float fy, float cx, float cy, const float *c2w_host, int32_t H, int32_t W,
                           const int32_t *pix, const float *jitter, int32_t N, int32_t S, float bound,
                           float *rays_o, float *rays_d, int32_t *ray_idx, float *t_starts, float *t_ends,
                           float *xyz, int32_t *ray_start, int32_t *ray_cnt, void *stream);

/* Occupancy-grid marcher (nerfacc OccGridEstimator.sampling call shape, morpheus.py:628-638): fixed `step`,
 * one jitter per ray (NULL = none), binary grid [R,R,R] uint8 over the AABB [-bound,bound]^3.  Interval k of a ray:
 * ts = t_near + u*step + k*step, te = min(ts+step, t_far), kept iff the cell of its midpoint is occupied.  A miss (the rule
 * stated at mh_sample_uniform) has no interval: ray_cnt = 0, and it never sets *overflow.
 * One wavefront per ray (64 steps per iteration, ballot/popcount compaction), single pass:
 * mh_march_slots writes ray_cnt [N] and the kept intervals of ray r to slot_ts/slot_te [r*cap .. r*cap+cnt), cap >=
 * mh_march_cap(step, bound) (steps on the AABB diagonal for unit-or-longer directions); *overflow (device int, zeroed by
 * the caller) is set if some ray needed more than cap slots -- the caller then marches again with a longer slot row.
 * After the exclusive scan of ray_cnt into ray_start, mh_march_pack copies the slot rows to the packed ray_idx /
 * t_starts / t_ends. */
int32_t mh_march_cap(float step, float bound);
int mh_march_slots(const float *rays_o, const float *rays_d, const float *jitter, int32_t N, float step, float bound,
                   int32_t R, const uint8_t *binary, int32_t cap, int32_t *ray_cnt, float *slot_ts, float *slot_te,
                   int32_t *overflow, void *stream);
int mh_march_pack(const int32_t *ray_start, const int32_t *ray_cnt, const float *slot_ts, const float *slot_te, int32_t N,
                  int32_t cap, int32_t *ray_idx, float *t_starts, float *t_ends, void *stream);

/* ---- visibility pruning of packed samples (csrc/visibility.hip) --------------------------------------------------------
 * What nerfacc's OccGridEstimator.sampling does with sigma_fn / alpha_fn, alpha_thre and early_stop_eps
 * (render_visibility_from_density / render_visibility_from_alpha of nerfacc 0.5.x).  nerfacc is third-party, un-vendored and
 * not installed where this library is built: the rules below are restated as recalled and are NOT verified against it
 * (tools/check_against_nerfacc.py prints the difference of the kept sets on a machine that has it).
 * Input: the marcher's packed samples -- samples of ray r are [ray_start[r], ray_start[r] + ray_cnt[r]) of the packed arrays
 * of length M, contiguous and ordered by t -- and one value per sample.  Per sample i of a ray, D = t_ends - t_starts:
 *   sigma form (alpha_form = 0): x_i = max(sigma_i * D_i, 0); a NaN x_i drops the sample and adds 0 to the sum;
 *                                alpha_i = -expm1f(-x_i);  T_i = expf(-sum_{j<i} x_j)  (an exclusive sum along the ray).
 *   alpha form (alpha_form = 1): alpha_i = values_i clamped to [0, 1], a NaN drops the sample and adds 0;
 *                                T_i = prod_{j<i} (1 - alpha_j), carried as the sum of x_j = -log1pf(-alpha_j)
 *                                (t_starts / t_ends are not read and may be NULL).
 *   keep_i = (T_i >= early_stop_eps) && (alpha_i >= *alpha_thre)          (alpha_thre NULL: 0; 0 <= early_stop_eps <= 1)
 * alpha_thre is a DEVICE scalar: the caller forms min(alpha_thre, mean(occs)) -- the rule nerfacc applies when a sigma_fn or
 * alpha_fn is given -- on the device and no host read is needed.
 * The clamp x >= 0 makes T non-increasing along a ray.  That is what lets a wavefront stop reading a ray once the running
 * sum alone gives T < early_stop_eps: every later sample of that ray is dropped, and its keep bytes are still written (0).
 * mh_visibility_mask: one wavefront per ray, 64-sample chunks with a carry (the compositor's scan); writes keep [M] uint8 for
 * every sample a ray owns and kept_cnt [N] int32.  Ranges are clipped to [0, M).
 * mh_visibility_pack: new_start [N] = the exclusive scan of kept_cnt (the caller's, as for mh_march_pack); copies the kept
 * samples of ray r, in order, to [new_start[r], new_start[r] + kept_cnt[r]) of out_ray_idx / out_t_starts / out_t_ends
 * [M_out] and writes src_index [M_out] int32 = the packed position each kept sample had before.  The pruned set's ray_start /
 * ray_cnt are new_start / kept_cnt.  Writes beyond M_out are suppressed.
 * Two forms of the same entry points, as for the marcher:
 *   ragged:          M_out = sum(kept_cnt), read by the host once;
 *   fixed capacity:  M and M_out are the marcher's capacity, the entries no ray owns are padding the kernels never visit
 *                    (the caller zeroes keep and the outputs: ray 0, t = 0, src_index 0, the marcher's padding convention),
 *                    n_valid = sum(kept_cnt) stays on the device, no host synchronisation.  The kept set is a subset of the
 *                    marched one, so it fits wherever the marched one did.
 * Bad arguments give MH_ERR_ARG before any launch; N == 0 or M == 0 (or M_out == 0) give MH_OK without one. */
int mh_visibility_mask(const float *values, int32_t alpha_form, const float *t_starts, const float *t_ends,
                       const int32_t *ray_start, const int32_t *ray_cnt, int32_t N, int64_t M, float early_stop_eps,
                       const float *alpha_thre, uint8_t *keep, int32_t *kept_cnt, void *stream);
int mh_visibility_pack(const uint8_t *keep, const float *t_starts, const float *t_ends, const int32_t *ray_start,
                       const int32_t *ray_cnt, const int32_t *new_start, int32_t N, int64_t M, int64_t M_out,
                       int32_t *out_ray_idx, float *out_t_starts, float *out_t_ends, int32_t *src_index, void *stream);

/* ---- glue of the field queries as single launches (csrc/normal.hip) ----------------------------------------------------
 * Finite-difference normals (models/model.py:367-398): mh_fd_taps writes the 6 clamped taps of every sample, point-major
 * (+x,-x,+y,-y,+z,-z; taps [6M,3]) and replicates topo [M,topo_dim] to topo6 [6M,topo_dim] (topo NULL: skipped);
 * mh_fd_taps_bwd sums the taps' gradients back (clamp passes inside [-bound, bound]); g_x / g_topo NULL: not computed.
 * mh_fd_normal_fwd: sdf6 [M,6] -> raw [M,3] = 0.5 (s+ - s-) / eps and normal = nan_to_num(raw / sqrt(max(|raw|^2, 1e-20)));
 * mh_fd_normal_bwd: (g_normal, g_raw; either may be NULL) -> g_sdf6 [M,6].
 * Sample assembly (morpheus.py:644-647): xyz[m] = rays_o[r] + rays_d[r] * (t_starts[m] + t_ends[m]) / 2, r = ray_idx[m];
 * backward = per-ray segment sums over the packed samples (ray_start / ray_cnt), one wavefront per ray. */
int mh_fd_taps(const float *x, const float *topo, int32_t topo_dim, float eps, float bound, int64_t M, float *taps,
               float *topo6, void *stream);
int mh_fd_taps_bwd(const float *x, const float *g_taps, const float *g_topo6, int32_t topo_dim, float eps, float bound,
                   int64_t M, float *g_x, float *g_topo, void *stream);
int mh_fd_normal_fwd(const float *sdf6, float eps, int64_t M, float *normal, float *raw, void *stream);
int mh_fd_normal_bwd(const float *sdf6, const float *g_normal, const float *g_raw, float eps, int64_t M, float *g_sdf6,
                     void *stream);
int mh_sample_positions(const float *rays_o, const float *rays_d, const int32_t *ray_idx, const float *t_starts,
                        const float *t_ends, int64_t M, float *xyz, void *stream);
/* MultiCode.sample (models/deform_code.py:20-38): three [C, size_l] tables (the reference's volumes [1,C,size,1]) sampled
 * linearly in time, grid_sample(align_corners=True) coordinate rule, t clamped to [0,1]; out [F, 3*C] level-major.
 * Backward accumulates into g0/g1/g2 (same shapes as the tables, ZEROED by the caller) with atomics. */
int mh_multicode_fwd(const float *t, const float *v0, const float *v1, const float *v2, int32_t s0, int32_t s1, int32_t s2,
                     int32_t C, int32_t F, float *out, void *stream);
int mh_multicode_bwd(const float *t, const float *g_out, float *g0, float *g1, float *g2, int32_t s0, int32_t s1, int32_t s2,
                     int32_t C, int32_t F, void *stream);
/* get_sdf_loss (utils.py:91-113) on packed samples: per-ray depth [N] / mask [N] (NULL: none) are read through ray_idx, the
 * sample depth is (t_starts + t_ends)/2.  sums [3] (device) = free-space sum, near-surface sum, count of samples whose target
 * depth is non-zero; the caller divides the two sums by the count.  Backward: g_fs / g_sl are device scalars (NULL = 0).
 * n_valid: NULL, or a DEVICE int: only the first *n_valid of the M packed entries are samples (fixed-capacity sampling pads
 * the packed arrays so that a captured HIP graph sees constant shapes); the padding adds nothing and gets zero gradient. */
int mh_sdf_losses_fwd(const float *pred_sdf, const float *t_starts, const float *t_ends, const int32_t *ray_idx,
                      const float *rays_depth, const float *rays_mask, float trunc, int64_t M, const int32_t *n_valid,
                      float *sums, void *stream);
int mh_sdf_losses_bwd(const float *pred_sdf, const float *t_starts, const float *t_ends, const int32_t *ray_idx,
                      const float *rays_depth, const float *rays_mask, float trunc, int64_t M, const int32_t *n_valid,
                      const float *sums, const float *g_fs, const float *g_sl, float *g_pred, void *stream);
int mh_sample_positions_bwd(const float *g_xyz, const float *t_starts, const float *t_ends, const int32_t *ray_start,
                            const int32_t *ray_cnt, int32_t N, float *g_o, float *g_d, void *stream);

/* ---- fused tiny-MLP evaluators: the warp nets (deform_net + topo_net) and the field nets (sdf_net + color_net) ---------------
 * One entry point per pass.  Values, parked tiles, accumulation and results are fp32 in either arithmetic; `arith` says how a
 * product reaches the matrix cores and which pack the weight operand (a `const void *`) is:
 *   MH_ARITH_F32 (0): the native fp32 MFMA (v_mfma_f32_32x32x2_f32; csrc/mlp.hip).  Weights are PRE-PACKED by the host into the
 *     MFMA A-fragment order (morpheus_amd/packing.py): for layer l, tile mt, k-quad q: float4 per lane; a pack is the
 *     concatenation of all layers of the net(s) (mh_*_wpack_floats / mh_*_wpackT_floats floats), layer geometry fixed by the kernel.
 *   MH_ARITH_B3 (1): exact fp32 products on the bf16 matrix pipe (csrc/mlp_b3.hip; what the Python side calls by default --
 *     morpheus_amd/ops.py, MORPHEUS_MLP).  Every fp32 operand is cut into three bf16 slices (hi + mid + lo == x exactly) and a
 *     product is the six significant cross terms through v_mfma_f32_32x32x16_bf16 with fp32 accumulation: fp32-grade results (what
 *     is dropped is <= 3 * 2^-24 of a product), 6/16 of the fp32-MFMA cycles.  Only the weight operand has its own pack, the
 *     SLICED one (mh_*_w3_bytes / mh_*_w3T_bytes bytes), cut by mh_b3_slice; activations and gradients are sliced on the fly.
 *   Any other value: MH_ERR_ARG.  Both forms of a pass take the same arguments otherwise, give the same outputs up to fp32
 *   summation order, and write and read the same parked tiles -- a scratch parked by one may be consumed by the other.
 * Activation scratch ("acts") is written by the forward when acts != NULL and consumed by the backward: per 32-point tile, per
 * layer, feature-major [F][32] fp32 (the weight-gradient GEMM's operand), followed by the hidden layers' ReLU sign masks (one bit
 * per lane and output row) that backward-data reads instead of the activations themselves.
 *
 * mh_b3_slice: fp32 fragments in the 32x32x16 order (packing.py: fwd3_index; per layer [out tile][k16 step][lane][8]) ->
 *   per layer three bf16 planes [hi | mid | lo][out tile][k16 step][lane][8 bf16].  src_off / n in floats (n % 8 == 0),
 *   dst_off in 16-byte units; host arrays of n_layers entries (<= 16).
 * Sliced packs: mh_warp_w3_bytes() per warp net (layer 0 padded to whole 512 x 16-byte DMA rounds), mh_warp_w3T_bytes() per warp
 *   net TRANSPOSED (T5, T4..T1, T0; packing.py: bwd3_index), mh_field_w3_bytes() for the six field layers (resident in LDS:
 *   packing.py field_joint_packer().b3_layers), mh_field_w3T_bytes() for them transposed (field_joint_packer().b3T_layers:
 *   TC2 | TC1 | TC0 | TS2 | TS1 | TS0). */
#define MH_ARITH_F32 0
#define MH_ARITH_B3 1
int64_t mh_mlp_tiles(int64_t M);        /* 32-point tiles the kernels touch: 4 * ceil(M/128) */
int64_t mh_warp_acts_floats(int64_t M);
int64_t mh_warp_dpre_floats(int64_t M);
int64_t mh_warp_wpack_floats(void);   /* per net, forward pack */
int64_t mh_warp_wpackT_floats(void);  /* per net, transposed pack */
int64_t mh_warp_w3_bytes(void);
int64_t mh_warp_w3T_bytes(void);
int64_t mh_field_acts_floats(int64_t M);
int64_t mh_field_wpack_floats(void);
int64_t mh_field_wpackT_floats(void);
int64_t mh_field_w3_bytes(void);
int64_t mh_field_w3T_bytes(void);
int mh_b3_slice(const float *src, void *dst, int32_t n_layers, const int32_t *src_off_host, const int32_t *n_host,
                const int32_t *dst_off_f4_host, void *stream);

/* Line words and eliding (MH_ARITH_B3 only; every eliding flag with MH_ARITH_F32 is MH_ERR_ARG).
 * Line words: the b3 warp forward parks, in the dead rows of the tile's H0 block (from row 40 on: [net][hidden layer 1..5][half h]
 * uint64, 160 bytes), which of the tile's parked rows carry a non-zero: bit 16 t + r of half h <-> row 32 t + (r & 3) + 8 (r >> 2)
 * + 4 h of that layer's H block.  The per-layer kernels of mh_warp_wgrad (large batches) fetch a zero line in place of a row
 * whose bit is 0 -- of an H block and of the dPre block masked by the same ReLU signs; every result keeps its bits.
 * mh_warp_skip_zero_lines: process-wide switch of that skipping (1 = on, the default; 0 = every row is fetched; set < 0: query
 * only).  Returns the value in force.  The words are parked either way.
 * Eliding: a writer that does not send an all-zero parked line (a row whose word bit is 0) to memory.  A call with its flag at 0
 * writes every line, and whoever reads whole tiles may rely on it.  One flag per call:
 * mh_warp_fwd(elide = 1): the H rows without a non-zero are NOT written; the line words, the sign masks and the encoding rows
 *   always are.  Same outputs.  Needs acts.
 * mh_warp_bwd_data(elided = 1): the dPre rows of layers 0..4 whose bit is 0 are NOT written and hold whatever the scratch
 *   held before (dPre5's live rows are always written; dPre4 follows skip_dpre4).  g_x keeps its bits.
 * mh_warp_wgrad(elided = 1): the tiles were written by an eliding call, so the launches go by the words whatever
 *   mh_warp_skip_zero_lines says at that moment -- every gradient keeps its bits.
 * A flag of 1 needs mh_warp_regen_dpre4(M) (the per-layer weight-gradient kernels: the merged small-batch kernels read every row),
 * else MH_ERR_ARG.  The caller decides once, at forward time, with mh_warp_elides(M), and whoever elided a scratch hands it on
 * only with elided = 1 (morpheus_amd/ops.py: warp_mlp(elide=True) carries the decision to its backward in the autograd ctx).
 * mh_warp_elides(M): what a call on M points may elide: 0 = nothing (no mh_warp_regen_dpre4(M), or mh_warp_skip_zero_lines off),
 *   else the value of mh_warp_elide_zero_lines.
 * mh_warp_elide_zero_lines: process-wide switch for the A/B: 2 = forward and backward-data elide (the default), 1 = backward-data
 *   only, 0 = no call elides; set < 0: query only.  Returns the value in force.  MORPHEUS_WARP_ELIDE_ZERO_LINES sets it when the
 *   library is loaded.
 * mh_warp_regen_dpre4(M): 1 when a call on M points takes the large-batch weight-gradient path (one launch per layer), the only
 *   one that can make dPre4 again; see mh_warp_bwd_data. */
int64_t mh_warp_skip_zero_lines(int64_t set);
int64_t mh_warp_elide_zero_lines(int64_t set);
int32_t mh_warp_elides(int64_t M);
int32_t mh_warp_regen_dpre4(int64_t M);

/* mh_warp_fwd: deform = deform_net([freq(x), code]), topo = topo_net(same)
 *   x [M,3]; slot [M] int32 -> row of bias0 (per-frame first-layer bias  W0[:,39:87].code + b0,
 *   computed by the caller; one row per distinct frame time); bias0_{d,t}: [n_slots,128];
 *   w_{d,t}: one net's forward pack of `arith`;  n_bands: frequency bands kept (progressive max_level), 0..6;
 *   out_deform [M,3]; out_topo [M,2];  acts: NULL or scratch of mh_warp_acts_floats(M) floats;  elide: see above. */
int mh_warp_fwd(const float *x, const int32_t *slot, const float *bias0_d, const float *bias0_t, const void *w_d, const void *w_t,
                const float *bias_d, const float *bias_t, int32_t n_bands, float *out_deform, float *out_topo, float *acts,
                int64_t M, int32_t arith, int32_t elide, void *stream);
/* mh_warp_bwd_data: consumes g_deform [M,3], g_topo [M,2] (either may be NULL = zero), acts from the forward and the TRANSPOSED
 *   packs wT_{d,t} of `arith`; writes g_x [M,3] (d/dx through the frequency encoding; pass NULL when the sample positions carry no
 *   gradient and the first-layer transposed GEMM is skipped) and dpre scratch (mh_warp_dpre_floats(M) floats) for mh_warp_wgrad.
 *   skip_dpre4 = 1 (MH_ARITH_B3 only, else MH_ERR_ARG): the 128 dPre4 rows of both nets (16 KB of a tile's 172) are NOT written --
 *   mh_warp_wgrad(regen_dpre4 = 1) makes them again from the incoming gradient, the ReLU sign words and the T5 slices, bit for bit
 *   (dPre4 = relu'(H5) W5^T dPre5 and dPre5 IS the incoming gradient); allowed when mh_warp_regen_dpre4(M) says so (the
 *   large-batch weight-gradient path).  elided: see above. */
int mh_warp_bwd_data(const float *x, const float *g_deform, const float *g_topo, const void *wT_d, const void *wT_t,
                     int32_t n_bands, const float *acts, float *dpre, float *g_x, int64_t M, int32_t arith, int32_t skip_dpre4,
                     int32_t elided, void *stream);
/* mh_warp_wgrad: the weight gradients of the 12 layers of the two warp nets from the tiles the two calls above parked (their
 *   geometry is on this side of the ABI):  dW_l[out][in] = sum_pts dpre_l[out][pt] * act_l[in][pt],  db_l[out] = sum_pts dpre_l[out][pt].
 *   MFMA launches (one per layer for large batches, one or two for all layers otherwise) write per-chunk partials into `workspace`
 *   (mh_warp_wgrad_workspace_floats(M) floats), one reduction launch sums them into raw (mh_warp_raw_floats() floats) =
 *   [dW of deform layers 0..5 | topo layers 0..5][db of the same twelve], feature counts padded to multiples of 32, in tile-row
 *   order (the caller maps rows back to the natural layout, morpheus_amd/packing.py).
 *   Live rows: 40 of the first layer's 64 input rows and 3 | 2 of the last layer's 32 dPre rows carry values.  Rows behind them
 *   are never read -- the producing kernels do not write them -- and the dW rows / columns of those pad features are unspecified
 *   (the caller's row map does not gather them).
 *   MH_ARITH_B3: both fp32 operands are sliced on the fly; g_deform / g_topo / w3T_{d,t}: what mh_warp_bwd_data was given (the
 *   packs must not be NULL; the rest is read only with regen_dpre4 = 1, and the gradients may be NULL = zero).  regen_dpre4,
 *   elided: see above.  MH_ARITH_F32: regen_dpre4, elided and those four pointers must be 0 / NULL, else MH_ERR_ARG. */
int64_t mh_warp_wgrad_workspace_floats(int64_t M);
int64_t mh_warp_raw_floats(void);
int mh_warp_wgrad(const float *acts, const float *dpre, const float *g_deform, const float *g_topo, const void *w3T_d,
                  const void *w3T_t, int32_t arith, int32_t regen_dpre4, int32_t elided, float *workspace, float *raw, int64_t M,
                  void *stream);

/* mh_field_fwd: canonical field  sdf_net([freq(xc), hash, topo]) -> sdf, sigma (Laplace), geo;
 *               color_net([hash_c, geo]) -> sigmoid -> albedo.
 *   xc [M,3]; feat_s / feat_c [M,32] (hash features); topo NULL or [M,2]; w: the forward pack of `arith` for the six field layers;
 *   beta: DEVICE scalar = |beta_p|+1e-4 (a pointer, so the host never synchronises to read the learnable beta);
 *   with_color = 0 skips color_net (FD-normal taps, occupancy queries);  acts: NULL or mh_field_acts_floats(M) floats. */
int mh_field_fwd(const float *xc, const float *feat_s, const float *feat_c, const float *topo, const void *w, const float *bias,
                 const float *beta, int32_t n_bands, int32_t with_color, float *sdf, float *sigma, float *albedo, float *acts,
                 int64_t M, int32_t arith, void *stream);
/* mh_field_bwd_fused: backward of the field nets: backward-data AND weight gradients in one pass per net; the weight-gradient
 * accumulators stay in registers, so the pre-activation gradients never reach HBM (no `dpre` buffer).
 *   g_sdf, g_sigma [M], g_albedo [M,3] (any may be NULL) -> g_xc [M,3] or NULL (freq path only; the hash path's d/dx comes
 *   from mh_grid_encode_bwd), g_feat_s, g_feat_c [M,32], g_topo [M,2].  sdf / albedo are the forward's outputs (Laplace and
 *   sigmoid derivatives are formed from them).  wT: the TRANSPOSED pack of `arith`.
 *   gmax_bits: NULL, or 2 DEVICE words zeroed by the caller that receive max |g_feat_s| and max |g_feat_c| as raw float
 *   bits (atomicMax) -- what mh_grid_encode_bwd_binned needs for its fixed-point accumulation.
 *   dgeo_scratch [mh_field_dgeo_floats(M)] (d(geo) handed from the colour launch to the sdf launch; may be NULL when
 *   with_color == 0), workspace [mh_field_bwd_fused_workspace_floats(M)] (per-wave partial sums), and
 *   raw [24 928 + 1] = the weight gradient in mh_warp_wgrad's tile-row format for the layer list s0, s1, s2, c0, c1, c2
 *   (dW tiles | db tiles; the colour part is zero when with_color == 0) followed by dL/dbeta (one float, summed in a fixed
 *   order).  accumulate == 0: raw is written; != 0: this call's gradients are ADDED to raw -- the field queries of one
 *   training step (render, finite-difference taps, regularisers) sum their weight gradients in place, no caller-side adds.
 * mh_field_bwd_pair_min_points: tuning knob (process-wide) of the MH_ARITH_B3 form: a with-colour call of at least this many
 *   points runs the pair form of its two launches (512-thread workgroups, two waves per SIMD that share a tile's chain and
 *   weight-gradient work); smaller calls and the sdf-only pass run the one-wave kernels.  Every output is bit-identical either
 *   way.  set < 0: query only.  Returns the value in force (default 0: every with-colour call). */
int64_t mh_field_bwd_fused_workspace_floats(int64_t M);
int64_t mh_field_dgeo_floats(int64_t M);
int64_t mh_field_bwd_pair_min_points(int64_t set);
int mh_field_bwd_fused(const float *xc, const float *sdf, const float *albedo, const float *g_sdf, const float *g_sigma,
                       const float *g_albedo, const void *wT, const float *beta, int32_t n_bands, int32_t with_color,
                       const float *acts, float *dgeo_scratch, float *workspace, float *raw, int32_t accumulate, float *g_xc,
                       float *g_feat_s, float *g_feat_c, float *g_topo, uint32_t *gmax_bits, int64_t M, int32_t arith, void *stream);

/* ---- weight-norm parametrisation of every weight-normed layer, one launch each way ---------- */
/* Replaces nn.utils.weight_norm on the Linear layers of deform_net / topo_net / color_net (models/decoders.py:51-52),
 * recomputed per forward: W_l[r,:] = v_l[r,:] * g_l[r] / ||v_l[r,:]||, and its backward (dv_l, dg_l from dW_l).
 * The *_host arguments are HOST arrays (n_layers <= 32) of DEVICE pointers / sizes; v_l, W_l, dW_l, dv_l are
 * [rows_l, cols_l] row-major, g_l and dg_l are [rows_l].  dw_host[l] may be NULL (no gradient): dv_l = dg_l = 0. */
int mh_weight_norm_fwd(int32_t n_layers, const float *const *v_host, const float *const *g_host, float *const *w_host,
                       const int32_t *rows_host, const int32_t *cols_host, void *stream);
int mh_weight_norm_bwd(int32_t n_layers, const float *const *v_host, const float *const *g_host,
                       const float *const *dw_host, float *const *dv_host, float *const *dg_host,
                       const int32_t *rows_host, const int32_t *cols_host, void *stream);

/* ---- optimiser step over the flat parameter bucket (the step after the path) ---- */
/* Replaces torch.optim.Adam(model.get_params_all(lr), betas=(0.9,0.99), eps=1e-15).step() of morpheus.py:154-155,
 * :1401-1424 (no weight decay, no amsgrad).  params/grads/exp_avg/exp_avg_sq: [n] fp32 device buffers, 16-byte aligned.
 * The bucket is cut into contiguous segments, normally ONE PER PARAMETER TENSOR (plus alignment pads): seg_end_host[s] =
 * exclusive end offset (last == n), seg_lr_host[s] = its group's learning rate, seg_step_host[s] = the 1-based step count
 * of that parameter for its bias corrections, or 0 = the parameter has no gradient this time and is left untouched
 * (moments, value and count), which is what torch.optim.Adam does for grad None (HOST arrays, n_segs <= 160). */
int mh_adam_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, int32_t n_segs,
                 const int64_t *seg_end_host, const float *seg_lr_host, const int64_t *seg_step_host, float beta1,
                 float beta2, float eps, void *stream);
/* The same step with the per-segment bookkeeping ON THE DEVICE, for data-parallel runs: seg_flag_dev [n_segs] > 0 = the
 * segment's parameter has a gradient this step ON SOME RANK (the all-reduced has-gradient flags of the gradient bucket, which
 * only the device knows without a synchronisation); seg_step_dev [n_segs] int64 in/out = the per-segment step counts,
 * incremented where the flag is set; seg_scratch_dev [2 * n_segs] floats of workspace.  A segment whose flag is 0 is left
 * untouched (value, moments, count).  Two launches (one thread per segment, then the update). */
int mh_adam_step_dev(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, int32_t n_segs,
                     const int64_t *seg_end_host, const float *seg_lr_host, const float *seg_flag_dev, int64_t *seg_step_dev,
                     float *seg_scratch_dev, float beta1, float beta2, float eps, void *stream);

/* ---- optimiser: fused Adan over one flat fp32 bucket (csrc/adan.hip) ---------------------------------------------------
 * Replaces Adan(model.get_params_all(5 lr), eps=1e-8, weight_decay=2e-5, max_grad_norm=5.0, foreach=False), morpheus.py:146-150,
 * the rule of models/optimizer.py:101-256 (_single_tensor_adan, every operator rounded in its order).  params / grads / exp_avg /
 * exp_avg_sq / exp_avg_diff / neg_pre_grad: [n] fp32 device buffers, 16-byte aligned, cut into the segments of mh_adam_step
 * (n_segs <= 160).  HOST arrays per segment: seg_end_host (exclusive ends, last == n), seg_lr_host (its group's learning rate, a
 * double as Python holds it), seg_step_host (its GROUP's 1-based step count: Adan counts per group, whether or not a parameter
 * had a gradient), seg_flag_host (bit 0: no gradient this time -- value and all four states keep their bits; bit 1: the
 * parameter's first gradient -- neg_pre_grad starts as -c g; a group step of 1 implies it).  Step sizes, bias corrections and the
 * decay factor are formed in double on the host and rounded to fp32.  betas in [0, 1); eps, weight_decay, max_grad_norm >= 0.
 * max_grad_norm > 0: c = min(max_grad_norm / (sqrt(sum g g) + eps), 1) over the segments that have a gradient, summed in double
 * in a fixed order (no atomics: the same bits on every run), rounded once to fp32 and left on the device; the gradients are scaled
 * by it IN PLACE, as the reference scales p.grad.  max_grad_norm == 0: c = 1, no norm pass, grads are only read.
 * workspace: mh_adan_workspace_bytes() bytes, 16-byte aligned; its first three floats are c, the sum of squares and the norm of
 * the last call; the segment table follows.  The host never reads it: no synchronisation.
 * Bad arguments return MH_ERR_ARG before any launch; n == 0 returns MH_OK without one. */
int64_t mh_adan_workspace_bytes(void);
int mh_adan_step(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *exp_avg_diff, float *neg_pre_grad,
                 int64_t n, int32_t n_segs, const int64_t *seg_end_host, const double *seg_lr_host, const int64_t *seg_step_host,
                 const int32_t *seg_flag_host, double beta1, double beta2, double beta3, double eps, double weight_decay,
                 double max_grad_norm, int32_t no_prox, void *workspace, void *stream);
/* The same step with "has a gradient" ON THE DEVICE, for data-parallel runs: seg_flag_dev [n_segs] > 0 = the segment is stepped
 * (the all-reduced has-gradient flags of the bucket; 0, a negative value or NaN: skipped); seg_seen_dev [n_segs] int64 in/out =
 * how many gradients the segment has seen: it goes up where the flag is positive, and 0 before makes this the first gradient.
 * Group steps advance unconditionally, so they still come from the host. */
int mh_adan_step_dev(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *exp_avg_diff, float *neg_pre_grad,
                     int64_t n, int32_t n_segs, const int64_t *seg_end_host, const double *seg_lr_host,
                     const int64_t *seg_step_host, const float *seg_flag_dev, int64_t *seg_seen_dev, double beta1, double beta2,
                     double beta3, double eps, double weight_decay, double max_grad_norm, int32_t no_prox, void *workspace,
                     void *stream);

/* ---- caller-side glue as single launches (csrc/losses.hip) -------------------------------------------------------------
 * Per-sample means of the training losses.  kind: 0 a, 1 a^2, 2 |a|, 3 binary entropy in bits of clamp(a, 1e-5, 1 - 1e-5)
 * (morpheus.py:1093-1096), 4 eikonal (|row| - 1)^2 of [M,3] rows (morpheus.py:1117-1119), 5 |a - b|, 6 (a - b)^2
 * (morpheus.py:764-777, :556).  a, b: [M, C] contiguous fp32 (b only for kinds 5, 6).  n_valid: device int32 or NULL -- only
 * the first n_valid rows count (fixed-capacity sampling); w_row [M] or NULL -- per-row weights.  out[0] = sum / den, out[1] =
 * den, with den = per_row * max(rows, 1) without weights (the reference's `.mean()`; per_row = C, 1 for kind 4) and
 * max(per_row * sum(w_row), 1) with them (morpheus.py:556).  ws: mh_masked_mean_workspace_floats() floats.  Two launches
 * forward (block partials, then one block adding them in a fixed order: deterministic, nothing to zero), one backward:
 * g_a = g * f'(a) * w_row / den inside the valid rows and 0 behind them, g_b = -g_a (either may be NULL); g: device scalar. */
int64_t mh_masked_mean_workspace_floats(void);
int mh_masked_mean_fwd(int32_t kind, const float *a, const float *b, const float *w_row, int64_t M, int32_t C,
                       const int32_t *n_valid, float *ws, float *out, void *stream);
int mh_masked_mean_bwd(int32_t kind, const float *a, const float *b, const float *w_row, int64_t M, int32_t C,
                       const int32_t *n_valid, const float *out, const float *g, float *g_a, float *g_b, void *stream);
/* out = x + scale * (cos(phi) u + sin(phi) v), u = normalize((n^_y, -n^_x, 0)), v = n^ x u, n^ = normalize(n): the random
 * direction orthogonal to the normal of morpheus.py:518-528 (get_ortho_normal_dir) applied to the points (:549, :766).
 * x, n, out [M,3], phi [M] (the caller's uniform draw times 2 pi).  Backward: g_x = g_out (no launch), g_n from *_bwd. */
int mh_ortho_perturb_fwd(const float *x, const float *n, const float *phi, float scale, int64_t M, float *out, void *stream);
int mh_ortho_perturb_bwd(const float *n, const float *phi, const float *g_out, float scale, int64_t M, float *g_n, void *stream);
/* The points of get_normal_smoothness_loss (morpheus.py:530-547): pts[k, n, :] = (depth[n] + off[k]) * rays_d[n, :] + rays_o[n, :],
 * keep[k, n] = |pts| < 1.1 as 0 / 1 (the reference drops the others with a boolean index, :546-547; here they leave the mean
 * through this weight).  depth [N], off [K], rays_o / rays_d [N,3], pts [K*N,3], keep [K*N].  Every product and sum rounded on
 * its own, in the operator chain's order: the same bits.  Backward: g_depth [N], g_o, g_d [N,3] (any may be NULL), the K points
 * of a ray added in index order.  One launch each way (12 / 8 as torch operators). */
int mh_smooth_points_fwd(const float *depth, const float *off, const float *rays_o, const float *rays_d, int64_t N, int32_t K,
                         float *pts, float *keep, void *stream);
int mh_smooth_points_bwd(const float *g_pts, const float *depth, const float *off, const float *rays_d, int64_t N, int32_t K,
                         float *g_depth, float *g_o, float *g_d, void *stream);
/* image = color + (1 - opacity) * bg with a per-ray background (morpheus.py:686-694; bg from get_bg_color, :887-903): color, bg,
 * image [N,3], opacity [N].  Backward: g_color = g_image (nothing to launch), g_opacity [N] = -sum_c g_image bg, g_bg [N,3] =
 * (1 - opacity) g_image (NULL: not wanted).  One launch each way (3 / 4 as torch operators), the chain's rounding. */
int mh_bg_blend_fwd(const float *color, const float *opacity, const float *bg, int64_t N, float *image, void *stream);
int mh_bg_blend_bwd(const float *g_image, const float *opacity, const float *bg, int64_t N, float *g_opacity, float *g_bg, void *stream);

/* Per-frame pose correction of a ray batch made of B rows of n_per_row rays, ONE frame per row (models/pose.py:4-64 PoseArray,
 * models/model.py:335-346 pose_optimisation): o' = o + t_f, d' = R(a, b, g)_f d with pose [n_frames, 6] = (a, b, g, t) per frame
 * and frame_of_row [B] (int64).  Backward: g_pose [n_frames, 6] = the full gradient (zeroed inside; rows of one frame add up
 * in row order); g_o / g_d may be NULL; ws: mh_pose_bwd_workspace_floats(B, n_per_row) floats.  One launch forward, two back. */
int64_t mh_pose_bwd_workspace_floats(int64_t B, int64_t n_per_row);
int mh_pose_apply_fwd(const float *rays_o, const float *rays_d, const float *pose, const int64_t *frame_of_row, int64_t B,
                      int64_t n_per_row, float *o_out, float *d_out, void *stream);
int mh_pose_apply_bwd(const float *rays_d, const float *pose, const int64_t *frame_of_row, int64_t B, int64_t n_per_row,
                      int64_t n_frames, const float *g_o, const float *g_d, float *ws, float *g_pose, void *stream);

/* The real-view render loss of a ray batch (morpheus.py:930-945 get_gt_from_data + :946-983 get_real_view_render_loss): per ray
 * m = mask > 0.5, gt_rgb = image m + bg (1 - m), valid = depth > 0 and |o + depth d| <= 1.1 and m;  rgb = mean (pred_rgb -
 * gt_rgb)^2, mask = BCE(clip(opacity, 1e-5, 1 - 1e-5), m), depth = mean (valid (pred_depth - depth))^2.  pred_rgb, bg, rays_o,
 * rays_d [N,3]; image [3,N] (channel-major, the dataset's layout); the others [N].  out[0] = w_rgb rgb + w_mask mask + w_depth
 * depth, out[1..3] = the terms; gt_rgb [3,N] and valid [N] are returned for the surface-point loss (:1001-1026).  One launch
 * (one workgroup walks the rays: deterministic) and one backward (g: device scalar; any of g_rgb / g_depth / g_opacity NULL). */
int mh_render_loss_fwd(const float *pred_rgb, const float *pred_depth, const float *opacity, const float *image,
                       const float *depth, const float *mask, const float *bg, const float *rays_o, const float *rays_d,
                       int64_t N, float w_rgb, float w_mask, float w_depth, float *gt_rgb, float *valid, float *out, void *stream);
int mh_render_loss_bwd(const float *pred_rgb, const float *pred_depth, const float *opacity, const float *gt_rgb,
                       const float *depth, const float *mask, const float *valid, int64_t N, float w_rgb, float w_mask,
                       float w_depth, const float *g, float *g_rgb, float *g_depth, float *g_opacity, void *stream);

/* ---- HIP-graph hygiene (no reference counterpart: the reference runs its step eagerly; morpheus.py:1147-1236 is the step
 * trainstep.GraphedRealViewStep captures).  graph = a hipGraph_t obtained by stream capture, not yet instantiated.
 * On ROCm 7.2 a small memset node replays wrongly from the second launch on (csrc/graph.hip); the library itself never
 * memsets, PyTorch's multi-block reductions do.  mh_graph_count_memset_nodes reports what a captured graph holds;
 * mh_graph_replace_memset_nodes turns every memset node into a fill-kernel node with the same edges (1-, 2- or 4-byte
 * patterns, 1-D or pitched 2-D; anything else -> MH_ERR_ARG and the graph is left as far as it got: discard it). */
int mh_graph_count_memset_nodes(void *graph, int64_t *n_nodes, int64_t *n_memset, int64_t *smallest_bytes);
int mh_graph_replace_memset_nodes(void *graph, int64_t *n_replaced);

/* ---- marching cubes (export_mesh, morpheus.py:367-408: mcubes.marching_cubes on the host there; csrc/mesh.hip) ----------
 * vol: dense fp32 [nx][ny][nz], C order (z fastest), nx, ny, nz >= 2 and nx*ny*nz < 2^31.  Conventions:
 *   corners: a corner is inside when f < iso (a NaN corner is outside); case index and the 12 edges in Bourke's numbering
 *     (csrc/mc_table.inc, generated by tools/gen_mc_table.py; every ambiguous face is cut the same way from both cells that
 *     share it -- each inside corner separated -- so closed level sets give closed meshes);
 *   vertices [V,3] in index space: the vertex on the edge from grid point p (value f0) to p + e_a (value f1) has coordinate
 *     a = (float)p_a + t, t = (iso - f0) / (f1 - f0) in fp32 (t = 0.5 when !(0 <= t <= 1): NaN / inf corners), the other
 *     two are p's;
 *   order: vertices by owner point (i*ny + j)*nz + k, then axis x < y < z; triangles [T,3] int32 by cell (the cell's corner 0
 *     point), then table order.  Deterministic run to run;
 *   winding: (v1 - v0) x (v2 - v0) points toward increasing f (outward for an SDF negative inside).
 * The triangle set is meant to equal mcubes.marching_cubes' up to vertex order and winding; that is NOT verified (mcubes was
 * not available to compare with).
 * mh_mc_workspace_bytes: workspace size (host only; -1 for an invalid shape).  mh_mc_count writes counts = {V, T} (DEVICE
 * int64 [2]) and waits for them on the stream: MH_ERR_OVERFLOW when V or T >= 2^31 (counts still written).  mh_mc_emit
 * (same vol, iso and workspace as the mh_mc_count before it) writes vertices [V,3] and triangles [T,3]; it never writes
 * outside those rows. */
int64_t mh_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int mh_mc_count(const float *vol, int32_t nx, int32_t ny, int32_t nz, float iso, void *workspace, int64_t *counts, void *stream);
int mh_mc_emit(const float *vol, int32_t nx, int32_t ny, int32_t nz, float iso, void *workspace, float *vertices,
               int32_t *triangles, void *stream);

/* The masked pair, for a volume with unobserved points (TSDF fusion below): weight [nx][ny][nz] fp32, a point is observed when
 * weight > 0 (a NaN weight is not).  A cell exists only when all eight of its corners are observed; such a cell gives the
 * triangles the unmasked pair gives it.  A vertex exists on a crossed edge only when at least one of the (up to four) cells
 * around the edge exists -- so both of its ends are observed -- and is written as above.  Order, winding and determinism as
 * above; with every weight positive the masked pair returns exactly the bytes of the unmasked pair.  Same protocol:
 * mh_mc_masked_workspace_bytes (larger: one byte per point more), mh_mc_count_masked (reads weight), mh_mc_emit_masked (same
 * vol, iso and workspace as the mh_mc_count_masked before it). */
int64_t mh_mc_masked_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int mh_mc_count_masked(const float *vol, const float *weight, int32_t nx, int32_t ny, int32_t nz, float iso, void *workspace,
                       int64_t *counts, void *stream);
int mh_mc_emit_masked(const float *vol, int32_t nx, int32_t ny, int32_t nz, float iso, void *workspace, float *vertices,
                      int32_t *triangles, void *stream);

/* ---- mesh rendering (render_all_meshes, morpheus.py:418-470: an Open3D window per frame there; csrc/raster.hip) -----------
 * A triangle rasteriser over the arrays mh_mc_emit writes: vertices [V,3] fp32 world space, triangles [T,3] int32, optional
 * colors [V,3] and normals [V,3] fp32.  Every fp32 expression below is evaluated operator by operator, round to nearest, no
 * FMA, in the written order (tests/raster_oracle.py is written from this text).  A triangle with an index outside [0, V) is
 * skipped everywhere.
 *   camera: OpenCV camera space (x right, y down, z forward).  w2c_host: 12 HOST floats, row-major [3][4] = (R | t), the
 *     inverse of the camera-to-world pose, formed by the caller in float64.  fx, fy, cx, cy as in mh_generate_rays: the
 *     centre of pixel (i, j) = (column, row) is at screen coordinate (i + 0.5, j + 0.5).  (An OpenGL c2w becomes an OpenCV
 *     one by negating its columns 1 and 2.)  H, W in [1, 16384].
 *   vertex stage: Pc_r = ((w[r][0]*x + w[r][1]*y) + w[r][2]*z) + w[r][3];  sx = (fx*xc)/zc + cx, sy = (fy*yc)/zc + cy;
 *     X = (int32) rintf(sx*256), Y likewise (8 sub-pixel bits, ties to even).  A triangle with a vertex that has
 *     !(zc >= near) is dropped whole and counted in *clipped; so is one with a vertex whose rintf(sx*256) or rintf(sy*256)
 *     is not below 2^23 in magnitude (NaN included).  On-screen coordinates are below 2^22, differences below 2^25, edge
 *     products below 2^50: exact in int64.
 *   coverage: A2 = (X1-X0)*(Y2-Y0) - (Y1-Y0)*(X2-X0) in int64; A2 == 0: dropped; A2 < 0: vertices 1 and 2 trade places
 *     (both orientations are drawn).  For each edge e -> e+1 with (dx, dy) = (X[e+1]-X[e], Y[e+1]-Y[e]) and the centre
 *     (px, py) = (256 i + 128, 256 j + 128):  E = dx*(py - Y[e]) - dy*(px - X[e]).  The centre is covered when, on all three
 *     edges, E > 0, or E == 0 and (dy > 0 or (dy == 0 and dx > 0)).  The tie rule depends on the edge alone and holds for
 *     exactly one of an edge's two directions, so two triangles on opposite sides of a shared edge never both cover and
 *     never both miss a centre on it.  Candidates: i in [max((Xmin+127)>>8, 0), min((Xmax-128)>>8, W-1)], j likewise.
 *   depth: camera-space z of the ray through the pixel centre and the triangle's plane, from the UNSNAPPED camera-space
 *     vertices a, b, c in the caller's order: e1 = b-a, e2 = c-a, n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y -
 *     e1y*e2x), na = (nx*ax + ny*ay) + nz*az, dir = ((((float)i + 0.5f) - cx)/fx, (((float)j + 0.5f) - cy)/fy, 1),
 *     z = na / ((nx*dirx + ny*diry) + nz).  A fragment with !(near <= z < inf) is dropped.  This is the camera-space z that
 *     Open3D's capture_depth_float_buffer is understood to return (0 = background); NOT verified, Open3D was not available.
 *   depth test: one uint64 per pixel, key = (bits(z) << 32) | t, global atomic minimum; z > 0 makes the bits monotone, equal
 *     depths go to the lower triangle index.  depth, tri_id and clipped are therefore the same bytes run to run and for
 *     any order of the launches' work.  They are pinned bit for bit by the numpy restatement.
 *   resolve, one pixel: z, t from the key; P = (z*dirx, z*diry, z); r_k = vertex_k - P (k = a, b, c);
 *     w_a = n . (r_b x r_c), w_b = n . (r_c x r_a), w_c = n . (r_a x r_b) (cross and dot in the forms above), s = (w_a + w_b)
 *     + w_c, l_k = w_k / s (perspective correct: areas in 3-D; when an l_k is not finite -- a sliver whose sub-areas underflow
 *     or cancel -- all three are 1/3);  attribute = (l_a*A_a + l_b*A_b) + l_c*A_c.
 *     mode 0 "color": the interpolated colour, 0.7 grey without colors.  mode 1 "normal": the interpolated vertex normal,
 *     rotated by R, normalised (|v| = sqrtf((x*x + y*y) + z*z), (0,0,1) when that is not in (0, inf)), then (n + 1)/2.
 *     mode 2 "shaded": colour * (ambient + (1 - ambient) * |n^ . v^|), v^ = normalised -P: a head-light, back faces lit like
 *     front faces.  Agreement with Open3D's lighting is not a goal.  Empty pixels: depth 0, tri_id -1, image = background.
 *     The image and the normalised vertex normals are NOT pinned bit for bit: they are held to the error rule of DESIGN 4
 *     (error against float64 <= 3 x the numpy-fp32 restatement's own, floor 2^-22).
 *   vertex normals (Open3D compute_vertex_normals): c_t = (b-a) x (c-a) in world space (form above; a triangle with a
 *     component that is not finite is skipped).  m = max |component| over the mesh, E its biased fp32 exponent field,
 *     G = 2^(E-126) (a power of two strictly above m), q = G * 2^-40.  Each component is rounded once, k = llrint((double)c /
 *     q), and added to its three vertices with 64-bit integer atomics: acc [3V + 1] DEVICE int64 holds the sums [V][3] and,
 *     in its last word, the bits of m.  normal = normalise((float)k_x, (float)k_y, (float)k_z) as above.  The sums are
 *     order-free: bit-identical run to run and under any permutation of the triangles.
 * mh_raster_workspace_bytes: host only; -1 for H or W outside [1, 16384] or T outside [0, 2^31).
 * mh_raster_depth: vertex stage, coverage and depth test into `workspace`; clipped: DEVICE int64, overwritten.  small_area:
 *   a triangle whose clamped box holds more pixel centres than this is walked by whole wavefronts (queued on the device)
 *   instead of one lane; <= 0 takes the default; results do not depend on it.  No host synchronisation.
 * mh_raster_resolve: depth [H,W] fp32, tri_id [H,W] int32, image [H,W,3] fp32 from the workspace mh_raster_depth filled with
 *   the same mesh and camera.  mode 1 and 2 need normals.  T == 0 or V == 0 is valid and gives the background.
 * Bad arguments return MH_ERR_ARG before any launch. */
int mh_mesh_vertex_normals(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, int64_t *acc, float *normals,
                           void *stream);
int64_t mh_raster_workspace_bytes(int32_t H, int32_t W, int64_t T);
int mh_raster_depth(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, const float *w2c_host, float fx,
                    float fy, float cx, float cy, int32_t H, int32_t W, float near, int32_t small_area, void *workspace,
                    int64_t *clipped, void *stream);
int mh_raster_resolve(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, const float *colors,
                      const float *normals, const float *w2c_host, float fx, float fy, float cx, float cy, int32_t H, int32_t W,
                      int32_t mode, float ambient, float bg_r, float bg_g, float bg_b, const void *workspace, float *depth,
                      int32_t *tri_id, float *image, void *stream);

/* ---- mesh evaluation (tools/culling.py of the reference: cull_from_one_pose, trimesh.sample.sample_surface, the KD-tree
 * queries of accuracy / completion / completion_ratio, Open3D's point-to-point ICP; csrc/mesheval.hip, csrc/subdivide.hip) ---
 * Every fp32 expression below is evaluated operator by operator, round to nearest, no FMA, in the written order; so is every
 * float64 one (tests/mesheval_oracle.py is written from this text).  All counts are in [0, 2^31).
 *   nearest neighbour (mh_nn_search): query [Nq,3], ref [Nr,3] fp32.  For query q and reference point r:
 *     dx = q.x - r.x, dy = q.y - r.y, dz = q.z - r.z, d2 = (dx*dx + dy*dy) + dz*dz in fp32.  A candidate is admissible when
 *     d2 < +inf (a NaN or an overflowed d2 never wins) and d2 <= max_d2; max_d2 = +inf switches the second test off (the
 *     caller squares its distance bound once in fp32).  The winner is the admissible candidate of least d2, the lowest index
 *     among equals: idx [Nq] int32, d2 [Nq] fp32; idx = -1, d2 = +inf without one (Nr == 0 included).  Exact brute force
 *     over all Nq * Nr pairs.  The reference set is cut into `segments` runs (<= 0: a default from the sizes; at most 4096)
 *     whose results meet in a 64-bit atomic minimum on (bits(d2) << 32) | index -- d2 >= +0, so the key orders like (d2,
 *     index): idx and d2 are the same bytes run to run and for every value of `segments`.  workspace: mh_nn_workspace_bytes
 *     (Nq) = 8 Nq DEVICE bytes (host only; -1 for a bad Nq).  mh_nn_tile_points: reference points per LDS tile (host only;
 *     for tests that place sizes on the kernel's internal boundaries; 256 queries per workgroup, 64 per wavefront).
 *   culling (mh_cull_vertices, mh_cull_triangles): w2c_host = 12 HOST doubles, row-major [3][4] = (R | t), world -> OpenCV
 *     camera, the inverse of the pose formed by the caller in float64; K_host = 9 HOST doubles, row-major 3 x 3.  Per vertex
 *     (x, y, z) = (double) of its fp32 coordinates, all in float64:
 *       cam_r = ((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r];  uvz_r = (K[r][0]*cam_0 + K[r][1]*cam_1) + K[r][2]*cam_2;
 *       pz = uvz_2 + 1e-8;  px = uvz_0 / pz;  py = uvz_1 / pz;
 *       frustum  = 0 <= px and px <= W-1 and 0 <= py and py <= H-1 and pz > 0   (false whenever a NaN takes part);
 *       u = (int)px, v = (int)py (truncation), read only when frustum holds;
 *       observed = frustum and pz < (double)(rendered_depth[v][u] + eps)   -- the sum is an fp32 addition of two fp32 values;
 *       invalid  = frustum and depth_gt[v][u] <= 0   (false everywhere when depth_gt is NULL).
 *     rendered_depth, depth_gt: fp32 [H][W], H, W in [1, 16384].  The three masks are uint8 [V] of 0 / 1.
 *     mh_cull_triangles: keep[t] = 1 when any of the triangle's vertices is observed and not all three are invalid; 0 for a
 *     triangle with an index outside [0, V).
 *   area weights (mh_mesh_area_weights): per triangle (a, b, c), with the cross product of the rasteriser's depth stage in
 *     world space (e1 = b-a, e2 = c-a, n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x)):
 *     area = sqrtf((nx*nx + ny*ny) + nz*nz) * 0.5f; 0 when that is not finite or an index is outside [0, V).  areas [T] fp32.
 *     m = the largest area, E its biased fp32 exponent field, G = 2^(E-126) (a power of two strictly above m), q = G * 2^-40;
 *     qarea[t] = llrint((double)area / q) (the division is exact: a multiplication by 2^(166-E)); qarea [T + 1] DEVICE int64,
 *     its last word the bits of m.  The caller's inclusive prefix sum over qarea[:T] is integer and exact in any order.
 *   sampling (mh_sample_surface): cum [T] = that inclusive prefix sum, total = cum[T-1] > 0; uniforms [count,3] fp32 in
 *     [0, 1).  target = (int64)((double)u0 * (double)total) (0 for u0 < 0 or NaN, total-1 for u0 >= 1, and never above
 *     total-1); face = the first f with cum[f] > target (binary search: lo = 0, hi = T-1; while lo < hi: mid = (lo+hi)>>1;
 *     cum[mid] > target ? hi = mid : lo = mid+1), so a face of quantised area 0 is never chosen.  r1 = u1, r2 = u2; if
 *     r1 + r2 > 1 (fp32): r1 = 1 - r1, r2 = 1 - r2; point_a = (v0_a + r1*(v1_a - v0_a)) + r2*(v2_a - v0_a) in fp32.  points
 *     [count,3] fp32 (NaN for a face with an index outside [0, V)), face [count] int32.
 *   rigid alignment (mh_icp_transform, mh_icp_sums): T_host = 12 HOST doubles, row-major [3][4].  out_r = (float)(((T[r][0]*x
 *     + T[r][1]*y) + T[r][2]*z) + T[r][3]) in float64 from the fp32 source point, rounded once.  mh_icp_sums: over the points
 *     i with 0 <= idx[i] < Nt, with p = p[i], q = target[idx[i]] (fp32 values taken to float64): sums [17] DEVICE doubles =
 *     {n, sum d2[i], sum p (3), sum q (3), sum p_a*q_b (9, at 8 + 3a + b)}.  Float64 sums in a fixed order (a lane's points in
 *     index order, the lanes of a wavefront in an xor butterfly, the wavefronts and then the workgroups' partials in index
 *     order): the same bytes run to run; against another summation order they differ by float64 round-off only.  workspace:
 *     mh_icp_workspace_bytes() DEVICE bytes (host only).
 *   subdivision (mh_subdiv_count, mh_subdiv_emit; csrc/subdivide.hip, restated by tests/subdivide_oracle.py): midpoint
 *     subdivision to a maximum edge, trimesh.remesh.subdivide_to_size as cull_one_mesh runs it before culling.  A midpoint split
 *     halves all three edges in all four children, so the recursion ends, per input triangle, at a uniform tessellation of
 *     depth d; this is that closed form.  max_edge is fp32, finite and > 0; max_iter in [0, 10]; m = (double)max_edge, m2 = m*m.
 *     Per edge (p, q) of a triangle (a, b, c) -- (a, b), (b, c), (c, a) -- in float64 from the fp32 coordinates:
 *       dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z, l2 = (dx*dx + dy*dy) + dz*dz;
 *       d_e = the smallest d in [0, max_iter + 1] for which  l2 * 4^-d > m2  is false (4^-d is exact; no square root; a NaN l2
 *       gives 0, an infinite one max_iter + 1).
 *     depth[t] = the largest of the three d_e; 0 for a triangle with an index outside [0, V).  depth = max_iter + 1 means "too
 *     long": the caller refuses such a mesh; both entry points treat the triangle as one of depth 0.
 *     mh_subdiv_count: depth int32 [T]; n_vert, n_tri DEVICE int64 [T]: with n = 2^d and L = (n + 1)(n + 2)/2, a triangle of
 *     depth d in [1, max_iter] adds L - 3 vertices and becomes n*n triangles; any other adds 0 and stays 1.  The caller's
 *     exclusive prefix sums vert_start, tri_start (DEVICE int64 [T + 1], [0] = 0, [T] = the totals) are integer and exact in any
 *     order.
 *     mh_subdiv_emit: lattice point (i, j) of a split triangle with corners A, B, C, i, j >= 0, i + j <= n, k = n - i - j:
 *       P(i, j)_x = (float)(((k*A_x + i*B_x) + j*C_x) / n)   -- k, i, j, n and the fp32 coordinates taken to float64, every
 *       operator rounded in float64 in the written order, one rounding to fp32 (y, z and the three colour channels alike).
 *     Its full lattice index is q(i, j) = j(n + 1) - j(j - 1)/2 + i in [0, L).  q = 0, q = n and q = L - 1 are the input
 *     vertices a, b, c and are not emitted; any other q is output vertex V + vert_start[t] + (q < n ? q - 1 : q - 2).
 *     out_vertices [V + n_new_vertices, 3]: the V input vertices unchanged, then every split triangle's new ones in triangle
 *     order (vertices are not welded across triangles; lattice points on an edge that two triangles of equal depth share are
 *     the same bytes from both sides, up to the sign of a zero).  out_colors likewise from colors [V,3]; both NULL or neither.
 *     out_triangles int32 [n_triangles, 3] in input-triangle order from tri_start[t]: a triangle that is not split is copied;
 *     a split one gives rows j = 0 .. n-1, row j starting at local index j(2n - j), s = 0 .. 2(n - j) - 2, i = s >> 1:
 *       s even: (P(i, j), P(i+1, j), P(i, j+1));   s odd: (P(i+1, j), P(i+1, j+1), P(i, j+1))   -- the winding of (a, b, c).
 *     out_index int32 [n_triangles] or NULL: the input triangle t of every output triangle.  n_new_vertices, n_triangles: the
 *     two totals as the caller read them, n_triangles >= T; MH_ERR_OVERFLOW when V + n_new_vertices or n_triangles >= 2^31.
 *     One thread per output vertex and per output triangle; each finds t as the last t with start[t] <= its output index.
 * Bad arguments return MH_ERR_ARG before any launch; an empty input (Nq, V, T, count or N of 0) returns MH_OK without a launch
 * and writes nothing. */
int64_t mh_nn_workspace_bytes(int64_t Nq);
int32_t mh_nn_tile_points(void);
int mh_nn_search(const float *query, int64_t Nq, const float *ref, int64_t Nr, float max_d2, int32_t segments, void *workspace,
                 int32_t *idx, float *d2, void *stream);
int mh_cull_vertices(const float *vertices, int64_t V, const double *w2c_host, const double *K_host, int32_t H, int32_t W,
                     const float *rendered_depth, const float *depth_gt, float eps, uint8_t *frustum, uint8_t *observed,
                     uint8_t *invalid, void *stream);
int mh_cull_triangles(const int32_t *triangles, int64_t T, int64_t V, const uint8_t *observed, const uint8_t *invalid,
                      uint8_t *keep, void *stream);
int mh_mesh_area_weights(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, float *areas, int64_t *qarea,
                         void *stream);
int mh_sample_surface(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, const int64_t *cum,
                      const float *uniforms, int64_t count, float *points, int32_t *face, void *stream);
int mh_subdiv_count(const float *vertices, int64_t V, const int32_t *triangles, int64_t T, float max_edge, int32_t max_iter,
                    int32_t *depth, int64_t *n_vert, int64_t *n_tri, void *stream);
int mh_subdiv_emit(const float *vertices, const float *colors, int64_t V, const int32_t *triangles, int64_t T,
                   const int32_t *depth, const int64_t *vert_start, const int64_t *tri_start, int64_t n_new_vertices,
                   int64_t n_triangles, float *out_vertices, float *out_colors, int32_t *out_triangles, int32_t *out_index,
                   void *stream);
int64_t mh_icp_workspace_bytes(void);
int mh_icp_transform(const float *src, int64_t N, const double *T_host, float *out, void *stream);
int mh_icp_sums(const float *p, int64_t N, const float *target, int64_t Nt, const int32_t *idx, const float *d2,
                void *workspace, double *sums, void *stream);

/* ---- pose initialisation (preprocess/pose_init/registrate.py of the reference: mask2camera, and the robust rigid registration
 * it hands to the external program FRICP, method 3; csrc/poseinit.hip) ------------------------------------------------------------
 * Every fp32 and float64 expression below is evaluated operator by operator, round to nearest, no FMA, in the written order
 * (tests/poseinit_oracle.py is written from this text).  All counts are in [0, 2^31).
 *   masked back-projection (mh_depth_points_count, mh_depth_points_emit): depth [H][W] fp32 in metres, mask [H][W] uint8, H, W in
 *     [0, 16384].  Pixel (u, v) = (column, row) is KEPT when mask[v][u] != 0 and depth[v][u] > 0 (false for a NaN depth).  fx, fy,
 *     cx, cy are HOST doubles, fx and fy non-zero, none a NaN.  With d = depth[v][u], in float64 from the fp32 depth, one rounding:
 *       x = (float)(((double)d * ((double)u - cx)) / fx),  y = (float)(((double)d * ((double)v - cy)) / fy),  z = d
 *     -- the pixel's integer coordinates, as mask2camera has them (no half-pixel offset).  The image is cut, in row-major pixel
 *     order i = v*W + u, into tiles of mh_depth_points_tile() pixels (host only).  mh_depth_points_count: counts [tiles] DEVICE
 *     int64, the kept pixels of each tile, tiles = ceil(H*W / tile).  The caller's exclusive prefix sum tile_start (DEVICE int64
 *     [tiles], or [tiles + 1] with the total behind) is integer and exact in any order; n = the total, as the caller read it.
 *     mh_depth_points_emit: points [n,3] fp32 in row-major pixel order (the order of numpy.nonzero(mask)); pixel [n] int32 or
 *     NULL: the index i of every point.  A point whose place falls outside [0, n) is not written.  H == 0, W == 0 or (emit)
 *     n == 0 return MH_OK without a launch.
 *   k nearest distances (mh_knn_d2): points [N,3] fp32, k in [1, 8].  For point i, over all j != i (excluded by INDEX: another
 *     point with the same coordinates counts, with d2 = 0): dx = p_i.x - p_j.x, dy, dz likewise, d2 = (dx*dx + dy*dy) + dz*dz in
 *     fp32, as in mh_nn_search.  out_d2 [N][k] fp32: the k smallest admissible d2 in ascending order; a d2 is admissible when
 *     d2 < +inf (a NaN or an overflowed d2 never enters); entries for which none is left are +inf.  Exact brute force over all
 *     N * N pairs; values only, so equal d2 need no tie rule.  mh_knn_tile_points: points per LDS tile (host only; for tests; 256
 *     points per workgroup).
 *   Welsch-weighted sums (mh_icp_wsums): mh_icp_sums with a weight per correspondence.  inv_2nu2 = 1 / (2 nu^2) is a HOST
 *     double, >= 0 and finite.  Over the points i with 0 <= idx[i] < Nt, with p = p[i], q = target[idx[i]] and dd = d2[i] (fp32
 *     values taken to float64; dd finite), all in float64:
 *       w = exp(-dd * inv_2nu2)   (the device's float64 exp: within an ulp or so of the correctly rounded value);  wp_a = w * p_a;
 *     sums [19] DEVICE doubles = {sum w, sum w*dd, sum wp_a (3), sum w*q_b (3), sum wp_a*q_b (9, at 8 + 3a + b), sum (1.0 - w),
 *     the number of such i}.  The partition of the points, the order of every addition and the meeting of lanes, wavefronts and
 *     workgroups are mh_icp_sums': with inv_2nu2 = 0 (w = 1.0) sums[0..16] are the bytes mh_icp_sums returns, and the rigid
 *     motion of the weighted least-squares problem comes from sums[0..16] by the same formulas.  The same bytes run to run.
 *     workspace: mh_icp_wsums_workspace_bytes() DEVICE bytes (host only).
 * Bad arguments return MH_ERR_ARG before any launch; N == 0 returns MH_OK without a launch and writes nothing. */
int32_t mh_depth_points_tile(void);
int mh_depth_points_count(const float *depth, const uint8_t *mask, int32_t H, int32_t W, int64_t *counts, void *stream);
int mh_depth_points_emit(const float *depth, const uint8_t *mask, int32_t H, int32_t W, double fx, double fy, double cx, double cy,
                         const int64_t *tile_start, int64_t n, float *points, int32_t *pixel, void *stream);
int32_t mh_knn_tile_points(void);
int mh_knn_d2(const float *points, int64_t N, int32_t k, float *out_d2, void *stream);
int64_t mh_icp_wsums_workspace_bytes(void);
int mh_icp_wsums(const float *p, int64_t N, const float *target, int64_t Nt, const int32_t *idx, const float *d2, double inv_2nu2,
                 void *workspace, double *sums, void *stream);

/* ---- TSDF fusion (run_tsdf_fusion / back_proj_frame, tools/vis.py:251-361 of the reference: Open3D's ScalableTSDFVolume on the
 * host there; csrc/tsdf.hip) ----------------------------------------------------------------------------------------------------
 * RGB-D frames are fused into a truncated signed distance volume whose zero set mh_mc_*_masked extracts.  The rules restate
 * Open3D's UniformTSDFVolume::Integrate / ScalableTSDFVolume as documented and remembered; Open3D was not available, so
 * agreement with it is NOT verified.  Every fp32 expression below is evaluated operator by operator, round to nearest, no FMA,
 * in the written order (tests/tsdf_oracle.py is written from this text).
 *   volume: an axis-aligned box at origin (ox, oy, oz) of nbx x nby x nbz blocks of 8^3 voxels, nx = 8 nbx voxels along x (ny,
 *     nz likewise), nx*ny*nz < 2^31, voxel side voxel_length > 0.  Voxel (i, j, k) stands at p = (ox + ((float)i + 0.5f) *
 *     voxel_length, oy + ..j.., oz + ..k..).  Dense arrays in C order (k fastest): tsdf [nx][ny][nz] fp32, weight [nx][ny][nz]
 *     fp32 (the number of frames that updated the voxel), color [3][nx][ny][nz] fp32 in [0, 255] (three planes), active
 *     [nbx][nby][nbz] uint8 (one byte per block, 0 or 1).  The caller zeroes all four before the first frame.
 *   frame: depth [H][W] fp32, rgb [H][W][3] uint8, mask [H][W] uint8 or NULL, H, W in [1, 16384].  fx, fy (non-zero), cx, cy
 *     as in mh_generate_rays and mh_raster_*: the centre of pixel (i, j) = (column, row) is at (i + 0.5, j + 0.5).  Intrinsics
 *     that put pixel centres at integers (Open3D's) are the same kernels with cx + 0.5, cy + 0.5.
 *   usable depth: d = depth[j][i] / depth_scale; the pixel is usable when mask is NULL or mask[j][i] != 0, and d > 0 and
 *     d <= depth_trunc (a NaN or infinite d is not usable).  depth_scale > 0, depth_trunc > 0.
 *   back-projection (touch, bounds): c2w_host = 12 HOST floats, row-major [3][4] = (R | t), the OpenCV camera-to-world pose.
 *     xc = ((((float)i + 0.5f) - cx) / fx) * d, yc = ((((float)j + 0.5f) - cy) / fy) * d, zc = d;
 *     P_r = ((c[r][0]*xc + c[r][1]*yc) + c[r][2]*zc) + c[r][3].  Sampled pixels: i and j multiples of `stride` >= 1.
 *   touch (mh_tsdf_touch, per frame, before its integration): for every sampled usable pixel and every axis a, with
 *     L = 8.0f * voxel_length: lo_a = floorf(((P_a - sdf_trunc) - o_a) / L), hi_a = floorf(((P_a + sdf_trunc) - o_a) / L); when
 *     hi_a >= 0 and lo_a <= nb_a - 1 on all three axes (false for a NaN), every block in [max(lo, 0), min(hi, nb - 1)]^3 gets
 *     active = 1.  Plain stores of the same byte: order-free.  A block that is not active when a frame is integrated does not
 *     see that frame.
 *   integrate (mh_tsdf_integrate, every voxel of every active block): w2c_host = 12 HOST floats, row-major [3][4], the float64
 *     inverse of the OpenCV camera-to-world pose rounded once, as mh_raster_depth takes it.
 *     pc_r = ((w[r][0]*px + w[r][1]*py) + w[r][2]*pz) + w[r][3]; skipped unless pc_z > 0.
 *     u = floorf((fx*pc_x)/pc_z + cx), v = floorf((fy*pc_y)/pc_z + cy); skipped unless 0 <= u < W and 0 <= v < H (false for a
 *     NaN); the pixel is (i, j) = (u, v); skipped unless it is usable, with depth d.
 *     a = (((float)i + 0.5f) - cx) / fx, b = (((float)j + 0.5f) - cy) / fy, m = sqrtf((1.0f + a*a) + b*b) (the length of the
 *     pixel's ray at z = 1);  sdf = (d - pc_z) * m; skipped unless sdf > -sdf_trunc;  q = sdf / sdf_trunc, t = q < 1 ? q : 1.
 *     With w = weight and w1 = w + 1.0f:  tsdf = (tsdf*w + t) / w1;  color_c = (color_c*w + (float)rgb[j][i][c]) / w1 for the
 *     three channels;  weight = w1.  One lane owns a voxel and frames are applied in the order of the calls, so a volume is the
 *     same bytes run to run.  tsdf, weight, color and active are pinned bit for bit by the numpy restatement.
 *   bounds (mh_tsdf_bounds): bounds = 6 DEVICE int32 {min x, y, z, max x, y, z} of the finite P of the sampled usable pixels, as
 *     ordered bit patterns (o = bits >= 0 ? bits : bits ^ 0x7fffffff, which orders like the value), folded into what the words
 *     hold by integer atomic minimum / maximum: the caller starts them at INT32_MAX (3) and INT32_MIN (3), may run any number
 *     of frames into them and reads them once.  Order-free.
 *   vertex colours (mh_tsdf_vertex_colors): vertices [V,3] in the index space of mh_mc_emit_masked over tsdf.  Per coordinate
 *     a: f_a = floorf(x_a) (a vertex with an f_a outside [0, n_a - 1] gets colour 0), r_a = x_a - f_a.  The edge's axis is the
 *     first a with r_a > 0 and f_a + 1 < n_a, t = r_a there; p0 = the point (f_x, f_y, f_z), p1 = p0 + e_a (p1 = p0, t = 0
 *     without such an axis).  out_c = ((1.0f - t)*color_c[p0] + t*color_c[p1]) / 255.0f: out [V,3] fp32 in [0, 1].
 * mh_tsdf_group_blocks: how many blocks along z one workgroup of mh_tsdf_integrate covers (host only; for tests that place box
 * sizes on the kernel's internal boundaries).  No entry point synchronises with the host.  Bad arguments return MH_ERR_ARG
 * before any launch; V == 0 returns MH_OK without one; a frame without a usable pixel and a box without an active block are
 * valid and change nothing. */
int32_t mh_tsdf_group_blocks(void);
int mh_tsdf_bounds(const float *depth, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                   const float *c2w_host, float depth_scale, float depth_trunc, int32_t stride, int32_t *bounds, void *stream);
int mh_tsdf_touch(const float *depth, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                  const float *c2w_host, float depth_scale, float depth_trunc, int32_t stride, float ox, float oy, float oz,
                  float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby, int32_t nbz, uint8_t *active, void *stream);
int mh_tsdf_integrate(const float *depth, const uint8_t *rgb, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy,
                      float cx, float cy, const float *w2c_host, float depth_scale, float depth_trunc, float ox, float oy, float oz,
                      float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby, int32_t nbz, const uint8_t *active, float *tsdf,
                      float *weight, float *color, void *stream);
int mh_tsdf_vertex_colors(const float *vertices, int64_t V, const float *color, int32_t nx, int32_t ny, int32_t nz, float *out,
                          void *stream);

/* ---- TSDF fusion, the pooled block-sparse store (csrc/tsdf_sparse.hip) --------------------------------------------------------
 * The same fusion into a volume that holds only the blocks a frame reached, so that the logical box may have more than 2^31
 * voxels (Open3D's ScalableTSDFVolume is unbounded; this one is a bounded box with unbounded-looking cost).  The frame, the
 * usable depth, the back-projection, the voxel position and every fp32 expression of touch and integrate are the dense text's
 * above, with the GLOBAL voxel index: voxel (i, j, k) of the logical box stands at ox + ((float)i + 0.5f) * voxel_length.
 * tests/tsdf_sparse_oracle.py is written from this text.
 *   logical box: nbx x nby x nbz blocks of 8^3 voxels at origin.  Each side has at most 4096 blocks (32768 voxels: (float)i is
 *     exact and a marching-cubes coordinate (float)i + t still resolves 2^-9 of a voxel), and nbx*nby*nbz < 2^31; the voxel count
 *     may exceed 2^31 (2048 x 2048 x 1024 voxels is 2^25 blocks).  mh_tsdf_sparse_max_side_blocks returns the 4096.
 *   index volume: slot [nbx][nby][nbz] int32, C order, 4 bytes a block; the linear block id is (bx*nby + by)*nbz + bz.  -1: no
 *     storage; s in [0, capacity): the block's voxels are in slot s of the pool.  The one other value, -2, is no storage either
 *     (a block being won inside mh_tsdf_sparse_touch, or one that found the pool full).  The caller fills it with -1.
 *   pool: `capacity` >= 1 slots; slot s holds its block's 512 voxels contiguously, voxel (i, j, k) of the block at
 *     s*512 + (i*8 + j)*8 + k.  Five fp32 planes: tsdf [capacity][512], weight [capacity][512], color [3][capacity][512]
 *     (10 240 bytes a slot).  slot_block [capacity] int32: the block id of each slot.  counters: 2 DEVICE int32 {the number of
 *     blocks that were given or refused a slot, the overflow flag}; min(counters[0], capacity) slots are live.  The caller
 *     zeroes the planes and the counters once, before the first frame.
 *   the block rule is the dense one: a block gets storage when a frame's touch pass reaches it (the same lo / hi block range,
 *     clipped to the box in the same way), and that frame is the first it sees; a block without storage when a frame is
 *     integrated does not see that frame, and reads as tsdf 0, weight 0, colour 0.
 *   touch (mh_tsdf_sparse_touch): for every block of a pixel's range whose entry is -1, exactly one lane wins it (compare and
 *     swap, -1 -> -2), takes s = the counter's next value and, when s < capacity, writes slot_block[s] and the entry.  With
 *     s >= capacity nothing is written but the overflow flag (the entry stays -2, the counter goes on counting, so counters[0]
 *     is the number of slots the frames so far needed).  Which block gets which slot differs from run to run; nothing an entry
 *     point returns depends on it: every result below is defined by block coordinates.
 *   integrate (mh_tsdf_sparse_integrate): walks the live slots (the launch is sized by capacity; mh_tsdf_sparse_group_slots
 *     slots per workgroup, host only, for tests), decodes the block from slot_block, one lane per voxel, no atomics.
 *   mh_tsdf_sparse_mark: the touch pass of mh_tsdf_touch (one byte per block, active [nbx][nby][nbz] uint8) over a logical box
 *     with the limits of this section: run over all frames and summed, it is the number of slots the frames will need.
 *   mh_tsdf_sparse_to_dense: scatters the live slots into zeroed dense arrays of the dense section's layout (the box must be
 *     one the dense store takes: fewer than 2^31 voxels) and sets active = 1 for their blocks.
 *   mh_tsdf_sparse_from_dense: the reverse, into a fresh store (entries -1, counters 0): block b of the dense arrays gets a slot
 *     when keep is NULL or keep[b] != 0 (keep [nbx][nby][nbz] uint8).  order: NULL, or DEVICE int32 [nbx*nby*nbz], a permutation
 *     of the block ids: the order in which the blocks are dispatched, hence (loosely) the order of their slots; ids outside the
 *     box are skipped.  More kept blocks than capacity: the overflow flag, as in touch.
 *   marching cubes (mh_mc_count_sparse / mh_mc_emit_sparse): the masked pair's rules over the logical box -- a point is
 *     observed when its block has storage and its weight > 0; a cell exists when its eight corners are observed; a crossed edge
 *     owns a vertex only when one of the (up to four) cells around it exists; vertex formula, winding and triangles per cell as
 *     above -- with corner values read through the index volume from the block and its neighbours.  Vertices are in the index
 *     space of the logical box ((float)i + t with the global i).  sorted_blocks: DEVICE int32 [capacity] whose first
 *     min(counters[0], capacity) entries are the live slots' block ids in ascending order (the rest is not read).  Order:
 *     blocks in ascending block id; inside a block vertices by owner point (i*8 + j)*8 + k, then axis x < y < z, triangles by
 *     cell, then table order.  The same bytes run to run and for every assignment of slots.  For a box the dense store takes,
 *     the vertex and triangle SETS are those of mh_mc_*_masked over the scattered volume; the order differs (by block there,
 *     by point here).  mh_mc_sparse_workspace_bytes(capacity): host only, -1 for capacity < 1.  mh_mc_count_sparse writes
 *     counts = {V, T} (DEVICE int64 [2]) and does NOT wait for them; the caller reads them (with the counters) and refuses
 *     V or T >= 2^31.  mh_mc_emit_sparse (same arguments and workspace) never writes outside its V and T rows.
 *   vertex colours (mh_tsdf_sparse_vertex_colors): the dense rule with n_a = 8 nb_a; colour reads go through the index volume
 *     and give 0 for a block without storage.
 * No entry point synchronises with the host.  Bad arguments return MH_ERR_ARG before any launch.  A slot read from memory is
 * used only inside [0, capacity) and a block id only inside the box, so no state of the arrays makes a kernel write outside
 * them. */
int32_t mh_tsdf_sparse_group_slots(void);
int32_t mh_tsdf_sparse_max_side_blocks(void);
int mh_tsdf_sparse_mark(const float *depth, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                        const float *c2w_host, float depth_scale, float depth_trunc, int32_t stride, float ox, float oy, float oz,
                        float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby, int32_t nbz, uint8_t *active, void *stream);
int mh_tsdf_sparse_touch(const float *depth, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                         const float *c2w_host, float depth_scale, float depth_trunc, int32_t stride, float ox, float oy, float oz,
                         float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity, int32_t *slot,
                         int32_t *slot_block, int32_t *counters, void *stream);
int mh_tsdf_sparse_integrate(const float *depth, const uint8_t *rgb, const uint8_t *mask, int32_t H, int32_t W, float fx, float fy,
                             float cx, float cy, const float *w2c_host, float depth_scale, float depth_trunc, float ox, float oy,
                             float oz, float voxel_length, float sdf_trunc, int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity,
                             const int32_t *slot_block, const int32_t *counters, float *tsdf, float *weight, float *color,
                             void *stream);
int mh_tsdf_sparse_to_dense(int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity, const int32_t *slot_block,
                            const int32_t *counters, const float *pool_tsdf, const float *pool_weight, const float *pool_color,
                            float *tsdf, float *weight, float *color, uint8_t *active, void *stream);
int mh_tsdf_sparse_from_dense(const float *tsdf, const float *weight, const float *color, const uint8_t *keep, const int32_t *order,
                              int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity, int32_t *slot, int32_t *slot_block,
                              int32_t *counters, float *pool_tsdf, float *pool_weight, float *pool_color, void *stream);
int64_t mh_mc_sparse_workspace_bytes(int32_t capacity);
int mh_mc_count_sparse(const float *pool_tsdf, const float *pool_weight, const int32_t *slot, const int32_t *sorted_blocks,
                       const int32_t *counters, int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity, float iso, void *workspace,
                       int64_t *counts, void *stream);
int mh_mc_emit_sparse(const float *pool_tsdf, const float *pool_weight, const int32_t *slot, const int32_t *sorted_blocks,
                      const int32_t *counters, int32_t nbx, int32_t nby, int32_t nbz, int32_t capacity, float iso, void *workspace,
                      float *vertices, int32_t *triangles, void *stream);
int mh_tsdf_sparse_vertex_colors(const float *vertices, int64_t V, const float *pool_color, const int32_t *slot, int32_t nbx,
                                 int32_t nby, int32_t nbz, int32_t capacity, float *out, void *stream);

/* ---- frequency and spherical-harmonics encoders (csrc/encoders.hip) ---------------------------
 * The reference's other two native encoders.  No entry point synchronises with the host; B == 0 returns MH_OK without a launch;
 * a null pointer with B > 0 or an argument outside the stated range returns MH_ERR_ARG before any device call.  Buffers that are
 * 16-byte aligned are moved 16 bytes a lane; others are served by the same kernels a dword at a time, with the same results.
 *
 * mh_freq_encode_fwd: x [B,D] -> out [B,C], C = D + 2 D degree; 1 <= D <= 8, 0 <= degree <= 16, 0 <= n_keep <= degree.
 *   columns [0, D): x, copied bit for bit; then for band f = 0 .. degree-1 a block of D sines and a block of D cosines of
 *   2^f x[d] (freqencoder.cu:28-58; FreqEncoder_torch's layout, encodings.py:42-55).  The blocks of the bands f >= n_keep are
 *   written as +0.0: the progressive max_level of FreqEncoder_torch, which the reference's CUDA kernel does not have.
 *   The argument is ldexpf(x, f), exact, and sine and cosine both come from that one argument (sincosf).  The reference takes the
 *   cosine as __sinf(arg + pi/2): the addition throws away up to half an ulp of an argument as large as 2^(degree-1) |x|, an error
 *   of that size in the result, and __sinf is the fast approximation.  Neither is reproduced here.
 * mh_freq_encode_bwd: grad [B,C] -> grad_x [B,D], WRITTEN (not accumulated):
 *   grad_x[d] = grad[d] + sum_{f < n_keep} 2^f (g_sin[f,d] cos(2^f x[d]) - g_cos[f,d] sin(2^f x[d]))        (freqencoder.cu:63-94)
 *   with sine and cosine recomputed from x as in the forward (the forward's output is not an operand: nothing of B C floats is
 *   kept alive for the backward).  Order: the sum starts from grad[d]; bands ascending; per band two rounded products, their
 *   rounded difference, the exact scaling by 2^f, one rounded addition.
 *
 * mh_sh_encode_fwd: x [B,3] -> out [B, degree^2], 1 <= degree <= 8.  Column c = l^2 + l + m (0 <= l < degree, -l <= m <= l) holds the
 *   real spherical harmonic in the reference's convention (shencoder.cu:50-120): polynomials in (x, y, z) with x^2 + y^2 + z^2 = 1
 *   already substituted, evaluated as they stand for ANY input -- nothing is normalised:
 *     m = 0:  K(l,0) P_l(z)
 *     m > 0:  (-1)^m sqrt(2) K(l,m)   T(l,m)(z)   Re (x + iy)^m
 *     m < 0:  (-1)^m sqrt(2) K(l,|m|) T(l,|m|)(z) Im (x + iy)^|m|
 *   K(l,m) = sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!), T(l,m) = d^m P_l / dz^m, P_l the Legendre polynomial.  The evaluation is the
 *   straight-line fp32 program of csrc/sh_table.inc (generated by tools/make_sh_table.py from this definition; every operator
 *   rounded on its own, one fixed order), so the result is that program's, bit for bit.
 * mh_sh_encode_bwd: grad [B, degree^2] -> grad_x [B,3], WRITTEN: grad_x[a] = sum_c grad[c] dY_c/dx_a, the derivative polynomials
 *   evaluated by the same program (the reference stores dy_dx [B, 3 degree^2] in the forward and reads it back,
 *   sphere_harmonics.py:27-34; here nothing is stored).  Order: each sum starts at +0; columns ascending; the product
 *   grad[c] (dY_c/dx_a) is rounded, then added to the running sum.  A derivative that is identically zero (d/dx and d/dy of the
 *   m = 0 columns, d/dy of m = 1, d/dx of m = -1, d/dz of |m| = l) contributes no term. */
int mh_freq_encode_fwd(const float *x, int64_t B, int32_t D, int32_t degree, int32_t n_keep, float *out, void *stream);
int mh_freq_encode_bwd(const float *x, const float *grad, int64_t B, int32_t D, int32_t degree, int32_t n_keep, float *grad_x,
                       void *stream);
int mh_sh_encode_fwd(const float *x, int64_t B, int32_t degree, float *out, void *stream);
int mh_sh_encode_bwd(const float *x, const float *grad, int64_t B, int32_t degree, float *grad_x, void *stream);

/* ---- nerfacc's volume-rendering functions (csrc/volrend.hip; morpheus_amd/volrend.py is their Python face) ---------------
 * render_transmittance / render_weight _from_density / _from_alpha, accumulate_along_rays and pack_info of nerfacc 0.5.x under
 * their own names, forward and backward.  nerfacc is third-party, un-vendored and not installed where this library is built: the
 * definitions are restated as recalled and are NOT verified against it (tools/check_against_nerfacc.py compares on a machine
 * that has it).  mh_composite_* above stays the fused form of the shipped render loop; these are its parts.  Purely additive:
 * MH_ABI_VERSION is unchanged (the precedent is mh_subdiv_*).
 * Samples of ray r are [ray_start[r], ray_start[r] + ray_cnt[r]) of the packed arrays, ordered by t; x_i = sigma_i (te_i - ts_i).
 *   density form (alpha_form = 0): alpha_i = -expm1f(-x_i);  T_i = expf(-sum_{j<i} x_j)
 *   alpha form   (alpha_form = 1): alpha_i = values_i, taken as <= 1;  T_i = prod_{j<i} (1 - alpha_j); t_starts / t_ends may be NULL
 *   both: w_i = T_i alpha_i.  One wavefront per ray, 64-sample chunks, a wave scan and a scalar carry; the exclusive sum takes
 *   the lane below instead of subtracting the sample's own term where x_i >= 1 (the compositor's rule), the exclusive product
 *   always does.  sigma = +inf: the sample takes the remaining transmittance, exact zeros behind it; a NaN stays in its ray.
 * mh_pack_info: ray_indices int32 or int64 [M], NON-DECREASING (not checked) -> ray_start, ray_cnt int32 [N], for every ray,
 *   the rays no sample names included (count 0); a bisection per ray, one launch, no host synchronisation; indices outside
 *   [0, N) belong to no ray; every read is inside [0, M).  M < 2^31.
 * mh_ray_weights_fwd: writes weights, trans, alphas [M], each of which may be NULL (not all three).
 * mh_ray_weights_bwd: g_weights, g_trans, g_alphas [M] may each be NULL (= zeros; g_alphas must be NULL in alpha form);
 *   writes d_values [M] = dL/dsigma or dL/dalpha for every sample a ray owns.
 *   density: dL/dx_i = (g_w_i T_i + g_a_i)(1 - alpha_i) - sum_{j>i} (g_w_j w_j + g_T_j T_j), d_sigma_i = (te_i - ts_i) dL/dx_i;
 *            one reverse pass that READS `trans`, the forward's output (required).
 *   alpha:   dL/dalpha_i = g_w_i T_i - sum_{j>i} (g_w_j alpha_j + g_T_j) prod_{k<j, k != i} (1 - alpha_k) -- the product with
 *            factor i left out, never T_j / (1 - alpha_i): finite and correct at alpha_i = 1.  A forward pass parks the product
 *            of the non-zero factors and the count of zero factors in d_values, a reverse pass forms one suffix sum per count;
 *            `trans` is not read and may be NULL.
 * mh_accumulate_fwd: out [N, D] = sum_{i in ray} weights_i values[i, :], values [M, D], 1 <= D <= 256; values NULL = a column
 *   of ones (D must be 1).  A ray without samples writes exact zeros; no atomics: a ray's sums do not depend on other rays.
 *   D <= 4: a lane per sample, sums in registers; larger D: the power of two >= D (at most 64) lanes per sample.
 * mh_accumulate_bwd: g_out [N, D] -> d_weights [M] = sum_c g_out[ray, c] values[i, c] (values NULL: g_out[ray, 0]) and
 *   d_values [M, D] = weights_i g_out[ray, :]; either may be NULL (not both); d_values needs values and weights.
 * Bad arguments (a NULL required pointer, N < 0, D outside 1 .. 256) return MH_ERR_ARG before any launch; N == 0 returns MH_OK
 * without one. */
int mh_pack_info(const void *ray_indices, int32_t idx_is_i64, int64_t M, int32_t N, int32_t *ray_start, int32_t *ray_cnt,
                 void *stream);
int mh_ray_weights_fwd(const float *values, const float *t_starts, const float *t_ends, int32_t alpha_form,
                       const int32_t *ray_start, const int32_t *ray_cnt, int32_t N, float *weights, float *trans, float *alphas,
                       void *stream);
int mh_ray_weights_bwd(const float *values, const float *t_starts, const float *t_ends, int32_t alpha_form,
                       const int32_t *ray_start, const int32_t *ray_cnt, int32_t N, const float *trans, const float *g_weights,
                       const float *g_trans, const float *g_alphas, float *d_values, void *stream);
int mh_accumulate_fwd(const float *weights, const float *values, int32_t D, const int32_t *ray_start, const int32_t *ray_cnt,
                      int32_t N, float *out, void *stream);
int mh_accumulate_bwd(const float *weights, const float *values, int32_t D, const int32_t *ray_start, const int32_t *ray_cnt,
                      int32_t N, const float *g_out, float *d_weights, float *d_values, void *stream);

/* ---- device-resident dataset (csrc/dataset.hip; morpheus_amd/dataset.py is its Python face) -------------------------------
 * Stands where the reference's datasets/dataset.py:DeformDataset stands.  Frames stay on the device in their file precision:
 * rgb uint8 [F,H,W,3], depth uint16 (depth_is_f32 = 0) or fp32 (1) [F,H,W], mask uint8 [F,H,W]; poses fp32 [F,4,4] row-major;
 * theta, phi, radius fp32 [F].  Purely additive: MH_ABI_VERSION is unchanged.
 * mh_dataset_sample: ONE launch per real-view batch (dataset.py:398-433).  frame_idx int64 [B], pix int32 [N] (NULL: the whole
 *   frame, pixel n = n, N <= H W).  Ray (b, n) looks through pixel pix[n] of frame frame_idx[b], both CLAMPED into their
 *   ranges -- no read leaves the tables whatever the arrays hold:
 *     rays_o, rays_d [B,N,3]   the arithmetic of mh_generate_rays on the frame's device pose, the same bits
 *     rays_t [B,N]             (float)f / (float)F;      rays_id int64 [B,N] = f
 *     image [B,3,N]            (float)((double)u8 / 255.0)
 *     depth_out [B,N]          (float)((double)raw / depth_scale)
 *     mask_out int64 [B,N]     1 where the byte is 255, else 0 (`/ 255.0`, then the truncation of `.to(int64)`)
 *     pose_out [B,4,4], theta_out, phi_out, radius_out [B]   the frame's row of each table
 * mh_generate_rays_dev: rays of B DEVICE poses [B,4,4]: rays_o, rays_d [B,N,3] with the arithmetic of mh_generate_rays; pix
 *   int32 [N] is shared by the poses and clamped (NULL: the whole image).  With frame_idx int64 [B] (clamped into [0, F)) it
 *   also writes rays_t [B,N] = (float)f / (float)F and rays_id int64 [B,N] = f; either may be NULL.
 * mh_dataset_virtual_pose: B virtual views (dataset.py:435-501, 268-330, 559-563) of the frames frame_idx (clamped).  mode:
 *     0  a, b = theta, phi in radians, fp32 (the theta/phi box; phi < 0 is moved up by 2 pi, as the reference does)
 *     1  a, b, c = the three normal draws of the uniform-sphere branch
 *     2  a, b = theta, phi in DEGREES (is_train = False, get_c2w_from_polar); radians = deg / 180 * pi in fp32
 *   radius = radius[f] * radius_factor in fp32.  The pose rule: the look-at chain (sin / cos or normalize, two
 *   normalised cross products, safe_normalize with its 1e-20 clamp) is evaluated in DOUBLE from those fp32 inputs and rounded
 *   to fp32 once -- not the bits of the reference's fp32 chain (torch's CPU sin is another program), judged against float64.
 *   In mode 1 the fp32 angles restate the reference's fp32 chain: norm = sqrt(fma(z, z, fma(y, y, x * x))), unit = v /
 *   max(norm, 1e-12), phi = the C library's atan2f (fdlibm) plus 2 pi where negative, theta = the double acos(unit_y) rounded once
 *   (the reference's CPU acos, a vendor vector routine, is within one fp32 step of it and equal in about 92 % of draws).
 *   Bit for bit the reference's, given the fp32 angles: dir_out int64 [B], the six-way label of datasets/utils.py:70-91
 *   (phi % 2 pi and the six thresholds compared at fp32: front_half = front / 2, back_lo = pi - front / 2, left_lo = pi +
 *   front / 2, wrap_lo = 2 pi - front / 2, overhead, bottom = pi - overhead, each rounded from the caller's float64 value);
 *   deg_out [B,2] = (theta, phi) / pi * 180; polar_out = theta_deg - theta[f]; azimuth_out = phi_deg - phi[f], minus 360 where
 *   it exceeds 180; dradius_out = radius - radius[f].  pose_out [B,4,4].
 * Bad arguments return MH_ERR_ARG before any launch; B == 0 or N == 0 returns MH_OK without one. */
int mh_dataset_sample(float fx, float fy, float cx, float cy, const float *poses, const uint8_t *rgb, const void *depth,
                      int32_t depth_is_f32, double depth_scale, const uint8_t *mask, const float *theta, const float *phi,
                      const float *radius, int32_t F, int32_t H, int32_t W, const int64_t *frame_idx, int32_t B,
                      const int32_t *pix, int32_t N, float *rays_o, float *rays_d, float *rays_t, int64_t *rays_id, float *image,
                      float *depth_out, int64_t *mask_out, float *pose_out, float *theta_out, float *phi_out, float *radius_out,
                      void *stream);
int mh_generate_rays_dev(float fx, float fy, float cx, float cy, const float *poses, int32_t B, int32_t H, int32_t W,
                         const int32_t *pix, int32_t N, const int64_t *frame_idx, int32_t F, float *rays_o, float *rays_d,
                         float *rays_t, int64_t *rays_id, void *stream);
int mh_dataset_virtual_pose(int32_t mode, const float *a, const float *b, const float *c, const int64_t *frame_idx, int32_t B,
                            const float *radius, const float *theta, const float *phi, int32_t F, float radius_factor,
                            float front_half, float back_lo, float left_lo, float wrap_lo, float overhead, float bottom,
                            float *pose_out, int64_t *dir_out, float *polar_out, float *azimuth_out, float *dradius_out,
                            float *deg_out, void *stream);

/* ---- preprocessing of a raw RGB-D sequence (csrc/preprocess.hip; morpheus_amd/preprocess.py is its Python face) -----------
 * Stands where the reference's preprocess/preprocess.py:DataProcessor.rotate_and_crop_frames and its four imwrite lines stand.
 * Purely additive: MH_ABI_VERSION is unchanged (the precedents are mh_subdiv_*, volrend and dataset).
 * mh_prep_frames: ALL frames of a sequence in one launch.  In: rgb uint8 [F,H,W,3], depth uint16 [F,H,W] (raw), mask uint8
 *   [F,H,W]; origin int32 [F,2] = (top, left) of each frame's window; inv_affine float64 [F,6], the inverse affine map of each
 *   frame, formed on the host; rotated uint8 [F], 0 = the frame is not rotated (inv_affine of that frame is not read);
 *   table_inside, table_padded uint16 [65536].  Out, DeviceDataset's storage layout: rgb_out uint8 [F,h,w,3], depth_out uint16
 *   [F,h,w], mask_out uint8 [F,h,w], padding_out uint8 [F,h,w].
 *   Window: output pixel (y, x) of frame f looks at canvas pixel (Y, X) = (top + y, left + x) (64-bit sums).  Outside [0,H) x
 *   [0,W): rgb, depth and mask 0, padding 255; inside: padding 0.  This holds for EVERY position of the window.  The reference
 *   raises a numpy shape error for a window that crosses two different sides of the frame, one wholly outside the frame and one
 *   larger than the frame; this build defines those three kinds by the same rule.
 *   Depth: depth_out = table_inside[raw] when the frame's window passes the reference's inside test, top >= 0 && left >= 0 &&
 *   top + h < H && left + w < W (strict: touching the bottom or right edge is not inside), else table_padded[raw].  The caller
 *   tabulates the reference's two write expressions (fp32 and float64 products; morpheus_amd.preprocess.depth_tables).
 *   Unrotated frames: rgb and mask bytes are copied.
 *   Rotated frames: this build's own definition, agreement with cv2 unverified (cv2.warpAffine's fixed-point coordinates are not
 *   restated).  With a = inv_affine[f], canvas (X, Y) samples the source at u = (a0 X + a1 Y) + a2, v = (a3 X + a4 Y) + a5 in
 *   float64 without contraction.  depth, mask: nearest, column floor(u + 0.5), row floor(v + 0.5), 0 outside the image (raw 0 ->
 *   table[0]).  rgb: bilinear on byte / 255.0 in float64, taps outside the image 0, fu = floor(u), ax = u - fu (v alike),
 *   val = ((p00 (1-ax)(1-ay) + p01 ax (1-ay)) + p10 (1-ax) ay) + p11 ax ay, byte = (uint8)(val * 255.0), a truncation.
 *   tests/preprocess_oracle.py states the same order; equal bit for bit.
 *   One lane writes 4 consecutive pixels of the flat output as whole dwords: the four outputs must be 4-byte aligned (depth_out
 *   8), F h w < 2^31, H W < 2^31.  Every read is inside the frames and the tables whatever origin and inv_affine hold.
 * Bad sizes, null pointers or misaligned outputs return MH_ERR_ARG before any launch; F == 0 returns MH_OK without one. */
int mh_prep_frames(const uint8_t *rgb, const uint16_t *depth, const uint8_t *mask, int32_t F, int32_t H, int32_t W,
                   const int32_t *origin, const double *inv_affine, const uint8_t *rotated, const uint16_t *table_inside,
                   const uint16_t *table_padded, int32_t h, int32_t w, uint8_t *rgb_out, uint16_t *depth_out, uint8_t *mask_out,
                   uint8_t *padding_out, void *stream);

/* ---- occupancy estimator in full (csrc/estimator.hip; morpheus_amd/estimator.py:OccGridEstimator is its Python face) -------
 * Stands where nerfacc 0.5.x's OccGridEstimator stands for a render loop written against it: names, buffers and the update rule
 * are RECALLED from its public source, agreement unverified; the interval placement is this build's definition.
 * Purely additive: MH_ABI_VERSION is unchanged.  tests/estimator_oracle.py restates every rule below in fp32, one rounding per
 * operation; the kernels are compiled without contraction and equal it bit for bit.
 * Grid: L levels (1 .. 16) of Rx x Ry x Rz cells, L Rx Ry Rz < 2^31; aabbs fp32 [L,6] (lo xyz, hi xyz) on the DEVICE, level L - 1
 * the coarsest; binary uint8 [L,Rx,Ry,Rz]; occs fp32 [L * cells], cells = Rx Ry Rz, cell index (i Ry + j) Rz + k.
 *
 * mh_est_march_slots: mh_march_slots (same slot rows, counts and overflow flag; mh_march_pack packs them) with
 *   - the clip against the coarsest level's box, (lo - o) / d and (hi - o) / d per axis, and the MISS rule decided on it alone;
 *   - then t_near = near_plane if near_plane > t_near, then t_min[r] alike; t_far = far_plane if far_plane < t_far, then
 *     t_max[r] alike (t_min / t_max fp32 [N] or NULL; a NaN never passes a comparison and is ignored);
 *   - t0 = t_near + u * step; cone_angle == 0: ts_k = t0 + k * step, te_k = min(ts_k + step, t_far); cone_angle > 0:
 *     ts_0 = t0, dt_k = min(max(ts_k * cone_angle, step), 1e10f), te_k = min(ts_k + dt_k, t_far), ts_{k+1} = ts_k + dt_k;
 *     kept while ts_k < t_far;
 *   - a step is a sample iff the cell of its midpoint is occupied in the finest level whose box holds the midpoint (lo <= x <
 *     hi on the three axes; none: the coarsest); cell = clamp(floor((x - lo) / (hi - lo) * R), 0, R - 1).
 *   mh_est_march_cap, given the diagonal of the coarsest box, = (int)(min(diagonal, far_plane - near_plane) / step) + 4,
 *   0 for bad arguments: the slot row a ray of unit-or-longer direction cannot overflow (every step is >= `step` long).
 *
 * mh_est_traverse_slots: the second, opt-in placement (OccGridEstimator(traversal = "dda")): the grid is walked cell by cell, an
 *   empty cell is jumped to its exit and stepping starts again where the next occupied cell is entered.  Same arguments, argument
 *   rules, slot rows, counts and overflow flag as mh_est_march_slots; mh_march_pack packs the rows.  This is this build's statement
 *   of nerfacc 0.5.x's traverse_grids as RECALLED, agreement unverified, with the one departure named in point 5.  fp32, one
 *   IEEE rounding per operation, no contraction; tests/traverse_oracle.py restates it and the kernel equals that bit for bit.
 *   1. Clip, miss rule, planes, per-ray limits: slab_clip against the coarsest box, the first two points of mh_est_march_slots.
 *      Then t_near = t_near + u * step: the jitter shifts the near end only; later runs start at cell entries, unjittered.
 *   2. Level segments.  For every finer level l, coarse to fine: (a_l, b_l) = slab_clip(o, d, box_l), then
 *      a_l = min(max(a_l, a_{l+1}), b_{l+1}) and b_l = max(min(b_l, b_{l+1}), a_l); a level that is a miss has a_l = b_l =
 *      b_{l+1}; a_{L-1}, b_{L-1} = t_near, t_far.  The ray is the segments [a_{L-1}, a_{L-2}] at level L - 1, ..., [a_0, b_0] at
 *      level 0, [b_0, b_1] at level 1, ..., [b_{L-2}, b_{L-1}] at level L - 1; a segment with e <= s is skipped.
 *   3. Cell spans of a segment [s, e] at level l.  Start cell c_a = clamp(floor(((o_a + d_a s) - lo_a) / (hi_a - lo_a) * R_a), 0,
 *      R_a - 1).  Plane k of axis a = lo_a + ((float)k / (float)R_a) * (hi_a - lo_a): closed form from the integer index, never an
 *      accumulated increment.  Exit of the current cell on axis a = (plane(c_a + (d_a > 0)) - o_a) / d_a, +inf when d_a == 0.  The
 *      span ends at x = max(min(min(min(exit_x, exit_y), exit_z), e), start).  x >= e: the segment is done.  Otherwise the first
 *      axis (x, y, z order) whose exit is the minimum is stepped; an index outside [0, R_a - 1] ends the segment.  A segment has
 *      at most Rx + Ry + Rz + 3 spans: the walk is bounded by that count, not by a comparison of times alone.
 *   4. Runs.  A span with end <= start is ignored: it neither extends nor breaks a run.  A run is a maximal sequence of
 *      consecutive occupied spans (binary[l, c] != 0), across segment and level changes, from the first span's start A to the
 *      last span's end B.
 *   5. Samples of a run start at A' = max(A, te of the last sample of this ray).  cone_angle == 0: ts_k = A' + (float)k * step,
 *      te_k = A' + (float)(k + 1) * step (te_k and ts_{k+1} are the same bits).  cone_angle > 0: ts_0 = A', dt_k = min(max(ts_k *
 *      cone_angle, step), 1e10f), te_k = ts_k + dt_k, ts_{k+1} = te_k.  A sample is kept while (ts_k + te_k) / 2.0f < B.  te is NOT
 *      clamped to B or t_far: a run's last sample may reach up to half a step past its end.
 *      max(A, last te) is a deliberate departure from the recalled rule, which restarts at the cell entry A: behind an empty gap
 *      shorter than half a step that rule lets two samples overlap, and mh_sample_pdf / mh_resample_packed and the compositor
 *      assume t_starts[k] >= t_ends[k-1] inside a ray.
 *   Slot row: every sample is at least `step` long, the samples are disjoint and every ts lies in [t_near, t_far), so
 *   mh_est_march_cap bounds the row exactly as it does for the lattice; ray_cnt = min(n, cap), nothing is written past cap and
 *   the flag is set when a ray has more than cap samples.
 * The update, no device->host read:
 *   mh_est_occ_count / mh_est_occ_pack: one wavefront per chunk of mh_est_occ_chunk cells; chunk_cnt int32 [L, n_chunks],
 *     n_chunks = ceil(cells / chunk).  The caller scans each level's row into chunk_start (exclusive); pack writes the occupied
 *     cells of level l, in index order, to occ_list [l * cells ...).
 *   mh_est_select: ids int32 [L,n] and points fp32 [L,n,3] in one launch.  warmup != 0: n = cells, entry i is cell i.  Else
 *     n = 2 k, k = cells / 4: entry i < k is uniform[l,i] (int32 [L,k]); entry k + j, with c = occ_cnt[l]: c > k -> the
 *     min((int)(u_occ[l,j] * (float)c), c - 1)-th occupied cell, else the j-th while j < c and padding (-1) behind.
 *     point = lo + ((ijk + u_point[l,i,:]) / R) * (hi - lo); padding gets cell 0's point.
 *   mh_est_ema: occs[cell] = max over the entries naming it of max(old * decay, occ > 0 ? occ : 0) -- a reset pass, then an
 *     integer atomic max; padding and cells with old < 0 (invisible) are skipped.  old_occs: the caller's copy of occs.
 *   mh_est_threshold: *thre = mean < cap ? mean : cap, mean = the float64 sum of occs[occs >= 0] over their count, summed in a
 *     fixed order and rounded to fp32 once (no such cell: cap); binaries (may be NULL) = occs > *thre.  partials: float64
 *     [2 * mh_est_max_partials] scratch.
 * mh_est_mark_invisible: K fp32 [C,3,3], c2w fp32 [C,3,4] (OpenCV convention).  Cell point x = lo + ijk / (R - 1) * (hi - lo);
 *   x_c = R^T x - R^T t; uvd = K x_c (sums of three products are (p0 + p1) + p2); in the image iff d >= 0, 0 <= u / d < width,
 *   0 <= v / d < height.  occs = 0 where some camera has the cell in the image with d >= near_plane and none has it in the image
 *   with d < near_plane, -1 elsewhere.
 * Bad arguments return MH_ERR_ARG before any launch. */
int32_t mh_est_occ_chunk(void);
int32_t mh_est_max_partials(void);
int32_t mh_est_march_cap(float step, float diagonal, float near_plane, float far_plane);
int mh_est_march_slots(const float *rays_o, const float *rays_d, const float *jitter, const float *t_min, const float *t_max,
                       int32_t N, float step, float cone_angle, float near_plane, float far_plane, const float *aabbs,
                       int32_t L, int32_t Rx, int32_t Ry, int32_t Rz, const uint8_t *binary, int32_t cap, int32_t *ray_cnt,
                       float *slot_ts, float *slot_te, int32_t *overflow, void *stream);
int mh_est_traverse_slots(const float *rays_o, const float *rays_d, const float *jitter, const float *t_min, const float *t_max,
                          int32_t N, float step, float cone_angle, float near_plane, float far_plane, const float *aabbs,
                          int32_t L, int32_t Rx, int32_t Ry, int32_t Rz, const uint8_t *binary, int32_t cap, int32_t *ray_cnt,
                          float *slot_ts, float *slot_te, int32_t *overflow, void *stream);
int mh_est_occ_count(const uint8_t *binary, int32_t L, int64_t cells, int32_t *chunk_cnt, void *stream);
int mh_est_occ_pack(const uint8_t *binary, int32_t L, int64_t cells, const int32_t *chunk_start, int32_t *occ_list,
                    void *stream);
int mh_est_select(int32_t warmup, int32_t L, int32_t Rx, int32_t Ry, int32_t Rz, int64_t n, const int32_t *uniform,
                  const float *u_occ, const float *u_point, const int32_t *occ_list, const int32_t *occ_cnt,
                  const float *aabbs, int32_t *ids, float *points, void *stream);
int mh_est_ema(const int32_t *ids, const float *occ, int32_t L, int64_t n, int64_t cells, const float *old_occs, float decay,
               float *occs, void *stream);
int mh_est_threshold(const float *occs, int64_t n, float cap, double *partials, float *thre, uint8_t *binaries, void *stream);
int mh_est_mark_invisible(const float *K, const float *c2w, int32_t C, float width, float height, float near_plane,
                          const float *aabbs, int32_t L, int32_t Rx, int32_t Ry, int32_t Rz, float *occs, void *stream);

/* ---- importance resampling (csrc/resample.hip; morpheus_amd/resample.py is its Python face) -------------------------------
 * Purely additive: MH_ABI_VERSION is unchanged.  One wavefront per ray; csrc/resample.hip's header states every operation, how
 * the searched CDF is kept non-decreasing and why the cut is a merge by rank; tests/resample_oracle.py restates it.
 * mh_sample_pdf: the reference's utils.sample_pdf (utils.py:10-44), dense: bins fp32 [B,T], weights fp32 [B,T-1], u fp32 [B,n]
 *   -> samples fp32 [B,n] in the order of u.  T >= 2, n >= 1.  scratch: fp32 [B*T], read and written only when
 *   T - 1 > mh_resample_stage() (may be NULL otherwise).
 * mh_resample_packed: packed ragged samples (ray_start, ray_cnt int32 [N]; t_starts, t_ends, weights fp32 [M]; ranges are
 *   clipped to [0, M)).  A ray with c >= 1 intervals draws n points from the piecewise-constant pdf (w_i + eps) / sum over its c
 *   intervals (gaps between intervals carry none) at u_k = ((float)k + j_k) / (float)n, jitter j fp32 [N,n] in [0,1), NULL:
 *   j_k = 0.5; every draw lies inside its interval [ts_i, te_i]; u at or above the last CDF value is the last interval's end.
 *   Output: the coarse intervals cut at the draws -- c + n intervals in order from new_start[r], every coarse ts / te unchanged,
 *   a cut point the same bits as the end of one interval and the start of the next, zero-width intervals where draws coincide
 *   with an edge or each other; out_ray_idx = r.  A ray without samples writes nothing.  xyz (NULL: skipped) fp32 [M_out,3] =
 *   rays_o[r] + rays_d[r] * ((ts + te) / 2) for EVERY entry of the output arrays, read through out_ray_idx.
 *   Writes past M_out are suppressed.  scratch_cdf fp32 [M + N] and scratch_cnt int32 [M] stage the rays longer than
 *   mh_resample_stage() intervals and are required when M exceeds it.
 * mh_resample_ranges: new_cnt[r] = c_r + n (0 for an empty ray), new_start = its exclusive scan, *total = its sum, all held to
 *   `limit` (start <= limit, start + cnt <= limit).  One launch, no host read.
 * Two forms, as for the marcher: ragged -- the host reads *total once and sizes the outputs by it; fixed capacity -- the outputs
 *   have length M + n N (M the input capacity), *total is n_valid and stays on the device, the caller zeroes the outputs (ray 0,
 *   t = 0: the marcher's padding), nothing is synchronised and the calls may be captured in a graph.
 * Bad arguments return MH_ERR_ARG before any launch; N == 0, M == 0 or M_out == 0 launch nothing. */
int32_t mh_resample_stage(void);
int mh_sample_pdf(const float *bins, const float *weights, const float *u, int32_t B, int32_t T, int32_t n, float *scratch,
                  float *samples, void *stream);
int mh_resample_ranges(const int32_t *ray_start, const int32_t *ray_cnt, int32_t N, int64_t M, int32_t n, int64_t limit,
                       int32_t *new_start, int32_t *new_cnt, int32_t *total, void *stream);
int mh_resample_packed(const float *weights, const float *t_starts, const float *t_ends, const int32_t *ray_start,
                       const int32_t *ray_cnt, const int32_t *new_start, int32_t N, int64_t M, int32_t n, const float *jitter,
                       float eps, float *scratch_cdf, int32_t *scratch_cnt, int64_t M_out, const float *rays_o,
                       const float *rays_d, int32_t *out_ray_idx, float *out_t_starts, float *out_t_ends, float *xyz,
                       void *stream);

/* ---- image resampling (csrc/imageops.hip; morpheus_amd/imageops.py is its Python face) ---------------------------------------
 * Purely additive: MH_ABI_VERSION is unchanged.  csrc/imageops.hip's header states every operation; tests/imageops_oracle.py
 * restates it.
 * mh_resize_bilinear_fwd: x fp32, B images of C <= 4 channels at Hi x Wi, [B,Hi,Wi,C] (nhwc != 0) or [B,C,Hi,Wi] -> y fp32
 *   [B,C,Ho,Wo] = mul * bilinear(x) + add, PyTorch's upsample_bilinear2d with align_corners=False and no scale factor.
 * mh_resize_bilinear_bwd: gy fp32 [B,C,Ho,Wo] -> gx fp32 in x's layout = mul * (the adjoint of the interpolation applied to gy),
 *   every element written; a gather in a fixed order without atomics: the same bits on every run.
 * mh_resize_area_masked: image [Hi,Wi,3] fp32 in [0,1] or uint8 (image_u8 != 0: value / 255), mask fp32 [Hi,Wi] or NULL (all
 *   kept) -> out fp32 [3,Ho,Wo]: img * m + (1 - m), m = mask > 0.5, averaged over each output pixel's source box with the exact
 *   fractional overlaps.  Ho <= Hi and Wo <= Wi; an enlarging axis is MH_ERR_ARG.
 * mh_frame_to_u8: out[i] = (uint8) of x[i] * 255 held to [0, 255] (NaN: 0), truncated.
 * mh_depth_to_u8: out[i] = (uint8) of (d[i] - min) / (max - min + 1e-6f) * 255, min / max over the n values found on the device
 *   (two launches, no host read; NaN-free input); range: int32 scratch of mh_depth_range_words words. */
int mh_resize_bilinear_fwd(const float *x, int32_t B, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t nhwc,
                           float mul, float add, float *y, void *stream);
int mh_resize_bilinear_bwd(const float *gy, int32_t B, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t nhwc,
                           float mul, float *gx, void *stream);
int mh_resize_area_masked(const void *image, int32_t image_u8, const float *mask, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                          float *out, void *stream);
int mh_frame_to_u8(const float *x, int64_t n, uint8_t *out, void *stream);
int32_t mh_depth_range_words(void);
int mh_depth_to_u8(const float *depth, int64_t n, int32_t *range, uint8_t *out, void *stream);

/* ---- the Zero-1-to-3 guidance shell (csrc/guidance.hip; morpheus_amd/guidance.py is its Python face) -------------------------
 * Purely additive: MH_ABI_VERSION is unchanged.  What zero123_utils.py:Zero123.train_step does around its networks; the file's
 * header states every operation, tests/guidance_oracle.py restates it.  Every entry point is one launch; nothing is read back.
 * mh_sds_view: the view deltas polar / azimuth (degrees) and radius fp32 [B] against R <= mh_sds_max_refs reference views
 *   (ref_polars, ref_azimuths, ref_radii, user_ws fp32 [R]) -> T fp32 [R,B,4], angles fp32 [B,R] (degrees), scale fp32 [B],
 *   ws fp32 [B,R].
 * mh_sds_view_bank: the same with R = 1 against a bank of K keyframes (kf_index int64 [K], the four fp32 [K] arrays): the keyframe
 *   nearest to frame_id[0] (int64, device; the lowest index on a tie), or with target != 0 keyframe 0 with the view re-expressed
 *   relative to it; chosen int64 [1] = the keyframe's index in the bank.
 * mh_sds_angles: v1 fp32 [N1,3], v2 fp32 [N2,3] rows [r, theta, phi] in radians -> out fp32 [N1,N2], the angle in radians.
 * mh_sds_noise: latents, noise fp32 [B,n], t int64 [B], alphas_cumprod fp32 [T] -> x_in fp32 [2B,n]:
 *   sqrt(a_t) latents + sqrt(1 - a_t) noise in both halves.  t outside [0, T) is held to the table's ends.
 * mh_sds_grad: noise_preds fp32 [R,2B,n] (unconditional half first), ws fp32 [B,R], noise fp32 [B,n], scale fp32 [B] ->
 *   grad fp32 [B,n] = nan_to_num(scale (1 - a_t) (sum_k w_k (u_k + s (c_k - u_k)) / sum_k w_k - noise)) and loss fp32 [1] =
 *   0.5 sum grad^2 / B, summed in a fixed order.  partials: float64 scratch of mh_sds_grad_blocks values; ticket: uint32 [1],
 *   zero before the first call and left zero by every call. */
int32_t mh_sds_max_refs(void);
int32_t mh_sds_grad_blocks(void);
int mh_sds_view(const float *polar, const float *azimuth, const float *radius, int32_t B, const float *ref_polars,
                const float *ref_azimuths, const float *ref_radii, const float *user_ws, int32_t R, float grad_scale, float *T,
                float *angles, float *scale, float *ws, void *stream);
int mh_sds_view_bank(const float *polar, const float *azimuth, const float *radius, int32_t B, const int64_t *frame_id,
                     const int64_t *kf_index, int32_t K, const float *ref_polars, const float *ref_azimuths,
                     const float *ref_radii, const float *user_ws, int32_t target, float grad_scale, int64_t *chosen, float *T,
                     float *angles, float *scale, float *ws, void *stream);
int mh_sds_angles(const float *v1, int32_t N1, const float *v2, int32_t N2, float *out, void *stream);
int mh_sds_noise(const float *latents, const float *noise, const int64_t *t, const float *alphas_cumprod, int32_t T, int32_t B,
                 int64_t n, float *x_in, void *stream);
int mh_sds_grad(const float *noise_preds, const float *ws, const float *noise, const int64_t *t, const float *alphas_cumprod,
                int32_t T, const float *scale, float guidance_scale, int32_t R, int32_t B, int64_t n, float *grad,
                double *partials, uint32_t *ticket, float *loss, void *stream);

/* ---- video output: baseline JPEG frames (csrc/video.hip; morpheus_amd/video.py is its Python face) ---------------------------
 * Purely additive: MH_ABI_VERSION is unchanged.  csrc/video.hip's header is the definition -- colour transform, sub-sampling,
 * integer DCT, quantiser, scan order, entropy coder, each with its rounding -- and tests/video_oracle.py restates it; the two agree
 * byte for byte.  Integer arithmetic only.
 * mh_jpeg_blocks: the 8 x 8 blocks of one frame of H x W pixels (1 .. 65535) with `channels` = 1 (one component) or 3 (RGB ->
 *   YCbCr, `subsampling` 420 or 444; ignored for one channel); -1 for other arguments or more blocks than a frame's int32 bit
 *   count allows (1 295 225).
 * mh_jpeg_scan_capacity: the proven worst case of one frame's entropy-coded segment in bytes, a multiple of 32: a block is at
 *   most 20 + 63 * 26 = 1658 bits and byte stuffing at most doubles the bytes.  -1 for blocks outside [1, 1 295 225].
 * mh_jpeg_workspace_bytes: the scratch of one mh_jpeg_encode call with per-frame capacity cap; -1 for arguments it would refuse.
 * mh_jpeg_quant_table: table int32 [64] on the HOST, natural order = the Annex K table (chroma: 0 luminance, 1 chrominance)
 *   scaled by the IJG rule for quality 1 .. 100.
 * mh_jpeg_encode: frames uint8 [F,H,W,channels] on the device (4-byte aligned, F <= 65535) -> out uint8 [F,cap]: frame f's
 *   entropy-coded segment, stuffed and 1-padded, in out[f][0 .. nbytes[f]); the markers around it are the caller's.  cap: a
 *   positive multiple of 32, mh_jpeg_scan_capacity(blocks) for a call that cannot overflow.  With a smaller cap every write is
 *   still held inside out[f][0 .. cap) and the workspace, nbytes[f] <= cap, and *overflow (int32, device; cleared by the call)
 *   becomes 1.  workspace: mh_jpeg_workspace_bytes(F, blocks, cap) bytes, 16-byte aligned.  Nine launches, no host read. */
int64_t mh_jpeg_blocks(int32_t H, int32_t W, int32_t channels, int32_t subsampling);
int64_t mh_jpeg_scan_capacity(int64_t blocks);
int64_t mh_jpeg_workspace_bytes(int32_t F, int64_t blocks, int64_t cap);
int mh_jpeg_quant_table(int32_t quality, int32_t chroma, int32_t *table);
int mh_jpeg_encode(const uint8_t *frames, int32_t F, int32_t H, int32_t W, int32_t channels, int32_t subsampling, int32_t quality,
                   void *workspace, uint8_t *out, int64_t cap, int32_t *nbytes, int32_t *overflow, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MORPHEUS_HIP_H */
