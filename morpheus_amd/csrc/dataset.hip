// Device-resident dataset: real-view batches, virtual-view poses and rays from device poses.
//
// Stands where the reference's datasets/dataset.py:DeformDataset stands (morpheus_amd/dataset.py is the Python face).
// The frames stay on the device in their file precision (rgb uint8 [F,H,W,3], depth uint16 or fp32 [F,H,W], mask uint8
// [F,H,W]); no table of rays is built.  Three kernels:
//
//   dataset_sample_kernel     one launch per real-view batch (dataset.py:398-433): thread (b, n) looks through pixel pix[n]
//       of frame frame_idx[b]: the ray from that frame's device pose with pixel_ray (rays.h, the arithmetic of
//       mh_generate_rays: the same bits), rays_t = (float)f / (float)F, rays_id = f, and the gather
//         image = (float)((double)u8 / 255.0)            depth = (float)((double)u16 / depth_scale)
//         mask  = 1 where the byte is 255, else 0        (the reference's `/ 255.0` followed by `.to(int64)`)
//       Thread n == 0 of a batch row also copies the frame's pose, theta, phi and radius.  Frame and pixel indices are
//       CLAMPED to their tables: no read leaves them whatever the index arrays hold.
//   virtual_pose_kernel       one thread per virtual view (dataset.py:435-501, 268-330, 559-563): the look-at pose, the
//       six-way view label (datasets/utils.py:70-91) and the polar / azimuth / radius deltas.
//   generate_rays_dev_kernel  pixel_ray for B device poses: the whole image or a pixel subset, optionally with rays_t / rays_id.
//
// The pose rule.  The look-at chain (sin / cos, the two normalised cross products, safe_normalize with its 1e-20 clamp; in
// the sphere branch F.normalize with its 1e-12 clamp in place of sin / cos) is evaluated in DOUBLE from the fp32 inputs
// (the fp32 radius product, the fp32 angles in radians or the three fp32 normal draws) and rounded to fp32 ONCE.  torch's
// CPU sin and the device's sinf are different programs, so bit equality with the reference's fp32 chain is not on offer;
// the result is judged against float64 instead, with the reference's own fp32 error as the measure.  What follows from the
// fp32 angles by rounded fp32 operators alone IS the reference's, bit for bit: the radians of the is_train=False branch
// (deg / 180 * pi), phis % 2pi and the label thresholds (compared at fp32, the host hands them over rounded from its
// float64 expressions), the degree values (rad / pi * 180), the deltas and the `> 180 -> -360` wrap.
//
// The sphere branch's angles.  There the fp32 angles are not inputs: the reference forms them as F.normalize -> acos / atan2
// in fp32 on the CPU, and the label, degree values and deltas follow from THOSE bits.  So the angles (not the pose) restate
// that fp32 chain, each step as the reference's CPU runs it:
//   norm   sqrt(fma(z, z, fma(y, y, x * x))): torch's reduction accumulates `acc + v * v` contracted to one fma per term;
//   unit   v / max(norm, 1e-12), a rounded fp32 quotient;
//   phi    atan2f of the C library (fdlibm's e_atan2f.c / s_atanf.c, libm_atan2f below), which is what torch's CPU atan2
//          runs on the strided columns of a [B,3] tensor; then `+ 2 pi` at fp32 where negative;
//   theta  the double acos of the fp32 u_y, rounded once to fp32.  The reference's CPU acos is a vendor vector library
//          accurate to one unit in the last place: equal bits in about 92 % of draws (measured over 10^6), one step apart
//          in the rest.  This is the one value of the chain that is not restated; the recorded golden views agree.
// The pose of that branch is still the double chain from the three draws.
#include "common.h"

// the conversions, the ray and the label chains are pinned bit for bit (tests/dataset_oracle.py): no FMA contraction
#pragma clang fp contract(off)

#include "rays.h"

__device__ __forceinline__ int clamp_frame(const int64_t *frame_idx, int b, int F) {
    const int64_t f = frame_idx[b];
    return f < 0 ? 0 : (f > (int64_t)(F - 1) ? F - 1 : (int)f);
}

__global__ __launch_bounds__(256) void dataset_sample_kernel(
    float fx, float fy, float cx, float cy, const float *__restrict__ poses, const uint8_t *__restrict__ rgb,
    const void *__restrict__ depth, int depth_is_f32, double depth_scale, const uint8_t *__restrict__ mask,
    const float *__restrict__ theta, const float *__restrict__ phi, const float *__restrict__ radius, int F, int H, int W,
    const int64_t *__restrict__ frame_idx, int B, const int32_t *__restrict__ pix, int N, float *__restrict__ rays_o,
    float *__restrict__ rays_d, float *__restrict__ rays_t, int64_t *__restrict__ rays_id, float *__restrict__ image,
    float *__restrict__ depth_out, int64_t *__restrict__ mask_out, float *__restrict__ pose_out, float *__restrict__ theta_out,
    float *__restrict__ phi_out, float *__restrict__ radius_out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)B * N) return;
    const int b = (int)(gid / N);
    const int n = (int)(gid - (int64_t)b * N);
    const int f = clamp_frame(frame_idx, b, F);
    const int HW = H * W;
    int p = pix ? pix[n] : n;
    p = p < 0 ? 0 : (p > HW - 1 ? HW - 1 : p);

    const float *c2w = poses + (int64_t)f * 16;
    const Pose pose = pose_from_c2w(c2w);
    float o[3], d[3];
    pixel_ray(fx, fy, cx, cy, pose, W, p, o, d);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        rays_o[gid * 3 + a] = o[a];
        rays_d[gid * 3 + a] = d[a];
    }
    rays_t[gid] = (float)f / (float)F;
    rays_id[gid] = (int64_t)f;

    const int64_t src = (int64_t)f * HW + p;
#pragma unroll
    for (int c = 0; c < 3; c++) image[((int64_t)b * 3 + c) * N + n] = (float)((double)rgb[src * 3 + c] / 255.0);
    const double raw = depth_is_f32 ? (double)reinterpret_cast<const float *>(depth)[src]
                                    : (double)reinterpret_cast<const uint16_t *>(depth)[src];
    depth_out[gid] = (float)(raw / depth_scale);
    mask_out[gid] = mask[src] == 255 ? 1 : 0;

    if (n == 0) {
        for (int k = 0; k < 16; k++) pose_out[(int64_t)b * 16 + k] = c2w[k];
        theta_out[b] = theta[f];
        phi_out[b] = phi[f];
        radius_out[b] = radius[f];
    }
}

__global__ __launch_bounds__(256) void generate_rays_dev_kernel(float fx, float fy, float cx, float cy,
                                                                const float *__restrict__ poses, int B, int H, int W,
                                                                const int32_t *__restrict__ pix, int N,
                                                                const int64_t *__restrict__ frame_idx, int F,
                                                                float *__restrict__ rays_o, float *__restrict__ rays_d,
                                                                float *__restrict__ rays_t, int64_t *__restrict__ rays_id) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)B * N) return;
    const int b = (int)(gid / N);
    const int n = (int)(gid - (int64_t)b * N);
    const int HW = H * W;
    int p = pix ? pix[n] : n;
    p = p < 0 ? 0 : (p > HW - 1 ? HW - 1 : p);
    const Pose pose = pose_from_c2w(poses + (int64_t)b * 16);
    float o[3], d[3];
    pixel_ray(fx, fy, cx, cy, pose, W, p, o, d);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        rays_o[gid * 3 + a] = o[a];
        rays_d[gid * 3 + a] = d[a];
    }
    if (frame_idx) {
        const int f = clamp_frame(frame_idx, b, F);
        if (rays_t) rays_t[gid] = (float)f / (float)F;
        if (rays_id) rays_id[gid] = (int64_t)f;
    }
}

// x / sqrt(max(x.x, 1e-20)): the reference's safe_normalize, in double
__device__ __forceinline__ void safe_normalize3(const double *x, double *y) {
    double s = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    s = s < 1e-20 ? 1e-20 : s;
    const double r = sqrt(s);
    for (int a = 0; a < 3; a++) y[a] = x[a] / r;
}

__device__ __forceinline__ void cross3(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// atanf / atan2f as fdlibm states them (s_atanf.c, e_atan2f.c): the program the C library runs where the reference's CPU
// `torch.atan2` meets its strided [B] columns.  Rounded fp32 operators only, so under contract(off) the bits are the same.
// Arguments are finite here (components of a normalised vector); NaN passes through.
__device__ __forceinline__ float libm_atanf(float x) {
    const float atanhi[4] = {4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f};
    const float atanlo[4] = {5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f};
    const float aT[11] = {3.3333334327e-01f, -2.0000000298e-01f, 1.4285714924e-01f, -1.1111110449e-01f,
                          9.0908870101e-02f, -7.6918758452e-02f, 6.6610731184e-02f, -5.8335702866e-02f,
                          4.9768779427e-02f, -3.6531571299e-02f, 1.6285819933e-02f};
    const int32_t hx = __float_as_int(x), ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x4c800000) {      // |x| >= 2^26
        if (ix > 0x7f800000) return x + x;
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3ee00000) {       // |x| < 7/16
        if (ix < 0x31000000) return x;
        id = -1;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000) {
            if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
            else { id = 1; x = (x - 1.0f) / (x + 1.0f); }
        } else {
            if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }
            else { id = 3; x = -1.0f / x; }
        }
    }
    const float z = x * x, w = z * z;
    const float s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const float s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    const float r = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return hx < 0 ? -r : r;
}

__device__ __forceinline__ float libm_atan2f(float y, float x) {
    const float tiny = 1.0e-30f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const int32_t hx = __float_as_int(x), hy = __float_as_int(y), ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;
    if (hx == 0x3f800000) return libm_atanf(y);
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);      // 2 sign(x) + sign(y)
    if (iy == 0) return m < 2 ? y : (m == 2 ? pi + tiny : -pi - tiny);
    if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = (iy - ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0f;
    else z = libm_atanf(fabsf(y / x));
    if (m == 0) return z;
    if (m == 1) return -z;
    if (m == 2) return pi - (z - pi_lo);
    return (z - pi_lo) - pi;
}

struct LabelBounds {      // the thresholds of get_view_direction, each rounded to fp32 from the host's float64 expression
    float front_half;     // front / 2
    float back_lo;        // pi - front / 2
    float left_lo;        // pi + front / 2
    float wrap_lo;        // 2 pi - front / 2
    float overhead;       // overhead
    float bottom;         // pi - overhead
};

#define MH_VV_ANGLES 0      // a, b: theta, phi in radians (the theta/phi box of get_virtual_view_data)
#define MH_VV_SPHERE 1      // a, b, c: the three normal draws of the uniform-sphere branch
#define MH_VV_POLAR 2       // a, b: theta, phi in DEGREES (is_train=False through get_c2w_from_polar)

__global__ __launch_bounds__(64) void virtual_pose_kernel(int mode, const float *__restrict__ da, const float *__restrict__ db,
                                                          const float *__restrict__ dc, const int64_t *__restrict__ frame_idx,
                                                          int B, const float *__restrict__ radius_tab,
                                                          const float *__restrict__ theta_tab, const float *__restrict__ phi_tab,
                                                          int F, float radius_factor, LabelBounds lb, float *__restrict__ pose_out,
                                                          int64_t *__restrict__ dir_out, float *__restrict__ polar_out,
                                                          float *__restrict__ azimuth_out, float *__restrict__ dradius_out,
                                                          float *__restrict__ deg_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float pi_f = (float)3.141592653589793;
    const float twopi_f = (float)(2.0 * 3.141592653589793);
    const int f = clamp_frame(frame_idx, b, F);
    const float rad = radius_tab[f] * radius_factor;      // fp32, as radius[t] * novel_view_scale_factor

    float th, ph, th_deg, ph_deg;
    double c[3];
    if (mode == MH_VV_SPHERE) {
        // the angles: the reference's fp32 chain (see the header comment)
        const float w[3] = {da[b], fabsf(db[b]), dc[b]};
        float n32 = (float)sqrt((double)fmaf(w[2], w[2], fmaf(w[1], w[1], w[0] * w[0])));
        n32 = n32 < 1e-12f ? 1e-12f : n32;      // F.normalize's eps
        const float u0 = w[0] / n32, u1 = w[1] / n32, u2 = w[2] / n32;
        th = (float)acos((double)u1);
        ph = libm_atan2f(u0, u2);
        if (ph < 0.0f) ph += twopi_f;
        // the pose: the same chain in double from the three draws
        const double v[3] = {(double)w[0], (double)w[1], (double)w[2]};
        double nrm = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        nrm = nrm < 1e-12 ? 1e-12 : nrm;
        for (int a = 0; a < 3; a++) c[a] = (double)rad * (v[a] / nrm);
    } else {
        if (mode == MH_VV_POLAR) {
            th_deg = da[b];
            ph_deg = db[b];
            th = th_deg / 180.0f * pi_f;
            ph = ph_deg / 180.0f * pi_f;
        } else {
            th = da[b];
            ph = db[b];
            if (ph < 0.0f) ph += twopi_f;
        }
        const double st = sin((double)th), ct = cos((double)th), sp = sin((double)ph), cp = cos((double)ph);
        c[0] = (double)rad * st * sp;
        c[1] = (double)rad * ct;
        c[2] = (double)rad * st * cp;
    }
    if (mode != MH_VV_POLAR) {      // back to degrees, fp32 operators
        th_deg = th / pi_f * 180.0f;
        ph_deg = ph / pi_f * 180.0f;
    }

    // OpenGL look-at towards the origin, keep_chirality: forward = normalize(c), right = normalize(up0 x forward),
    // up = normalize(forward x right); the columns of R are (right, up, forward)
    double fwd[3], right[3], up[3], tmp[3];
    const double up0[3] = {0.0, 1.0, 0.0};
    safe_normalize3(c, fwd);
    cross3(up0, fwd, tmp);
    safe_normalize3(tmp, right);
    cross3(fwd, right, tmp);
    safe_normalize3(tmp, up);
    float *P = pose_out + (int64_t)b * 16;
    for (int a = 0; a < 3; a++) {
        P[a * 4 + 0] = (float)right[a];
        P[a * 4 + 1] = (float)up[a];
        P[a * 4 + 2] = (float)fwd[a];
        P[a * 4 + 3] = (float)c[a];
    }
    P[12] = 0.f;
    P[13] = 0.f;
    P[14] = 0.f;
    P[15] = 1.f;

    // the view label: first by phi % 2pi (torch.remainder: fmod, moved into [0, 2pi) when negative), then by theta
    float m = fmodf(ph, twopi_f);
    if (m != 0.0f && m < 0.0f) m += twopi_f;
    int64_t res = 0;
    if (m >= lb.left_lo && m < lb.wrap_lo) res = 1;
    if (m >= lb.back_lo && m < lb.left_lo) res = 2;
    if (m >= lb.front_half && m < lb.back_lo) res = 3;
    if (th <= lb.overhead) res = 4;
    if (th >= lb.bottom) res = 5;
    dir_out[b] = res;

    polar_out[b] = th_deg - theta_tab[f];
    float az = ph_deg - phi_tab[f];
    if (az > 180.0f) az -= 360.0f;
    azimuth_out[b] = az;
    dradius_out[b] = rad - radius_tab[f];
    deg_out[(int64_t)b * 2 + 0] = th_deg;
    deg_out[(int64_t)b * 2 + 1] = ph_deg;
}

extern "C" int mh_dataset_sample(float fx, float fy, float cx, float cy, const float *poses, const uint8_t *rgb, const void *depth,
                                 int32_t depth_is_f32, double depth_scale, const uint8_t *mask, const float *theta,
                                 const float *phi, const float *radius, int32_t F, int32_t H, int32_t W,
                                 const int64_t *frame_idx, int32_t B, const int32_t *pix, int32_t N, float *rays_o,
                                 float *rays_d, float *rays_t, int64_t *rays_id, float *image, float *depth_out,
                                 int64_t *mask_out, float *pose_out, float *theta_out, float *phi_out, float *radius_out,
                                 void *stream) {
    if (B == 0 || N == 0) return MH_OK;
    if (!poses || !rgb || !depth || !mask || !theta || !phi || !radius || !frame_idx || !rays_o || !rays_d || !rays_t ||
        !rays_id || !image || !depth_out || !mask_out || !pose_out || !theta_out || !phi_out || !radius_out || F <= 0 ||
        H <= 0 || W <= 0 || B < 0 || N < 0 || (int64_t)H * W > 0x7fffffffLL || !(depth_scale > 0.0))
        return MH_ERR_ARG;
    if (!pix && (int64_t)N > (int64_t)H * W) return MH_ERR_ARG;      // whole-frame mode: ray n is pixel n
    const int64_t total = (int64_t)B * N;
    if ((total + 255) / 256 > 0x7fffffffLL) return MH_ERR_ARG;
    hipLaunchKernelGGL(dataset_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, mh_stream(stream), fx, fy, cx,
                       cy, poses, rgb, depth, (int)depth_is_f32, depth_scale, mask, theta, phi, radius, (int)F, (int)H, (int)W,
                       frame_idx, (int)B, pix, (int)N, rays_o, rays_d, rays_t, rays_id, image, depth_out, mask_out, pose_out,
                       theta_out, phi_out, radius_out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_generate_rays_dev(float fx, float fy, float cx, float cy, const float *poses, int32_t B, int32_t H, int32_t W,
                                    const int32_t *pix, int32_t N, const int64_t *frame_idx, int32_t F, float *rays_o,
                                    float *rays_d, float *rays_t, int64_t *rays_id, void *stream) {
    if (B == 0 || N == 0) return MH_OK;
    if (!poses || !rays_o || !rays_d || H <= 0 || W <= 0 || B < 0 || N < 0 || (int64_t)H * W > 0x7fffffffLL) return MH_ERR_ARG;
    if (!pix && (int64_t)N > (int64_t)H * W) return MH_ERR_ARG;
    if ((rays_t || rays_id) && (!frame_idx || F <= 0)) return MH_ERR_ARG;
    const int64_t total = (int64_t)B * N;
    if ((total + 255) / 256 > 0x7fffffffLL) return MH_ERR_ARG;
    hipLaunchKernelGGL(generate_rays_dev_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, mh_stream(stream), fx, fy,
                       cx, cy, poses, (int)B, (int)H, (int)W, pix, (int)N, frame_idx, (int)F, rays_o, rays_d, rays_t, rays_id);
    MH_CHECK_LAUNCH();
    return MH_OK;
}

extern "C" int mh_dataset_virtual_pose(int32_t mode, const float *a, const float *b, const float *c, const int64_t *frame_idx,
                                       int32_t B, const float *radius, const float *theta, const float *phi, int32_t F,
                                       float radius_factor, float front_half, float back_lo, float left_lo, float wrap_lo,
                                       float overhead, float bottom, float *pose_out, int64_t *dir_out, float *polar_out,
                                       float *azimuth_out, float *dradius_out, float *deg_out, void *stream) {
    if (B == 0) return MH_OK;
    if (mode < MH_VV_ANGLES || mode > MH_VV_POLAR || !a || !b || (mode == MH_VV_SPHERE && !c) || !frame_idx || !radius ||
        !theta || !phi || F <= 0 || B < 0 || !pose_out || !dir_out || !polar_out || !azimuth_out || !dradius_out || !deg_out)
        return MH_ERR_ARG;
    const LabelBounds lb = {front_half, back_lo, left_lo, wrap_lo, overhead, bottom};
    hipLaunchKernelGGL(virtual_pose_kernel, dim3((B + 63) / 64), dim3(64), 0, mh_stream(stream), (int)mode, a, b, c, frame_idx,
                       (int)B, radius, theta, phi, (int)F, radius_factor, lb, pose_out, dir_out, polar_out, azimuth_out,
                       dradius_out, deg_out);
    MH_CHECK_LAUNCH();
    return MH_OK;
}
