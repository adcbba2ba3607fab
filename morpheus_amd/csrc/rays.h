// The pinhole ray of one pixel, shared by sampler.hip and dataset.hip so that both produce the same bits.
// Reference: datasets/utils.py:28-65 (OpenGL pinhole, directions NOT normalised) and datasets/dataset.py:363-366
// (rays_d = sum_k dirs_k * R[:,k]; rays_o = c2w[:3,3]).
#pragma once

// No FMA contraction: every mul/add/div below is a separate IEEE round-to-nearest operation, exactly the sequence torch
// executes on the CPU.  (Both including files state the same pragma at file scope; it is repeated here so that the
// arithmetic does not depend on where the header is included.)
#pragma clang fp contract(off)

struct Pose {
    float r[9];
    float t[3];
};

// one pinhole ray: pixel idx = j*W + i -> camera direction ((i+.5-cx)/fx, -(j+.5-cy)/fy, -1) rotated by R
__device__ __forceinline__ void pixel_ray(float fx, float fy, float cx, float cy, const Pose &pose, int W, int idx,
                                          float *o, float *d) {
    const int j = idx / W, i = idx - j * W;
    const float d0 = (((float)i + 0.5f) - cx) / fx;
    const float d1 = -((((float)j + 0.5f) - cy) / fy);
    const float d2 = -1.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        d[a] = (d0 * pose.r[a * 3 + 0] + d1 * pose.r[a * 3 + 1]) + d2 * pose.r[a * 3 + 2];
        o[a] = pose.t[a];
    }
}

// the Pose of a row-major 4x4 camera-to-world matrix (host or device memory, read where the caller runs)
__host__ __device__ __forceinline__ Pose pose_from_c2w(const float *c2w) {
    Pose p;
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) p.r[a * 3 + b] = c2w[a * 4 + b];
        p.t[a] = c2w[a * 4 + 3];
    }
    return p;
}
