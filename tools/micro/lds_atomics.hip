// micro-benchmark: LDS atomic throughput on gfx950 (f32 add vs u32 add vs u64 add), conflict-free and 4-way same-address
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
template <int MODE, int CONFLICT>
__global__ __launch_bounds__(256) void k(float *out, int iters) {
    __shared__ unsigned long long buf[4096];
    for (int i = threadIdx.x; i < 4096; i += 256) buf[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x;
    int idx = CONFLICT ? (lane / 4) : lane;  // CONFLICT: 4 lanes share an address
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int a = (idx + u * 257 + it * 31) & 4095;
            if (MODE == 0) atomicAdd(reinterpret_cast<float *>(buf) + a, 1.0f);
            if (MODE == 1) atomicAdd(reinterpret_cast<unsigned *>(buf) + a, 1u);
            if (MODE == 2) atomicAdd(buf + a, 1ull);
            if (MODE == 4) atomicAdd(reinterpret_cast<double *>(buf) + a, 1.0);
            if (MODE == 5) __builtin_amdgcn_ds_faddf((__attribute__((address_space(3))) float *)(reinterpret_cast<float *>(buf) + a), 1.0f, 0, 0, false);
            if (MODE == 3) reinterpret_cast<float *>(buf)[a] += 1.0f;  // plain RMW (racy) as a reference rate
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (float)buf[1];
}
template <int MODE, int CONFLICT>
void run(const char *name) {
    float *out; hipMalloc(&out, 4096 * 4);
    const int blocks = 1024, iters = 200;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((k<MODE, CONFLICT>), dim3(blocks), dim3(256), 0, 0, out, iters);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL((k<MODE, CONFLICT>), dim3(blocks), dim3(256), 0, 0, out, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    double ops = (double)blocks * 256 * iters * 16;
    printf("%-28s %8.3f ms  %7.1f G lane-atomics/s  (%.2f cycles per wave-instr per CU @2.2GHz, 256 CUs)\n", name, ms, ops / ms / 1e6,
           ms * 1e-3 * 2.2e9 / (ops / 64 / 256));
}
// ds_add_u64 by ADDRESS PATTERN (what the hash-grid backward's accumulator layout decides).  An 8-byte LDS write is served in four
// groups of 16 contiguous lanes; the bank pair of byte address a is (a / 8) mod 16.  36 KB = 4608 words = 288 rows of 16 words.
//   PAT 0: word = 16 * (random row) + column, the 16 lanes of a group on 16 different columns (a different permutation per group)
//   PAT 1: random word of the 4608
//   PAT 2: word = 3 * (random slot of 1536) + (0 | 1): the 24-byte vertex slots {sum x, sum y, row}
//   PAT 3: the control -- PAT 1's instructions on consecutive words (lane + 256 u): conflict-free under any grouping
// Per lane sixteen random numbers drawn once, moved by a wave-uniform offset every iteration (add, wrap: 3 VALU + the pattern's 1).
template <int PAT>
__global__ __launch_bounds__(256) void kp(float *out, int iters) {
    constexpr int WORDS = 4608, N = PAT == 0 ? WORDS / 16 : (PAT == 2 ? WORDS / 3 : WORDS);
    __shared__ unsigned long long buf[WORDS];
    for (int i = threadIdx.x; i < WORDS; i += 256) buf[i] = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x;
    unsigned r[16], h = lane * 2654435761u + blockIdx.x * 40503u + 12345u;
#pragma unroll
    for (int u = 0; u < 16; u++) {
        h ^= h << 13, h ^= h >> 17, h ^= h << 5;
        r[u] = PAT == 3 ? (lane + 256u * u) % (unsigned)N : h % (unsigned)N;
    }
    const unsigned col = ((lane & 15) * 5 + (lane >> 4) * 3) & 15;     // odd multiplier: a permutation of 0..15 inside every group
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const unsigned s = (unsigned)(it * 37 + u * 11) % (unsigned)N;       // wave-uniform
            const unsigned t = r[u] + s, v = min(t, t - (unsigned)N);            // (r + s) mod N
            const unsigned a = PAT == 0 ? (v << 4 | col) : (PAT == 2 ? 3 * v + (u & 1) : v);
            atomicAdd(buf + a, 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (float)buf[1];
}
template <int PAT>
void runp(const char *name) {
    float *out; hipMalloc(&out, 4096 * 4);
    const int blocks = 1024, iters = 200;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((kp<PAT>), dim3(blocks), dim3(256), 0, 0, out, iters);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL((kp<PAT>), dim3(blocks), dim3(256), 0, 0, out, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    double ops = (double)blocks * 256 * iters * 16;
    printf("%-44s %8.3f ms  %7.1f G lane-atomics/s  (%.2f cycles per wave-instr per CU @2.2GHz, 256 CUs)\n", name, ms, ops / ms / 1e6,
           ms * 1e-3 * 2.2e9 / (ops / 64 / 256));
}
int main() {
    runp<0>("ds_add_u64 16 columns per lane group");
    runp<1>("ds_add_u64 random words of 36 KB");
    runp<2>("ds_add_u64 24-byte slots, random");
    runp<3>("ds_add_u64 consecutive words, same arithmetic");
    run<0, 0>("ds_add_f32 conflict-free"); run<0, 1>("ds_add_f32 4-way same addr");
    run<1, 0>("ds_add_u32 conflict-free"); run<1, 1>("ds_add_u32 4-way same addr");
    run<2, 0>("ds_add_u64 conflict-free"); run<2, 1>("ds_add_u64 4-way same addr");
    run<4, 0>("ds_add_f64 conflict-free"); run<4, 1>("ds_add_f64 4-way same addr");
    run<5, 0>("ds_faddf builtin conflict-free");
    run<3, 0>("plain f32 RMW");
    return 0;
}
