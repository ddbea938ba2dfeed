// az_solver_dev.h -- the device code that the trainers' kernels inline (az_trainer.hip: the shared kernels; az_det_solver.hip:
// the softmax loss; az_skip.hip / az_skip_train.hip: the skip front): the counter-based generator, the map view, RoIPool's bin
// range, the GEMM tile's constants and its fp32 staging, and the fixed f64 workgroup sum.  Nothing here is a kernel or a launch.
#pragma once
#include "az_ctx.h"

#include <cfloat>

namespace {

// ---- counter-based generator (include/aznet_hip.h: az_solver_step) ------------------------------------------------------
__host__ __device__ inline unsigned long long az_mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr unsigned long long AZ_GOLD = 0x9E3779B97F4A7C15ull;
__host__ __device__ inline unsigned long long az_layer_key(unsigned long long seed, unsigned long long iter, unsigned layer)
{
    return az_mix64(az_mix64(az_mix64(seed + AZ_GOLD) + iter) + layer);
}
__host__ __device__ inline unsigned long long az_elem_bits(unsigned long long key, unsigned long long e)
{
    return az_mix64(key + AZ_GOLD * (e + 1ull));
}

// ---- a batch of maps in either memory format; RoIPool's 7x7 bins (same rounding / bin edges / clamp as k_roi_pool, az_head.hip) --
struct MapView { int N, C, H, W, cl; };
__device__ __forceinline__ size_t map_index(const MapView &m, int n, int c, int h, int w)
{
    return m.cl ? (((size_t)n * m.H + h) * m.W + w) * m.C + c : (((size_t)n * m.C + c) * m.H + h) * m.W + w;
}

__device__ __forceinline__ void bin_range(int p, float b, int start, int lim, int *lo, int *hi)
{
    int s = (int)floorf((float)p * b) + start;
    int e = (int)ceilf((float)(p + 1) * b) + start;
    *lo = min(max(s, 0), lim); *hi = min(max(e, 0), lim);
}

// ---- the GEMM tile (k_solver_gemm, az_trainer.hip; k_skip_conv, az_skip.hip): 128 x 128 outputs, K through LDS 32 at a time as
// sP[k][i] with rows of GLD floats; the bf16 image is sP[i][k] with rows of BLD elements (80 B) -----------------------------------
constexpr int GT = 128, GK = 32, GLD = GT + 1, BLD = GK + 8;

template <bool KC>
__device__ __forceinline__ void gemm_stage(const float *__restrict__ P, long long li, long long lk, int i0, int nI, int k0, int kend,
                                           float *__restrict__ sP, int tid)
{
    if (KC) {
        const int k = tid & 31, ib = tid >> 5;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = ib + 8 * q;
            const bool ok = (i0 + i < nI) && (k0 + k < kend);
            sP[k * GLD + i] = ok ? P[(long long)(i0 + i) * li + (long long)(k0 + k) * lk] : 0.0f;
        }
    } else {
        const int i = tid & 127, kb = tid >> 7;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = kb + 2 * q;
            const bool ok = (i0 + i < nI) && (k0 + k < kend);
            sP[k * GLD + i] = ok ? P[(long long)(i0 + i) * li + (long long)(k0 + k) * lk] : 0.0f;
        }
    }
}

typedef float az_f32x16 __attribute__((ext_vector_type(16)));

// ---- the sum of a 256-thread workgroup's values over a fixed tree (sh: 256 doubles of LDS) -----------------------------------
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

}  // namespace
