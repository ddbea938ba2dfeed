// az_solver_dev.h -- the device code that the trainers' kernels inline (az_trainer.hip: the shared kernels; az_det_solver.hip:
// the softmax loss; az_skip.hip / az_skip_train.hip: the skip front, whose own pool + GRN body is az_skip_dev.h): the
// counter-based generator, the map view, RoIPool's window and bin range, the GEMM tile (constants, fp32 staging, the fp32 K loop
// and the walk over the accumulators that every GEMM kernel stores through), and the fixed f64 workgroup sum.  Nothing here is
// a kernel or a launch.
#pragma once
#include "az_ctx.h"

#include <cfloat>

// These two records are at global scope, not in the unnamed namespace below, because they appear in the signature of a function
// with external linkage (tr_pool_gather, az_trainer.h), which another translation unit (az_skip_train.hip) calls.
struct MapView { int N, C, H, W, cl; };           // a batch of maps in either memory format
struct PoolStrides { int sr, sc, sp, off; };      // channel c's bin p of roi r in a pooled tensor: word r * sr + off + c * sc + p * sp

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
__device__ __forceinline__ size_t map_index(const MapView &m, int n, int c, int h, int w)
{
    return m.cl ? (((size_t)n * m.H + h) * m.W + w) * m.C + c : (((size_t)n * m.C + c) * m.H + h) * m.W + w;
}

// a roi's window on a map at scale ss: its first / last column and row, and the height / width of one of its 7 x 7 bins
struct RoiWindow { int rsw, rsh, rew, reh; float bh, bw; };
__device__ __forceinline__ RoiWindow roi_window(const float *__restrict__ roi, float ss)
{
    RoiWindow g;
    g.rsw = (int)roundf(roi[1] * ss); g.rsh = (int)roundf(roi[2] * ss);
    g.rew = (int)roundf(roi[3] * ss); g.reh = (int)roundf(roi[4] * ss);
    int rh = g.reh - g.rsh + 1; rh = rh < 1 ? 1 : rh;
    int rw = g.rew - g.rsw + 1; rw = rw < 1 ? 1 : rw;
    g.bh = (float)rh / 7.0f; g.bw = (float)rw / 7.0f;
    return g;
}

__device__ __forceinline__ void bin_range(int p, float b, int start, int lim, int *lo, int *hi)
{
    int s = (int)floorf((float)p * b) + start;
    int e = (int)ceilf((float)(p + 1) * b) + start;
    *lo = min(max(s, 0), lim); *hi = min(max(e, 0), lim);
}

// ---- the GEMM tile (k_solver_gemm, k_solver_gemm_bf16, az_trainer.hip; k_skip_conv, az_skip.hip): 128 x 128 outputs, K through LDS 32 at a time as
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

// A wave owns 64 x 64 of the tile as 2 x 2 accumulators of the 32 x 32 MFMA, at (wi, wj) inside it.  (tile_fp32 and tile_store
// each build this record from tid themselves: handed one from the kernel, k_solver_gemm<false, false> takes 110 VGPRs for
// 103 and loses its third wave per SIMD.)
struct TileLane {
    int lr, lk, wi, wj;                   // lane & 31, lane >> 5; the wave's corner
    __device__ __forceinline__ explicit TileLane(int tid)
    {
        const int lane = tid & 63, wave = tid >> 6;
        lr = lane & 31; lk = lane >> 5; wi = (wave >> 1) * 64; wj = (wave & 1) * 64;
    }
};

__device__ __forceinline__ void tile_zero(az_f32x16 (&acc)[2][2])
{
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.0f;
}

// acc = sum over k in [kbeg, kend), ascending, of A(i0 + i, k) * B(j0 + j, k) on v_mfma_f32_32x32x2_f32: zeroed, then K staged
// through the function's own LDS (sA[k][i], sB[k][j]) 32 at a time; an operand fragment is one conflict-free 4-byte read
// (lane l holds A[i = l & 31][k = l >> 5]).  Bitwise an fmaf chain per output, whatever the tile.
template <bool AK, bool BK>
__device__ __forceinline__ void tile_fp32(const float *A, long long lai, long long lak, const float *B, long long lbj, long long lbk,
                                          int i0, int M, int j0, int N, int kbeg, int kend, int tid, az_f32x16 (&acc)[2][2])
{
    const TileLane t(tid);
    __shared__ float sA[GK * GLD];
    __shared__ float sB[GK * GLD];
    tile_zero(acc);
    for (int k0 = kbeg; k0 < kend; k0 += GK) {
        __syncthreads();
        gemm_stage<AK>(A, lai, lak, i0, M, k0, kend, sA, tid);
        gemm_stage<BK>(B, lbj, lbk, j0, N, k0, kend, sB, tid);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2) {
            const float a0 = sA[(kk + t.lk) * GLD + t.wi + t.lr], a1 = sA[(kk + t.lk) * GLD + t.wi + 32 + t.lr];
            const float b0 = sB[(kk + t.lk) * GLD + t.wj + t.lr], b1 = sB[(kk + t.lk) * GLD + t.wj + 32 + t.lr];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}

// store(i, j, value, store.column(j)) for every output of the tile inside M x N; column(j) is what the functor wants read once
// per output column and not once per output (k_skip_conv: the bias).  C/D layout of the 32x32 MFMA (fp32 and bf16 alike):
// col = lane & 31, row = (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5)
template <typename F>
__device__ __forceinline__ void tile_store(const az_f32x16 (&acc)[2][2], int tid, int i0, int M, int j0, int N, const F &store)
{
    const TileLane t(tid);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int j = j0 + t.wj + 32 * b + t.lr;
            const auto cj = j < N ? store.column(j) : decltype(store.column(j))();
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = i0 + t.wi + 32 * a + (v & 3) + 8 * (v >> 2) + 4 * t.lk;
                if (i < M && j < N) store(i, j, acc[a][b][v], cj);
            }
        }
}

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
