// az_solver_dev.h -- the kernels and launch helpers that the two trainers share (az_solver.hip: AZ-net; az_det_solver.hip:
// the detection net): the counter-based generator, RoIPool with arg-max and its gather backward, the bounds-checked fp32 MFMA
// GEMM in its three operand orders and its bf16-operand twin, split-K slabs summed in slab order, bias / ReLU / dropout,
// column sums, SmoothL1, the two-level gradient norm and the SGD update.  Everything sits in an anonymous namespace: each translation unit gets its own
// copy.  fc_forward / gemm_any serve any trainer struct with the members c (az_ctx *), w[], part and prec (AZ_TRAIN_*).
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

// ---- RoIPool 7x7 with arg-max (Caffe ROIPoolingLayer; same rounding / bin edges / clamp as k_roi_pool, az_head.hip) -----
// geo [R][8]: batch, rsw, rsh, rew, reh (ints), then bh, bw (float bits), unused -- kept for the backward gather.
struct MapView { int N, C, H, W, cl; };
__device__ __forceinline__ size_t map_index(const MapView &m, int n, int c, int h, int w)
{
    return m.cl ? (((size_t)n * m.H + h) * m.W + w) * m.C + c : (((size_t)n * m.C + c) * m.H + h) * m.W + w;
}

__global__ void __launch_bounds__(256) k_solver_roi_geo(const float *__restrict__ rois, int R, float ss, int *__restrict__ geo)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float *roi = rois + 5 * (size_t)r;
    const int rsw = (int)roundf(roi[1] * ss), rsh = (int)roundf(roi[2] * ss);
    const int rew = (int)roundf(roi[3] * ss), reh = (int)roundf(roi[4] * ss);
    int rh = reh - rsh + 1; rh = rh < 1 ? 1 : rh;
    int rw = rew - rsw + 1; rw = rw < 1 ? 1 : rw;
    int *g = geo + 8 * (size_t)r;
    g[0] = (int)roi[0]; g[1] = rsw; g[2] = rsh; g[3] = rew; g[4] = reh;
    g[5] = __float_as_int((float)rh / 7.0f); g[6] = __float_as_int((float)rw / 7.0f); g[7] = 0;
}

__device__ __forceinline__ void bin_range(int p, float b, int start, int lim, int *lo, int *hi)
{
    int s = (int)floorf((float)p * b) + start;
    int e = (int)ceilf((float)(p + 1) * b) + start;
    *lo = min(max(s, 0), lim); *hi = min(max(e, 0), lim);
}

__global__ void __launch_bounds__(256) k_solver_roi_pool(const float *__restrict__ feat, MapView m, const int *__restrict__ geo,
                                                         int R, float *__restrict__ pool5, int *__restrict__ argmax)
{
    const long long total = (long long)R * 49 * m.C;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int c = (int)(idx % m.C);
        const int p = (int)((idx / m.C) % 49);
        const int r = (int)(idx / ((long long)m.C * 49));
        const int *g = geo + 8 * (size_t)r;
        const int ph = p / 7, pw = p - ph * 7;
        int hs, he, ws, we;
        bin_range(ph, __int_as_float(g[5]), g[2], m.H, &hs, &he);
        bin_range(pw, __int_as_float(g[6]), g[1], m.W, &ws, &we);
        const bool empty = (he <= hs) || (we <= ws);
        float best = empty ? 0.0f : -FLT_MAX;
        int at = -1;
        for (int h = hs; h < he; ++h)
            for (int w = ws; w < we; ++w) {
                const float v = feat[map_index(m, g[0], c, h, w)];
                if (v > best) { best = v; at = h * m.W + w; }
            }
        const size_t o = (size_t)r * 49 * m.C + (size_t)c * 49 + p;
        pool5[o] = best;
        argmax[o] = at;
    }
}

// d conv5_3: each pooled gradient goes to its arg-max cell.  One thread per cell GATHERS over the rois of its image in row
// order and over the bins whose window can hold the cell (the float bin range widened by one on both sides, then decided by
// the stored arg-max: exactly the adjoint of the forward).
__global__ void __launch_bounds__(256) k_solver_roi_pool_bwd(const float *__restrict__ dpool, const int *__restrict__ argmax,
                                                             const int *__restrict__ geo, int R, MapView m,
                                                             float *__restrict__ dmap)
{
    const long long total = (long long)m.N * m.C * m.H * m.W;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int n, c, h, w;
    if (m.cl) { c = (int)(idx % m.C); w = (int)((idx / m.C) % m.W); h = (int)((idx / ((long long)m.C * m.W)) % m.H); n = (int)(idx / ((long long)m.C * m.W * m.H)); }
    else { w = (int)(idx % m.W); h = (int)((idx / m.W) % m.H); c = (int)((idx / ((long long)m.W * m.H)) % m.C); n = (int)(idx / ((long long)m.W * m.H * m.C)); }
    const int cell = h * m.W + w;
    float sum = 0.0f;
    for (int r = 0; r < R; ++r) {
        const int *g = geo + 8 * (size_t)r;
        if (g[0] != n) continue;
        const float bh = __int_as_float(g[5]), bw = __int_as_float(g[6]);
        int p0 = (int)floorf((float)(h - g[2]) / bh) - 1, p1 = (int)ceilf((float)(h - g[2] + 1) / bh) + 1;
        int q0 = (int)floorf((float)(w - g[1]) / bw) - 1, q1 = (int)ceilf((float)(w - g[1] + 1) / bw) + 1;
        p0 = min(max(p0, 0), 7); p1 = min(max(p1, 0), 7); q0 = min(max(q0, 0), 7); q1 = min(max(q1, 0), 7);
        const size_t base = (size_t)r * 49 * m.C + (size_t)c * 49;
        for (int ph = p0; ph < p1; ++ph)
            for (int pw = q0; pw < q1; ++pw)
                if (argmax[base + ph * 7 + pw] == cell) sum += dpool[base + ph * 7 + pw];
    }
    dmap[idx] = sum;
}

// ---- fp32 GEMM on the matrix cores ------------------------------------------------------------------------------------------
// D[i][j] = sum_{k in slab} A(i, k) * B(j, k), i < M, j < N; A(i, k) = A[i * lai + k * lak], B(j, k) = B[j * lbj + k * lbk].
// A 256-thread workgroup owns a 128 x 128 tile of D, each of its four waves 64 x 64 of it as 2 x 2 v_mfma_f32_32x32x2_f32
// accumulators; K goes through LDS 32 at a time as sA[k][i] / sB[k][j] (an operand fragment is one conflict-free 4-byte read:
// lane l holds A[i = l & 31][k = l >> 5]).  blockIdx.z is the split-K slab: its result goes to D + z * slab.  The three
// products of a layer differ only in which index is contiguous in memory (AK / BK: along k):
//   forward  y  = x W^T     A = x  [M][K]  (AK)   B = W  [N][K]  (BK)
//   dx          = dy W      A = dy [M][K]  (AK)   B = W  [K][N]
//   dW          = dy^T x    A = dy [K][M]         B = x  [K][N]
// Every element is loaded with a bounds check (zero beyond M / N / the slab), so any M, N, K is served; the k order inside a
// slab is ascending: bitwise an fmaf chain per output, whatever the tile.
constexpr int GT = 128, GK = 32, GLD = GT + 1;

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

template <bool AK, bool BK>
__global__ void __launch_bounds__(256) k_solver_gemm(const float *__restrict__ A, long long lai, long long lak,
                                                     const float *__restrict__ B, long long lbj, long long lbk,
                                                     float *__restrict__ D, long long ldd, long long slab, int M, int N, int K,
                                                     int Kc, int accumulate)
{
    __shared__ float sA[GK * GLD];
    __shared__ float sB[GK * GLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * GT, i0 = blockIdx.y * GT;
    const int kbeg = blockIdx.z * Kc, kend = min(K, kbeg + Kc);
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    az_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.0f;
    const int lr = lane & 31, lk = lane >> 5;
    for (int k0 = kbeg; k0 < kend; k0 += GK) {
        __syncthreads();
        gemm_stage<AK>(A, lai, lak, i0, M, k0, kend, sA, tid);
        gemm_stage<BK>(B, lbj, lbk, j0, N, k0, kend, sB, tid);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2) {
            const float a0 = sA[(kk + lk) * GLD + wi + lr], a1 = sA[(kk + lk) * GLD + wi + 32 + lr];
            const float b0 = sB[(kk + lk) * GLD + wj + lr], b1 = sB[(kk + lk) * GLD + wj + 32 + lr];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5)
    float *Dz = D + (long long)blockIdx.z * slab;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int j = j0 + wj + 32 * b + lr;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = i0 + wi + 32 * a + (v & 3) + 8 * (v >> 2) + 4 * lk;
                if (i < M && j < N) {
                    float *d = Dz + (long long)i * ldd + j;
                    *d = accumulate ? *d + acc[a][b][v] : acc[a][b][v];
                }
            }
        }
}

// ---- the same GEMM with bf16 operands (AZ_TRAIN_BF16) -------------------------------------------------------------------------
// Same arguments, forms, slabs, bounds checks and epilogue as k_solver_gemm.  The operands stay fp32 in HBM; each element is
// rounded to bf16 (round to nearest even: v_cvt_pk_bf16_f32) on its way into LDS, and the products are summed in fp32 by
// v_mfma_f32_32x32x16_bf16 (same C/D layout as the fp32 instruction; lane l holds A[i = l & 31][k = 8 (l >> 5) + j], j < 8).
// LDS image: sP[i][k], k contiguous, rows of 32 k (64 B) padded to 80 B: the 16 lanes that one ds_read_b128 serves together
// (rows {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} of one k half) then fall on 16 different 16-byte slots of the 256-byte
// bank row (5 r mod 16 is a bijection on either set), and a fragment is one 16-byte read.  The next stage's 32 elements per
// thread are loaded into registers before the current one is consumed.  Slabs and the stages inside them are consumed in
// ascending k; the order of the 16 products inside one instruction is the instruction's own.
constexpr int BLD = GK + 8;                     // row stride of the bf16 image, in elements (80 B)
typedef __bf16 az_bf16x8 __attribute__((ext_vector_type(8)));

// KC (k contiguous in memory): thread -> (row tid >> 2 [+ 64], k = 8 (tid & 3) ..+7); else (i contiguous): thread ->
// (row tid & 127, k = 16 (tid >> 7) ..+15).  Either way a thread holds two runs of 8 consecutive k: v[0..7], v[8..15].
template <bool KC>
__device__ __forceinline__ void bf16_stage_load(const float *__restrict__ P, long long li, long long lk, int i0, int nI, int k0,
                                                int kend, int tid, float (&v)[16])
{
    if (KC) {
        const int kc = 8 * (tid & 3);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = (tid >> 2) + 64 * q;
            const float *p = P + (long long)(i0 + i) * li + (long long)(k0 + kc) * lk;
            if (i0 + i < nI && k0 + kc + 8 <= kend && lk == 1 && (((unsigned long long)p) & 15ull) == 0) {
                const float4 x = *(const float4 *)p, y = *(const float4 *)(p + 4);
                v[8 * q + 0] = x.x; v[8 * q + 1] = x.y; v[8 * q + 2] = x.z; v[8 * q + 3] = x.w;
                v[8 * q + 4] = y.x; v[8 * q + 5] = y.y; v[8 * q + 6] = y.z; v[8 * q + 7] = y.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool ok = (i0 + i < nI) && (k0 + kc + j < kend);
                    v[8 * q + j] = ok ? p[(long long)j * lk] : 0.0f;
                }
            }
        }
    } else {
        const int i = tid & 127, kb = 16 * (tid >> 7);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool ok = (i0 + i < nI) && (k0 + kb + j < kend);
            v[j] = ok ? P[(long long)(i0 + i) * li + (long long)(k0 + kb + j) * lk] : 0.0f;
        }
    }
}

template <bool KC>
__device__ __forceinline__ void bf16_stage_store(const float (&v)[16], __bf16 *__restrict__ sP, int tid)
{
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        az_bf16x8 f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (__bf16)v[8 * q + j];
        const int at = KC ? ((tid >> 2) + 64 * q) * BLD + 8 * (tid & 3) : (tid & 127) * BLD + 16 * (tid >> 7) + 8 * q;
        *(az_bf16x8 *)(sP + at) = f;
    }
}

template <bool AK, bool BK>
__global__ void __launch_bounds__(256) k_solver_gemm_bf16(const float *__restrict__ A, long long lai, long long lak,
                                                          const float *__restrict__ B, long long lbj, long long lbk,
                                                          float *__restrict__ D, long long ldd, long long slab, int M, int N,
                                                          int K, int Kc, int accumulate)
{
    __shared__ __attribute__((aligned(16))) __bf16 sA[GT * BLD];
    __shared__ __attribute__((aligned(16))) __bf16 sB[GT * BLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * GT, i0 = blockIdx.y * GT;
    const int kbeg = blockIdx.z * Kc, kend = min(K, kbeg + Kc);
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    az_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.0f;
    const int lr = lane & 31, lk = lane >> 5;
    float va[16], vb[16];
    if (kbeg < kend) {
        bf16_stage_load<AK>(A, lai, lak, i0, M, kbeg, kend, tid, va);
        bf16_stage_load<BK>(B, lbj, lbk, j0, N, kbeg, kend, tid, vb);
    }
    for (int k0 = kbeg; k0 < kend; k0 += GK) {
        __syncthreads();
        bf16_stage_store<AK>(va, sA, tid);
        bf16_stage_store<BK>(vb, sB, tid);
        __syncthreads();
        if (k0 + GK < kend) {
            bf16_stage_load<AK>(A, lai, lak, i0, M, k0 + GK, kend, tid, va);
            bf16_stage_load<BK>(B, lbj, lbk, j0, N, k0 + GK, kend, tid, vb);
        }
#pragma unroll
        for (int kk = 0; kk < GK; kk += 16) {
            const az_bf16x8 a0 = *(const az_bf16x8 *)(sA + (wi + lr) * BLD + kk + 8 * lk);
            const az_bf16x8 a1 = *(const az_bf16x8 *)(sA + (wi + 32 + lr) * BLD + kk + 8 * lk);
            const az_bf16x8 b0 = *(const az_bf16x8 *)(sB + (wj + lr) * BLD + kk + 8 * lk);
            const az_bf16x8 b1 = *(const az_bf16x8 *)(sB + (wj + 32 + lr) * BLD + kk + 8 * lk);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    float *Dz = D + (long long)blockIdx.z * slab;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int j = j0 + wj + 32 * b + lr;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = i0 + wi + 32 * a + (v & 3) + 8 * (v >> 2) + 4 * lk;
                if (i < M && j < N) {
                    float *d = Dz + (long long)i * ldd + j;
                    *d = accumulate ? *d + acc[a][b][v] : acc[a][b][v];
                }
            }
        }
}

// slabs summed in slab order (+ what `out` holds when accumulate, + bias[j]); forward layers: pre-activation, ReLU, dropout
__global__ void __launch_bounds__(256) k_solver_finish(const float *__restrict__ part, int S, long long slab, const float *__restrict__ bias,
                                                       long long MN, int N, int accumulate, float *__restrict__ out,
                                                       float *__restrict__ act, int relu, unsigned char *__restrict__ mask,
                                                       unsigned long long key, unsigned thr, float scale)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= MN) return;
    float s = part[e];
    for (int q = 1; q < S; ++q) s += part[(long long)q * slab + e];
    if (accumulate) s = out[e] + s;
    if (bias) s += bias[e % N];
    out[e] = s;
    if (!act) return;
    float a = relu ? (s > 0.0f ? s : 0.0f) : s;
    if (mask) {
        const bool keep = (unsigned)(az_elem_bits(key, (unsigned long long)e) >> 40) >= thr;
        mask[e] = keep ? 1 : 0;
        a = keep ? a * scale : 0.0f;
    }
    act[e] = a;
}

// ReLU (in place after the layer) and dropout backward: d_pre = d_act * mask * scale where pre > 0
__global__ void __launch_bounds__(256) k_solver_act_bwd(float *__restrict__ d, const float *__restrict__ pre,
                                                        const unsigned char *__restrict__ mask, float scale, long long n)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float g = d[e];
    if (mask) g = mask[e] ? g * scale : 0.0f;
    d[e] = pre[e] > 0.0f ? g : 0.0f;
}

// db[j] = sum over rows, in row order
__global__ void __launch_bounds__(256) k_solver_colsum(const float *__restrict__ dy, int R, int N, float *__restrict__ db)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    float s = 0.0f;
    for (int r = 0; r < R; ++r) s += dy[(size_t)r * N + j];
    db[j] = s;
}

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

// SigmoidCrossEntropyLoss: loss = -1/num sum(x (t - [x >= 0]) - log(1 + exp(x - 2 x [x >= 0]))), dx = (sigmoid(x) - t) / num
__global__ void __launch_bounds__(256) k_solver_sigmoid_ce(const float *__restrict__ x, const float *__restrict__ t, int n, int num,
                                                           float *__restrict__ dx, float *__restrict__ loss)
{
    __shared__ double sh[256];
    double s = 0.0;
    const float inv = 1.0f / (float)num;
    for (int e = threadIdx.x; e < n; e += 256) {
        const float v = x[e], tt = t[e];
        const float ge = v >= 0.0f ? 1.0f : 0.0f;
        const float ex = expf(v - 2.0f * v * ge);           // exp(-|x|)
        s += (double)(v * (tt - ge) - log1pf(ex));
        const float sg = v >= 0.0f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
        dx[e] = (sg - tt) * inv;
    }
    const double tot = block_sum(s, sh);
    if (threadIdx.x == 0) *loss = (float)(-tot / (double)num);
}

// SmoothL1Loss with three bottoms: d = w (x - t); f = 0.5 d^2 if |d| < 1 else |d| - 0.5; loss = sum f / num
__global__ void __launch_bounds__(256) k_solver_smooth_l1(const float *__restrict__ x, const float *__restrict__ t,
                                                          const float *__restrict__ w, int n, int num, float *__restrict__ dx,
                                                          float *__restrict__ loss)
{
    __shared__ double sh[256];
    double s = 0.0;
    const float inv = 1.0f / (float)num;
    for (int e = threadIdx.x; e < n; e += 256) {
        const float d = w[e] * (x[e] - t[e]);
        const float ad = fabsf(d);
        s += (double)(ad < 1.0f ? 0.5f * d * d : ad - 0.5f);
        const float g = ad < 1.0f ? d : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
        dx[e] = w[e] * g * inv;
    }
    const double tot = block_sum(s, sh);
    if (threadIdx.x == 0) *loss = (float)(tot / (double)num);
}

// sum of squares, two fixed levels: workgroup b sums chunk b of the array (strided per thread, then the LDS tree) into
// part[b]; one workgroup then adds all partials of all arrays in index order
constexpr int SQ_BLOCKS = 512;
__global__ void __launch_bounds__(256) k_solver_sumsq(const float *__restrict__ g, long long n, double *__restrict__ part)
{
    __shared__ double sh[256];
    const long long chunk = (n + SQ_BLOCKS - 1) / SQ_BLOCKS;
    const long long b0 = (long long)blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
    double s = 0.0;
    for (long long e = b0 + threadIdx.x; e < b1; e += 256) { const double v = (double)g[e]; s += v * v; }
    const double tot = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(256) k_solver_sumsq_final(const double *__restrict__ part, int n, double *__restrict__ out)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (int e = threadIdx.x; e < n; e += 256) s += part[e];
    const double tot = block_sum(s, sh);
    if (threadIdx.x == 0) *out = tot;
}

// Caffe SGDSolver: g = clip_scale * g + decay * w; hist = momentum * hist + rate * g; w -= hist (one rounding per operation)
__global__ void __launch_bounds__(256) k_solver_sgd(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ hist,
                                                    long long n, float rate, float momentum, float decay, float clip)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        float gg = g[e] * clip;
        gg = gg + decay * w[e];
        const float h = momentum * hist[e] + rate * gg;
        hist[e] = h;
        w[e] = w[e] - h;
    }
}

// Caffe's gaussian filler (mean 0): Box-Muller on two 24-bit uniforms of the element's word
__global__ void __launch_bounds__(256) k_solver_fill_gauss(float *__restrict__ w, long long n, float stdv, unsigned long long key)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const unsigned long long b = az_elem_bits(key, (unsigned long long)e);
        const float u1 = ((float)(unsigned)(b >> 40) + 1.0f) * (1.0f / 16777216.0f);
        const float u2 = (float)(unsigned)((b >> 16) & 0xFFFFFFu) * (1.0f / 16777216.0f);
        w[e] = stdv * sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
    }
}

int grid_for(long long n, int cap = 65535 * 16) { long long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > cap ? cap : b)); }

void pick_split(int M, int N, int K, int *S, int *Kc)
{
    const long long tiles = (long long)((M + GT - 1) / GT) * ((N + GT - 1) / GT);
    long long s = 256 / tiles;
    s = s < 1 ? 1 : (s > 16 ? 16 : s);
    int kc = (int)(((K + s - 1) / s + GK - 1) / GK) * GK;
    if (kc < GK) kc = GK;
    *Kc = kc;
    *S = (K + kc - 1) / kc;
}

// form 0: A [M][K], B [N][K]; 1: A [M][K], B [K][N]; 2: A [K][M], B [K][N]; prec: AZ_TRAIN_FP32 / AZ_TRAIN_BF16 (operands)
template <bool AK, bool BK>
void launch_gemm_form(hipStream_t s, int prec, dim3 grid, const float *A, long long lai, long long lak, const float *B, long long lbj,
                      long long lbk, float *D, long long slab, int M, int N, int K, int Kc, int accumulate)
{
    if (prec == AZ_TRAIN_BF16)
        hipLaunchKernelGGL((k_solver_gemm_bf16<AK, BK>), grid, dim3(256), 0, s, A, lai, lak, B, lbj, lbk, D, (long long)N, slab, M, N, K, Kc, accumulate);
    else
        hipLaunchKernelGGL((k_solver_gemm<AK, BK>), grid, dim3(256), 0, s, A, lai, lak, B, lbj, lbk, D, (long long)N, slab, M, N, K, Kc, accumulate);
}

void launch_gemm(hipStream_t s, int form, const float *A, const float *B, float *D, long long slab, int M, int N, int K, int S,
                 int Kc, int accumulate, int prec)
{
    const dim3 grid((N + GT - 1) / GT, (M + GT - 1) / GT, S);
    if (form == 0)
        launch_gemm_form<true, true>(s, prec, grid, A, (long long)K, 1LL, B, (long long)K, 1LL, D, slab, M, N, K, Kc, accumulate);
    else if (form == 1)
        launch_gemm_form<true, false>(s, prec, grid, A, (long long)K, 1LL, B, 1LL, (long long)N, D, slab, M, N, K, Kc, accumulate);
    else
        launch_gemm_form<false, false>(s, prec, grid, A, 1LL, (long long)M, B, 1LL, (long long)N, D, slab, M, N, K, Kc, accumulate);
}

// y = x W^T + b into `pre` (and, for the hidden layers, ReLU + dropout into `act`)
template <typename Solver>
void fc_forward(Solver *s, const char *name, const float *x, int pw, int R, int N, int K, float *pre, float *act,
                unsigned char *mask, unsigned long long key, float ratio)
{
    az_ctx *c = s->c;
    int S, Kc;
    pick_split(R, N, K, &S, &Kc);
    const long long slab = (long long)R * N;
    { Timed t(c, name, 0, 1); launch_gemm(c->stream, 0, x, s->w[pw], s->part, slab, R, N, K, S, Kc, 0, s->prec); }
    const unsigned thr = (unsigned)((double)ratio * 16777216.0);
    Timed t(c, "fc_finish", 0);
    hipLaunchKernelGGL(k_solver_finish, dim3(grid_for(slab)), dim3(256), 0, c->stream, s->part, S, slab, s->w[pw + 1], slab, N, 0,
                       pre, act, act ? 1 : 0, mask, key, thr, 1.0f / (1.0f - ratio));
}

// D (+)= product of the given form, split-K through the slabs when the tile count alone would leave the chip idle
template <typename Solver>
void gemm_any(Solver *s, const char *name, int form, const float *A, const float *B, float *D, int M, int N, int K, int accumulate)
{
    az_ctx *c = s->c;
    int S, Kc;
    pick_split(M, N, K, &S, &Kc);
    const long long slab = (long long)M * N;
    if (S == 1) { Timed t(c, name, 0, 1); launch_gemm(c->stream, form, A, B, D, 0, M, N, K, 1, Kc, accumulate, s->prec); return; }
    { Timed t(c, name, 0, 1); launch_gemm(c->stream, form, A, B, s->part, slab, M, N, K, S, Kc, 0, s->prec); }
    Timed t(c, "slab_sum", 0);
    hipLaunchKernelGGL(k_solver_finish, dim3(grid_for(slab)), dim3(256), 0, c->stream, s->part, S, slab, (const float *)nullptr, slab,
                       N, accumulate, D, (float *)nullptr, 0, (unsigned char *)nullptr, 0ull, 0u, 1.0f);
}

}  // namespace
