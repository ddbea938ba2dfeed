// az_trainer.hip -- the core of the two trainers (az_trainer.h): every kernel they share, defined once, and the host functions
// on az_trainer.  The kernels: RoIPool with arg-max and its gather backward (the skip front's gathers are launches of the same
// kernel with other strides), the bounds-checked fp32 MFMA GEMM in its three operand orders and its bf16-operand twin (the tile
// they and k_skip_conv share is az_solver_dev.h's: tile_fp32, tile_store), split-K slabs summed in slab order, bias / ReLU / dropout, column sums, the sigmoid
// and SmoothL1 losses, the two-level gradient norm, the SGD update and the gaussian filler.
//
// Every reduction has a fixed order (no floating-point atomics): split-K slabs are summed in slab order, column sums walk
// the rows in order, RoIPool backward GATHERS over the rois in row order, loss sums and the gradient norm are a strided
// per-thread sum followed by a fixed LDS tree.  The same step from the same state gives the same bits.
#include "az_trainer.h"

namespace {

// ---- RoIPool 7x7 with arg-max (Caffe ROIPoolingLayer; same rounding / bin edges / clamp as k_roi_pool, az_head.hip) -----
// geo [R][8]: batch, rsw, rsh, rew, reh (ints), then bh, bw (float bits), unused -- kept for the backward gather.
__global__ void __launch_bounds__(256) k_solver_roi_geo(const float *__restrict__ rois, int R, float ss, int *__restrict__ geo)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float *roi = rois + 5 * (size_t)r;
    const RoiWindow w = roi_window(roi, ss);
    int *g = geo + 8 * (size_t)r;
    g[0] = (int)roi[0]; g[1] = w.rsw; g[2] = w.rsh; g[3] = w.rew; g[4] = w.reh;
    g[5] = __float_as_int(w.bh); g[6] = __float_as_int(w.bw); g[7] = 0;
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

// d map: each pooled gradient goes to its arg-max cell.  One thread per cell GATHERS over the rois of its image in row
// order and over the bins whose window can hold the cell (the float bin range widened by one on both sides, then decided by
// the stored arg-max: exactly the adjoint of the forward).  Channel c's bin p of roi r is word r * sr + off + c * sc + p * sp
// of dpool / argmax: the trainers' pool5 [r][c * 49 + p], or one source's columns of the skip front's [(r, p)][sumC].
__global__ void __launch_bounds__(256) k_solver_roi_pool_bwd(const float *__restrict__ dpool, const int *__restrict__ argmax,
                                                             const int *__restrict__ geo, int R, MapView m, PoolStrides st,
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
        const size_t base = (size_t)r * st.sr + st.off + (size_t)c * st.sc;
        for (int ph = p0; ph < p1; ++ph)
            for (int pw = q0; pw < q1; ++pw) {
                const size_t o = base + (size_t)(ph * 7 + pw) * st.sp;
                if (argmax[o] == cell) sum += dpool[o];
            }
    }
    dmap[idx] = sum;
}

// ---- fp32 GEMM on the matrix cores ------------------------------------------------------------------------------------------
// what both GEMM kernels do with an output: into the slab, or added to what it holds
struct SlabStore {
    float *__restrict__ Dz; long long ldd; int accumulate;
    __device__ __forceinline__ int column(int) const { return 0; }     // (nothing per column)
    __device__ __forceinline__ void operator()(int i, int j, float v, int) const
    {
        float *d = Dz + (long long)i * ldd + j;
        *d = accumulate ? *d + v : v;
    }
};

// D[i][j] = sum_{k in slab} A(i, k) * B(j, k), i < M, j < N; A(i, k) = A[i * lai + k * lak], B(j, k) = B[j * lbj + k * lbk].
// A 256-thread workgroup owns a 128 x 128 tile of D, each of its four waves 64 x 64 of it as 2 x 2 v_mfma_f32_32x32x2_f32
// accumulators; K goes through LDS 32 at a time as sA[k][i] / sB[k][j] (tile_fp32, az_solver_dev.h).  blockIdx.z is the
// split-K slab: its result goes to D + z * slab.  The three products of a layer differ only in which index is contiguous in
// memory (AK / BK: along k):
//   forward  y  = x W^T     A = x  [M][K]  (AK)   B = W  [N][K]  (BK)
//   dx          = dy W      A = dy [M][K]  (AK)   B = W  [K][N]
//   dW          = dy^T x    A = dy [K][M]         B = x  [K][N]
// Every element is loaded with a bounds check (zero beyond M / N / the slab), so any M, N, K is served; the k order inside a
// slab is ascending: bitwise an fmaf chain per output, whatever the tile.
template <bool AK, bool BK>
__global__ void __launch_bounds__(256) k_solver_gemm(const float *__restrict__ A, long long lai, long long lak,
                                                     const float *__restrict__ B, long long lbj, long long lbk,
                                                     float *__restrict__ D, long long ldd, long long slab, int M, int N, int K,
                                                     int Kc, int accumulate)
{
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * GT, i0 = blockIdx.y * GT;
    const int kbeg = blockIdx.z * Kc, kend = min(K, kbeg + Kc);
    az_f32x16 acc[2][2];
    tile_fp32<AK, BK>(A, lai, lak, B, lbj, lbk, i0, M, j0, N, kbeg, kend, tid, acc);
    tile_store(acc, tid, i0, M, j0, N, SlabStore{D + (long long)blockIdx.z * slab, ldd, accumulate});
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
    const int tid = threadIdx.x;
    const TileLane t(tid);
    const int j0 = blockIdx.x * GT, i0 = blockIdx.y * GT;
    const int kbeg = blockIdx.z * Kc, kend = min(K, kbeg + Kc);
    const int wi = t.wi, wj = t.wj, lr = t.lr, lk = t.lk;
    az_f32x16 acc[2][2];
    tile_zero(acc);
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
    tile_store(acc, tid, i0, M, j0, N, SlabStore{D + (long long)blockIdx.z * slab, ldd, accumulate});
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

// db[j] = sum over rows, in row order (+ what db holds when accumulate: one add, after the rows)
__global__ void __launch_bounds__(256) k_solver_colsum(const float *__restrict__ dy, int R, int N, int accumulate, float *__restrict__ db)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    float s = 0.0f;
    for (int r = 0; r < R; ++r) s += dy[(size_t)r * N + j];
    db[j] = accumulate ? db[j] + s : s;
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

}  // namespace

int grid_for(long long n, int cap) { long long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > cap ? cap : b)); }

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

template <bool AK, bool BK>
static void launch_gemm_form(hipStream_t s, int prec, dim3 grid, const float *A, long long lai, long long lak, const float *B, long long lbj,
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

// ---- memory ------------------------------------------------------------------------------------------------------------------
void tr_release(az_trainer *t, size_t mark)
{
    t->allocs.release(mark);
    for (int p = t->np; p < TR_MAXP; ++p) { t->pn[p] = 0; t->w[p] = t->g[p] = t->h[p] = nullptr; }
}

int tr_init(az_trainer *t, az_ctx *c, const char *tag, const char *const *pname, int C, int max_rois, size_t widest)
{
    t->c = c; t->tag = tag; t->pname = pname; t->C = C; t->K6 = C * 49; t->maxR = max_rois;
    const size_t R = (size_t)max_rois, K6 = (size_t)t->K6;
    t->part_elems = R * widest > (size_t)4 << 20 ? R * widest : (size_t)4 << 20;
    int rc = AZ_OK;
#define SA(p, n) if (rc == AZ_OK) rc = tr_alloc(t, &t->p, (n))
    SA(rois, R * 5); SA(geo, R * 8); SA(argmax, R * K6); SA(pool5, R * K6); SA(dpool, R * K6);
    SA(part, t->part_elems); SA(loss, 4); SA(sq_part, (size_t)TR_MAXP * SQ_BLOCKS); SA(sq, 2);
#undef SA
    return rc;
}

// ---- parameters ----------------------------------------------------------------------------------------------------------------
int tr_alloc_params(az_trainer *t, int p0, int p1, const size_t *pn)
{
    int rc = AZ_OK;
    for (int p = p0; p < p1 && rc == AZ_OK; ++p) {
        const size_t n = t->pn[p] = pn[p - p0];
        t->lr_mult[p] = (p & 1) ? 2.0f : 1.0f;
        t->decay_mult[p] = (p & 1) ? 0.0f : 1.0f;
        if ((rc = tr_alloc(t, &t->w[p], n)) == AZ_OK && (rc = tr_alloc(t, &t->g[p], n)) == AZ_OK) rc = tr_alloc(t, &t->h[p], n);
    }
    return rc;
}

int tr_fill_params(az_trainer *t, int p0, int p1, const float *stdv, uint64_t seed)
{
    hipStream_t st = t->c->stream;
    for (int p = p0; p < p1; ++p) {
        const size_t n = t->pn[p];
        hipMemsetAsync(t->h[p], 0, n * sizeof(float), st);
        hipMemsetAsync(t->g[p], 0, n * sizeof(float), st);
        if (p & 1) hipMemsetAsync(t->w[p], 0, n * sizeof(float), st);
        else if (stdv) hipLaunchKernelGGL(k_solver_fill_gauss, dim3(grid_for((long long)n, 8192)), dim3(256), 0, st, t->w[p], (long long)n,
                                          stdv[(p - p0) / 2], az_layer_key(seed, 0, 16 + p));
    }
    return hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess ? AZ_OK : AZ_ERR_HIP;
}

int tr_load(az_trainer *t, int p0, int p1, const float *const *src)
{
    az_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    for (int p = p0; p < p1; ++p)
        if (src[p - p0]) HIPCHK(c, hipMemcpyAsync(t->w[p], src[p - p0], t->pn[p] * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AZ_OK;
}

int tr_read(az_trainer *t, int p0, int p1, float *const *dst)
{
    az_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    for (int p = p0; p < p1; ++p)
        if (dst[p - p0]) HIPCHK(c, hipMemcpyAsync(dst[p - p0], t->w[p], t->pn[p] * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AZ_OK;
}

int tr_load_history(az_trainer *t, int p0, int p1, const float *const *src)
{
    az_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    for (int p = p0; p < p1; ++p)
        if (src[p - p0]) HIPCHK(c, hipMemcpyAsync(t->h[p], src[p - p0], t->pn[p] * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AZ_OK;
}

int tr_set_hyper(az_trainer *t, int n, const float *lr_mult, const float *decay_mult, const float *dropout_ratio, float *drop, int ndrop)
{
    const std::string who = std::string(t->tag) + "_set_hyper";
    if (dropout_ratio) for (int i = 0; i < ndrop; ++i) if (!(dropout_ratio[i] >= 0.0f && dropout_ratio[i] < 1.0f)) return fail(t->c, AZ_ERR_INVALID, who + ": dropout ratio outside [0, 1)");
    if (lr_mult) for (int p = 0; p < n; ++p) if (!(lr_mult[p] >= 0.0f)) return fail(t->c, AZ_ERR_INVALID, who + ": negative lr_mult");
    if (decay_mult) for (int p = 0; p < n; ++p) if (!(decay_mult[p] >= 0.0f)) return fail(t->c, AZ_ERR_INVALID, who + ": negative decay_mult");
    if (lr_mult) for (int p = 0; p < n; ++p) t->lr_mult[p] = lr_mult[p];
    if (decay_mult) for (int p = 0; p < n; ++p) t->decay_mult[p] = decay_mult[p];
    if (dropout_ratio) for (int i = 0; i < ndrop; ++i) drop[i] = dropout_ratio[i];
    return AZ_OK;
}

int tr_set_precision(az_trainer *t, int precision)
{
    if (!t) return AZ_ERR_INVALID;
    if (precision != AZ_TRAIN_FP32 && precision != AZ_TRAIN_BF16)
        return fail(t->c, AZ_ERR_INVALID, std::string(t->tag) + "_set_precision: AZ_TRAIN_FP32 or AZ_TRAIN_BF16");
    t->prec = precision;
    return AZ_OK;
}

int tr_set_accumulate(az_trainer *t, int on)
{
    if (!t) return AZ_ERR_INVALID;
    if (on != 0 && on != 1) return fail(t->c, AZ_ERR_INVALID, std::string(t->tag) + "_set_accumulate: 0 or 1");
    t->acc = on;
    return AZ_OK;
}

// ---- one step --------------------------------------------------------------------------------------------------------------------
int tr_check_rois(az_trainer *t, int N, const float *rois, int R, const std::string &who)
{
    if (R < 1 || R > t->maxR) return fail(t->c, AZ_ERR_INVALID, who + ": R must be in [1, max_rois = " + std::to_string(t->maxR) + "]");
    for (int r = 0; r < R; ++r) {
        const float *roi = rois + 5 * (size_t)r;
        if (!(roi[0] >= 0.0f && roi[0] < (float)N) || roi[0] != std::floor(roi[0]))
            return fail(t->c, AZ_ERR_INVALID, who + ": roi " + std::to_string(r) + " names image " + std::to_string(roi[0]) + " of " + std::to_string(N));
        for (int q = 1; q < 5; ++q)
            if (!std::isfinite(roi[q]) || std::fabs(roi[q]) > 1e8f) return fail(t->c, AZ_ERR_INVALID, who + ": roi coordinate not finite");
    }
    return AZ_OK;
}

int tr_check_step(az_trainer *t, const float *conv, int N, int H, int W, const float *rois, int R, const std::string &who)
{
    if (!t) return AZ_ERR_INVALID;
    if (!conv || !rois) return fail(t->c, AZ_ERR_INVALID, who + ": null conv5_3 or rois");
    if (N < 1 || H < 1 || W < 1 || (long long)H * W > 0x3fffffff) return fail(t->c, AZ_ERR_INVALID, who + ": bad map shape");
    return tr_check_rois(t, N, rois, R, who);
}

void tr_roi_geo(hipStream_t st, const float *rois_dev, int R, float scale, int *geo)
{
    hipLaunchKernelGGL(k_solver_roi_geo, dim3((R + 255) / 256), dim3(256), 0, st, rois_dev, R, scale, geo);
}

int tr_roi_pool_forward(az_trainer *t, const float *conv, int N, int H, int W, int cl, const float *rois, int R)
{
    az_ctx *c = t->c;
    HIPCHK(c, hipMemcpyAsync(t->rois, rois, (size_t)R * 5 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const MapView m{N, t->C, H, W, cl ? 1 : 0};
    Timed tm(c, "roi_pool_argmax", 0);
    tr_roi_geo(c->stream, t->rois, R, c->spatial_scale, t->geo);
    hipLaunchKernelGGL(k_solver_roi_pool, dim3(grid_for((long long)R * t->K6, 16384)), dim3(256), 0, c->stream, conv, m, t->geo, R,
                       t->pool5, t->argmax);
    t->R = R; t->N = N; t->H = H; t->W = W;
    return AZ_OK;
}

void tr_pool_gather(az_ctx *c, const char *name, const float *dpool, const int *argmax, const int *geo, int R, const MapView &m,
                    const PoolStrides &st, float *dmap)
{
    Timed tm(c, name, 0);
    hipLaunchKernelGGL(k_solver_roi_pool_bwd, dim3(grid_for((long long)m.N * m.C * m.H * m.W, 1 << 30)), dim3(256), 0, c->stream, dpool,
                       argmax, geo, R, m, st, dmap);
}

void tr_roi_pool_backward(az_trainer *t, int N, int H, int W, int cl, float *dmap)
{
    const MapView m{N, t->C, H, W, cl ? 1 : 0};
    tr_pool_gather(t->c, "roi_pool_bwd", t->dpool, t->argmax, t->geo, t->R, m, PoolStrides{49 * t->C, 49, 1, 0}, dmap);
}

void fc_forward(az_trainer *t, const char *name, const float *x, int pw, int R, int N, int K, float *pre, float *act,
                unsigned char *mask, unsigned long long key, float ratio)
{
    az_ctx *c = t->c;
    int S, Kc;
    pick_split(R, N, K, &S, &Kc);
    const long long slab = (long long)R * N;
    { Timed tm(c, name, 0, 1); launch_gemm(c->stream, 0, x, t->w[pw], t->part, slab, R, N, K, S, Kc, 0, t->prec); }
    const unsigned thr = (unsigned)((double)ratio * 16777216.0);
    Timed tm(c, "fc_finish", 0);
    hipLaunchKernelGGL(k_solver_finish, dim3(grid_for(slab)), dim3(256), 0, c->stream, t->part, S, slab, t->w[pw + 1], slab, N, 0,
                       pre, act, act ? 1 : 0, mask, key, thr, 1.0f / (1.0f - ratio));
}

void gemm_any(az_trainer *t, const char *name, int form, const float *A, const float *B, float *D, int M, int N, int K, int accumulate)
{
    az_ctx *c = t->c;
    int S, Kc;
    pick_split(M, N, K, &S, &Kc);
    const long long slab = (long long)M * N;
    if (S == 1) { Timed tm(c, name, 0, 1); launch_gemm(c->stream, form, A, B, D, 0, M, N, K, 1, Kc, accumulate, t->prec); return; }
    { Timed tm(c, name, 0, 1); launch_gemm(c->stream, form, A, B, t->part, slab, M, N, K, S, Kc, 0, t->prec); }
    Timed tm(c, "slab_sum", 0);
    hipLaunchKernelGGL(k_solver_finish, dim3(grid_for(slab)), dim3(256), 0, c->stream, t->part, S, slab, (const float *)nullptr, slab,
                       N, accumulate, D, (float *)nullptr, 0, (unsigned char *)nullptr, 0ull, 0u, 1.0f);
}

void tr_colsum(az_trainer *t, const float *dy, int R, int N, float *db, int accumulate)
{
    hipLaunchKernelGGL(k_solver_colsum, dim3((N + 255) / 256), dim3(256), 0, t->c->stream, dy, R, N, accumulate, db);
}

void tr_act_bwd(az_trainer *t, float *d, const float *pre, const unsigned char *mask, float ratio, int R, int N)
{
    Timed tm(t->c, "act_bwd", 0);
    hipLaunchKernelGGL(k_solver_act_bwd, dim3(grid_for((long long)R * N)), dim3(256), 0, t->c->stream, d, pre, ratio > 0.f ? mask : nullptr,
                       1.0f / (1.0f - ratio), (long long)R * N);
}

void tr_sigmoid_ce(az_trainer *t, const float *x, const float *tgt, int n, int num, float *dx, float *loss)
{
    hipLaunchKernelGGL(k_solver_sigmoid_ce, dim3(1), dim3(256), 0, t->c->stream, x, tgt, n, num, dx, loss);
}

void tr_smooth_l1(az_trainer *t, const float *x, const float *tgt, const float *wgt, int n, int num, float *dx, float *loss)
{
    hipLaunchKernelGGL(k_solver_smooth_l1, dim3(1), dim3(256), 0, t->c->stream, x, tgt, wgt, n, num, dx, loss);
}

int tr_grad_norm(az_trainer *t, int n, int k, float *losses_out, double *sumsq_out)
{
    az_ctx *c = t->c;
    hipStream_t st = c->stream;
    { Timed tm(c, "grad_sumsq", 0);
      for (int p = 0; p < n; ++p)
          hipLaunchKernelGGL(k_solver_sumsq, dim3(SQ_BLOCKS), dim3(256), 0, st, t->g[p], (long long)t->pn[p], t->sq_part + (size_t)p * SQ_BLOCKS);
      hipLaunchKernelGGL(k_solver_sumsq_final, dim3(1), dim3(256), 0, st, t->sq_part, n * SQ_BLOCKS, t->sq); }
    float hl[4]; double hs = 0.0;
    HIPCHK(c, hipMemcpyAsync(hl, t->loss, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&hs, t->sq, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (losses_out) for (int i = 0; i < k; ++i) losses_out[i] = hl[i];
    if (sumsq_out) *sumsq_out = hs;
    return AZ_OK;
}

int tr_update(az_trainer *t, int n, double rate, double momentum, double weight_decay, double clip_scale)
{
    az_ctx *c = t->c;
    const std::string tag(t->tag);
    if (!(rate >= 0.0) || !(momentum >= 0.0) || !(weight_decay >= 0.0) || !(clip_scale > 0.0) || !std::isfinite(rate + momentum + weight_decay + clip_scale))
        return fail(c, AZ_ERR_INVALID, tag + "_update: rate, momentum, weight_decay >= 0 and clip_scale > 0, all finite");
    if (!t->trained) return fail(c, AZ_ERR_STATE, tag + "_update: no " + tag + "_step has produced gradients");
    HIPCHK(c, hipSetDevice(c->device));
    { Timed tm(c, "sgd_update", 0);
      for (int p = 0; p < n; ++p)
          hipLaunchKernelGGL(k_solver_sgd, dim3(grid_for((long long)t->pn[p], 16384)), dim3(256), 0, c->stream, t->w[p], t->g[p], t->h[p],
                             (long long)t->pn[p], (float)(rate * (double)t->lr_mult[p]), (float)momentum,
                             (float)(weight_decay * (double)t->decay_mult[p]), (float)clip_scale); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return AZ_OK;
}

int tr_fetch(az_trainer *t, const std::string &nm, const void *src, size_t bytes, void *out, long long cap_bytes, long long *bytes_out)
{
    az_ctx *c = t->c;
    const std::string who = std::string(t->tag) + "_fetch";
    bool is_param = false;
    if (!src && nm.size() > 2 && nm[1] == '_' && (nm[0] == 'g' || nm[0] == 'h' || nm[0] == 'w'))
        for (int p = 0; p < t->np; ++p)
            if (nm.substr(2) == t->pname[p]) { src = nm[0] == 'g' ? t->g[p] : (nm[0] == 'h' ? t->h[p] : t->w[p]); bytes = t->pn[p] * 4; is_param = true; }
    if (!src) return fail(c, AZ_ERR_INVALID, who + ": no saved tensor named '" + nm + "'");
    if (!is_param && t->R == 0) return fail(c, AZ_ERR_STATE, who + ": no forward pass has run");
    *bytes_out = (long long)bytes;
    if (!out) return AZ_OK;
    if (cap_bytes < (long long)bytes) return fail(c, AZ_ERR_CAPACITY, who + ": '" + nm + "' needs " + std::to_string(bytes) + " bytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return AZ_OK;
}

// ---- entry points that belong to no particular net ---------------------------------------------------------------------------
extern "C" {

int az_sgd_update(az_ctx *c, float *w_dev, const float *g_dev, float *hist_dev, long long n, double rate, double momentum,
                  double decay, double clip_scale)
{
    if (!c) return AZ_ERR_INVALID;
    if (!w_dev || !g_dev || !hist_dev || n < 1 || !(rate >= 0.0) || !(momentum >= 0.0) || !(decay >= 0.0) || !(clip_scale > 0.0) ||
        !std::isfinite(rate + momentum + decay + clip_scale))
        return fail(c, AZ_ERR_INVALID, "az_sgd_update: null pointer, n < 1 or a coefficient out of range");
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_solver_sgd, dim3(grid_for(n, 16384)), dim3(256), 0, c->stream, w_dev, g_dev, hist_dev, n, (float)rate,
                       (float)momentum, (float)decay, (float)clip_scale);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return AZ_OK;
}

int az_solver_gemm_unit(az_ctx *c, int form, const float *a, const float *b, float *d, int M, int N, int K)
{
    return az_solver_gemm_unit_prec(c, form, AZ_TRAIN_FP32, a, b, d, M, N, K);
}

int az_solver_gemm_unit_prec(az_ctx *c, int form, int precision, const float *a, const float *b, float *d, int M, int N, int K)
{
    if (!c) return AZ_ERR_INVALID;
    if (precision != AZ_TRAIN_FP32 && precision != AZ_TRAIN_BF16)
        return fail(c, AZ_ERR_INVALID, "az_solver_gemm_unit_prec: AZ_TRAIN_FP32 or AZ_TRAIN_BF16");
    if (!a || !b || !d || form < 0 || form > 2 || M < 1 || N < 1 || K < 1 || (long long)M * N > (1LL << 28) || (long long)M * K > (1LL << 28) || (long long)N * K > (1LL << 28))
        return fail(c, AZ_ERR_INVALID, "az_solver_gemm_unit: bad form, shape or pointer");
    HIPCHK(c, hipSetDevice(c->device));
    int S, Kc;
    pick_split(M, N, K, &S, &Kc);
    const size_t slab = (size_t)M * N;
    Buf buf[4];
    hipError_t e = reserve_group({{&buf[0], (size_t)M * K * 4}, {&buf[1], (size_t)N * K * 4}, {&buf[2], slab * S * 4}, {&buf[3], slab * 4}});
    float *da = buf[0].as<float>(), *db = buf[1].as<float>(), *dp = buf[2].as<float>(), *dd = buf[3].as<float>();
    if (e == hipSuccess) e = hipMemcpyAsync(da, a, (size_t)M * K * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, (size_t)N * K * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_gemm(c->stream, form, da, db, dp, (long long)slab, M, N, K, S, Kc, 0, precision);
        hipLaunchKernelGGL(k_solver_finish, dim3(grid_for((long long)slab)), dim3(256), 0, c->stream, dp, S, (long long)slab, (const float *)nullptr,
                           (long long)slab, N, 0, dd, (float *)nullptr, 0, (unsigned char *)nullptr, 0ull, 0u, 1.0f);
        e = hipMemcpyAsync(d, dd, slab * 4, hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(c, AZ_ERR_HIP, std::string("az_solver_gemm_unit: ") + hipGetErrorString(e));
    return AZ_OK;
}

}  // extern "C"
