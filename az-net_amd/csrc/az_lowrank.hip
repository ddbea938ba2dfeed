// az_lowrank.hip -- the U stage of a truncated-SVD layer (Fast R-CNN section 4.4: fc6_U / fc7_U) on gfx950.
//
// A compressed layer y = relu(U (L x) + b) runs as two products.  The L stage ([in] -> [r], deep K, narrow N) is the
// split-K GEMM of az_head.hip with a split count of its own (azk_lowrank_split below) and a linear slab sum.  The U
// stage ([r] -> [out]) has K = r <= AZ_LOWRANK_MAX: far too short for K slabs, whose round trip through memory would cost
// more than the product.  It is ONE launch here:
//   Y[m][n] = act(sum_k X[m][k] * W[n][k] + b[n]),   X [M, K] (ldx), W [N, K] row-major (Caffe's [out, in]), K = r
// over the whole K, with bias and ReLU applied to the accumulators and the rows written straight into dh6 / dh7.
//
// Workgroup = 4 waves = a 64 (M) x 64 (N) tile, wave (w >> 1, w & 1) owns one 32 x 32 block: one accumulator of
// v_mfma_f32_32x32x2_f32 (64 cycles per instruction: one chain per wave keeps its SIMD's matrix pipe busy).  Tiles of
// 64 x 64 rather than az_head.hip's 128 x 128: 300 rows x 4096 outputs are 320 tiles for 256 CUs instead of 96.  (That
// is still 1280 wave blocks of 32 x 32 x K for 1024 SIMDs: a quarter of the SIMDs run two of them, which sets the
// launch's length -- 45 us at K = 1024, 35 % of the matrix pipe.  Cutting K inside the workgroup would even it out.)
// K-steps of 32: global -> registers (float4) -> LDS (padded rows) one step ahead of the MFMAs, two LDS buffers, one
// barrier per step; fragments come back as in k_fc_splitk -- lane l reads 4 consecutive k of row (l & 31) at k-offset
// 4 * (l >> 5), which feeds 4 MFMAs with the k pairs {j, 4 + j}.
//
// Numerics: the MFMA is bitwise a k-ordered fmaf chain, so an output element is
//   fmaf chain over k = 0,4,1,5,2,6,3,7 | 8,12,9,13,... (zero terms where K % 32 != 0 pads the last step), then + b[n]
// whatever tile it falls into and whatever M is: a roi's bits do not depend on which rois share the launch.
#include "az_dev.h"

namespace {

// (K step: 64 measured 46.6 us against 45.3 for fc6_U at 300 rows, 128 -- one workgroup per CU -- 53 us)
constexpr int LR_BM = 64, LR_BN = 64, LR_BK = 32;
constexpr int LR_LDT = LR_BK + 4;        // padded LDS row (floats): stride 4 mod 32 banks, conflict-free b128 reads (az_head.hip)
constexpr int LR_TPR = LR_BK / 4;        // staging: threads (float4s) per tile row,
constexpr int LR_RPP = 256 / LR_TPR;     // rows per pass of the 256 threads,
constexpr int LR_NP = LR_BM / LR_RPP;    // passes per 64-row tile
static_assert(LR_BK % 8 == 0 && LR_BK >= 8 && LR_BK <= 128 && LR_BM == LR_BN && LR_NP * LR_RPP == LR_BM, "K step: whole 8-wide k groups");
constexpr int LR_GRID = 1024;            // tiles are dealt grid-stride: 300 rows x 4096 outputs = 320 of them

typedef float lr_floatx16 __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(256, 2)
k_lowrank_gemm(const float *__restrict__ X, int ldx, const float *__restrict__ W, const float *__restrict__ bias,
               const int *Mptr, int N, int K, int relu, float *__restrict__ Y, int ldy)
{
    __shared__ __attribute__((aligned(16))) float sA[2][LR_BM * LR_LDT];
    __shared__ __attribute__((aligned(16))) float sB[2][LR_BN * LR_LDT];

    const int M = *Mptr;
    if (M <= 0) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lrow = lane & 31, lk = (lane >> 5) * 4;
    const int nt = (N + LR_BN - 1) / LR_BN, mt = (M + LR_BM - 1) / LR_BM;
    const int nk = (K + LR_BK - 1) / LR_BK;
    // staging: thread t owns float4 f = t + 256 * i (i < LR_NP): row f / LR_TPR, columns (f % LR_TPR) * 4 .. + 3 of both tiles
    const int srow = tid / LR_TPR, sc4 = (tid % LR_TPR) * 4;

    for (int item = blockIdx.x; item < nt * mt; item += gridDim.x) {
        // (n fastest: the workgroups resident together share a strip of X rows and walk W once)
        const int mtile = item / nt, ntile = item - mtile * nt;
        const int m0 = mtile * LR_BM, n0 = ntile * LR_BN;
        // rows past the operand's end are clamped to its last row: their products land in outputs that are never stored
        const float *pa[LR_NP], *pb[LR_NP];
#pragma unroll
        for (int i = 0; i < LR_NP; ++i) {
            pa[i] = X + (size_t)min(m0 + srow + LR_RPP * i, M - 1) * ldx + sc4;
            pb[i] = W + (size_t)min(n0 + srow + LR_RPP * i, N - 1) * K + sc4;
        }
        float4 ra[LR_NP], rb[LR_NP];
        // K % 4 == 0: a float4 lies wholly inside the row or wholly past it (then: zeros, exact no-ops of the chain)
        auto gload = [&](int kt) {
            const int k = kt * LR_BK;
            const bool ok = k + sc4 < K;
#pragma unroll
            for (int i = 0; i < LR_NP; ++i) {
                ra[i] = ok ? *reinterpret_cast<const float4 *>(pa[i] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
                rb[i] = ok ? *reinterpret_cast<const float4 *>(pb[i] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        auto lstore = [&](int buf) {
#pragma unroll
            for (int i = 0; i < LR_NP; ++i) {
                *reinterpret_cast<float4 *>(&sA[buf][(srow + LR_RPP * i) * LR_LDT + sc4]) = ra[i];
                *reinterpret_cast<float4 *>(&sB[buf][(srow + LR_RPP * i) * LR_LDT + sc4]) = rb[i];
            }
        };
        lr_floatx16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;

        gload(0);
        lstore(0);             // (the previous item's last step ended with a barrier: nobody reads either buffer)
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) gload(kt + 1);
            const float *a = &sA[buf][(wr * 32 + lrow) * LR_LDT + lk];
            const float *b = &sB[buf][(wc * 32 + lrow) * LR_LDT + lk];
#pragma unroll
            for (int g8 = 0; g8 < LR_BK / 8; ++g8) {
                const float4 af = *reinterpret_cast<const float4 *>(a + g8 * 8);
                const float4 bf = *reinterpret_cast<const float4 *>(b + g8 * 8);
                // k pairs {j, 4 + j}: accumulation order 0,4,1,5,2,6,3,7 within the 8-wide group
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, acc, 0, 0, 0);
            }
            if (kt + 1 < nk) lstore(buf ^ 1);      // (its readers, step kt - 1, are past the previous barrier)
            __syncthreads();
        }

        // C/D layout of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
        const int col = n0 + wc * 32 + (lane & 31);
        if (col < N) {
            const float bn = bias[col];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + wr * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                float v = acc[e] + bn;
                if (relu) v = v > 0.f ? v : 0.f;
                if (row < M) Y[(size_t)row * ldy + col] = v;
            }
        }
    }
}

}  // namespace

// Y[M, N] (ldy) = act(X[M, K] (ldx) . W[N, K]^T + b): the U stage.  M = *Mptr (device), rows past it are left alone.
// N, K: positive multiples of 4, K <= AZ_LOWRANK_MAX (the callers check).
void azk_lowrank_gemm(hipStream_t s, const float *x, int ldx, const float *W, const float *bias, const int *Mptr,
                      int capM, int N, int K, int relu, float *y, int ldy)
{
    const long long tiles = (long long)((N + LR_BN - 1) / LR_BN) * ((capM + LR_BM - 1) / LR_BM);
    const int grid = (int)(tiles < LR_GRID ? (tiles > 0 ? tiles : 1) : LR_GRID);
    hipLaunchKernelGGL(k_lowrank_gemm, dim3(grid), dim3(256), 0, s, x, ldx, W, bias, Mptr, N, K, relu, y, ldy);
}

// K chunks of the L stage ([M, K] x [K, r] on azk_fc_gemm): a fixed function of (K, r) -- the number of chunks is part
// of a row's bits.  One (n-tile, chunk) group per resident workgroup of that kernel (512), counted with chunks of at
// least 128: K = 25088, r = 1024 -> 8 n-tiles x 61 chunks of 416.  The kernel cuts K into that many chunks of
// azk_fc_chunk(K, S) -- a multiple of its K step, as it requires; every one of them is non-empty.
int azk_lowrank_split(int K, int r)
{
    const int nt = (r + 127) / 128;
    int S = 512 / nt;
    if (S < 1) S = 1;
    int Kc = azk_fc_chunk(K, S);
    if (Kc < 128) Kc = 128;
    return (K + Kc - 1) / Kc;
}

// K chunks of the AZ head's L stage (pool5 [M, K6] x L6^T [K6, r6] through fc_gemm_fp32): a fixed function of (K, r) -- the
// number of chunks is part of a row's bits, so the row count has no say.  Among the splits S that keep the many-row kernel
// eligible (azk_fc_gemm12_fits: whole n-tiles, nt = r / 128, nt S >= 256, S chunks of exactly K / S in whole K steps) the
// one with the least
//     4 ceil(nt S / 256) (K / S)  +  nt S
// (ties: the smaller S).  First term: k_fc_splitk12 deals its nt S (n-tile, chunk) groups statically to 256 workgroups, so
// the launch lasts as long as the workgroup with the most groups, each K / S deep.  Second term: every chunk writes a slab
// of M x r floats that the slab sum reads again; its weight against the first is the measured one (688 and 2672 rows at
// K = 25088, r = 1024, DESIGN 4y: a slab costs what 2 K elements of a group cost).  There: 56 chunks of 448 (448 groups: 192
// workgroups run two, 64 one), measured ahead of 49, 98, 112 and 196 at both row counts.  Where no split fits (r no
// multiple of 128, K no multiple of 32, a shallow K) the launch stays on k_fc_splitk whatever the row count, with
// azk_lowrank_split's chunks.
int azk_az_lowrank_split(int K, int r)
{
    long long best = -1;
    int bestS = 0;
    if (r % 128 == 0) {
        const int nt = r / 128;
        for (int S = (256 + nt - 1) / nt; S <= K / 64; ++S) {
            if (!azk_fc_gemm12_fits(r, K, S)) continue;
            const long long cost = 4LL * (((long long)nt * S + 255) / 256) * (K / S) + (long long)nt * S;
            if (best < 0 || cost < best) { best = cost; bestS = S; }
        }
    }
    return bestS ? bestS : azk_lowrank_split(K, r);
}
