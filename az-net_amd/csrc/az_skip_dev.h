// az_skip_dev.h -- what the skip-connection front's inference kernels (az_skip.hip) and training kernels (az_skip_train.hip)
// share: the sources' record and its builder, and the one pool + GRN body of k_skip_pool_norm and k_skip_train_pool.  The
// window (roi_window), the bin range, the GEMM tile and the gather backward are the trainers' (az_solver_dev.h, az_trainer.hip).
#pragma once
#include "az_solver_dev.h"

namespace {

// the front's maps: n sources of N images each, all channel-last (cl) or all NCHW, side by side in the [rows][sumC] tensors.
// One record for both fronts: the inference kernel reads scale and not n / N / cl (one channel-last image); the training
// kernels read those and never scale, which is 0 in a record built without scales (their windows come from geo).
struct SkipSrcs {
    const float *map[AZ_SKIP_MAX_SRC];
    int C[AZ_SKIP_MAX_SRC], H[AZ_SKIP_MAX_SRC], W[AZ_SKIP_MAX_SRC], off[AZ_SKIP_MAX_SRC];
    float scale[AZ_SKIP_MAX_SRC];
    int sumC, n, N, cl;
};

inline SkipSrcs skip_srcs(int n, const int *C, const int *H, const int *W, const void *const *maps, int N, int cl,
                          const float *scales = nullptr)
{
    SkipSrcs a{};
    for (int i = 0; i < n; ++i) {
        a.map[i] = (const float *)maps[i]; a.C[i] = C[i]; a.H[i] = H[i]; a.W[i] = W[i]; a.off[i] = a.sumC;
        a.scale[i] = scales ? scales[i] : 0.0f;
        a.sumC += C[i];
    }
    a.n = n; a.N = N; a.cl = cl ? 1 : 0;
    return a;
}

// max() as both fronts take it (strict >: of equal values the earlier stays)
__device__ __forceinline__ void larger(float v, float &m)
{
    if (v > m) m = v;
}
// with the arg-max: a cell's value meets the running maximum of its group (cells in ascending order: the first maximum stays)
__device__ __forceinline__ void take(float v, int cell, float &m, int &at)
{
    if (v > m) { m = v; at = cell; }
}
// the partial result of a later cell group meets an earlier one's: the larger value, among equal ones the lower cell
__device__ __forceinline__ void meet(float v, int cell, float &m, int &at)
{
    if (v > m || (v == m && cell >= 0 && (at < 0 || cell < at))) { m = v; at = cell; }
}

// One workgroup pools one 7 x 7 bin -- rows [hs, he), columns [ws, we) of one image's map fm [fH][fW][C] (cl) or [C][fH][fW] --
// into out[0 .. C), and with `normalise` rescales it by f = gain / sqrt(sum_c out[c]^2 + eps).  The window is k_roi_pool's
// (az_head.hip) through roi_window / bin_range; max() is exact, so how the cells are dealt to the threads does not show in a
// bit.  A lane holds four consecutive channels; with fewer than 256 channel quads the workgroup splits the window's cells over
// 256 / quads groups and the partial maxima meet in LDS.  ARG (the training entry) also keeps the arg-max cell h * fW + w of
// every channel in aout (-1 in an empty bin) -- a group scans its cells in ascending order and the groups meet lowest cell
// first, so it is the first maximum of the row-major scan, as k_solver_roi_pool picks it -- and f in *fac, and reads either
// memory format; without it there is no arg-max register, no arg-max LDS and no NCHW read (cl is taken as set).
template <bool ARG>
__device__ __forceinline__ void skip_pool_grn(const float *__restrict__ fm, int C, int fH, int fW, int cl, int hs, int he, int ws,
                                              int we, float *__restrict__ out, int *__restrict__ aout, double *__restrict__ fac,
                                              double gain, double eps, int normalise)
{
    __shared__ float4 smax[256];
    __shared__ double sred[4];
    int4 *sarg = nullptr;
    if constexpr (ARG) {
        __shared__ int4 sarg_[256];
        sarg = sarg_;
    }
    const int tid = threadIdx.x, nq = C >> 2;
    const bool empty = (he <= hs) || (we <= ws);
    const int nw = we - ws, ncell = empty ? 0 : (he - hs) * nw;
    double ssq = 0.0;
    for (int q0 = 0; q0 < nq; q0 += 256) {
        const int nqb = min(256, nq - q0), G = 256 / nqb;
        const int g = tid / nqb, q = tid - g * nqb;
        float4 m = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX);
        [[maybe_unused]] int4 at = make_int4(-1, -1, -1, -1);
        if (g < G)
            for (int i = g; i < ncell; i += G) {
                const int hh = hs + i / nw, ww = ws + i % nw, c0 = 4 * (q0 + q);
                const size_t cell = (size_t)hh * fW + ww;
                if constexpr (ARG) {
                    float4 v;
                    if (cl) v = *reinterpret_cast<const float4 *>(fm + cell * C + c0);
                    else {
                        const size_t hw = (size_t)fH * fW;
                        v.x = fm[(size_t)c0 * hw + cell]; v.y = fm[(size_t)(c0 + 1) * hw + cell];
                        v.z = fm[(size_t)(c0 + 2) * hw + cell]; v.w = fm[(size_t)(c0 + 3) * hw + cell];
                    }
                    take(v.x, (int)cell, m.x, at.x); take(v.y, (int)cell, m.y, at.y);
                    take(v.z, (int)cell, m.z, at.z); take(v.w, (int)cell, m.w, at.w);
                } else {
                    const float4 v = *reinterpret_cast<const float4 *>(fm + cell * C + c0);
                    larger(v.x, m.x); larger(v.y, m.y); larger(v.z, m.z); larger(v.w, m.w);
                }
            }
        smax[tid] = m;
        if constexpr (ARG) sarg[tid] = at;
        __syncthreads();
        if (tid < nqb) {
            float4 r = smax[tid];
            [[maybe_unused]] int4 ra = at;
            if constexpr (ARG) ra = sarg[tid];
            for (int g2 = 1; g2 < G; ++g2) {
                const float4 v = smax[g2 * nqb + tid];
                if constexpr (ARG) {
                    const int4 va = sarg[g2 * nqb + tid];
                    meet(v.x, va.x, r.x, ra.x); meet(v.y, va.y, r.y, ra.y);
                    meet(v.z, va.z, r.z, ra.z); meet(v.w, va.w, r.w, ra.w);
                } else {
                    larger(v.x, r.x); larger(v.y, r.y); larger(v.z, r.z); larger(v.w, r.w);
                }
            }
            if (empty) { r = make_float4(0.f, 0.f, 0.f, 0.f); ra = make_int4(-1, -1, -1, -1); }   // an empty bin pools to 0 (Caffe)
            *reinterpret_cast<float4 *>(out + 4 * (q0 + tid)) = r;
            if constexpr (ARG) *reinterpret_cast<int4 *>(aout + 4 * (q0 + tid)) = ra;
            ssq += (double)r.x * r.x;
            ssq += (double)r.y * r.y;
            ssq += (double)r.z * r.z;
            ssq += (double)r.w * r.w;
        }
        __syncthreads();
    }
    if (!normalise) return;
    // sum of squares over the source's channels: a fixed tree (lanes, then waves in order), so a row's bits do not depend
    // on where it runs; in f64, as is the factor -- the stored value is gain * x / sqrt(ss + eps) rounded once
    for (int o = 32; o > 0; o >>= 1) ssq += __shfl_down(ssq, o, 64);
    if ((tid & 63) == 0) sred[tid >> 6] = ssq;
    __syncthreads();
    const double tot = ((sred[0] + sred[1]) + sred[2]) + sred[3] + eps;
    const double f = tot > 0.0 ? gain / sqrt(tot) : 0.0;               // (all-zero vector, eps 0: zeros, never NaN)
    if constexpr (ARG) { if (tid == 0) *fac = f; }
    for (int q = tid; q < nq; q += 256) {                              // (the quads this thread stored itself)
        float4 r = *reinterpret_cast<float4 *>(out + 4 * q);
        r.x = (float)((double)r.x * f); r.y = (float)((double)r.y * f);
        r.z = (float)((double)r.z * f); r.w = (float)((double)r.w * f);
        *reinterpret_cast<float4 *>(out + 4 * q) = r;
    }
}

}  // namespace
