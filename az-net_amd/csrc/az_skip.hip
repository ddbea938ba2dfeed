// az_skip.hip -- the skip-connection front of the detection head (models/COCO/VGG16_skip/frcnn/test_fc.prototxt):
// roi_pool3/4/5 (Caffe ROIPooling 7x7 of conv3_3 / conv4_3 / conv5_3, each at its own spatial_scale and map size),
// roi_norm3/4/5 (GRN: y[c] = x[c] / sqrt(sum_c x[c]^2 + eps), per roi, bin and source), concat5, scale5 (x gain) and
// conv_pool5 + relu_pool (1x1 convolution sumC -> Cout with bias).  pool5 is [roi][bin][C] in HBM (k_roi_pool, az_head.hip;
// W6's columns are permuted to match), so the convolution is ONE plain GEMM whose rows are (roi, bin): its result, bias and
// ReLU applied as it is stored, IS the pool5 the unchanged fc6 ... cls_prob / bbox_pred chain reads.
//   k_skip_pool_norm  one workgroup per (roi, bin, source): window maximum per channel, sum of squares, scaled store into
//                     the row-major `cat` [rows][sumC]
//   k_skip_conv       pool5[rows][Cout] = relu(cat . Wp^T + bp) on the fp32 matrix cores: the trainer's 128 x 128 tile
//                     (k_solver_gemm form 0, az_trainer.hip; gemm_stage, az_solver_dev.h) with the row count read from the device, the whole K in one
//                     pass and the bias / ReLU epilogue
// `cat` holds AZ_SKIP_CHUNK rois (49 x sumC x 4 B each: 251 KB at the VGG16 sizes); both kernels run once per chunk over
// the host-known bound on the row count, and rows past the device-side count leave at once.
#include "az_solver_dev.h"

namespace {

struct SkipSrcs {
    const float *map[AZ_SKIP_MAX_SRC];
    int C[AZ_SKIP_MAX_SRC], H[AZ_SKIP_MAX_SRC], W[AZ_SKIP_MAX_SRC], off[AZ_SKIP_MAX_SRC];
    float scale[AZ_SKIP_MAX_SRC];
    int sumC;
};

// Row `blockIdx.x` of the chunk = bin p of roi roi0 + blockIdx.x / 49; source src0 + blockIdx.y.  The window is
// k_roi_pool's (az_head.hip): the same roundf / floorf / ceilf expressions (bin_range, az_solver_dev.h) with this source's
// scale and map size; max() is exact, so how the cells are dealt to the threads does not show in a bit.  A lane holds
// four consecutive channels (the maps are channel-last); with fewer than 256 channel quads the workgroup splits the
// window's cells over 256 / quads groups and the partial maxima meet in LDS.
__global__ void __launch_bounds__(256) k_skip_pool_norm(SkipSrcs a, int src0, const float *__restrict__ urois, const int *Uptr,
                                                        int roi0, int normalise, double gain, double eps,
                                                        float *__restrict__ cat)
{
    __shared__ float4 smax[256];
    __shared__ double sred[4];
    const int row = blockIdx.x, u = roi0 + row / 49, p = row % 49;
    if (u >= *Uptr) return;
    const int s = src0 + blockIdx.y, tid = threadIdx.x;
    const int C = a.C[s], fH = a.H[s], fW = a.W[s], nq = C >> 2;
    const float ss_ = a.scale[s];
    const float *roi = urois + 5 * (size_t)u;
    const int rsw = (int)roundf(roi[1] * ss_), rsh = (int)roundf(roi[2] * ss_);
    const int rew = (int)roundf(roi[3] * ss_), reh = (int)roundf(roi[4] * ss_);
    int rh = reh - rsh + 1; rh = rh < 1 ? 1 : rh;
    int rw = rew - rsw + 1; rw = rw < 1 ? 1 : rw;
    const int ph = p / 7, pw = p - ph * 7;
    int hs, he, ws, we;
    bin_range(ph, (float)rh / 7.0f, rsh, fH, &hs, &he);
    bin_range(pw, (float)rw / 7.0f, rsw, fW, &ws, &we);
    const bool empty = (he <= hs) || (we <= ws);
    const int nw = we - ws, ncell = empty ? 0 : (he - hs) * nw;
    const float *fm = a.map[s];
    float *out = cat + (size_t)row * a.sumC + a.off[s];
    double ssq = 0.0;
    for (int q0 = 0; q0 < nq; q0 += 256) {
        const int nqb = min(256, nq - q0), G = 256 / nqb;
        const int g = tid / nqb, q = tid - g * nqb;
        float4 m = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX);
        if (g < G)
            for (int i = g; i < ncell; i += G) {
                const int hh = hs + i / nw, ww = ws + i % nw;
                const float4 v = *reinterpret_cast<const float4 *>(fm + ((size_t)hh * fW + ww) * C + 4 * (q0 + q));
                m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y;
                m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w;
            }
        smax[tid] = m;
        __syncthreads();
        if (tid < nqb) {
            float4 r = smax[tid];
            for (int g2 = 1; g2 < G; ++g2) {
                const float4 v = smax[g2 * nqb + tid];
                r.x = v.x > r.x ? v.x : r.x; r.y = v.y > r.y ? v.y : r.y;
                r.z = v.z > r.z ? v.z : r.z; r.w = v.w > r.w ? v.w : r.w;
            }
            if (empty) r = make_float4(0.f, 0.f, 0.f, 0.f);            // an empty bin pools to 0 (Caffe)
            *reinterpret_cast<float4 *>(out + 4 * (q0 + tid)) = r;
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
    for (int q = tid; q < nq; q += 256) {                              // (the quads this thread stored itself)
        float4 r = *reinterpret_cast<float4 *>(out + 4 * q);
        r.x = (float)((double)r.x * f); r.y = (float)((double)r.y * f);
        r.z = (float)((double)r.z * f); r.w = (float)((double)r.w * f);
        *reinterpret_cast<float4 *>(out + 4 * q) = r;
    }
}

// D[i][j] = relu(sum_k A[i][k] * B[j][k] + bias[j]), i < M, j < N: k_solver_gemm<true, true>'s tile and k order (ascending:
// bitwise an fmaf chain per output, whatever the tile) with M = the rows of this chunk that exist on the device --
// min(*Uptr * 49 - row0, cap) (Uptr NULL: cap) -- and no split of K: 14 700 x 512 outputs are 460 tiles already.
__global__ void __launch_bounds__(256) k_skip_conv(const float *__restrict__ A, const float *__restrict__ B,
                                                   const float *__restrict__ bias, float *__restrict__ D, const int *Uptr,
                                                   int row0, int cap, int N, int K)
{
    __shared__ float sA[GK * GLD];
    __shared__ float sB[GK * GLD];
    int M = cap;
    if (Uptr) { const long long left = (long long)*Uptr * 49 - row0; M = left < cap ? (int)(left < 0 ? 0 : left) : cap; }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * GT, i0 = blockIdx.y * GT;
    if (i0 >= M) return;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    az_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.0f;
    const int lr = lane & 31, lk = lane >> 5;
    for (int k0 = 0; k0 < K; k0 += GK) {
        __syncthreads();
        gemm_stage<true>(A, (long long)K, 1LL, i0, M, k0, K, sA, tid);
        gemm_stage<true>(B, (long long)K, 1LL, j0, N, k0, K, sB, tid);
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
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int j = j0 + wj + 32 * b + lr;
            const float bj = j < N ? bias[j] : 0.0f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = i0 + wi + 32 * a + (v & 3) + 8 * (v >> 2) + 4 * lk;
                if (i < M && j < N) {
                    const float y = acc[a][b][v] + bj;
                    D[(long long)i * N + j] = y > 0.0f ? y : 0.0f;
                }
            }
        }
}

SkipSrcs skip_srcs(const az_ctx *c)
{
    const az_ctx::SkipFront &k = c->skip;
    SkipSrcs a{};
    int off = 0;
    for (int i = 0; i < k.n; ++i) {
        a.map[i] = k.maps[i]; a.C[i] = k.C[i]; a.H[i] = k.H[i]; a.W[i] = k.W[i]; a.off[i] = off; a.scale[i] = k.scale[i];
        off += k.C[i];
    }
    a.sumC = k.sumC;
    return a;
}

// rois per pass of the front: what `cat` holds (a context limited to fewer regions never needs more)
int skip_chunk(const az_ctx *c) { return c->maxR < AZ_SKIP_CHUNK ? c->maxR : AZ_SKIP_CHUNK; }

// pool (+ norm) of the rois [roi0, roi0 + n) into cat; with every launch group timed, one launch per source
void launch_pool_norm(az_ctx *c, const int *Uptr, int roi0, int n, int normalise)
{
    const az_ctx::SkipFront &k = c->skip;
    const SkipSrcs a = skip_srcs(c);
    if (c->profiling & 2) {
        static const char *names[AZ_SKIP_MAX_SRC] = {"skip_pool_norm_0", "skip_pool_norm_1", "skip_pool_norm_2"};
        for (int s = 0; s < k.n; ++s) {
            Timed t(c, names[s], 0);
            hipLaunchKernelGGL(k_skip_pool_norm, dim3(n * 49, 1), dim3(256), 0, c->stream, a, s, c->urois, Uptr, roi0,
                               normalise, k.gain, k.eps, k.cat);
        }
        return;
    }
    hipLaunchKernelGGL(k_skip_pool_norm, dim3(n * 49, k.n), dim3(256), 0, c->stream, a, 0, c->urois, Uptr, roi0, normalise,
                       k.gain, k.eps, k.cat);
}

void launch_conv(az_ctx *c, const int *Uptr, int row0, int rows, float *out)
{
    const az_ctx::SkipFront &k = c->skip;
    Timed t(c, "skip_conv_gemm", 0, 1);
    hipLaunchKernelGGL(k_skip_conv, dim3((k.Cout + GT - 1) / GT, (rows + GT - 1) / GT), dim3(256), 0, c->stream, k.cat, k.Wp,
                       k.bp, out, Uptr, row0, rows, k.Cout, k.sumC);
}

}  // namespace

int skip_check(az_ctx *c, const char *who, bool need_maps)
{
    if (!c) return AZ_ERR_INVALID;
    const std::string w(who);
    if (!c->det_loaded) return fail(c, AZ_ERR_STATE, w + ": az_load_det_head has not been called");
    if (!c->skip.loaded) return fail(c, AZ_ERR_STATE, w + ": az_load_skip_front has not been called");
    if (c->gemm_parts) return fail(c, AZ_ERR_STATE, w + ": fp32 only (the 16-bit-term GEMM modes are not supported)");
    if (c->pyr_S) return fail(c, AZ_ERR_STATE, w + ": the skip front does not read a pyramid set");
    if (need_maps && !c->skip.maps_set) return fail(c, AZ_ERR_STATE, w + ": no maps set (az_set_skip_maps_dev_nhwc)");
    join_s2(c);
    return AZ_OK;
}

void skip_front_launch(az_ctx *c, const int *Uptr, int rows_bound)
{
    const int chunk = skip_chunk(c);
    for (int roi0 = 0; roi0 < rows_bound; roi0 += chunk) {
        const int n = rows_bound - roi0 < chunk ? rows_bound - roi0 : chunk;
        launch_pool_norm(c, Uptr, roi0, n, 1);
        launch_conv(c, Uptr, roi0 * 49, n * 49, c->pool5 + (size_t)roi0 * 49 * c->skip.Cout);
    }
}

void skip_free(az_ctx *c)
{
    for (void *p : {(void *)c->skip.Wp, (void *)c->skip.bp, (void *)c->skip.cat}) if (p) hipFree(p);
    c->skip = az_ctx::SkipFront();
}

// az_skip_pool past its argument checks (the rois staged in c->urois, their count in cnt->U[0])
int skip_pool_unit(az_ctx *c, int R, int normalise, float *out)
{
    const int chunk = skip_chunk(c);
    const size_t sumC = (size_t)c->skip.sumC;
    for (int roi0 = 0; roi0 < R; roi0 += chunk) {
        const int n = R - roi0 < chunk ? R - roi0 : chunk;
        launch_pool_norm(c, &c->cnt->U[0], roi0, n, normalise);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpy(out + (size_t)roi0 * 49 * sumC, c->skip.cat, (size_t)n * 49 * sumC * 4, hipMemcpyDeviceToHost));
    }
    return AZ_OK;
}

extern "C" {

int az_load_skip_front(az_ctx *c, int n_src, const int *Cs, const float *spatial_scales, double gain, double eps, int Cout,
                       const float *Wp, const float *bp)
{
    if (!c) return AZ_ERR_INVALID;
    if (n_src < 1 || n_src > AZ_SKIP_MAX_SRC || !Cs || !spatial_scales || !Wp || !bp)
        return fail(c, AZ_ERR_INVALID, "az_load_skip_front: 1 to 3 sources; no null pointer");
    long long sumC = 0;
    for (int i = 0; i < n_src; ++i) {
        if (Cs[i] <= 0 || (Cs[i] & 3)) return fail(c, AZ_ERR_INVALID, "az_load_skip_front: channel counts are positive multiples of 4");
        if (!(spatial_scales[i] > 0.0f) || !std::isfinite(spatial_scales[i]))
            return fail(c, AZ_ERR_INVALID, "az_load_skip_front: every spatial_scale must be positive and finite");
        sumC += Cs[i];
    }
    if (sumC > AZ_SKIP_MAX_SUMC) return fail(c, AZ_ERR_INVALID, "az_load_skip_front: more than AZ_SKIP_MAX_SUMC channels in all");
    if (!std::isfinite(gain) || !(eps >= 0.0) || !std::isfinite(eps))
        return fail(c, AZ_ERR_INVALID, "az_load_skip_front: gain finite, eps >= 0");
    if (!c->det_loaded) return fail(c, AZ_ERR_STATE, "az_load_skip_front: az_load_det_head has not been called");
    if (c->gemm_parts) return fail(c, AZ_ERR_STATE, "az_load_skip_front: fp32 only (the 16-bit-term GEMM modes are not supported)");
    if (Cout != c->d.C) return fail(c, AZ_ERR_INVALID, "az_load_skip_front: Cout differs from the detection head's C");
    HIPCHK(c, hipSetDevice(c->device));
    join_s2(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // (the new front's buffers first: an error leaves the front loaded before in place)
    float *nW = nullptr, *nb = nullptr, *ncat = nullptr;
    const size_t wn = (size_t)Cout * sumC, catn = (size_t)skip_chunk(c) * 49 * sumC;
    if (hipMalloc((void **)&nW, wn * 4 + 256) != hipSuccess || hipMalloc((void **)&nb, (size_t)Cout * 4 + 256) != hipSuccess ||
        hipMalloc((void **)&ncat, catn * 4 + 256) != hipSuccess ||
        hipMemcpy(nW, Wp, wn * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(nb, bp, (size_t)Cout * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        for (void *p : {(void *)nW, (void *)nb, (void *)ncat}) if (p) hipFree(p);
        return fail(c, AZ_ERR_HIP, "az_load_skip_front: device memory");
    }
    skip_free(c);
    az_ctx::SkipFront &k = c->skip;
    k.n = n_src; k.sumC = (int)sumC; k.Cout = Cout; k.gain = gain; k.eps = eps;
    for (int i = 0; i < n_src; ++i) { k.C[i] = Cs[i]; k.scale[i] = spatial_scales[i]; }
    k.Wp = nW; k.bp = nb; k.cat = ncat;
    k.loaded = true;
    return AZ_OK;
}

int az_set_skip_maps_dev_nhwc(az_ctx *c, int n_src, const float *const *maps, const int *Cs, const int *Hs, const int *Ws)
{
    if (!c) return AZ_ERR_INVALID;
    if (!c->skip.loaded) return fail(c, AZ_ERR_STATE, "az_set_skip_maps_dev_nhwc: az_load_skip_front has not been called");
    if (!maps || !Cs || !Hs || !Ws) return fail(c, AZ_ERR_INVALID, "az_set_skip_maps_dev_nhwc: null pointer");
    if (n_src != c->skip.n) return fail(c, AZ_ERR_INVALID, "az_set_skip_maps_dev_nhwc: the loaded front has another number of sources");
    for (int i = 0; i < n_src; ++i) {
        if (!maps[i] || Hs[i] <= 0 || Ws[i] <= 0) return fail(c, AZ_ERR_INVALID, "az_set_skip_maps_dev_nhwc: null map or empty size");
        if (Cs[i] != c->skip.C[i]) return fail(c, AZ_ERR_INVALID, "az_set_skip_maps_dev_nhwc: channel counts differ from the loaded front's");
    }
    join_s2(c);
    for (int i = 0; i < n_src; ++i) { c->skip.maps[i] = maps[i]; c->skip.H[i] = Hs[i]; c->skip.W[i] = Ws[i]; }
    c->skip.maps_set = true;
    c->pyr_S = 0;            // these maps replace a pyramid set the context held (the skip entries refuse one)
    // the last source is also the context's ordinary map (as az_set_feature_map_dev_nhwc sets it) when it has the heads'
    // channel count: the AZ head on a shared context goes on reading conv5_3
    if (Cs[n_src - 1] == c->d.C) { c->feat = maps[n_src - 1]; c->d.H = Hs[n_src - 1]; c->d.W = Ws[n_src - 1]; }
    return AZ_OK;
}

int az_skip_conv(az_ctx *c, const float *cat_host, int rows, float *out)
{
    int rc = skip_check(c, "az_skip_conv", false);
    if (rc) return rc;
    if (rows < 0 || (rows && (!cat_host || !out))) return fail(c, AZ_ERR_INVALID, "az_skip_conv: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const az_ctx::SkipFront &k = c->skip;
    const int cap = skip_chunk(c) * 49;
    for (int r0 = 0; r0 < rows; r0 += cap) {
        const int n = rows - r0 < cap ? rows - r0 : cap;
        HIPCHK(c, hipMemcpyAsync(k.cat, cat_host + (size_t)r0 * k.sumC, (size_t)n * k.sumC * 4, hipMemcpyHostToDevice, c->stream));
        launch_conv(c, nullptr, 0, n, c->pool5);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpy(out + (size_t)r0 * k.Cout, c->pool5, (size_t)n * k.Cout * 4, hipMemcpyDeviceToHost));
    }
    return AZ_OK;
}

}  // extern "C"
