// az_skip.hip -- the skip-connection front of the detection head (models/COCO/VGG16_skip/frcnn/test_fc.prototxt):
// roi_pool3/4/5 (Caffe ROIPooling 7x7 of conv3_3 / conv4_3 / conv5_3, each at its own spatial_scale and map size),
// roi_norm3/4/5 (GRN: y[c] = x[c] / sqrt(sum_c x[c]^2 + eps), per roi, bin and source), concat5, scale5 (x gain) and
// conv_pool5 + relu_pool (1x1 convolution sumC -> Cout with bias).  pool5 is [roi][bin][C] in HBM (k_roi_pool, az_head.hip;
// W6's columns are permuted to match), so the convolution is ONE plain GEMM whose rows are (roi, bin): its result, bias and
// ReLU applied as it is stored, IS the pool5 the unchanged fc6 ... cls_prob / bbox_pred chain reads.
//   k_skip_pool_norm  one workgroup per (roi, bin, source): window maximum per channel, sum of squares, scaled store into
//                     the row-major `cat` [rows][sumC].  The entry works out the bin's window (roi_window, bin_range:
//                     az_solver_dev.h); the body is skip_pool_grn<false> (az_skip_dev.h), which the training front's
//                     k_skip_train_pool (az_skip_train.hip) instantiates with the arg-max
//   k_skip_conv       pool5[rows][Cout] = relu(cat . Wp^T + bp) on the fp32 matrix cores: the trainer's 128 x 128 tile
//                     (tile_fp32 / tile_store, az_solver_dev.h: k_solver_gemm form 0's own code) with the row count read from
//                     the device, the whole K in one pass and the bias / ReLU store
// `cat` holds AZ_SKIP_CHUNK rois (49 x sumC x 4 B each: 251 KB at the VGG16 sizes); both kernels run once per chunk over
// the host-known bound on the row count, and rows past the device-side count leave at once.
// skip_front_check, what az_load_skip_front, az_det_solver_attach_skip and az_skip_pool_bwd_unit refuse in a front's
// description, is defined here.
#include "az_skip_dev.h"

namespace {

// Row `blockIdx.x` of the chunk = bin p of roi roi0 + blockIdx.x / 49; source src0 + blockIdx.y, at its own scale and map size.
__global__ void __launch_bounds__(256) k_skip_pool_norm(SkipSrcs a, int src0, const float *__restrict__ urois, const int *Uptr,
                                                        int roi0, int normalise, double gain, double eps,
                                                        float *__restrict__ cat)
{
    const int row = blockIdx.x, u = roi0 + row / 49, p = row % 49;
    if (u >= *Uptr) return;
    const int s = src0 + blockIdx.y;
    const RoiWindow w = roi_window(urois + 5 * (size_t)u, a.scale[s]);
    const int ph = p / 7, pw = p - ph * 7;
    int hs, he, ws, we;
    bin_range(ph, w.bh, w.rsh, a.H[s], &hs, &he);
    bin_range(pw, w.bw, w.rsw, a.W[s], &ws, &we);
    skip_pool_grn<false>(a.map[s], a.C[s], a.H[s], a.W[s], 1, hs, he, ws, we, cat + (size_t)row * a.sumC + a.off[s], nullptr, nullptr,
                         gain, eps, normalise);
}

// what k_skip_conv does with an output (tile_store's functor): the column's bias, read once per column, and the ReLU
struct BiasRelu {
    const float *bias; float *D; int N;
    __device__ __forceinline__ float column(int j) const { return bias[j]; }
    __device__ __forceinline__ void operator()(int i, int j, float v, float bj) const
    {
        const float y = v + bj;
        D[(long long)i * N + j] = y > 0.0f ? y : 0.0f;
    }
};

// D[i][j] = relu(sum_k A[i][k] * B[j][k] + bias[j]), i < M, j < N: k_solver_gemm<true, true>'s tile and k order (ascending:
// bitwise an fmaf chain per output, whatever the tile) with M = the rows of this chunk that exist on the device --
// min(*Uptr * 49 - row0, cap) (Uptr NULL: cap) -- and no split of K: 14 700 x 512 outputs are 460 tiles already.
__global__ void __launch_bounds__(256) k_skip_conv(const float *__restrict__ A, const float *__restrict__ B,
                                                   const float *__restrict__ bias, float *__restrict__ D, const int *Uptr,
                                                   int row0, int cap, int N, int K)
{
    int M = cap;
    if (Uptr) { const long long left = (long long)*Uptr * 49 - row0; M = left < cap ? (int)(left < 0 ? 0 : left) : cap; }
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * GT, i0 = blockIdx.y * GT;
    if (i0 >= M) return;
    az_f32x16 acc[2][2];
    tile_fp32<true, true>(A, (long long)K, 1LL, B, (long long)K, 1LL, i0, M, j0, N, 0, K, tid, acc);
    tile_store(acc, tid, i0, M, j0, N, BiasRelu{bias, D, N});
}

// rois per pass of the front: what `cat` holds (a context limited to fewer regions never needs more)
int skip_chunk(const az_ctx *c) { return c->maxR < AZ_SKIP_CHUNK ? c->maxR : AZ_SKIP_CHUNK; }

// pool (+ norm) of the rois [roi0, roi0 + n) into cat; with every launch group timed, one launch per source
void launch_pool_norm(az_ctx *c, const int *Uptr, int roi0, int n, int normalise)
{
    const az_ctx::SkipFront &k = c->skip;
    // (one image, channel-last; the builder takes the trainer ABI's untyped map pointers)
    const SkipSrcs a = skip_srcs(k.n, k.C, k.H, k.W, (const void *const *)k.maps, /* N */ 1, /* cl */ 1, k.scale);
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

int skip_front_check(az_ctx *c, const std::string &who, int n_src, const int *Cs, const float *scales, double gain, double eps,
                     long long *sumC_out)
{
    if (n_src < 1 || n_src > AZ_SKIP_MAX_SRC || !Cs || !scales) return fail(c, AZ_ERR_INVALID, who + ": 1 to 3 sources; no null pointer");
    long long sumC = 0;
    for (int i = 0; i < n_src; ++i) {
        if (Cs[i] <= 0 || (Cs[i] & 3)) return fail(c, AZ_ERR_INVALID, who + ": channel counts are positive multiples of 4");
        if (!(scales[i] > 0.0f) || !std::isfinite(scales[i])) return fail(c, AZ_ERR_INVALID, who + ": every spatial_scale must be positive and finite");
        sumC += Cs[i];
    }
    if (sumC > AZ_SKIP_MAX_SUMC) return fail(c, AZ_ERR_INVALID, who + ": more than AZ_SKIP_MAX_SUMC channels in all");
    if (!std::isfinite(gain) || !(eps >= 0.0) || !std::isfinite(eps)) return fail(c, AZ_ERR_INVALID, who + ": gain finite, eps >= 0");
    *sumC_out = sumC;
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
    if (!Wp || !bp) return fail(c, AZ_ERR_INVALID, "az_load_skip_front: 1 to 3 sources; no null pointer");
    long long sumC = 0;
    int rc = skip_front_check(c, "az_load_skip_front", n_src, Cs, spatial_scales, gain, eps, &sumC);
    if (rc != AZ_OK) return rc;
    if (!c->det_loaded) return fail(c, AZ_ERR_STATE, "az_load_skip_front: az_load_det_head has not been called");
    if (c->gemm_parts) return fail(c, AZ_ERR_STATE, "az_load_skip_front: fp32 only (the 16-bit-term GEMM modes are not supported)");
    if (Cout != c->d.C) return fail(c, AZ_ERR_INVALID, "az_load_skip_front: Cout differs from the detection head's C");
    HIPCHK(c, hipSetDevice(c->device));
    join_s2(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // (the new front's buffers first: an error leaves the front loaded before in place)
    az_ctx::SkipFront nk;
    float *&nW = nk.Wp, *&nb = nk.bp;
    const size_t wn = (size_t)Cout * sumC, catn = (size_t)skip_chunk(c) * 49 * sumC;
    if (nk.own.alloc(&nW, wn) != hipSuccess || nk.own.alloc(&nb, (size_t)Cout) != hipSuccess || nk.own.alloc(&nk.cat, catn) != hipSuccess ||
        hipMemcpy(nW, Wp, wn * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(nb, bp, (size_t)Cout * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, AZ_ERR_HIP, "az_load_skip_front: device memory");
    }
    az_ctx::SkipFront &k = c->skip = std::move(nk);
    k.n = n_src; k.sumC = (int)sumC; k.Cout = Cout; k.gain = gain; k.eps = eps;
    for (int i = 0; i < n_src; ++i) { k.C[i] = Cs[i]; k.scale[i] = spatial_scales[i]; }
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
