// az_skip_train.hip -- the skip-connection front of the detection net in TRAIN phase (models/COCO/VGG16_skip/frcnn/finetune
// and frozen train nets): roi_pool3/4/5 with arg-max, roi_norm3/4/5 (GRN), concat5, scale5, conv_pool5 + relu_pool in front
// of the detection trainer's fc6 .. losses (az_det_solver.hip), and their backward down to the three maps.
//   k_skip_train_pool    one workgroup per (roi, bin, source): k_skip_pool_norm's body (skip_pool_grn, az_skip_dev.h: one
//                        function, instantiated with the arg-max here) on a batch of N maps in either memory format; it
//                        also stores the arg-max cell of every channel (the first maximum in row-major window order) and
//                        the row's factor f = gain / sqrt(ss + eps).  The entry takes its window from geo
//   conv_pool5 forward   cat . Wp^T: k_solver_gemm form 0, rows (roi, bin); k_skip_finish_t sums the slabs in slab order, adds
//                        the bias, applies the ReLU and stores Caffe-flattened: pool5[r][j * 49 + p]
//   k_skip_dy            d_y[(r, p)][j] = d_pool5[r][j * 49 + p] * (pool5 > 0): gate and transpose in one pass
//   g_Wp = d_y^T . cat (form 2, split K), g_bp = column sums in row order, d_cat = d_y . Wp (form 1)
//   k_skip_grn_bwd       per (row, source): d_raw[c] = f * (d_cat[c] - y[c] * (sum_c y[c] d_cat[c]) / gain^2), the sum in f64
//                        over a fixed tree.  (y = f x, so x * (sum_c x dy) / (ss + eps) == y * (sum_c y dy) / gain^2: `cat`
//                        and f are enough, the raw maxima are not kept.)
//   pool backward        the trainers' gather (k_solver_roi_pool_bwd through tr_pool_gather, az_trainer.hip) with this
//                        layout's strides, one launch per map: one thread per map cell GATHERS the rois of its image in row
//                        order, the candidate bins in bin order, decided by the stored arg-max.  No floating-point atomics
//                        anywhere: the same step from the same state gives the same bits.
// cat, arg-max, d_cat and d_raw are [rows][sumC], the arg-max beside the value it belongs to: a channel-last map's
// neighbouring threads (channels) read neighbouring words of it in the gather.
#include "az_det_solver.h"
#include "az_skip_dev.h"

namespace {

// Row blockIdx.x = bin p of roi r = blockIdx.x / 49; source src0 + blockIdx.y.  geo [n][R][8] is k_solver_roi_geo's record at
// the source's scale: the roi's image and its window.
__global__ void __launch_bounds__(256) k_skip_train_pool(SkipSrcs a, int src0, const int *__restrict__ geo, int R, int normalise,
                                                         double gain, double eps, float *__restrict__ cat,
                                                         int *__restrict__ arg, double *__restrict__ fac)
{
    const int row = blockIdx.x, r = row / 49, p = row % 49;
    const int s = src0 + blockIdx.y;
    const int C = a.C[s], fH = a.H[s], fW = a.W[s];
    const int *g = geo + ((size_t)s * R + r) * 8;
    const int ph = p / 7, pw = p - ph * 7;
    int hs, he, ws, we;
    bin_range(ph, __int_as_float(g[5]), g[2], fH, &hs, &he);
    bin_range(pw, __int_as_float(g[6]), g[1], fW, &ws, &we);
    const size_t o0 = (size_t)row * a.sumC + a.off[s];
    skip_pool_grn<true>(a.map[s] + (size_t)g[0] * C * fH * fW, C, fH, fW, a.cl, hs, he, ws, we, cat + o0, arg + o0,
                        fac + (size_t)row * a.n + s, gain, eps, normalise);
}

// pool5[r][j * 49 + p] = relu(sum over the slabs in slab order of part[(r, p)][j] + bias[j])
__global__ void __launch_bounds__(256) k_skip_finish_t(const float *__restrict__ part, int S, long long slab,
                                                       const float *__restrict__ bias, long long MN, int N,
                                                       float *__restrict__ pool5)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= MN) return;
    float s = part[e];
    for (int q = 1; q < S; ++q) s += part[(long long)q * slab + e];
    const int j = (int)(e % N);
    const long long row = e / N;
    s += bias[j];
    pool5[(row / 49) * 49 * N + (long long)j * 49 + row % 49] = s > 0.0f ? s : 0.0f;
}

__global__ void __launch_bounds__(256) k_skip_dy(const float *__restrict__ dpool, const float *__restrict__ pool5, long long MN,
                                                 int N, float *__restrict__ dy)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= MN) return;
    const int j = (int)(e % N);
    const long long row = e / N;
    const long long o = (row / 49) * 49 * N + (long long)j * 49 + row % 49;
    dy[e] = pool5[o] > 0.0f ? dpool[o] : 0.0f;
}

// GRN + scale backward of row blockIdx.x, source blockIdx.y
__global__ void __launch_bounds__(256) k_skip_grn_bwd(const float *__restrict__ cat, const float *__restrict__ dcat,
                                                      const double *__restrict__ fac, SkipSrcs a, double inv_gain2,
                                                      float *__restrict__ draw)
{
    __shared__ double sred[4];
    const int row = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, C = a.C[s];
    const size_t o0 = (size_t)row * a.sumC + a.off[s];
    const float *y = cat + o0, *dy = dcat + o0;
    double acc = 0.0;
    for (int c = tid; c < C; c += 256) acc += (double)y[c] * (double)dy[c];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((tid & 63) == 0) sred[tid >> 6] = acc;
    __syncthreads();
    const double k = (((sred[0] + sred[1]) + sred[2]) + sred[3]) * inv_gain2;
    const double f = fac[(size_t)row * a.n + s];
    for (int c = tid; c < C; c += 256) draw[o0 + c] = (float)(f * ((double)dy[c] - (double)y[c] * k));
}

// Caffe's xavier filler (fan_in): uniform in +-a from the 24 high bits of the element's word
__global__ void __launch_bounds__(256) k_solver_fill_uniform(float *__restrict__ w, long long n, float a, unsigned long long key)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const unsigned long long b = az_elem_bits(key, (unsigned long long)e);
        const float u = ((float)(unsigned)(b >> 40) + 0.5f) * (1.0f / 16777216.0f);
        w[e] = a * (2.0f * u - 1.0f);
    }
}

int check_maps(az_ctx *c, const std::string &who, int n_src, const int *Cs, const void *const *maps, const int *Hs, const int *Ws, int N)
{
    if (!maps || !Cs || !Hs || !Ws) return fail(c, AZ_ERR_INVALID, who + ": null pointer");
    if (N < 1) return fail(c, AZ_ERR_INVALID, who + ": bad map shape");
    for (int i = 0; i < n_src; ++i) {
        if (!maps[i]) return fail(c, AZ_ERR_INVALID, who + ": null map");
        if (Hs[i] < 1 || Ws[i] < 1 || (long long)Hs[i] * Ws[i] > 0x3fffffff || (long long)N * Cs[i] * Hs[i] * Ws[i] > (1LL << 38))
            return fail(c, AZ_ERR_INVALID, who + ": bad map shape");
    }
    return AZ_OK;
}

void launch_geo(hipStream_t st, const float *rois_dev, int R, int n, const float *scales, int *geo)
{
    for (int i = 0; i < n; ++i) tr_roi_geo(st, rois_dev, R, scales[i], geo + (size_t)i * R * 8);
}

// d map of source i: the trainers' gather on the [rows][sumC] layout (geo: this source's records)
void launch_gather(az_ctx *c, const SkipSrcs &a, int i, const float *draw, const int *arg, const int *geo, int R, float *dmap)
{
    static const char *names[AZ_SKIP_MAX_SRC] = {"skip_pool_bwd_0", "skip_pool_bwd_1", "skip_pool_bwd_2"};
    const MapView m{a.N, a.C[i], a.H[i], a.W[i], a.cl};
    tr_pool_gather(c, names[i], draw, arg, geo + (size_t)i * R * 8, R, m, PoolStrides{49 * a.sumC, 1, a.sumC, a.off[i]}, dmap);
}

int skip_step_check(az_det_solver *s, const std::string &who, int n_src, const int *Cs, const void *const *maps, const int *Hs,
                    const int *Ws, int N, const float *rois, int R)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    if (!s->sk.attached) return fail(c, AZ_ERR_STATE, who + ": no skip front attached (az_det_solver_attach_skip)");
    if (n_src != s->sk.n) return fail(c, AZ_ERR_INVALID, who + ": the attached front has another number of sources");
    if (!Cs) return fail(c, AZ_ERR_INVALID, who + ": null pointer");
    for (int i = 0; i < n_src; ++i) if (Cs[i] != s->sk.C[i]) return fail(c, AZ_ERR_INVALID, who + ": channel counts differ from the attached front's");
    int rc = check_maps(c, who, n_src, Cs, maps, Hs, Ws, N);
    if (rc != AZ_OK) return rc;
    if (!rois) return fail(c, AZ_ERR_INVALID, who + ": null rois");
    return tr_check_rois(s, N, rois, R, who);
}

// roi_pool* .. relu_pool into s->pool5, then the head
int skip_forward(az_det_solver *s, const SkipSrcs &a, const float *rois, int R, bool train, unsigned long long seed, unsigned long long iter)
{
    az_ctx *c = s->c;
    az_det_solver::Skip &k = s->sk;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(s->rois, rois, (size_t)R * 5 * sizeof(float), hipMemcpyHostToDevice, st));
    const int rows = R * 49, Cout = s->C;
    { Timed t(c, "skip_pool_argmax", 0);
      launch_geo(st, s->rois, R, k.n, k.scale, k.geo);
      hipLaunchKernelGGL(k_skip_train_pool, dim3(rows, k.n), dim3(256), 0, st, a, 0, k.geo, R, 1, k.gain, k.eps, k.cat, k.arg, k.fac); }
    int S, Kc;
    pick_split(rows, Cout, k.sumC, &S, &Kc);
    const long long slab = (long long)rows * Cout;
    { Timed t(c, "conv_pool5_fwd", 0, 1); launch_gemm(st, 0, k.cat, s->w[D_WP], s->part, slab, rows, Cout, k.sumC, S, Kc, 0, s->prec); }
    { Timed t(c, "conv_pool5_finish", 0);
      hipLaunchKernelGGL(k_skip_finish_t, dim3(grid_for(slab)), dim3(256), 0, st, s->part, S, slab, s->w[D_BP], slab, Cout, s->pool5); }
    det_head_forward(s, R, train, seed, iter);
    s->R = R; s->N = a.N; s->H = a.H[k.n - 1]; s->W = a.W[k.n - 1];
    k.rows = rows; k.has_dcat = 0;
    return AZ_OK;
}

}  // namespace

int skip_pass_check(az_det_solver *s, const std::string &who, int n_src, const int *Cs, const void *const *maps, const int *Hs,
                    const int *Ws, int N, const float *rois, int R)
{
    return skip_step_check(s, who, n_src, Cs, maps, Hs, Ws, N, rois, R);
}

int skip_test_forward(az_det_solver *s, const void *const *maps_dev, const int *Hs, const int *Ws, int N, int channels_last,
                      const float *rois, int R)
{
    const SkipSrcs a = skip_srcs(s->sk.n, s->sk.C, Hs, Ws, maps_dev, N, channels_last);
    return skip_forward(s, a, rois, R, false, 0, 0);
}

bool skip_train_fetch(az_det_solver *s, const std::string &nm, const void **src, size_t *bytes)
{
    const az_det_solver::Skip &k = s->sk;
    if (!k.attached) return false;
    const size_t rows = (size_t)k.rows, big = rows * k.sumC * 4;
    struct Ent { const char *n; const void *p; size_t b; };
    const Ent tab[] = {{"cat", k.cat, big}, {"skip_argmax", k.arg, big}, {"skip_factor", k.fac, rows * k.n * 8},
                       {"d_y", k.d_y, rows * s->C * 4}, {"d_cat", k.d_cat, big}, {"d_raw", k.d_raw, big}};
    for (const Ent &e : tab) if (nm == e.n) { *src = e.p; *bytes = e.b; return true; }
    return false;
}

extern "C" {

int az_det_solver_attach_skip(az_det_solver *s, int n_src, const int *Cs, const float *spatial_scales, double gain, double eps,
                              uint64_t seed)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    long long sumC = 0;
    int rc = skip_front_check(c, "az_det_solver_attach_skip", n_src, Cs, spatial_scales, gain, eps, &sumC);
    if (rc != AZ_OK) return rc;
    if (s->sk.attached) return fail(c, AZ_ERR_STATE, "az_det_solver_attach_skip: a front is attached already");
    const long long rows = (long long)s->maxR * 49;
    if (rows * sumC > 0x7fffffffLL) return fail(c, AZ_ERR_INVALID, "az_det_solver_attach_skip: max_rois * 49 * sumC does not fit in 31 bits");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t big = (size_t)(rows * sumC), Cout = (size_t)s->C, wn = Cout * (size_t)sumC;
    // the slabs: a split product never asks for more than az_det_solver_create's floor of 4M floats (pick_split: at most 256
    // tiles of 128 x 128 over all slabs; az_det_solver.hip, part_elems), an unsplit forward for rows x Cout
    const size_t part_need = (size_t)rows * Cout;
    // (everything new is allocated behind `mark` and kept aside: an error releases it and leaves the trainer as it was)
    const size_t mark = s->allocs.mark();
    const size_t pn2[2] = {wn, Cout};
    az_det_solver::Skip k;
    float *part = nullptr;
    rc = tr_alloc_params(s, D_WP, DNALL, pn2);
#define SA(p, n) if (rc == AZ_OK) rc = tr_alloc(s, &k.p, (n))
    SA(geo, (size_t)n_src * s->maxR * 8); SA(arg, big); SA(cat, big); SA(d_y, (size_t)rows * Cout); SA(d_cat, big); SA(d_raw, big);
    SA(fac, (size_t)rows * n_src);
#undef SA
    if (rc == AZ_OK && part_need > s->part_elems) rc = tr_alloc(s, &part, part_need);
    if (rc == AZ_OK) {
        hipLaunchKernelGGL(k_solver_fill_uniform, dim3(grid_for((long long)wn, 8192)), dim3(256), 0, c->stream, s->w[D_WP], (long long)wn,
                           sqrtf(3.0f / (float)sumC), az_layer_key(seed, 0, 16 + D_WP));
        rc = tr_fill_params(s, D_WP, DNALL, nullptr, seed);
    }
    if (rc != AZ_OK) {
        (void)hipGetLastError();
        tr_release(s, mark);
        return fail(c, AZ_ERR_HIP, "az_det_solver_attach_skip: device memory or fill");
    }
    if (part) { s->part = part; s->part_elems = part_need; }         // (the smaller slab buffer stays in allocs until destroy)
    s->np = DNALL;
    k.n = n_src; k.sumC = (int)sumC; k.gain = gain; k.eps = eps;
    int off = 0;
    for (int i = 0; i < n_src; ++i) { k.C[i] = Cs[i]; k.off[i] = off; k.scale[i] = spatial_scales[i]; off += Cs[i]; }
    k.attached = true;
    s->sk = k;
    return AZ_OK;
}

int az_det_solver_load_skip(az_det_solver *s, const float *Wp, const float *bp)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    if (!s->sk.attached) return fail(c, AZ_ERR_STATE, "az_det_solver_load_skip: no skip front attached");
    const float *src[2] = {Wp, bp};
    return tr_load(s, D_WP, DNALL, src);
}

int az_det_solver_load_skip_history(az_det_solver *s, const float *Wp, const float *bp)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    if (!s->sk.attached) return fail(c, AZ_ERR_STATE, "az_det_solver_load_skip_history: no skip front attached");
    const float *src[2] = {Wp, bp};
    return tr_load_history(s, D_WP, DNALL, src);
}

int az_det_solver_read_skip(az_det_solver *s, float *Wp, float *bp)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    if (!s->sk.attached) return fail(c, AZ_ERR_STATE, "az_det_solver_read_skip: no skip front attached");
    float *dst[2] = {Wp, bp};
    return tr_read(s, D_WP, DNALL, dst);
}

int az_det_solver_set_skip_hyper(az_det_solver *s, const float *lr_mult, const float *decay_mult)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    if (!s->sk.attached) return fail(c, AZ_ERR_STATE, "az_det_solver_set_skip_hyper: no skip front attached");
    for (int p = 0; p < 2; ++p)
        if ((lr_mult && !(lr_mult[p] >= 0.0f)) || (decay_mult && !(decay_mult[p] >= 0.0f)))
            return fail(c, AZ_ERR_INVALID, "az_det_solver_set_skip_hyper: negative lr_mult or decay_mult");
    for (int p = 0; p < 2; ++p) {
        if (lr_mult) s->lr_mult[D_WP + p] = lr_mult[p];
        if (decay_mult) s->decay_mult[D_WP + p] = decay_mult[p];
    }
    return AZ_OK;
}

int az_det_solver_step_skip(az_det_solver *s, int n_src, const int *Cs, const void *const *maps_dev, const int *Hs, const int *Ws,
                            int N, int channels_last, const float *rois, int R, const float *labels, const float *bbox_targets,
                            const float *bbox_loss_weights, uint64_t seed, long long iteration, float *losses_out,
                            double *sumsq_out, void *const *dmaps_dev)
{
    int rc = skip_step_check(s, "az_det_solver_step_skip", n_src, Cs, maps_dev, Hs, Ws, N, rois, R);
    if (rc != AZ_OK) return rc;
    az_ctx *c = s->c;
    az_det_solver::Skip &k = s->sk;
    if ((rc = det_stage_targets(s, R, labels, bbox_targets, bbox_loss_weights, iteration, "az_det_solver_step_skip")) != AZ_OK) return rc;
    hipStream_t st = c->stream;
    const SkipSrcs a = skip_srcs(s->sk.n, s->sk.C, Hs, Ws, maps_dev, N, channels_last);
    if ((rc = skip_forward(s, a, rois, R, true, seed, (unsigned long long)iteration)) != AZ_OK) return rc;
    det_head_backward(s, R, true);
    const int rows = R * 49, Cout = s->C;
    { Timed t(c, "relu_pool_bwd", 0);
      hipLaunchKernelGGL(k_skip_dy, dim3(grid_for((long long)rows * Cout)), dim3(256), 0, st, s->dpool, s->pool5, (long long)rows * Cout,
                         Cout, k.d_y); }
    gemm_any(s, "conv_pool5_dw", 2, k.d_y, k.cat, s->g[D_WP], Cout, k.sumC, rows, s->acc);
    { Timed t(c, "bias_grads", 0); tr_colsum(s, k.d_y, rows, Cout, s->g[D_BP], s->acc); }
    bool any = false;
    if (dmaps_dev) for (int i = 0; i < k.n; ++i) any = any || dmaps_dev[i];
    if (any) {
        gemm_any(s, "conv_pool5_dx", 1, k.d_y, s->w[D_WP], k.d_cat, rows, k.sumC, Cout, 0);
        { Timed t(c, "skip_grn_bwd", 0);
          hipLaunchKernelGGL(k_skip_grn_bwd, dim3(rows, k.n), dim3(256), 0, st, k.cat, k.d_cat, k.fac, a,
                             k.gain != 0.0 ? 1.0 / (k.gain * k.gain) : 0.0, k.d_raw); }
        for (int i = 0; i < k.n; ++i)
            if (dmaps_dev[i]) launch_gather(c, a, i, k.d_raw, k.arg, k.geo, R, (float *)dmaps_dev[i]);
        k.has_dcat = 1;
    }
    if ((rc = tr_grad_norm(s, DNALL, 2, losses_out, sumsq_out)) != AZ_OK) return rc;
    s->trained = any ? 2 : 1;
    k.trained = 1;
    return AZ_OK;
}

int az_det_solver_forward_test_skip(az_det_solver *s, int n_src, const int *Cs, const void *const *maps_dev, const int *Hs,
                                    const int *Ws, int N, int channels_last, const float *rois, int R, float *cls_prob,
                                    float *bbox_pred)
{
    int rc = skip_step_check(s, "az_det_solver_forward_test_skip", n_src, Cs, maps_dev, Hs, Ws, N, rois, R);
    if (rc != AZ_OK) return rc;
    az_ctx *c = s->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (!(c->profiling & 4)) clear_events(c);
    const SkipSrcs a = skip_srcs(s->sk.n, s->sk.C, Hs, Ws, maps_dev, N, channels_last);
    if ((rc = skip_forward(s, a, rois, R, false, 0, 0)) != AZ_OK) return rc;
    s->trained = 0; s->sk.trained = 0;
    det_softmax_test(s, R);
    if (cls_prob) HIPCHK(c, hipMemcpyAsync(cls_prob, s->prob, (size_t)R * s->ncls * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (bbox_pred) HIPCHK(c, hipMemcpyAsync(bbox_pred, s->s_bb, (size_t)R * 4 * s->ncls * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return AZ_OK;
}

int az_skip_pool_bwd_unit(az_ctx *c, int n_src, const int *Cs, const float *spatial_scales, const float *const *maps_host,
                          const int *Hs, const int *Ws, int N, int channels_last, const float *rois, int R,
                          const float *d_raw_host, float *pooled_out, int32_t *argmax_out, float *const *dmaps_out)
{
    if (!c) return AZ_ERR_INVALID;
    const std::string who = "az_skip_pool_bwd_unit";
    long long sumC = 0;
    int rc = skip_front_check(c, who, n_src, Cs, spatial_scales, 1.0, 0.0, &sumC);
    if (rc != AZ_OK) return rc;
    if ((rc = check_maps(c, who, n_src, Cs, (const void *const *)maps_host, Hs, Ws, N)) != AZ_OK) return rc;
    if (!rois || R < 1 || R > 4096 || (long long)R * 49 * sumC > 0x7fffffffLL) return fail(c, AZ_ERR_INVALID, who + ": 1 <= R <= 4096, R * 49 * sumC in 31 bits");
    for (int r = 0; r < R; ++r) {
        const float *roi = rois + 5 * (size_t)r;
        if (!(roi[0] >= 0.0f && roi[0] < (float)N) || roi[0] != std::floor(roi[0])) return fail(c, AZ_ERR_INVALID, who + ": a roi names an image outside the batch");
        for (int q = 1; q < 5; ++q)
            if (!std::isfinite(roi[q]) || std::fabs(roi[q]) > 1e8f) return fail(c, AZ_ERR_INVALID, who + ": roi coordinate not finite");
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t big = (size_t)R * 49 * sumC;
    DevList tmp;                // (released on every exit)
    bool ok = true;
    auto grab = [&](size_t bytes) -> void * {
        char *q = nullptr;
        if (ok && tmp.alloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); ok = false; }
        return q;
    };
    void *dmaps[AZ_SKIP_MAX_SRC] = {nullptr, nullptr, nullptr};
    float *dm[AZ_SKIP_MAX_SRC] = {nullptr, nullptr, nullptr};
    size_t msz[AZ_SKIP_MAX_SRC] = {0, 0, 0};
    for (int i = 0; i < n_src; ++i) {
        msz[i] = (size_t)N * Cs[i] * Hs[i] * Ws[i] * 4;
        dmaps[i] = grab(msz[i]); dm[i] = (float *)grab(msz[i]);
    }
    const SkipSrcs a = skip_srcs(n_src, Cs, Hs, Ws, dmaps, N, channels_last);
    float *drois = (float *)grab((size_t)R * 5 * 4), *cat = (float *)grab(big * 4), *draw = (float *)grab(big * 4);
    int *geo = (int *)grab((size_t)n_src * R * 8 * 4), *arg = (int *)grab(big * 4);
    double *fac = (double *)grab((size_t)R * 49 * n_src * 8);
    if (!ok) return fail(c, AZ_ERR_HIP, who + ": device memory");
    for (int i = 0; i < n_src; ++i) HIPCHK(c, hipMemcpyAsync(dmaps[i], maps_host[i], msz[i], hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(drois, rois, (size_t)R * 5 * 4, hipMemcpyHostToDevice, st));
    if (d_raw_host) HIPCHK(c, hipMemcpyAsync(draw, d_raw_host, big * 4, hipMemcpyHostToDevice, st));
    launch_geo(st, drois, R, n_src, spatial_scales, geo);
    hipLaunchKernelGGL(k_skip_train_pool, dim3(R * 49, n_src), dim3(256), 0, st, a, 0, geo, R, 0, 1.0, 0.0, cat, arg, fac);
    if (d_raw_host && dmaps_out)
        for (int i = 0; i < n_src; ++i) if (dmaps_out[i]) launch_gather(c, a, i, draw, arg, geo, R, dm[i]);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (pooled_out) HIPCHK(c, hipMemcpy(pooled_out, cat, big * 4, hipMemcpyDeviceToHost));
    if (argmax_out) HIPCHK(c, hipMemcpy(argmax_out, arg, big * 4, hipMemcpyDeviceToHost));
    if (d_raw_host && dmaps_out)
        for (int i = 0; i < n_src; ++i) if (dmaps_out[i]) HIPCHK(c, hipMemcpy(dmaps_out[i], dm[i], msz[i], hipMemcpyDeviceToHost));
    return AZ_OK;
}

}  // extern "C"
