// az_det_solver.hip -- detection-net (Fast R-CNN) TRAINING from conv5_3 on (models/*/VGG16/frcnn/train.prototxt): RoIPool with
// arg-max -> fc6 -> fc7 -> {cls_score, bbox_pred}, SoftmaxWithLoss and SmoothL1Loss, the backward pass, the gradient norm and
// Caffe's momentum-SGD update.  The parameter store and the kernels are the trainer core's (az_trainer.h) in this graph's order;
// the one kernel of its own is the softmax loss.  fp32 master weights in Caffe layout ([out][in], roi_pool5 flattened c*49 + p).
//
// Every reduction has a fixed order (no floating-point atomics): see az_trainer.hip; the softmax sums a row lane-strided and
// then over a fixed butterfly, the row losses in row order per wave and then over the LDS tree.  The same step from the same
// state gives the same bits.
#include "az_det_solver.h"

namespace {

__device__ __forceinline__ float wave_max(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);       // both partners add the same two numbers: one value in all lanes
    return v;
}

// Caffe SoftmaxWithLoss, normalised by the R rows.  One workgroup of four waves; wave w serves the rows w, w + 4, ...: the row
// maximum by a wave reduction, e = exp(x - max), the sum lane-strided (columns lane, lane + 64, ...) and then over the
// butterfly, p = e / sum.  With labels: loss_row = -log(max(p[label], FLT_MIN)), d = (p - onehot) / R, and the row losses
// summed in f64, per wave in row order and then over block_sum's tree.  Without (TEST phase): only p.  ncls <= 256.
constexpr int SM_PER_LANE = 4;
__global__ void __launch_bounds__(256) k_solver_softmax_loss(const float *__restrict__ x, const float *__restrict__ labels, int R, int ncls,
                                                             float *__restrict__ prob, float *__restrict__ dx, float *__restrict__ loss)
{
    __shared__ double sh[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv = 1.0f / (float)R;
    double acc = 0.0;
    for (int r = wave; r < R; r += 4) {
        const float *xr = x + (size_t)r * ncls;
        float v[SM_PER_LANE];
        float m = -FLT_MAX;
#pragma unroll
        for (int q = 0; q < SM_PER_LANE; ++q) {
            const int j = lane + 64 * q;
            v[q] = j < ncls ? xr[j] : -FLT_MAX;
            m = fmaxf(m, v[q]);
        }
        m = wave_max(m);
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < SM_PER_LANE; ++q) {
            const int j = lane + 64 * q;
            v[q] = j < ncls ? expf(v[q] - m) : 0.0f;
            s = s + v[q];
        }
        s = wave_sum(s);
        const int lab = labels ? (int)labels[r] : -1;
#pragma unroll
        for (int q = 0; q < SM_PER_LANE; ++q) {
            const int j = lane + 64 * q;
            if (j >= ncls) continue;
            const float p = v[q] / s;
            prob[(size_t)r * ncls + j] = p;
            if (labels) {
                dx[(size_t)r * ncls + j] = (p - (j == lab ? 1.0f : 0.0f)) * inv;
                if (j == lab) acc += (double)(-logf(fmaxf(p, FLT_MIN)));
            }
        }
    }
    if (!labels) return;
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) *loss = (float)(tot / (double)R);
}

}  // namespace

// fc6 -> fc7 -> {cls_score, bbox_pred}; train: dropout on fc6 / fc7 with the step's masks (layer ids 0 / 1)
void det_head_forward(az_det_solver *s, int R, bool train, unsigned long long seed, unsigned long long iter)
{
    const bool m6 = train && s->drop[0] > 0.f, m7 = train && s->drop[1] > 0.f;
    fc_forward(s, "fc6_fwd", s->pool5, D_W6, R, s->n6, s->K6, s->pre6, s->a6, m6 ? s->m6 : nullptr, az_layer_key(seed, iter, 0), train ? s->drop[0] : 0.f);
    fc_forward(s, "fc7_fwd", s->a6, D_W7, R, s->n7, s->n6, s->pre7, s->a7, m7 ? s->m7 : nullptr, az_layer_key(seed, iter, 1), train ? s->drop[1] : 0.f);
    fc_forward(s, "cls_score_fwd", s->a7, D_WC, R, s->ncls, s->n7, s->s_cls, nullptr, nullptr, 0, 0.f);
    fc_forward(s, "bbox_pred_fwd", s->a7, D_WB, R, 4 * s->ncls, s->n7, s->s_bb, nullptr, nullptr, 0, 0.f);
}

int det_stage_targets(az_det_solver *s, int R, const float *labels, const float *bbox_targets, const float *bbox_loss_weights,
                      long long iteration, const std::string &who)
{
    az_ctx *c = s->c;
    if (!labels || !bbox_targets || !bbox_loss_weights || iteration < 0)
        return fail(c, AZ_ERR_INVALID, who + ": null label / target array or negative iteration");
    const int nc = s->ncls, nb = 4 * s->ncls;
    for (int r = 0; r < R; ++r)            // before anything is enqueued
        if (!(labels[r] >= 0.0f && labels[r] < (float)nc) || labels[r] != std::floor(labels[r]))
            return fail(c, AZ_ERR_INVALID, who + ": label " + std::to_string(labels[r]) + " of row " + std::to_string(r) + " is no class in [0, " + std::to_string(nc) + ")");
    HIPCHK(c, hipSetDevice(c->device));
    if (!(c->profiling & 4)) clear_events(c);
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(s->labels, labels, (size_t)R * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s->tgt, bbox_targets, (size_t)R * nb * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s->wgt, bbox_loss_weights, (size_t)R * nb * sizeof(float), hipMemcpyHostToDevice, st));
    return AZ_OK;
}

// SoftmaxWithLoss, SmoothL1Loss and the backward pass down to d_pre6 (want_dpool: and d_pool5)
void det_head_backward(az_det_solver *s, int R, bool want_dpool)
{
    az_ctx *c = s->c;
    hipStream_t st = c->stream;
    const int nc = s->ncls, nb = 4 * s->ncls, n6 = s->n6, n7 = s->n7, K6 = s->K6;
    { Timed t(c, "losses", 0);
      hipLaunchKernelGGL(k_solver_softmax_loss, dim3(1), dim3(256), 0, st, s->s_cls, s->labels, R, nc, s->prob, s->d_cls, s->loss + 0);
      tr_smooth_l1(s, s->s_bb, s->tgt, s->wgt, R * nb, R, s->d_bb, s->loss + 1); }
    s->has_prob = 1;
    // the two output layers: dW = dy^T x, db, and their two dx, which add into d7
    gemm_any(s, "cls_score_dw", 2, s->d_cls, s->a7, s->g[D_WC], nc, n7, R, s->acc);
    gemm_any(s, "bbox_pred_dw", 2, s->d_bb, s->a7, s->g[D_WB], nb, n7, R, s->acc);
    { Timed t(c, "bias_grads", 0); tr_colsum(s, s->d_cls, R, nc, s->g[D_BC], s->acc); tr_colsum(s, s->d_bb, R, nb, s->g[D_BB], s->acc); }
    gemm_any(s, "cls_score_dx", 1, s->d_cls, s->w[D_WC], s->d7, R, n7, nc, 0);
    gemm_any(s, "bbox_pred_dx", 1, s->d_bb, s->w[D_WB], s->d7, R, n7, nb, 1);
    tr_act_bwd(s, s->d7, s->pre7, s->m7, s->drop[1], R, n7);
    gemm_any(s, "fc7_dw", 2, s->d7, s->a6, s->g[D_W7], n7, n6, R, s->acc);
    { Timed t(c, "bias_grads", 0); tr_colsum(s, s->d7, R, n7, s->g[D_B7], s->acc); }
    gemm_any(s, "fc7_dx", 1, s->d7, s->w[D_W7], s->d6, R, n6, n7, 0);
    tr_act_bwd(s, s->d6, s->pre6, s->m6, s->drop[0], R, n6);
    gemm_any(s, "fc6_dw", 2, s->d6, s->pool5, s->g[D_W6], n6, K6, R, s->acc);
    { Timed t(c, "bias_grads", 0); tr_colsum(s, s->d6, R, n6, s->g[D_B6], s->acc); }
    if (want_dpool) gemm_any(s, "fc6_dx", 1, s->d6, s->w[D_W6], s->dpool, R, K6, n6, 0);
}

// TEST phase: cls_prob of the raw scores
void det_softmax_test(az_det_solver *s, int R)
{
    hipLaunchKernelGGL(k_solver_softmax_loss, dim3(1), dim3(256), 0, s->c->stream, s->s_cls, (const float *)nullptr, R, s->ncls, s->prob,
                       (float *)nullptr, (float *)nullptr);
    s->has_prob = 1;
}

void az_det_solver_free_all(az_ctx *c)
{
    while (!c->det_solvers.empty()) az_det_solver_destroy(c->det_solvers.back());
}

extern "C" {

int az_det_solver_create(az_ctx *c, int C, int n6, int n7, int num_classes, int max_rois, uint64_t seed, az_det_solver **out)
{
    if (!c || !out) return AZ_ERR_INVALID;
    *out = nullptr;
    if (C < 4 || C % 4 || n6 < 4 || n6 % 4 || n7 < 4 || n7 % 4 || num_classes < 2 || num_classes > 64 * SM_PER_LANE || max_rois < 1 ||
        max_rois > 4096 || (long long)C * 49 * n6 > (1LL << 33) || (long long)n6 * n7 > (1LL << 33))
        return fail(c, AZ_ERR_INVALID, "az_det_solver_create: C, n6, n7 must be positive multiples of 4, 2 <= num_classes <= 256, 1 <= max_rois <= 4096");
    HIPCHK(c, hipSetDevice(c->device));
    az_det_solver *s = new az_det_solver();
    s->n6 = n6; s->n7 = n7; s->ncls = num_classes; s->np = DNPARAM;
    const size_t K6 = (size_t)C * 49, R = (size_t)max_rois, nc = (size_t)num_classes, nb = 4 * nc;
    // the slabs of a split-K product hold at most 256 tiles of 128 x 128 (pick_split); an unsplit forward layer R x its width
    // (az_det_solver_attach_skip relies on the 4M-float floor for the front's split products)
    size_t nmax = (size_t)(n6 > n7 ? n6 : n7); nmax = nmax > nb ? nmax : nb; nmax = nmax > K6 ? nmax : K6;
    int rc = tr_init(s, c, "az_det_solver", DPNAME, C, max_rois, nmax);
    const size_t pn[DNPARAM] = {n6 * K6, (size_t)n6, (size_t)n7 * n6, (size_t)n7, nc * n7, nc, nb * n7, nb};
    if (rc == AZ_OK) rc = tr_alloc_params(s, 0, DNPARAM, pn);
#define SA(p, n) if (rc == AZ_OK) rc = tr_alloc(s, &s->p, (n))
    SA(labels, R); SA(tgt, R * nb); SA(wgt, R * nb);
    SA(pre6, R * n6); SA(a6, R * n6); SA(d6, R * n6); SA(m6, R * n6);
    SA(pre7, R * n7); SA(a7, R * n7); SA(d7, R * n7); SA(m7, R * n7);
    SA(s_cls, R * nc); SA(prob, R * nc); SA(d_cls, R * nc); SA(s_bb, R * nb); SA(d_bb, R * nb);
#undef SA
    if (rc == AZ_OK && tr_fill_params(s, 0, DNPARAM, DET_FILLER_STD, seed) != AZ_OK)
        rc = fail(c, AZ_ERR_HIP, "az_det_solver_create: initialising the parameters failed");
    if (rc != AZ_OK) { tr_release(s, 0); delete s; return rc; }
    c->det_solvers.push_back(s);
    *out = s;
    return AZ_OK;
}

int az_det_solver_destroy(az_det_solver *s) { return s ? tr_destroy(s, s->c->det_solvers) : AZ_ERR_INVALID; }

int az_det_solver_load(az_det_solver *s, const float *W6, const float *b6, const float *W7, const float *b7, const float *Wc,
                       const float *bc, const float *Wb, const float *bb)
{
    if (!s) return AZ_ERR_INVALID;
    const float *src[DNPARAM] = {W6, b6, W7, b7, Wc, bc, Wb, bb};
    return tr_load(s, 0, DNPARAM, src);
}

int az_det_solver_read(az_det_solver *s, float *W6, float *b6, float *W7, float *b7, float *Wc, float *bc, float *Wb, float *bb)
{
    if (!s) return AZ_ERR_INVALID;
    float *dst[DNPARAM] = {W6, b6, W7, b7, Wc, bc, Wb, bb};
    return tr_read(s, 0, DNPARAM, dst);
}

int az_det_solver_set_hyper(az_det_solver *s, const float *lr_mult, const float *decay_mult, const float *dropout_ratio)
{
    if (!s) return AZ_ERR_INVALID;
    return tr_set_hyper(s, DNPARAM, lr_mult, decay_mult, dropout_ratio, s->drop, 2);
}

int az_det_solver_step(az_det_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                       const float *labels, const float *bbox_targets, const float *bbox_loss_weights, uint64_t seed,
                       long long iteration, float *losses_out, double *sumsq_out, float *dmap_dev)
{
    int rc = tr_check_step(s, conv_dev, N, H, W, rois, R, "az_det_solver_step");
    if (rc != AZ_OK) return rc;
    if ((rc = det_stage_targets(s, R, labels, bbox_targets, bbox_loss_weights, iteration, "az_det_solver_step")) != AZ_OK) return rc;
    if ((rc = tr_roi_pool_forward(s, conv_dev, N, H, W, channels_last, rois, R)) != AZ_OK) return rc;
    det_head_forward(s, R, true, seed, (unsigned long long)iteration);
    det_head_backward(s, R, dmap_dev != nullptr);
    s->sk.trained = 0;
    if (dmap_dev) tr_roi_pool_backward(s, N, H, W, channels_last, dmap_dev);
    if ((rc = tr_grad_norm(s, DNPARAM, 2, losses_out, sumsq_out)) != AZ_OK) return rc;
    s->trained = dmap_dev ? 2 : 1;
    return AZ_OK;
}

int az_det_solver_set_precision(az_det_solver *s, int precision) { return tr_set_precision(s, precision); }

int az_det_solver_set_accumulate(az_det_solver *s, int on) { return tr_set_accumulate(s, on); }

int az_det_solver_load_history(az_det_solver *s, const float *W6, const float *b6, const float *W7, const float *b7,
                               const float *Wc, const float *bc, const float *Wb, const float *bb)
{
    if (!s) return AZ_ERR_INVALID;
    const float *src[DNPARAM] = {W6, b6, W7, b7, Wc, bc, Wb, bb};
    return tr_load_history(s, 0, DNPARAM, src);
}

int az_det_solver_update(az_det_solver *s, double rate, double momentum, double weight_decay, double clip_scale)
{
    if (!s) return AZ_ERR_INVALID;
    return tr_update(s, s->sk.trained ? DNALL : DNPARAM, rate, momentum, weight_decay, clip_scale);       // conv_pool5 too, behind a skip step
}

int az_det_solver_forward_test(az_det_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois,
                               int R, float *cls_prob, float *bbox_pred)
{
    int rc = tr_check_step(s, conv_dev, N, H, W, rois, R, "az_det_solver_forward_test");
    if (rc != AZ_OK) return rc;
    az_ctx *c = s->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (!(c->profiling & 4)) clear_events(c);
    if ((rc = tr_roi_pool_forward(s, conv_dev, N, H, W, channels_last, rois, R)) != AZ_OK) return rc;
    det_head_forward(s, R, false, 0, 0);
    s->trained = 0; s->sk.trained = 0;
    det_softmax_test(s, R);
    if (cls_prob) HIPCHK(c, hipMemcpyAsync(cls_prob, s->prob, (size_t)R * s->ncls * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (bbox_pred) HIPCHK(c, hipMemcpyAsync(bbox_pred, s->s_bb, (size_t)R * 4 * s->ncls * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return AZ_OK;
}

int az_det_solver_fetch(az_det_solver *s, const char *name, void *out, long long cap_bytes, long long *bytes_out)
{
    if (!s || !name || !bytes_out) return AZ_ERR_INVALID;
    const std::string nm(name);
    const size_t R = (size_t)s->R, nc = (size_t)s->ncls;
    const void *src = nullptr;
    size_t bytes = 0;
    struct Ent { const char *n; const void *p; size_t b; };
    const Ent tab[] = {
        {"pool5", s->pool5, R * s->K6 * 4}, {"argmax", s->argmax, R * s->K6 * 4}, {"d_pool5", s->dpool, R * s->K6 * 4},
        {"pre6", s->pre6, R * s->n6 * 4}, {"a6", s->a6, R * s->n6 * 4}, {"d_pre6", s->d6, R * s->n6 * 4}, {"mask6", s->m6, R * s->n6},
        {"pre7", s->pre7, R * s->n7 * 4}, {"a7", s->a7, R * s->n7 * 4}, {"d_pre7", s->d7, R * s->n7 * 4}, {"mask7", s->m7, R * s->n7},
        {"cls_score", s->s_cls, R * nc * 4}, {"cls_prob", s->prob, R * nc * 4}, {"bbox_pred", s->s_bb, R * nc * 16},
        {"d_cls_score", s->d_cls, R * nc * 4}, {"d_bbox_pred", s->d_bb, R * nc * 16},
    };
    for (const Ent &e : tab) if (nm == e.n) { src = e.p; bytes = e.b; }
    if (!src) skip_train_fetch(s, nm, &src, &bytes);
    if (!src) det_mine_fetch(s, nm, &src, &bytes);
    if ((nm == "d_cat" || nm == "d_raw") && src && !s->sk.has_dcat)
        return fail(s->c, AZ_ERR_STATE, "az_det_solver_fetch: the last skip pass asked for no map gradient, so it computed no '" + nm + "'");
    return tr_fetch(s, nm, src, bytes, out, cap_bytes, bytes_out);
}

}  // extern "C"
