// az_solver.hip -- AZ-net TRAINING from conv5_3 on (models/*/VGG16/az-net/train.prototxt): RoIPool with arg-max and its
// backward, the six InnerProduct layers forward / dX / dW on the fp32 matrix cores, ReLU + dropout, the three losses, the
// gradient norm and Caffe's momentum-SGD update.  fp32 master weights in Caffe layout ([out][in], roi_pool5 flattened
// c*49 + p), so the activations are in Caffe order as well and a snapshot is a plain copy.
//
// Every reduction has a fixed order (no floating-point atomics): split-K slabs are summed in slab order, column sums walk
// the rows in order, RoIPool backward GATHERS over the rois in row order, loss sums and the gradient norm are a strided
// per-thread sum followed by a fixed LDS tree.  The same step from the same state gives the same bits.
#include "az_solver_dev.h"

// parameter order of the ABI: W6 b6 W71 b71 W72 b72 Was bas Wab bab Wz bz
enum { P_W6, P_B6, P_W71, P_B71, P_W72, P_B72, P_WAS, P_BAS, P_WAB, P_BAB, P_WZ, P_BZ, NPARAM };
static const char *const PNAME[NPARAM] = {"W6", "b6", "W71", "b71", "W72", "b72", "Was", "bas", "Wab", "bab", "Wz", "bz"};
static const float FILLER_STD[6] = {1e-4f, 1e-4f, 1e-3f, 1e-2f, 1e-3f, 1e-2f};   // int6 int7_1 int7_2 adj_score adj_bbox zoom_score

struct az_solver {
    az_ctx *c = nullptr;
    int C = 0, n6 = 0, n71 = 0, n72 = 0, K6 = 0, maxR = 0;
    size_t pn[NPARAM] = {0};
    float *w[NPARAM] = {nullptr}, *g[NPARAM] = {nullptr}, *h[NPARAM] = {nullptr};
    float lr_mult[NPARAM], decay_mult[NPARAM];
    float drop[3] = {0.5f, 0.5f, 0.5f};
    // one step's activations and gradients (rows: maxR)
    float *rois = nullptr, *lab_as = nullptr, *tgt_ab = nullptr, *wgt_ab = nullptr, *lab_z = nullptr;
    int *geo = nullptr, *argmax = nullptr;
    float *pool5 = nullptr, *pre6 = nullptr, *a6 = nullptr, *pre71 = nullptr, *a71 = nullptr, *pre72 = nullptr, *a72 = nullptr;
    unsigned char *m6 = nullptr, *m71 = nullptr, *m72 = nullptr;
    float *s_as = nullptr, *s_ab = nullptr, *s_z = nullptr;          // raw adj_score / adj_bbox / zoom_score
    float *d_as = nullptr, *d_ab = nullptr, *d_z = nullptr, *d71 = nullptr, *d72 = nullptr, *d6 = nullptr, *dpool = nullptr;
    float *part = nullptr, *loss = nullptr;
    double *sq_part = nullptr, *sq = nullptr;
    size_t part_elems = 0;
    std::vector<void *> allocs;
    // shape of the last step (what the debug fetch sizes its answers by)
    int R = 0, N = 0, H = 0, W = 0, trained = 0;
    int prec = AZ_TRAIN_FP32;                                   // operands of every matrix product (az_solver_set_precision)
};

namespace {

template <typename T>
int salloc(az_solver *s, T **p, size_t n)
{
    void *q = nullptr;
    if (hipMalloc(&q, n * sizeof(T) + 256) != hipSuccess) return fail(s->c, AZ_ERR_HIP, "az_solver: hipMalloc(" + std::to_string(n * sizeof(T)) + " B) failed");
    s->allocs.push_back(q);
    *p = (T *)q;
    return AZ_OK;
}

int check_step_args(az_solver *s, const float *conv, int N, int H, int W, const float *rois, int R, const char *who)
{
    if (!s) return AZ_ERR_INVALID;
    if (!conv || !rois) return fail(s->c, AZ_ERR_INVALID, std::string(who) + ": null conv5_3 or rois");
    if (N < 1 || H < 1 || W < 1 || (long long)H * W > 0x3fffffff) return fail(s->c, AZ_ERR_INVALID, std::string(who) + ": bad map shape");
    if (R < 1 || R > s->maxR) return fail(s->c, AZ_ERR_INVALID, std::string(who) + ": R must be in [1, max_rois = " + std::to_string(s->maxR) + "]");
    for (int r = 0; r < R; ++r) {
        const float b = rois[5 * (size_t)r];
        if (!(b >= 0.0f && b < (float)N) || b != std::floor(b)) return fail(s->c, AZ_ERR_INVALID, std::string(who) + ": roi " + std::to_string(r) + " names image " + std::to_string(b) + " of " + std::to_string(N));
        for (int q = 1; q < 5; ++q) if (!std::isfinite(rois[5 * (size_t)r + q]) || std::fabs(rois[5 * (size_t)r + q]) > 1e8f) return fail(s->c, AZ_ERR_INVALID, std::string(who) + ": roi coordinate not finite");
    }
    return AZ_OK;
}

// RoIPool -> int6 -> {int7_1 -> adj_score, adj_bbox; int7_2 -> zoom_score}; train: dropout with the step's masks
int forward_pass(az_solver *s, const float *conv, int N, int H, int W, int cl, const float *rois, int R, bool train,
                 unsigned long long seed, unsigned long long iter)
{
    az_ctx *c = s->c;
    HIPCHK(c, hipMemcpyAsync(s->rois, rois, (size_t)R * 5 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const MapView m{N, s->C, H, W, cl ? 1 : 0};
    { Timed t(c, "roi_pool_argmax", 0);
      hipLaunchKernelGGL(k_solver_roi_geo, dim3((R + 255) / 256), dim3(256), 0, c->stream, s->rois, R, c->spatial_scale, s->geo);
      hipLaunchKernelGGL(k_solver_roi_pool, dim3(grid_for((long long)R * s->K6, 16384)), dim3(256), 0, c->stream, conv, m, s->geo, R,
                         s->pool5, s->argmax); }
    auto key = [&](unsigned layer) { return az_layer_key(seed, iter, layer); };
    fc_forward(s, "int6_fwd", s->pool5, P_W6, R, s->n6, s->K6, s->pre6, s->a6, train && s->drop[0] > 0.f ? s->m6 : nullptr, key(0), train ? s->drop[0] : 0.f);
    fc_forward(s, "int7_1_fwd", s->a6, P_W71, R, s->n71, s->n6, s->pre71, s->a71, train && s->drop[1] > 0.f ? s->m71 : nullptr, key(1), train ? s->drop[1] : 0.f);
    fc_forward(s, "int7_2_fwd", s->a6, P_W72, R, s->n72, s->n6, s->pre72, s->a72, train && s->drop[2] > 0.f ? s->m72 : nullptr, key(2), train ? s->drop[2] : 0.f);
    fc_forward(s, "adj_score_fwd", s->a71, P_WAS, R, 11, s->n71, s->s_as, nullptr, nullptr, 0, 0.f);
    fc_forward(s, "adj_bbox_fwd", s->a71, P_WAB, R, 44, s->n71, s->s_ab, nullptr, nullptr, 0, 0.f);
    fc_forward(s, "zoom_score_fwd", s->a72, P_WZ, R, 1, s->n72, s->s_z, nullptr, nullptr, 0, 0.f);
    s->R = R; s->N = N; s->H = H; s->W = W;
    return AZ_OK;
}

}  // namespace

void az_solver_free_all(az_ctx *c)
{
    while (!c->solvers.empty()) az_solver_destroy(c->solvers.back());
}

extern "C" {

int az_solver_create(az_ctx *c, int C, int n6, int n71, int n72, int max_rois, uint64_t seed, az_solver **out)
{
    if (!c || !out) return AZ_ERR_INVALID;
    *out = nullptr;
    if (C < 4 || C % 4 || n6 < 4 || n6 % 4 || n71 < 1 || n72 < 1 || max_rois < 1 || max_rois > 4096 || (long long)C * 49 * n6 > (1LL << 33))
        return fail(c, AZ_ERR_INVALID, "az_solver_create: C and n6 must be positive multiples of 4, n71 / n72 >= 1, 1 <= max_rois <= 4096");
    HIPCHK(c, hipSetDevice(c->device));
    az_solver *s = new az_solver();
    s->c = c; s->C = C; s->n6 = n6; s->n71 = n71; s->n72 = n72; s->K6 = C * 49; s->maxR = max_rois;
    const size_t K6 = (size_t)s->K6;
    const size_t pn[NPARAM] = {n6 * K6, (size_t)n6, (size_t)n71 * n6, (size_t)n71, (size_t)n72 * n6, (size_t)n72,
                               (size_t)11 * n71, 11, (size_t)44 * n71, 44, (size_t)n72, 1};
    int rc = AZ_OK;
    for (int p = 0; p < NPARAM && rc == AZ_OK; ++p) {
        s->pn[p] = pn[p];
        s->lr_mult[p] = (p & 1) ? 2.0f : 1.0f;
        s->decay_mult[p] = (p & 1) ? 0.0f : 1.0f;
        if ((rc = salloc(s, &s->w[p], pn[p])) == AZ_OK && (rc = salloc(s, &s->g[p], pn[p])) == AZ_OK) rc = salloc(s, &s->h[p], pn[p]);
    }
    const size_t R = (size_t)max_rois;
    int nmax = n6 > n71 ? n6 : n71; nmax = nmax > n72 ? nmax : n72; nmax = nmax > 44 ? nmax : 44;
    s->part_elems = R * nmax > (size_t)4 << 20 ? R * nmax : (size_t)4 << 20;
#define SA(p, n) if (rc == AZ_OK) rc = salloc(s, &s->p, (n))
    SA(rois, R * 5); SA(lab_as, R * 11); SA(tgt_ab, R * 44); SA(wgt_ab, R * 44); SA(lab_z, R); SA(geo, R * 8);
    SA(argmax, R * K6); SA(pool5, R * K6); SA(dpool, R * K6);
    SA(pre6, R * n6); SA(a6, R * n6); SA(d6, R * n6); SA(m6, R * n6);
    SA(pre71, R * n71); SA(a71, R * n71); SA(d71, R * n71); SA(m71, R * n71);
    SA(pre72, R * n72); SA(a72, R * n72); SA(d72, R * n72); SA(m72, R * n72);
    SA(s_as, R * 11); SA(s_ab, R * 44); SA(s_z, R); SA(d_as, R * 11); SA(d_ab, R * 44); SA(d_z, R);
    SA(part, s->part_elems); SA(loss, 4); SA(sq_part, (size_t)NPARAM * SQ_BLOCKS); SA(sq, 2);
#undef SA
    if (rc != AZ_OK) { for (void *q : s->allocs) hipFree(q); delete s; return rc; }
    // Caffe's fillers: gaussian weights, zero biases; history zero
    for (int p = 0; p < NPARAM; ++p) {
        hipMemsetAsync(s->h[p], 0, pn[p] * sizeof(float), c->stream);
        hipMemsetAsync(s->g[p], 0, pn[p] * sizeof(float), c->stream);
        if (p & 1) hipMemsetAsync(s->w[p], 0, pn[p] * sizeof(float), c->stream);
        else hipLaunchKernelGGL(k_solver_fill_gauss, dim3(grid_for((long long)pn[p], 8192)), dim3(256), 0, c->stream, s->w[p], (long long)pn[p],
                                FILLER_STD[p / 2], az_layer_key(seed, 0, 16 + p));
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) {
        for (void *q : s->allocs) hipFree(q);
        delete s;
        return fail(c, AZ_ERR_HIP, "az_solver_create: initialising the parameters failed");
    }
    c->solvers.push_back(s);
    *out = s;
    return AZ_OK;
}

int az_solver_destroy(az_solver *s)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    for (void *q : s->allocs) hipFree(q);
    for (size_t i = 0; i < c->solvers.size(); ++i) if (c->solvers[i] == s) { c->solvers.erase(c->solvers.begin() + i); break; }
    delete s;
    return AZ_OK;
}

int az_solver_load(az_solver *s, const float *W6, const float *b6, const float *W71, const float *b71, const float *W72,
                   const float *b72, const float *Was, const float *bas, const float *Wab, const float *bab, const float *Wz,
                   const float *bz)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    const float *src[NPARAM] = {W6, b6, W71, b71, W72, b72, Was, bas, Wab, bab, Wz, bz};
    HIPCHK(c, hipSetDevice(c->device));
    for (int p = 0; p < NPARAM; ++p)       // a null array keeps what the trainer holds
        if (src[p]) HIPCHK(c, hipMemcpyAsync(s->w[p], src[p], s->pn[p] * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AZ_OK;
}

int az_solver_read(az_solver *s, float *W6, float *b6, float *W71, float *b71, float *W72, float *b72, float *Was, float *bas,
                   float *Wab, float *bab, float *Wz, float *bz)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    float *dst[NPARAM] = {W6, b6, W71, b71, W72, b72, Was, bas, Wab, bab, Wz, bz};
    HIPCHK(c, hipSetDevice(c->device));
    for (int p = 0; p < NPARAM; ++p)
        if (dst[p]) HIPCHK(c, hipMemcpyAsync(dst[p], s->w[p], s->pn[p] * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AZ_OK;
}

int az_solver_set_hyper(az_solver *s, const float *lr_mult, const float *decay_mult, const float *dropout_ratio)
{
    if (!s) return AZ_ERR_INVALID;
    if (dropout_ratio) for (int i = 0; i < 3; ++i) if (!(dropout_ratio[i] >= 0.0f && dropout_ratio[i] < 1.0f)) return fail(s->c, AZ_ERR_INVALID, "az_solver_set_hyper: dropout ratio outside [0, 1)");
    if (lr_mult) for (int p = 0; p < NPARAM; ++p) if (!(lr_mult[p] >= 0.0f)) return fail(s->c, AZ_ERR_INVALID, "az_solver_set_hyper: negative lr_mult");
    if (decay_mult) for (int p = 0; p < NPARAM; ++p) if (!(decay_mult[p] >= 0.0f)) return fail(s->c, AZ_ERR_INVALID, "az_solver_set_hyper: negative decay_mult");
    if (lr_mult) for (int p = 0; p < NPARAM; ++p) s->lr_mult[p] = lr_mult[p];
    if (decay_mult) for (int p = 0; p < NPARAM; ++p) s->decay_mult[p] = decay_mult[p];
    if (dropout_ratio) for (int i = 0; i < 3; ++i) s->drop[i] = dropout_ratio[i];
    return AZ_OK;
}

int az_solver_step(az_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                   const float *adj_labels, const float *adj_targets, const float *adj_loss_weights, const float *zoom_labels,
                   uint64_t seed, long long iteration, float *losses_out, double *sumsq_out, float *dmap_dev)
{
    int rc = check_step_args(s, conv_dev, N, H, W, rois, R, "az_solver_step");
    if (rc != AZ_OK) return rc;
    az_ctx *c = s->c;
    if (!adj_labels || !adj_targets || !adj_loss_weights || !zoom_labels || iteration < 0)
        return fail(c, AZ_ERR_INVALID, "az_solver_step: null label / target array or negative iteration");
    HIPCHK(c, hipSetDevice(c->device));
    if (!(c->profiling & 4)) clear_events(c);
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(s->lab_as, adj_labels, (size_t)R * 11 * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s->tgt_ab, adj_targets, (size_t)R * 44 * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s->wgt_ab, adj_loss_weights, (size_t)R * 44 * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s->lab_z, zoom_labels, (size_t)R * sizeof(float), hipMemcpyHostToDevice, st));
    if ((rc = forward_pass(s, conv_dev, N, H, W, channels_last, rois, R, true, seed, (unsigned long long)iteration)) != AZ_OK) return rc;
    const int n6 = s->n6, n71 = s->n71, n72 = s->n72, K6 = s->K6;
    { Timed t(c, "losses", 0);
      hipLaunchKernelGGL(k_solver_sigmoid_ce, dim3(1), dim3(256), 0, st, s->s_z, s->lab_z, R, R, s->d_z, s->loss + 0);
      hipLaunchKernelGGL(k_solver_sigmoid_ce, dim3(1), dim3(256), 0, st, s->s_as, s->lab_as, R * 11, R, s->d_as, s->loss + 1);
      hipLaunchKernelGGL(k_solver_smooth_l1, dim3(1), dim3(256), 0, st, s->s_ab, s->tgt_ab, s->wgt_ab, R * 44, R, s->d_ab, s->loss + 2); }
    auto colsum = [&](const float *dy, int Nc, float *db) {
        hipLaunchKernelGGL(k_solver_colsum, dim3((Nc + 255) / 256), dim3(256), 0, st, dy, R, Nc, db);
    };
    auto act_bwd = [&](float *d, const float *pre, const unsigned char *mask, float ratio, int Nc) {
        Timed t(c, "act_bwd", 0);
        hipLaunchKernelGGL(k_solver_act_bwd, dim3(grid_for((long long)R * Nc)), dim3(256), 0, st, d, pre, ratio > 0.f ? mask : nullptr,
                           1.0f / (1.0f - ratio), (long long)R * Nc);
    };
    // the three output layers: dW = dy^T x, db, and the gradients of int7_1 / int7_2's outputs (two dx add into d71)
    gemm_any(s, "adj_score_dw", 2, s->d_as, s->a71, s->g[P_WAS], 11, n71, R, 0);
    gemm_any(s, "adj_bbox_dw", 2, s->d_ab, s->a71, s->g[P_WAB], 44, n71, R, 0);
    gemm_any(s, "zoom_score_dw", 2, s->d_z, s->a72, s->g[P_WZ], 1, n72, R, 0);
    { Timed t(c, "bias_grads", 0);
      colsum(s->d_as, 11, s->g[P_BAS]); colsum(s->d_ab, 44, s->g[P_BAB]); colsum(s->d_z, 1, s->g[P_BZ]); }
    gemm_any(s, "adj_score_dx", 1, s->d_as, s->w[P_WAS], s->d71, R, n71, 11, 0);
    gemm_any(s, "adj_bbox_dx", 1, s->d_ab, s->w[P_WAB], s->d71, R, n71, 44, 1);
    gemm_any(s, "zoom_score_dx", 1, s->d_z, s->w[P_WZ], s->d72, R, n72, 1, 0);
    act_bwd(s->d71, s->pre71, s->m71, s->drop[1], n71);
    act_bwd(s->d72, s->pre72, s->m72, s->drop[2], n72);
    gemm_any(s, "int7_1_dw", 2, s->d71, s->a6, s->g[P_W71], n71, n6, R, 0);
    gemm_any(s, "int7_2_dw", 2, s->d72, s->a6, s->g[P_W72], n72, n6, R, 0);
    { Timed t(c, "bias_grads", 0); colsum(s->d71, n71, s->g[P_B71]); colsum(s->d72, n72, s->g[P_B72]); }
    // int7_1 and int7_2 both read int6: their two dx add
    gemm_any(s, "int7_1_dx", 1, s->d71, s->w[P_W71], s->d6, R, n6, n71, 0);
    gemm_any(s, "int7_2_dx", 1, s->d72, s->w[P_W72], s->d6, R, n6, n72, 1);
    act_bwd(s->d6, s->pre6, s->m6, s->drop[0], n6);
    gemm_any(s, "int6_dw", 2, s->d6, s->pool5, s->g[P_W6], n6, K6, R, 0);
    { Timed t(c, "bias_grads", 0); colsum(s->d6, n6, s->g[P_B6]); }
    if (dmap_dev) {
        gemm_any(s, "int6_dx", 1, s->d6, s->w[P_W6], s->dpool, R, K6, n6, 0);
        const MapView m{N, s->C, H, W, channels_last ? 1 : 0};
        Timed t(c, "roi_pool_bwd", 0);
        hipLaunchKernelGGL(k_solver_roi_pool_bwd, dim3(grid_for((long long)N * s->C * H * W, 1 << 30)), dim3(256), 0, st, s->dpool,
                           s->argmax, s->geo, R, m, dmap_dev);
    }
    { Timed t(c, "grad_sumsq", 0);
      for (int p = 0; p < NPARAM; ++p)
          hipLaunchKernelGGL(k_solver_sumsq, dim3(SQ_BLOCKS), dim3(256), 0, st, s->g[p], (long long)s->pn[p], s->sq_part + (size_t)p * SQ_BLOCKS);
      hipLaunchKernelGGL(k_solver_sumsq_final, dim3(1), dim3(256), 0, st, s->sq_part, NPARAM * SQ_BLOCKS, s->sq); }
    float hl[3]; double hs = 0.0;
    HIPCHK(c, hipMemcpyAsync(hl, s->loss, sizeof(hl), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&hs, s->sq, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    s->trained = dmap_dev ? 2 : 1;
    if (losses_out) { losses_out[0] = hl[0]; losses_out[1] = hl[1]; losses_out[2] = hl[2]; }
    if (sumsq_out) *sumsq_out = hs;
    return AZ_OK;
}

int az_solver_update(az_solver *s, double rate, double momentum, double weight_decay, double clip_scale)
{
    if (!s) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    if (!(rate >= 0.0) || !(momentum >= 0.0) || !(weight_decay >= 0.0) || !(clip_scale > 0.0) || !std::isfinite(rate + momentum + weight_decay + clip_scale))
        return fail(c, AZ_ERR_INVALID, "az_solver_update: rate, momentum, weight_decay >= 0 and clip_scale > 0, all finite");
    if (!s->trained) return fail(c, AZ_ERR_STATE, "az_solver_update: no az_solver_step has produced gradients");
    HIPCHK(c, hipSetDevice(c->device));
    { Timed t(c, "sgd_update", 0);
      for (int p = 0; p < NPARAM; ++p)
          hipLaunchKernelGGL(k_solver_sgd, dim3(grid_for((long long)s->pn[p], 16384)), dim3(256), 0, c->stream, s->w[p], s->g[p], s->h[p],
                             (long long)s->pn[p], (float)(rate * (double)s->lr_mult[p]), (float)momentum,
                             (float)(weight_decay * (double)s->decay_mult[p]), (float)clip_scale); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return AZ_OK;
}

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

int az_solver_forward_test(az_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                           float *zoom_score, float *adj_score, float *adj_bbox)
{
    int rc = check_step_args(s, conv_dev, N, H, W, rois, R, "az_solver_forward_test");
    if (rc != AZ_OK) return rc;
    az_ctx *c = s->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (!(c->profiling & 4)) clear_events(c);
    if ((rc = forward_pass(s, conv_dev, N, H, W, channels_last, rois, R, false, 0, 0)) != AZ_OK) return rc;
    s->trained = 0;
    if (zoom_score) HIPCHK(c, hipMemcpyAsync(zoom_score, s->s_z, (size_t)R * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (adj_score) HIPCHK(c, hipMemcpyAsync(adj_score, s->s_as, (size_t)R * 11 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (adj_bbox) HIPCHK(c, hipMemcpyAsync(adj_bbox, s->s_ab, (size_t)R * 44 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return AZ_OK;
}

int az_solver_fetch(az_solver *s, const char *name, void *out, long long cap_bytes, long long *bytes_out)
{
    if (!s || !name || !bytes_out) return AZ_ERR_INVALID;
    az_ctx *c = s->c;
    const std::string nm(name);
    const size_t R = (size_t)s->R;
    const void *src = nullptr;
    size_t bytes = 0;
    struct Ent { const char *n; const void *p; size_t b; };
    const Ent tab[] = {
        {"pool5", s->pool5, R * s->K6 * 4}, {"argmax", s->argmax, R * s->K6 * 4}, {"d_pool5", s->dpool, R * s->K6 * 4},
        {"pre6", s->pre6, R * s->n6 * 4}, {"a6", s->a6, R * s->n6 * 4}, {"d_pre6", s->d6, R * s->n6 * 4}, {"mask6", s->m6, R * s->n6},
        {"pre71", s->pre71, R * s->n71 * 4}, {"a71", s->a71, R * s->n71 * 4}, {"d_pre71", s->d71, R * s->n71 * 4}, {"mask71", s->m71, R * s->n71},
        {"pre72", s->pre72, R * s->n72 * 4}, {"a72", s->a72, R * s->n72 * 4}, {"d_pre72", s->d72, R * s->n72 * 4}, {"mask72", s->m72, R * s->n72},
        {"adj_score", s->s_as, R * 11 * 4}, {"adj_bbox", s->s_ab, R * 44 * 4}, {"zoom_score", s->s_z, R * 4},
        {"d_adj_score", s->d_as, R * 11 * 4}, {"d_adj_bbox", s->d_ab, R * 44 * 4}, {"d_zoom_score", s->d_z, R * 4},
    };
    for (const Ent &e : tab) if (nm == e.n) { src = e.p; bytes = e.b; }
    if (!src && nm.size() > 2 && nm[1] == '_' && (nm[0] == 'g' || nm[0] == 'h' || nm[0] == 'w'))
        for (int p = 0; p < NPARAM; ++p)
            if (nm.substr(2) == PNAME[p]) { src = nm[0] == 'g' ? s->g[p] : (nm[0] == 'h' ? s->h[p] : s->w[p]); bytes = s->pn[p] * 4; }
    if (!src) return fail(c, AZ_ERR_INVALID, "az_solver_fetch: no saved tensor named '" + nm + "'");
    const bool is_param = nm[1] == '_' && (nm[0] == 'g' || nm[0] == 'h' || nm[0] == 'w') && nm != "d_pool5";
    if (!is_param && s->R == 0) return fail(c, AZ_ERR_STATE, "az_solver_fetch: no forward pass has run");
    *bytes_out = (long long)bytes;
    if (!out) return AZ_OK;
    if (cap_bytes < (long long)bytes) return fail(c, AZ_ERR_CAPACITY, "az_solver_fetch: '" + nm + "' needs " + std::to_string(bytes) + " bytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_solver_set_precision(az_solver *s, int precision)
{
    if (!s) return AZ_ERR_INVALID;
    if (precision != AZ_TRAIN_FP32 && precision != AZ_TRAIN_BF16)
        return fail(s->c, AZ_ERR_INVALID, "az_solver_set_precision: AZ_TRAIN_FP32 or AZ_TRAIN_BF16");
    s->prec = precision;
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
    float *da = nullptr, *db = nullptr, *dp = nullptr, *dd = nullptr;
    const size_t slab = (size_t)M * N;
    hipError_t e = hipMalloc((void **)&da, (size_t)M * K * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&db, (size_t)N * K * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&dp, slab * S * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&dd, slab * 4);
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
    for (float *q : {da, db, dp, dd}) if (q) hipFree(q);
    if (e != hipSuccess) return fail(c, AZ_ERR_HIP, std::string("az_solver_gemm_unit: ") + hipGetErrorString(e));
    return AZ_OK;
}

}  // extern "C"
