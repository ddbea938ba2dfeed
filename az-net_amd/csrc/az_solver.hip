// az_solver.hip -- AZ-net TRAINING from conv5_3 on (models/*/VGG16/az-net/train.prototxt): RoIPool with arg-max and its
// backward, the six InnerProduct layers forward / dX / dW on the fp32 matrix cores, ReLU + dropout, the three losses, the
// gradient norm and Caffe's momentum-SGD update.  fp32 master weights in Caffe layout ([out][in], roi_pool5 flattened
// c*49 + p), so the activations are in Caffe order as well and a snapshot is a plain copy.  The parameter store, the kernels
// and their fixed-order reductions are the trainer core's (az_trainer.h); this file is the net: its layers and its graph.
#include "az_trainer.h"

// parameter order of the ABI: W6 b6 W71 b71 W72 b72 Was bas Wab bab Wz bz
enum { P_W6, P_B6, P_W71, P_B71, P_W72, P_B72, P_WAS, P_BAS, P_WAB, P_BAB, P_WZ, P_BZ, NPARAM };
static const char *const PNAME[NPARAM] = {"W6", "b6", "W71", "b71", "W72", "b72", "Was", "bas", "Wab", "bab", "Wz", "bz"};
static const float FILLER_STD[6] = {1e-4f, 1e-4f, 1e-3f, 1e-2f, 1e-3f, 1e-2f};   // int6 int7_1 int7_2 adj_score adj_bbox zoom_score

struct az_solver : az_trainer {
    int n6 = 0, n71 = 0, n72 = 0;
    float drop[3] = {0.5f, 0.5f, 0.5f};
    // one step's activations and gradients (rows: maxR)
    float *lab_as = nullptr, *tgt_ab = nullptr, *wgt_ab = nullptr, *lab_z = nullptr;
    float *pre6 = nullptr, *a6 = nullptr, *pre71 = nullptr, *a71 = nullptr, *pre72 = nullptr, *a72 = nullptr;
    unsigned char *m6 = nullptr, *m71 = nullptr, *m72 = nullptr;
    float *s_as = nullptr, *s_ab = nullptr, *s_z = nullptr;          // raw adj_score / adj_bbox / zoom_score
    float *d_as = nullptr, *d_ab = nullptr, *d_z = nullptr, *d71 = nullptr, *d72 = nullptr, *d6 = nullptr;
};

namespace {

// RoIPool -> int6 -> {int7_1 -> adj_score, adj_bbox; int7_2 -> zoom_score}; train: dropout with the step's masks
int forward_pass(az_solver *s, const float *conv, int N, int H, int W, int cl, const float *rois, int R, bool train,
                 unsigned long long seed, unsigned long long iter)
{
    const int rc = tr_roi_pool_forward(s, conv, N, H, W, cl, rois, R);
    if (rc != AZ_OK) return rc;
    auto key = [&](unsigned layer) { return az_layer_key(seed, iter, layer); };
    fc_forward(s, "int6_fwd", s->pool5, P_W6, R, s->n6, s->K6, s->pre6, s->a6, train && s->drop[0] > 0.f ? s->m6 : nullptr, key(0), train ? s->drop[0] : 0.f);
    fc_forward(s, "int7_1_fwd", s->a6, P_W71, R, s->n71, s->n6, s->pre71, s->a71, train && s->drop[1] > 0.f ? s->m71 : nullptr, key(1), train ? s->drop[1] : 0.f);
    fc_forward(s, "int7_2_fwd", s->a6, P_W72, R, s->n72, s->n6, s->pre72, s->a72, train && s->drop[2] > 0.f ? s->m72 : nullptr, key(2), train ? s->drop[2] : 0.f);
    fc_forward(s, "adj_score_fwd", s->a71, P_WAS, R, 11, s->n71, s->s_as, nullptr, nullptr, 0, 0.f);
    fc_forward(s, "adj_bbox_fwd", s->a71, P_WAB, R, 44, s->n71, s->s_ab, nullptr, nullptr, 0, 0.f);
    fc_forward(s, "zoom_score_fwd", s->a72, P_WZ, R, 1, s->n72, s->s_z, nullptr, nullptr, 0, 0.f);
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
    s->n6 = n6; s->n71 = n71; s->n72 = n72; s->np = NPARAM;
    int nmax = n6 > n71 ? n6 : n71; nmax = nmax > n72 ? nmax : n72; nmax = nmax > 44 ? nmax : 44;
    int rc = tr_init(s, c, "az_solver", PNAME, C, max_rois, (size_t)nmax);
    const size_t K6 = (size_t)s->K6, R = (size_t)max_rois;
    const size_t pn[NPARAM] = {n6 * K6, (size_t)n6, (size_t)n71 * n6, (size_t)n71, (size_t)n72 * n6, (size_t)n72,
                               (size_t)11 * n71, 11, (size_t)44 * n71, 44, (size_t)n72, 1};
    if (rc == AZ_OK) rc = tr_alloc_params(s, 0, NPARAM, pn);
#define SA(p, n) if (rc == AZ_OK) rc = tr_alloc(s, &s->p, (n))
    SA(lab_as, R * 11); SA(tgt_ab, R * 44); SA(wgt_ab, R * 44); SA(lab_z, R);
    SA(pre6, R * n6); SA(a6, R * n6); SA(d6, R * n6); SA(m6, R * n6);
    SA(pre71, R * n71); SA(a71, R * n71); SA(d71, R * n71); SA(m71, R * n71);
    SA(pre72, R * n72); SA(a72, R * n72); SA(d72, R * n72); SA(m72, R * n72);
    SA(s_as, R * 11); SA(s_ab, R * 44); SA(s_z, R); SA(d_as, R * 11); SA(d_ab, R * 44); SA(d_z, R);
#undef SA
    // Caffe's fillers: gaussian weights, zero biases; history zero
    if (rc == AZ_OK && tr_fill_params(s, 0, NPARAM, FILLER_STD, seed) != AZ_OK)
        rc = fail(c, AZ_ERR_HIP, "az_solver_create: initialising the parameters failed");
    if (rc != AZ_OK) { tr_release(s, 0); delete s; return rc; }
    c->solvers.push_back(s);
    *out = s;
    return AZ_OK;
}

int az_solver_destroy(az_solver *s) { return s ? tr_destroy(s, s->c->solvers) : AZ_ERR_INVALID; }

int az_solver_load(az_solver *s, const float *W6, const float *b6, const float *W71, const float *b71, const float *W72,
                   const float *b72, const float *Was, const float *bas, const float *Wab, const float *bab, const float *Wz,
                   const float *bz)
{
    if (!s) return AZ_ERR_INVALID;
    const float *src[NPARAM] = {W6, b6, W71, b71, W72, b72, Was, bas, Wab, bab, Wz, bz};
    return tr_load(s, 0, NPARAM, src);
}

int az_solver_read(az_solver *s, float *W6, float *b6, float *W71, float *b71, float *W72, float *b72, float *Was, float *bas,
                   float *Wab, float *bab, float *Wz, float *bz)
{
    if (!s) return AZ_ERR_INVALID;
    float *dst[NPARAM] = {W6, b6, W71, b71, W72, b72, Was, bas, Wab, bab, Wz, bz};
    return tr_read(s, 0, NPARAM, dst);
}

int az_solver_set_hyper(az_solver *s, const float *lr_mult, const float *decay_mult, const float *dropout_ratio)
{
    if (!s) return AZ_ERR_INVALID;
    return tr_set_hyper(s, NPARAM, lr_mult, decay_mult, dropout_ratio, s->drop, 3);
}

int az_solver_step(az_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                   const float *adj_labels, const float *adj_targets, const float *adj_loss_weights, const float *zoom_labels,
                   uint64_t seed, long long iteration, float *losses_out, double *sumsq_out, float *dmap_dev)
{
    int rc = tr_check_step(s, conv_dev, N, H, W, rois, R, "az_solver_step");
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
      tr_sigmoid_ce(s, s->s_z, s->lab_z, R, R, s->d_z, s->loss + 0);
      tr_sigmoid_ce(s, s->s_as, s->lab_as, R * 11, R, s->d_as, s->loss + 1);
      tr_smooth_l1(s, s->s_ab, s->tgt_ab, s->wgt_ab, R * 44, R, s->d_ab, s->loss + 2); }
    // the three output layers: dW = dy^T x, db, and the gradients of int7_1 / int7_2's outputs (two dx add into d71)
    gemm_any(s, "adj_score_dw", 2, s->d_as, s->a71, s->g[P_WAS], 11, n71, R, s->acc);
    gemm_any(s, "adj_bbox_dw", 2, s->d_ab, s->a71, s->g[P_WAB], 44, n71, R, s->acc);
    gemm_any(s, "zoom_score_dw", 2, s->d_z, s->a72, s->g[P_WZ], 1, n72, R, s->acc);
    { Timed t(c, "bias_grads", 0);
      tr_colsum(s, s->d_as, R, 11, s->g[P_BAS], s->acc); tr_colsum(s, s->d_ab, R, 44, s->g[P_BAB], s->acc); tr_colsum(s, s->d_z, R, 1, s->g[P_BZ], s->acc); }
    gemm_any(s, "adj_score_dx", 1, s->d_as, s->w[P_WAS], s->d71, R, n71, 11, 0);
    gemm_any(s, "adj_bbox_dx", 1, s->d_ab, s->w[P_WAB], s->d71, R, n71, 44, 1);
    gemm_any(s, "zoom_score_dx", 1, s->d_z, s->w[P_WZ], s->d72, R, n72, 1, 0);
    tr_act_bwd(s, s->d71, s->pre71, s->m71, s->drop[1], R, n71);
    tr_act_bwd(s, s->d72, s->pre72, s->m72, s->drop[2], R, n72);
    gemm_any(s, "int7_1_dw", 2, s->d71, s->a6, s->g[P_W71], n71, n6, R, s->acc);
    gemm_any(s, "int7_2_dw", 2, s->d72, s->a6, s->g[P_W72], n72, n6, R, s->acc);
    { Timed t(c, "bias_grads", 0); tr_colsum(s, s->d71, R, n71, s->g[P_B71], s->acc); tr_colsum(s, s->d72, R, n72, s->g[P_B72], s->acc); }
    // int7_1 and int7_2 both read int6: their two dx add
    gemm_any(s, "int7_1_dx", 1, s->d71, s->w[P_W71], s->d6, R, n6, n71, 0);
    gemm_any(s, "int7_2_dx", 1, s->d72, s->w[P_W72], s->d6, R, n6, n72, 1);
    tr_act_bwd(s, s->d6, s->pre6, s->m6, s->drop[0], R, n6);
    gemm_any(s, "int6_dw", 2, s->d6, s->pool5, s->g[P_W6], n6, K6, R, s->acc);
    { Timed t(c, "bias_grads", 0); tr_colsum(s, s->d6, R, n6, s->g[P_B6], s->acc); }
    if (dmap_dev) {
        gemm_any(s, "int6_dx", 1, s->d6, s->w[P_W6], s->dpool, R, K6, n6, 0);
        tr_roi_pool_backward(s, N, H, W, channels_last, dmap_dev);
    }
    if ((rc = tr_grad_norm(s, NPARAM, 3, losses_out, sumsq_out)) != AZ_OK) return rc;
    s->trained = dmap_dev ? 2 : 1;
    return AZ_OK;
}

int az_solver_update(az_solver *s, double rate, double momentum, double weight_decay, double clip_scale)
{
    if (!s) return AZ_ERR_INVALID;
    return tr_update(s, NPARAM, rate, momentum, weight_decay, clip_scale);
}

int az_solver_forward_test(az_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                           float *zoom_score, float *adj_score, float *adj_bbox)
{
    int rc = tr_check_step(s, conv_dev, N, H, W, rois, R, "az_solver_forward_test");
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
    return tr_fetch(s, nm, src, bytes, out, cap_bytes, bytes_out);
}

int az_solver_set_precision(az_solver *s, int precision) { return tr_set_precision(s, precision); }

int az_solver_set_accumulate(az_solver *s, int on) { return tr_set_accumulate(s, on); }

int az_solver_load_history(az_solver *s, const float *W6, const float *b6, const float *W71, const float *b71, const float *W72,
                           const float *b72, const float *Was, const float *bas, const float *Wab, const float *bab,
                           const float *Wz, const float *bz)
{
    if (!s) return AZ_ERR_INVALID;
    const float *src[NPARAM] = {W6, b6, W71, b71, W72, b72, Was, bas, Wab, bab, Wz, bz};
    return tr_load_history(s, 0, NPARAM, src);
}

}  // extern "C"
