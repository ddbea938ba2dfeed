// az_trainer.h -- what the AZ-net trainer (az_solver.hip) and the detection trainer (az_det_solver.hip, az_skip_train.hip) are
// both made of: the parameter store, RoIPool's buffers, the split-K slabs and the reduction buffers, and the host functions on
// them (az_trainer.hip, which also holds every kernel they launch).  A trainer struct derives from az_trainer and adds its own
// layers' buffers; its forward and backward graphs stay written out in its own file, in calls to the functions below.
#pragma once
#include "az_solver_dev.h"

constexpr int TR_MAXP = 12;               // parameters of the largest trainer (az_solver: six layers' W and b)

struct az_trainer {
    az_ctx *c = nullptr;
    const char *tag = "";                 // "az_solver" / "az_det_solver": the prefix of the ABI's names in error messages
    const char *const *pname = nullptr;   // names of the parameters, in the ABI's order
    int np = 0;                           // parameters that exist (the detection trainer: 8, with a skip front 10)
    int C = 0, K6 = 0, maxR = 0;
    size_t pn[TR_MAXP] = {0};
    float *w[TR_MAXP] = {nullptr}, *g[TR_MAXP] = {nullptr}, *h[TR_MAXP] = {nullptr};
    float lr_mult[TR_MAXP], decay_mult[TR_MAXP];
    // RoIPool of one step (rows: maxR), the split-K slabs, the losses and the gradient norm's partials (TR_MAXP x SQ_BLOCKS)
    float *rois = nullptr;
    int *geo = nullptr, *argmax = nullptr;
    float *pool5 = nullptr, *dpool = nullptr;
    float *part = nullptr, *loss = nullptr;
    double *sq_part = nullptr, *sq = nullptr;
    size_t part_elems = 0;
    DevList allocs;
    // shape of the last step (what the debug fetch sizes its answers by)
    int R = 0, N = 0, H = 0, W = 0, trained = 0;
    int prec = AZ_TRAIN_FP32;             // operands of every matrix product (*_set_precision)
    int acc = 0;                          // 1: a step adds its parameter gradients to what g holds (*_set_accumulate)
};

// ---- memory ------------------------------------------------------------------------------------------------------------------
template <typename T>
int tr_alloc(az_trainer *t, T **p, size_t n)                                  // n elements in t->allocs, a view of them in *p
{
    if (t->allocs.alloc(p, n) == hipSuccess) return AZ_OK;
    return fail(t->c, AZ_ERR_HIP, std::string(t->tag) + ": " + alloc_what(n * sizeof(T)) + " failed");
}
// frees what was allocated from allocs[mark] on (0: everything) and forgets the parameters from t->np on
void tr_release(az_trainer *t, size_t mark);
// *_destroy: waits for the stream, frees the trainer's memory, takes it off its context's list and deletes it
template <typename S>
int tr_destroy(S *s, std::vector<S *> &list)
{
    hipSetDevice(s->c->device);
    hipStreamSynchronize(s->c->stream);
    tr_release(s, 0);
    for (size_t i = 0; i < list.size(); ++i) if (list[i] == s) { list.erase(list.begin() + i); break; }
    delete s;
    return AZ_OK;
}
// c, tag, names, C, K6, maxR; then rois .. sq: `widest` is the widest layer (part_elems = max(maxR * widest, 4M floats))
int tr_init(az_trainer *t, az_ctx *c, const char *tag, const char *const *pname, int C, int max_rois, size_t widest);

// ---- parameters [p0, p1) -------------------------------------------------------------------------------------------------------
// sizes pn[0 .. p1 - p0): w / g / h allocated, Caffe's multipliers (weights 1 / 1, biases 2 / 0).  t->np is the caller's to raise.
int tr_alloc_params(az_trainer *t, int p0, int p1, const size_t *pn);
// Caffe's fillers: gradients, history and biases zero, weight p gaussian with stdv[(p - p0) / 2] from the key (seed, 0, 16 + p)
// (stdv null: the weights are the caller's to fill, before this call); waits for the stream.  AZ_OK or AZ_ERR_HIP, no message.
int tr_fill_params(az_trainer *t, int p0, int p1, const float *stdv, uint64_t seed);
int tr_load(az_trainer *t, int p0, int p1, const float *const *src);         // a null array keeps what the trainer holds
int tr_read(az_trainer *t, int p0, int p1, float *const *dst);
int tr_load_history(az_trainer *t, int p0, int p1, const float *const *src); // tr_load into h; `trained` stays as it is
// *_set_hyper on the first n parameters: everything is checked before anything is stored (drop: the trainer's ndrop ratios)
int tr_set_hyper(az_trainer *t, int n, const float *lr_mult, const float *decay_mult, const float *dropout_ratio, float *drop, int ndrop);
int tr_set_precision(az_trainer *t, int precision);
int tr_set_accumulate(az_trainer *t, int on);

// ---- one step --------------------------------------------------------------------------------------------------------------------
int tr_check_rois(az_trainer *t, int N, const float *rois, int R, const std::string &who);
int tr_check_step(az_trainer *t, const float *conv, int N, int H, int W, const float *rois, int R, const std::string &who);
// geo [R][8] of device rois at one scale (k_solver_roi_geo)
void tr_roi_geo(hipStream_t st, const float *rois_dev, int R, float scale, int *geo);
// rois to the device, RoIPool 7x7 with arg-max into pool5 / argmax; notes the step's shape
int tr_roi_pool_forward(az_trainer *t, const float *conv, int N, int H, int W, int cl, const float *rois, int R);
void tr_roi_pool_backward(az_trainer *t, int N, int H, int W, int cl, float *dmap);       // dpool -> d conv5_3 by arg-max
// the gather behind it, for any layout of the pooled gradient (PoolStrides, az_solver_dev.h), timed as `name`
void tr_pool_gather(az_ctx *c, const char *name, const float *dpool, const int *argmax, const int *geo, int R, const MapView &m,
                    const PoolStrides &st, float *dmap);
// y = x W^T + b into `pre` (and, for the hidden layers, ReLU + dropout into `act`); pw: the layer's W (its b follows)
void fc_forward(az_trainer *t, const char *name, const float *x, int pw, int R, int N, int K, float *pre, float *act,
                unsigned char *mask, unsigned long long key, float ratio);
// D (+)= product of the given form, split-K through the slabs when the tile count alone would leave the chip idle
void gemm_any(az_trainer *t, const char *name, int form, const float *A, const float *B, float *D, int M, int N, int K, int accumulate);
// db[j] (+)= sum over rows, in row order (accumulate: the finished sum is added once to what db holds)
void tr_colsum(az_trainer *t, const float *dy, int R, int N, float *db, int accumulate);
// ReLU and dropout backward of a hidden layer, in place
void tr_act_bwd(az_trainer *t, float *d, const float *pre, const unsigned char *mask, float ratio, int R, int N);
// SigmoidCrossEntropyLoss / SmoothL1Loss of n elements normalised by num: the gradient into dx, the loss into *loss (device)
void tr_sigmoid_ce(az_trainer *t, const float *x, const float *tgt, int n, int num, float *dx, float *loss);
void tr_smooth_l1(az_trainer *t, const float *x, const float *tgt, const float *wgt, int n, int num, float *dx, float *loss);
// the sum of squares of the first n parameters' gradients; brings it and the first k losses back and waits for the stream
int tr_grad_norm(az_trainer *t, int n, int k, float *losses_out, double *sumsq_out);
int tr_update(az_trainer *t, int n, double rate, double momentum, double weight_decay, double clip_scale);   // SGD, first n
// *_fetch behind the trainer's own table: src null looks up g_ / h_ / w_ + a parameter's name; then the size query or the copy
int tr_fetch(az_trainer *t, const std::string &nm, const void *src, size_t bytes, void *out, long long cap_bytes, long long *bytes_out);

// ---- launch helpers (az_skip_train.hip's own kernels and its conv_pool5 forward) ----------------------------------------------
int grid_for(long long n, int cap = 65535 * 16);
void pick_split(int M, int N, int K, int *S, int *Kc);
// form 0: A [M][K], B [N][K]; 1: A [M][K], B [K][N]; 2: A [K][M], B [K][N]; prec: AZ_TRAIN_FP32 / AZ_TRAIN_BF16 (operands)
void launch_gemm(hipStream_t s, int form, const float *A, const float *B, float *D, long long slab, int M, int N, int K, int S,
                 int Kc, int accumulate, int prec);
