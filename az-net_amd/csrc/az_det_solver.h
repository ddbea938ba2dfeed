// az_det_solver.h -- the detection trainer's state, shared by az_det_solver.hip (the head behind pool5) and
// az_skip_train.hip (the skip-connection front in TRAIN phase, which produces pool5 in place of roi_pool5).
#pragma once
#include "az_trainer.h"

// parameter order of the ABI: W6 b6 W7 b7 Wc bc Wb bb (fc6, fc7, cls_score, bbox_pred); behind them, once a skip front is
// attached, conv_pool5's Wp bp
enum { D_W6, D_B6, D_W7, D_B7, D_WC, D_BC, D_WB, D_BB, DNPARAM, D_WP = DNPARAM, D_BP, DNALL };
static const char *const DPNAME[DNALL] = {"W6", "b6", "W7", "b7", "Wc", "bc", "Wb", "bb", "Wp", "bp"};
static const float DET_FILLER_STD[4] = {5e-3f, 5e-3f, 1e-2f, 1e-3f};      // fc6 fc7 (without a pretrained model) cls_score bbox_pred

struct az_det_solver : az_trainer {
    int n6 = 0, n7 = 0, ncls = 0;
    float drop[2] = {0.5f, 0.5f};
    // one step's activations and gradients (rows: maxR)
    float *labels = nullptr, *tgt = nullptr, *wgt = nullptr;
    float *pre6 = nullptr, *a6 = nullptr, *pre7 = nullptr, *a7 = nullptr;
    unsigned char *m6 = nullptr, *m7 = nullptr;
    float *s_cls = nullptr, *prob = nullptr, *s_bb = nullptr;                  // raw cls_score, cls_prob, bbox_pred
    float *d_cls = nullptr, *d_bb = nullptr, *d7 = nullptr, *d6 = nullptr;
    int has_prob = 0;
    // the skip front (az_det_solver_attach_skip): rows (roi, bin) x sumC channels
    struct Skip {
        bool attached = false;
        int n = 0, C[AZ_SKIP_MAX_SRC] = {0, 0, 0}, off[AZ_SKIP_MAX_SRC] = {0, 0, 0}, sumC = 0;
        float scale[AZ_SKIP_MAX_SRC] = {0.f, 0.f, 0.f};
        double gain = 0.0, eps = 0.0;
        int *geo = nullptr, *arg = nullptr;                     // geo [n][maxR][8]; arg-max [rows][sumC]
        float *cat = nullptr, *d_y = nullptr, *d_cat = nullptr, *d_raw = nullptr;
        double *fac = nullptr;                                  // f = gain / sqrt(ss + eps) [rows][n]
        int rows = 0, trained = 0, has_dcat = 0;                // of the last skip pass (has_dcat: it computed d_cat / d_raw)
    } sk;
    // hard-example mining (az_det_mine.hip); allocated at the first az_det_solver_mine*
    struct Mine {
        float *rec = nullptr, *loss = nullptr, *lcls = nullptr, *lbb = nullptr, *tgt4 = nullptr;   // records [maxR][5]; losses [maxR]; compact targets
        long long *keep = nullptr;                              // the NMS kernels' keep lists, image by image at its first row
        int *keep_rows = nullptr, *flag = nullptr;              // the same as global rows (-1 behind a list); "a loss is not finite"
        int *goff = nullptr, *gsel = nullptr, *nkeep = nullptr, *nsel = nullptr;     // per image (capN of them)
        int capN = 0, R = 0, N = 0;                             // R, N: of the last mining pass
        std::vector<int> off, small, h_sel, h_nsel;             // host: row ranges, the small groups, the result before it is handed over
    } mn;
};

// ---- az_det_solver.hip: the head behind pool5 [R][C * 49], for both fronts ----------------------------------------------------
// fc6 -> fc7 -> {cls_score, bbox_pred} on s->pool5
void det_head_forward(az_det_solver *s, int R, bool train, unsigned long long seed, unsigned long long iter);
// the two losses and the backward down to d_pre6 (and, with want_dpool, d_pool5)
void det_head_backward(az_det_solver *s, int R, bool want_dpool);
// labels / targets checked and copied to the device (before anything else is enqueued)
int det_stage_targets(az_det_solver *s, int R, const float *labels, const float *bbox_targets, const float *bbox_loss_weights,
                      long long iteration, const std::string &who);
void det_softmax_test(az_det_solver *s, int R);
// ---- az_det_mine.hip ------------------------------------------------------------------------------------------------------------
// the mining pass's saved tensors by name (mine_loss, mine_loss_cls, mine_loss_bbox, mine_keep, mine_nkeep)
bool det_mine_fetch(az_det_solver *s, const std::string &name, const void **src, size_t *bytes);
// ---- az_skip_train.hip ----------------------------------------------------------------------------------------------------------
// the front's saved tensors by name (cat, skip_argmax, skip_factor, d_y, d_cat, d_raw)
bool skip_train_fetch(az_det_solver *s, const std::string &name, const void **src, size_t *bytes);
// what az_det_solver_step_skip / _forward_test_skip refuse before they enqueue anything (`who`: the entry's name)
int skip_pass_check(az_det_solver *s, const std::string &who, int n_src, const int *Cs, const void *const *maps, const int *Hs,
                    const int *Ws, int N, const float *rois, int R);
// what az_det_solver_forward_test_skip enqueues in front of its softmax: roi_pool* .. relu_pool into pool5, then the head, TEST phase
int skip_test_forward(az_det_solver *s, const void *const *maps_dev, const int *Hs, const int *Ws, int N, int channels_last,
                      const float *rois, int R);
