// az_detect.hip -- the Fast R-CNN head on the shared conv map (lib/detect/test.py:259-318,432-445): its
// loaders, one record for what a pass reads (DetPass), one function that enqueues a pass (det_pass_enqueue: projection +
// dedup, head, gather) and the entries built from it: az_det_forward*, az_detect*, az_detect_batch; and az_skip_pool.
#include "az_ctx.h"

extern "C" {

static const size_t DET_SEG_HDR = (sizeof(AzDetSeg) + 255) / 256 * 256;
static size_t det_seg_bytes(const az_ctx *c) { return DET_SEG_HDR + (size_t)c->maxR * 4 * sizeof(double); }

// az_load_det_head / az_load_det_head_lowrank past their argument checks.  r6 / r7 == 0: that layer at full rank, W6 / W7
// its [out, in] weight, L6 / L7 unused; otherwise W6 / W7 is the layer's U factor [out, r] and L6 / L7 its L factor [r, in].
static int load_det_head(az_ctx *c, int C, int n6, int n7, int ncls, int r6, int r7, const float *L6, const float *W6,
                         const float *b6, const float *L7, const float *W7, const float *b7, const float *Wc,
                         const float *bc, const float *Wb, const float *bb)
{
    int rc = ensure_geom(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->allocs_det.release();
    if (!c->head_loaded) c->pool5 = nullptr;     // (without an AZ head pool5 was the detection head's own: gone with the list)
    c->det_loaded = false;
    c->det_fc6 = c->det_fc7 = FcLayer(); c->dlr_t = c->dlr_zero = nullptr;
    const size_t R = (size_t)c->maxR, K6 = (size_t)C * 49, NO = (size_t)5 * ncls;
    c->det_ncls = ncls;
    FcLayer &f6 = c->det_fc6, &f7 = c->det_fc7;
    f6 = FcLayer{n6, (int)K6, azk_fc_split((int)K6), r6, r6 ? azk_lowrank_split((int)K6, r6) : 0};
    f7 = FcLayer{n7, n6, azk_fc_split(n6), r7, r7 ? azk_lowrank_split(n6, r7) : 0};
    DevList &list = c->allocs_det;
    // (16-bit-term modes: fc6 as int6 where an AZ head's operand planes exist; a failed LDS opt-in leaves fc6 on the fp32 GEMM)
    const int parts6 = (!r6 && c->gemm_parts && c->pool5p && azk_fc_terms_prepare(c->gemm_parts) == 0) ? c->gemm_parts : 0;
    if ((rc = fc_layer_alloc(c, list, f6, parts6)) != AZ_OK || (rc = fc_layer_alloc(c, list, f7, 0)) != AZ_OK) return rc;
    if (r6 || r7) {
        // the L stages' output rows [R][r] (one buffer: the stream orders fc6_U before fc7_L) and their zero bias
        const size_t rm = (size_t)(r6 > r7 ? r6 : r7);
        AZ_A(dlr_t, R * rm); AZ_A(dlr_zero, rm);
        HIPCHK(c, hipMemsetAsync(c->dlr_zero, 0, rm * sizeof(float), c->stream));
        f6.zero = f7.zero = c->dlr_zero;
    }
    AZ_A(dWt, azk_tiled_elems((int)NO, n7)); AZ_A(dbt, NO);
    AZ_A(dh6, R * n6); AZ_A(dh7, R * n7);
    const size_t in6 = (size_t)f6.lead() * K6, in7 = (size_t)f7.lead() * n6;     // fc6's matrix is permuted through dpart
    AZ_A(dpart, std::max(std::max(f6.slab_elems(R), f7.slab_elems(R)), std::max((size_t)AZK_TAIL_SPLIT * R * NO, in6)));
    AZ_A(dprob_u, R * ncls); AZ_A(ddelta_u, R * 4 * ncls); AZ_A(dpred_u, R * ncls * 4); AZ_A(dprob, R * ncls); AZ_A(dpred, R * ncls * 4);
    AZ_A(dseg_dev, det_seg_bytes(c)); AZ_A(drow_hw, R * 2);
    c->dseg_own.reset(); c->dseg_host = nullptr;
    HIPCHK(c, c->dseg_own.reserve(det_seg_bytes(c)));
    c->dseg_host = c->dseg_own.as<unsigned char>();
    if (!c->pool5) { AZ_A(pool5, R * K6); }     // normally the AZ head's buffer is shared
    c->dgscale = nullptr;
    if (parts6) {
        AZ_A(dgscale, 4);
        HIPCHK(c, hipMemsetAsync(c->dgscale, 0, 4 * sizeof(float), c->stream));
    }
    if (!c->head_loaded) { c->d.C = C; c->d.pooled = 7; c->d.K6 = (int)K6; }
    {
        Buf tg;
        HIPCHK(c, tg.reserve(std::max(std::max(in6, in7), NO * n7) * 4));
        float *tmp = tg.as<float>();
        // (fc6: bin-major columns, like the AZ head)
        if ((rc = fc_layer_load(c, f6, L6, W6, b6, C, c->dpart, tmp)) != AZ_OK) return rc;
        if ((rc = fc_layer_load(c, f7, L7, W7, b7, 0, nullptr, tmp)) != AZ_OK) return rc;
        // rows 0..ncls-1 cls_score, ncls..5*ncls-1 bbox_pred
        HIPCHK(c, hipMemcpy(tmp, Wc, (size_t)ncls * n7 * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(tmp + (size_t)ncls * n7, Wb, (size_t)4 * ncls * n7 * 4, hipMemcpyHostToDevice));
        azk_tile_weights(c->stream, tmp, c->dWt, (int)NO, n7);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    HIPCHK(c, hipMemcpy(c->dbt, bc, (size_t)ncls * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->dbt + ncls, bb, (size_t)4 * ncls * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipDeviceSynchronize());
    c->det_loaded = true;
    if (c->skip.loaded && c->skip.Cout != C) c->skip = az_ctx::SkipFront();     // (a skip front folds to the head's C)
    return AZ_OK;
}

// what az_load_det_head and az_load_det_head_lowrank (`who`) both refuse first; ptrs: every pointer both take is there
static int det_head_args(az_ctx *c, const char *who, int C, int n6, int n7, int ncls, bool ptrs)
{
    if (!c) return AZ_ERR_INVALID;
    const std::string me(who);
    if (!ptrs) return fail(c, AZ_ERR_INVALID, me + ": null pointer");
    if (C <= 0 || (C & 3) || n6 <= 0 || (n6 & 3) || n7 <= 0 || (n7 & 3) || ncls < 2 || ncls > 256)
        return fail(c, AZ_ERR_INVALID, me + ": C, n6, n7 multiples of 4; 2 <= ncls <= 256");
    if (c->head_loaded && C != c->d.C) return fail(c, AZ_ERR_INVALID, me + ": C differs from the AZ head's");
    return AZ_OK;
}

int az_load_det_head(az_ctx *c, int C, int n6, int n7, int ncls, const float *W6, const float *b6,
                     const float *W7, const float *b7, const float *Wc, const float *bc, const float *Wb,
                     const float *bb)
{
    const int rc = det_head_args(c, "az_load_det_head", C, n6, n7, ncls, W6 && b6 && W7 && b7 && Wc && bc && Wb && bb);
    if (rc) return rc;
    return load_det_head(c, C, n6, n7, ncls, 0, 0, nullptr, W6, b6, nullptr, W7, b7, Wc, bc, Wb, bb);
}

// Truncated-SVD head (Fast R-CNN section 4.4): fc6 and / or fc7 as L [r, in] (no bias) then U [out, r] (+ bias, ReLU).
int az_load_det_head_lowrank(az_ctx *c, int C, int n6, int n7, int ncls, int r6, int r7, const float *L6,
                             const float *U6, const float *b6, const float *L7, const float *U7, const float *b7,
                             const float *Wc, const float *bc, const float *Wb, const float *bb)
{
    const int rc = det_head_args(c, "az_load_det_head_lowrank", C, n6, n7, ncls, U6 && b6 && U7 && b7 && Wc && bc && Wb && bb);
    if (rc) return rc;
    const long long K6 = (long long)C * 49;
    auto rank_ok = [](int r, long long out, long long in) {
        return r == 0 || (r >= 4 && !(r & 3) && r <= out && r <= in && r <= AZ_LOWRANK_MAX);
    };
    if (!rank_ok(r6, n6, K6) || !rank_ok(r7, n7, n6))
        return fail(c, AZ_ERR_INVALID, "az_load_det_head_lowrank: a rank is 0 (full) or a multiple of 4 in [4, min(out, in, AZ_LOWRANK_MAX)]");
    if ((r6 != 0) != (L6 != nullptr) || (r7 != 0) != (L7 != nullptr))
        return fail(c, AZ_ERR_INVALID, "az_load_det_head_lowrank: L is NULL exactly for a layer of rank 0");
    if (c->gemm_parts && (r6 || r7))
        return fail(c, AZ_ERR_STATE, "az_load_det_head_lowrank: fp32 only (the 16-bit-term GEMM modes do not run a low-rank head)");
    return load_det_head(c, C, n6, n7, ncls, r6, r7, L6, U6, b6, L7, U7, b7, Wc, bc, Wb, bb);
}

int az_lowrank_split(int K, int r) { return (K > 0 && r > 0) ? azk_lowrank_split(K, r) : AZ_ERR_INVALID; }

// The U-stage kernel alone (tests): Y [M, N] = act(X [M, K] . W [N, K]^T + b), host arrays.
int az_lowrank_gemm_unit(az_ctx *c, const float *X, const float *W, const float *b, int M, int N, int K, int relu,
                         float *Y)
{
    if (!c) return AZ_ERR_INVALID;
    if (M < 0 || N <= 0 || (N & 3) || K <= 0 || (K & 3) || K > AZ_LOWRANK_MAX)
        return fail(c, AZ_ERR_INVALID, "az_lowrank_gemm_unit: M >= 0; N, K positive multiples of 4; K <= AZ_LOWRANK_MAX");
    if (M > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_lowrank_gemm_unit: more rows than the region capacity");
    if (M == 0) return AZ_OK;
    if (!X || !W || !b || !Y) return fail(c, AZ_ERR_INVALID, "az_lowrank_gemm_unit: null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    constexpr int GUARD = 64;                     // rows behind row M that the launch must leave as they are
    const size_t ny = (size_t)(M + GUARD) * N;
    Buf bx, bw, bb, by, bm;
    HIPCHK(c, bx.reserve((size_t)M * K * 4)); HIPCHK(c, bw.reserve((size_t)N * K * 4)); HIPCHK(c, bb.reserve((size_t)N * 4));
    HIPCHK(c, by.reserve(ny * 4)); HIPCHK(c, bm.reserve(sizeof(int)));
    HIPCHK(c, hipMemcpy(bx.p, X, (size_t)M * K * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(bw.p, W, (size_t)N * K * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(bb.p, b, (size_t)N * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(bm.p, &M, sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(by.p, 0xA5, ny * 4));
    azk_lowrank_gemm(c->stream, bx.as<float>(), K, bw.as<float>(), bb.as<float>(), bm.as<int>(), M + GUARD, N, K,
                     relu ? 1 : 0, by.as<float>(), N);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned> guard((size_t)GUARD * N);
    HIPCHK(c, hipMemcpy(guard.data(), by.as<float>() + (size_t)M * N, guard.size() * 4, hipMemcpyDeviceToHost));
    for (unsigned g : guard)
        if (g != 0xA5A5A5A5u) return fail(c, AZ_ERR_HIP, "az_lowrank_gemm_unit: the kernel wrote a row past M");
    HIPCHK(c, hipMemcpy(Y, by.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return AZ_OK;
}

// What one pass of the detection head reads.  The family of entries is projection x pool source x rounds (DetIter, below).
struct DetPass {
    double dedup = 0.0; int batch_size = 1, im_h = 1, im_w = 1; double eps = 0.0;
    // projection: one `scale` | the image pyramid `pyr` | the `nseg` images `seg` (device) of an az_detect_batch pass, their
    // boxes side by side in seg_boxes and row_hw [row][2] every unique row's image size (null: im_h, im_w)
    double scale = 0.0; const AzPyrScales *pyr = nullptr;
    const AzDetSeg *seg = nullptr; int nseg = 0; const double *seg_boxes = nullptr; int *row_hw = nullptr;
    // pool source: the context's map | the map table feats / feat_hw (roi column 0 indexes it) | the skip-connection front
    // (az_skip.hip: pool5 comes from it instead of RoIPool)
    const float *const *feats = nullptr; const int *feat_hw = nullptr; bool skip = false;
};

// the detection head on the *Uptr rois in ctx->urois / ctx->ubox
// (rows_bound: what the host knows about the row count -- the number of boxes before the 1/16 dedup)
static void launch_det_head(az_ctx *c, const DetPass &p, const int *Uptr, int rows_bound)
{
    AzHeadDims d = c->d;
    const int K6 = d.C * 49, NO = 5 * c->det_ncls;
    d.K6 = K6;
    // many rows (the reference's 300 proposals per image): fc6 / fc7 on the many-row GEMM, as int6 (same bits either way)
    const bool many_rows = rows_bound >= c->gemm12_min_rows;
    const bool terms = c->gemm_parts && c->det_fc6.Wp;             // (16-bit-term modes: fc6, 86 % of this head's FLOPs, as int6)
    if (terms && c->gemm_parts == 2)
        azk_feat_scale(c->stream, c->feat, (long long)d.C * d.H * d.W, c->dgscale, c->det_fc6.w_scale);
    if (p.skip) skip_front_launch(c, Uptr, rows_bound);
    else
    { Timed t(c, "det_roi_pool", 0);
      azk_roi_pool(c->stream, c->feat, d, c->spatial_scale, c->urois, Uptr, c->maxR, c->pool5, terms ? c->pool5p : nullptr,
                   terms ? azk_act_plane_elems(c->maxR, K6) : 0, terms ? c->gemm_parts : 0, 0, 0,
                   (terms && c->gemm_parts == 2) ? c->dgscale : nullptr, p.feats, p.feat_hw); }
    // (a truncated-SVD layer's L stage stays on k_fc_splitk whatever the row count: its chunk count, azk_lowrank_split, was
    //  chosen for that kernel.  dlr_t [maxR][max(r6, r7)] serves both layers: all launches are on c->stream, so fc7_L's slab
    //  sum overwrites it only after fc6_U has read it)
    const FcLayer &f6 = c->det_fc6, &f7 = c->det_fc7;
    fc_layer_forward(c, c->stream, f6, {c->pool5, c->pool5p, azk_act_plane_elems(c->maxR, K6), c->dpart, c->dlr_t, c->dh6, c->dgscale},
                     Uptr, many_rows && !f6.r, {"det_fc6_gemm", "det_fc6_reduce", "det_fc6_L", "det_fc6_L_reduce", "det_fc6_U"}, 0);
    fc_layer_forward(c, c->stream, f7, {c->dh6, nullptr, 0, c->dpart, c->dlr_t, c->dh7, nullptr},
                     Uptr, many_rows && !f7.r, {"det_fc7_gemm", "det_fc7_reduce", "det_fc7_L", "det_fc7_L_reduce", "det_fc7_U"}, 0);
    { Timed t(c, "det_tail_gemm", 0, 1);
      azk_fc_gemm(c->stream, c->dh7, f7.N, c->dWt, f7.N, Uptr, c->maxR, NO, f7.N, AZK_TAIL_SPLIT,
                  c->dpart); }
    { Timed t(c, "det_epilogue", 0);
      azk_det_epilogue(c->stream, c->dpart, AZK_TAIL_SPLIT, c->det_ncls, c->dbt, c->ubox, Uptr, c->maxR, p.im_h, p.im_w,
                       p.eps, c->dprob_u, c->ddelta_u, c->dpred_u, p.row_hw); }
}

// One pass on c->stream: projection + 1/16 dedup of the boxes (B[0] / P[0], or the segments of a batch pass) into urois /
// ubox / U[0], the head over those rows and -- gather_n: the device count of boxes, null: none -- the un-dedup gather of
// every box's row into dprob / dpred.  Every az_detect* entry is made of this.
// (only the batch pass times its dedup: the lists of az_last_kernel_times are what bench and the perf scripts key on)
static void det_pass_enqueue(az_ctx *c, const DetPass &p, int rows_bound, const int *gather_n)
{
    hipStream_t s = c->stream;
    int *Uptr = &c->cnt->U[0];
    if (p.seg)
    { Timed t(c, "det_rois_dedup", 0);
      azk_rois_dedup(s, p.seg_boxes, p.seg, p.nseg, c->maxR, (float)p.dedup, p.batch_size, c->rois, c->key, c->grp, c->first,
                     c->index, c->inv, c->urois, c->ubox, Uptr, p.row_hw); }
    else
        azk_rois_dedup(s, c->B[0], &c->cnt->P[0], c->maxR, p.scale, p.pyr, (float)p.dedup, p.batch_size, c->rois, c->key,
                       c->grp, c->first, c->index, c->inv, c->urois, c->ubox, Uptr);
    launch_det_head(c, p, Uptr, rows_bound);
    if (gather_n) azk_det_gather(s, gather_n, c->inv, c->det_ncls, c->dprob_u, c->dpred_u, c->dprob, c->dpred);
}

static int check_det(az_ctx *c)
{
    if (!c) return AZ_ERR_INVALID;
    if (!c->det_loaded) return fail(c, AZ_ERR_STATE, "az_load_det_head has not been called");
    if (!c->feat) return fail(c, AZ_ERR_STATE, "no feature map set");
    return AZ_OK;
}

// az_det_forward / az_det_forward_skip: the head alone on R host rois
static int det_forward(az_ctx *c, const float *rois, int R, float *cls_prob, float *bbox_pred, bool skip)
{
    int rc = skip ? skip_check(c, "az_det_forward_skip", true) : check_det(c);
    if (rc) return rc;
    if (skip && R > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_det_forward_skip: too many rois");
    if ((rc = stage_rois(c, rois, R)) != AZ_OK) return rc;
    if (!(c->profiling & 4)) clear_events(c);
    DetPass p;
    p.skip = skip;
    launch_det_head(c, p, &c->cnt->U[0], R);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    const size_t nc = (size_t)c->det_ncls;
    if (R && cls_prob) HIPCHK(c, hipMemcpy(cls_prob, c->dprob_u, (size_t)R * nc * 4, hipMemcpyDeviceToHost));
    if (R && bbox_pred) HIPCHK(c, hipMemcpy(bbox_pred, c->ddelta_u, (size_t)R * 4 * nc * 4, hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_det_forward(az_ctx *c, const float *rois, int R, float *cls_prob, float *bbox_pred)
{
    return det_forward(c, rois, R, cls_prob, bbox_pred, false);
}

int az_det_forward_skip(az_ctx *c, const float *rois, int R, float *cls_prob, float *bbox_pred)
{
    return det_forward(c, rois, R, cls_prob, bbox_pred, true);
}

// the stream's detections of P boxes (dprob / dpred: every box's row, after the un-dedup gather) to the host
static int fetch_dets(az_ctx *c, int P, float *scores_out, double *boxes_out)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    const size_t nc = (size_t)c->det_ncls;
    if (scores_out) HIPCHK(c, hipMemcpy(scores_out, c->dprob, (size_t)P * nc * 4, hipMemcpyDeviceToHost));
    if (boxes_out) HIPCHK(c, hipMemcpy(boxes_out, c->dpred, (size_t)P * nc * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return AZ_OK;
}

// The rounds of az_detect_iter* and where their extras go; as constructed: the one round of az_detect*.
struct DetIter {
    int rounds = 1; double min_score = 0.0; int max_rows = 1;
    int32_t *cls = nullptr, *src = nullptr; float *score = nullptr; double *box = nullptr; int32_t *count = nullptr;
};

// what the entry `who` refuses about its boxes, its projection and its rounds
static int detect_args(az_ctx *c, const char *who, const double *boxes, int P, const DetPass &p, const DetIter &it)
{
    const std::string w(who);
    if (P < 0 || (P && !boxes) || p.batch_size <= 0 || (!p.pyr && !(p.scale > 0))) return fail(c, AZ_ERR_INVALID, w + ": bad arguments");
    if (p.pyr && c->pyr_S != p.pyr->S)
        return fail(c, AZ_ERR_STATE, w + ": no pyramid of that many maps set (az_set_feature_pyramid_dev_nhwc)");
    if (it.rounds < 1 || it.rounds > AZ_ITER_LOC_MAX_ROUNDS) return fail(c, AZ_ERR_INVALID, w + ": 1 <= rounds <= AZ_ITER_LOC_MAX_ROUNDS");
    if (it.max_rows < 1 || it.max_rows > AZ_TOPK_MAX) return fail(c, AZ_ERR_INVALID, w + ": 1 <= max_rows <= 4096");
    if (it.rounds > 1 && (!it.cls || !it.src || !it.score || !it.box || !it.count))
        return fail(c, AZ_ERR_INVALID, w + ": null extras pointer with rounds > 1");
    if (P > c->maxR) return fail(c, AZ_ERR_CAPACITY, w + ": too many boxes");
    if (it.max_rows > c->maxR) return fail(c, AZ_ERR_CAPACITY, w + ": max_rows above the region capacity");
    return AZ_OK;
}

// Every one-image entry past its state check.  Round 1: the boxes uploaded, one pass with the gather.  Every further round
// is k_iter_select (az_iterloc.hip: the sources, their boxes into B[0], the device row count) + the same pass without the
// gather + k_iter_take (the class column through inv, so dprob / dpred keep round 1's rows until the one download at the
// end).  The extras of all rounds live in scratch slot 0, round r at row r * max_rows.
// The 4-byte row count of a round is read back (AzEnv::iterloc_sync, the default): the next launches are sized by it and
// an empty round ends the loop; without the read-back every round is enqueued at max_rows rows and the host waits once.
static int detect(az_ctx *c, const char *who, const double *boxes, int P, const DetPass &p, const DetIter &it,
                  float *scores_out, double *boxes_out)
{
    int rc = detect_args(c, who, boxes, P, p, it);
    if (rc) return rc;
    const int NX = it.rounds - 1, max_rows = it.max_rows;
    for (int r = 0; r < NX; ++r) it.count[r] = 0;
    if (P == 0) return AZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t rows = (size_t)NX * max_rows, o_box = 256, o_score = o_box + rows * 4 * sizeof(double),
                 o_cls = o_score + rows * sizeof(float), o_src = o_cls + rows * sizeof(int);
    if (NX && (rc = scratch_grow(c, 0, o_src + rows * sizeof(int))) != AZ_OK) return rc;
    unsigned char *ar = c->scratch[0].as<unsigned char>();
    int *d_cnt = (int *)ar;                                   // [NX] (<= 7 ints)
    double *d_box = (double *)(ar + o_box);
    float *d_score = (float *)(ar + o_score);
    int *d_cls = (int *)(ar + o_cls), *d_src = (int *)(ar + o_src);
    if (!(c->profiling & 4)) clear_events(c);
    if ((rc = upload_boxes(c, boxes, P)) != AZ_OK) return rc;
    if (NX) HIPCHK(c, hipMemsetAsync(d_cnt, 0, 256, s));
    det_pass_enqueue(c, p, P, &c->cnt->P[0]);
    int32_t n_host[8] = {0};
    bool counted = true;                                      // n_host holds every enqueued round's count
    for (int r = 0; r < NX; ++r) {
        const size_t o = (size_t)r * max_rows, op = r ? o - max_rows : 0;
        { Timed t(c, "iter_select", r + 1);
          azk_iter_select(s, c->dprob, c->dpred, P, c->det_ncls, r ? d_cnt + r - 1 : nullptr, d_score + op, d_box + 4 * op,
                          d_cls + op, (float)it.min_score, max_rows, c->B[0], d_cls + o, d_src + o, d_cnt + r, &c->cnt->P[0],
                          &c->cnt->U[0]); }
        int bound = max_rows;
        if (c->env.iterloc_sync) {
            HIPCHK(c, hipMemcpyAsync(&c->h_cnt->scratch[0], d_cnt + r, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            n_host[r] = bound = c->h_cnt->scratch[0];
            if (bound == 0) break;
        } else counted = false;
        det_pass_enqueue(c, p, bound, nullptr);
        { Timed t(c, "iter_take", r + 1);
          azk_iter_take(s, d_cnt + r, max_rows, c->inv, d_cls + o, c->det_ncls, c->dprob_u, c->dpred_u, d_score + o,
                        d_box + 4 * o); }
    }
    if ((rc = fetch_dets(c, P, scores_out, boxes_out)) != AZ_OK) return rc;
    if (!counted) HIPCHK(c, hipMemcpy(n_host, d_cnt, (size_t)NX * sizeof(int), hipMemcpyDeviceToHost));
    size_t at = 0;
    for (int r = 0; r < NX; ++r) {
        const size_t n = (size_t)n_host[r], o = (size_t)r * max_rows;
        it.count[r] = n_host[r];
        if (!n) continue;
        HIPCHK(c, hipMemcpy(it.cls + at, d_cls + o, n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(it.src + at, d_src + o, n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(it.score + at, d_score + o, n * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(it.box + 4 * at, d_box + 4 * o, n * 4 * sizeof(double), hipMemcpyDeviceToHost));
        at += n;
    }
    return AZ_OK;
}

// az_detect / az_detect_skip (the skip-connection detector, az_skip.hip: the front in RoIPool's place) and the
// az_detect_iter pair past their state checks: one scale, the context's map or the front
static int detect_scale(az_ctx *c, const char *who, bool skip, const double *boxes, int P, double scale, double dedup,
                        int batch_size, int im_h, int im_w, double eps, const DetIter &it, float *scores_out, double *boxes_out)
{
    const int rc = skip ? skip_check(c, who, true) : check_det(c);
    if (rc) return rc;
    DetPass p{dedup, batch_size, im_h, im_w, eps};
    p.scale = scale; p.skip = skip;
    return detect(c, who, boxes, P, p, it, scores_out, boxes_out);
}

int az_detect(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h,
              int im_w, double eps, float *scores_out, double *boxes_out)
{
    return detect_scale(c, "az_detect", false, boxes, P, scale, dedup, batch_size, im_h, im_w, eps, DetIter(), scores_out, boxes_out);
}

int az_detect_skip(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h,
                   int im_w, double eps, float *scores_out, double *boxes_out)
{
    return detect_scale(c, "az_detect_skip", true, boxes, P, scale, dedup, batch_size, im_h, im_w, eps, DetIter(), scores_out, boxes_out);
}

int az_detect_iter(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h, int im_w,
                   double eps, int rounds, double min_score, int max_rows, float *scores_out, double *boxes_out,
                   int32_t *ex_cls, int32_t *ex_src, float *ex_score, double *ex_box, int32_t *ex_count)
{
    return detect_scale(c, "az_detect_iter", false, boxes, P, scale, dedup, batch_size, im_h, im_w, eps,
                        DetIter{rounds, min_score, max_rows, ex_cls, ex_src, ex_score, ex_box, ex_count}, scores_out, boxes_out);
}

int az_detect_iter_skip(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h, int im_w,
                        double eps, int rounds, double min_score, int max_rows, float *scores_out, double *boxes_out,
                        int32_t *ex_cls, int32_t *ex_src, float *ex_score, double *ex_box, int32_t *ex_count)
{
    return detect_scale(c, "az_detect_iter_skip", true, boxes, P, scale, dedup, batch_size, im_h, im_w, eps,
                        DetIter{rounds, min_score, max_rows, ex_cls, ex_src, ex_score, ex_box, ex_count}, scores_out, boxes_out);
}

// _frcnn_forward over an image pyramid: az_detect with the pyramid projection and RoIPool through the map table (each
// roi reads the map of its level); decode and clip in original image pixels as before.
int az_detect_pyramid(az_ctx *c, const double *boxes, int P, const double *scales, int S, double dedup, int batch_size,
                      int im_h, int im_w, double eps, float *scores_out, double *boxes_out)
{
    int rc = check_det(c);
    if (rc) return rc;
    AzPyrScales sc;
    if ((rc = pyramid_args(c, scales, S, &sc, "az_detect_pyramid")) != AZ_OK) return rc;
    DetPass p{dedup, batch_size, im_h, im_w, eps};
    p.pyr = &sc; p.feats = c->pyr_feats; p.feat_hw = c->pyr_hw;
    return detect(c, "az_detect_pyramid", boxes, P, p, DetIter(), scores_out, boxes_out);
}

int az_skip_pool(az_ctx *c, const float *rois, int R, int normalise, float *out)
{
    int rc = skip_check(c, "az_skip_pool", true);
    if (rc) return rc;
    if (R > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_skip_pool: too many rois");
    if (R < 0 || (R && (!rois || !out))) return fail(c, AZ_ERR_INVALID, "az_skip_pool: bad arguments");
    if ((rc = stage_rois(c, rois, R)) != AZ_OK) return rc;
    return skip_pool_unit(c, R, normalise ? 1 : 0, out);
}

// test_net (lib/detect/test.py:541-668) over saved proposals: _frcnn_forward (:259-318) of n images in one pass per
// region capacity's worth of boxes -- one upload (AzDetSeg + boxes), segmented projection + dedup, RoIPool through the
// map table, fc6 / fc7 / tail over the rows of all images, the epilogue with per-row image sizes, the un-dedup gather,
// one download.  Every launch reads its row count from the device; the host waits once per pass.
int az_detect_batch(az_ctx *c, int n, const float *const *maps, int C, const int32_t *Hs, const int32_t *Ws,
                    const double *boxes, const int32_t *box_off, const double *scales, const int32_t *im_hw,
                    double dedup, int batch_size, double eps, float *scores_out, double *boxes_out)
{
    if (!c) return AZ_ERR_INVALID;
    if (!c->det_loaded) return fail(c, AZ_ERR_STATE, "az_load_det_head has not been called");
    if (c->gemm_parts && c->det_fc6.Wp)
        return fail(c, AZ_ERR_STATE, "az_detect_batch: fp32 only (the 16-bit-term modes scale fc6 per map)");
    if (n < 1 || n > AZ_BATCH_MAX) return fail(c, AZ_ERR_INVALID, "az_detect_batch: 1 <= n <= AZ_BATCH_MAX");
    if (!box_off || box_off[0] != 0 || batch_size <= 0 || !scales || !im_hw)
        return fail(c, AZ_ERR_INVALID, "az_detect_batch: bad arguments");
    if (C != c->d.C) return fail(c, AZ_ERR_INVALID, "az_detect_batch: channel count differs from the detection head's");
    for (int i = 0; i < n; ++i) {
        const int P = box_off[i + 1] - box_off[i];
        if (P < 0) return fail(c, AZ_ERR_INVALID, "az_detect_batch: box offsets not ascending");
        if (P == 0) continue;
        if (!maps || !maps[i] || !Hs || !Ws || Hs[i] <= 0 || Ws[i] <= 0)
            return fail(c, AZ_ERR_INVALID, "az_detect_batch: an image with boxes needs a map");
        if (!(scales[i] > 0) || im_hw[2 * i] <= 0 || im_hw[2 * i + 1] <= 0)
            return fail(c, AZ_ERR_INVALID, "az_detect_batch: bad scale or image size");
        if (P > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_detect_batch: an image has more boxes than the region capacity");
    }
    if (box_off[n] && (!boxes || !scores_out || !boxes_out)) return fail(c, AZ_ERR_INVALID, "az_detect_batch: null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (!(c->profiling & 4)) clear_events(c);
    const size_t nc = (size_t)c->det_ncls;
    AzDetSeg *hs = (AzDetSeg *)c->dseg_host;
    // every pass reads the staged block's device copy: its segments and boxes, its map table (the device addresses of
    // the table fields) and the per-row image sizes the dedup writes
    DetPass pass{dedup, batch_size, 1, 1, eps};
    pass.seg = (const AzDetSeg *)c->dseg_dev;
    pass.seg_boxes = (const double *)(c->dseg_dev + DET_SEG_HDR);
    pass.feats = (const float *const *)(c->dseg_dev + offsetof(AzDetSeg, feats));
    pass.feat_hw = (const int *)(c->dseg_dev + offsetof(AzDetSeg, feat_hw));
    pass.row_hw = c->drow_hw;
    const int *d_off = (const int *)(c->dseg_dev + offsetof(AzDetSeg, off));
    for (int i0 = 0; i0 < n;) {
        // a pass: the following images while their boxes fit the region capacity (which bounds the unique rows)
        int i1 = i0, P = 0;
        for (; i1 < n && P + (box_off[i1 + 1] - box_off[i1]) <= c->maxR; ++i1) P += box_off[i1 + 1] - box_off[i1];
        if (P == 0) { i0 = i1; continue; }
        HIPCHK(c, hipStreamSynchronize(s));                 // (the staging block of the previous pass is free)
        memset(hs, 0, sizeof(AzDetSeg));
        hs->n = i1 - i0;
        int chunks = 0;
        for (int b = 0; b < hs->n; ++b) {
            const int i = i0 + b, Pi = box_off[i + 1] - box_off[i];
            hs->off[b + 1] = hs->off[b] + Pi;
            hs->chunk0[b] = chunks;
            chunks += (Pi + batch_size - 1) / batch_size;
            hs->im_hw[2 * b] = im_hw[2 * i]; hs->im_hw[2 * b + 1] = im_hw[2 * i + 1];
            hs->scale[b] = scales[i];
            if (Pi) { hs->feat_hw[2 * b] = Hs[i]; hs->feat_hw[2 * b + 1] = Ws[i]; hs->feats[b] = maps[i]; }
        }
        memcpy(c->dseg_host + DET_SEG_HDR, boxes + 4 * (size_t)box_off[i0], (size_t)P * 4 * sizeof(double));
        HIPCHK(c, hipMemcpyAsync(c->dseg_dev, c->dseg_host, DET_SEG_HDR + (size_t)P * 4 * sizeof(double),
                                 hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
        pass.nseg = hs->n;
        det_pass_enqueue(c, pass, P, d_off + hs->n);
        const int rc = fetch_dets(c, P, scores_out + (size_t)box_off[i0] * nc, boxes_out + (size_t)box_off[i0] * nc * 4);
        if (rc) return rc;
        i0 = i1;
    }
    return AZ_OK;
}

}  // extern "C"
