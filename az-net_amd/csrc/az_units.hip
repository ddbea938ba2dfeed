// az_units.hip -- the C ABI's unit entry points (one stage of the path at a time: host in, host out, same kernels), the
// Fast R-CNN head on the shared map, the zoom-threshold tuner, recall evaluation and the image front-end.
#include "az_ctx.h"

extern "C" {

// --------------------------------------------------------------------------------------
// Unit entry points: host in, host out, same kernels.
static int sift_common(az_ctx *c, int C, double min_side, double *out, int cap, int *n_out)
{
    hipStream_t s = c->stream;
    int *Nptr = &c->cnt->scratch[0], *Pn = &c->cnt->scratch[1], *err = &c->cnt->scratch[2];
    HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
    int rc = set_count(c, Nptr, C);
    if (rc) return rc;
    azk_region_keys(s, c->child, Nptr, c->maxCh, min_side, c->ckey);
    azk_dedup_regions(s, c->ckey, Nptr, c->maxCh, c->maxR, c->first, c->child, c->B[1], Pn, err, nullptr, nullptr);
    HIPCHK(c, hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(AzCounts), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (c->h_cnt->scratch[2]) return fail(c, AZ_ERR_CAPACITY, "sift_dup: region capacity exceeded");
    const int n = c->h_cnt->scratch[1];
    *n_out = n;
    if (n > cap) return fail(c, AZ_ERR_CAPACITY, "sift_dup: output cap too small");
    if (n) HIPCHK(c, hipMemcpy(out, c->B[1], (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_sift_dup(az_ctx *c, const double *regions, int C, double min_side, double *out, int cap, int *n_out)
{
    int rc = check_geom(c);
    if (rc) return rc;
    if (C < 0 || (C && !regions) || !n_out || !(min_side > 0)) return fail(c, AZ_ERR_INVALID, "az_sift_dup: bad arguments");
    if (C > c->maxCh) return fail(c, AZ_ERR_CAPACITY, "az_sift_dup: too many regions");
    HIPCHK(c, hipSetDevice(c->device));
    if (C) HIPCHK(c, hipMemcpyAsync(c->child, regions, (size_t)C * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return sift_common(c, C, min_side, out, cap, n_out);
}

int az_divide_region(az_ctx *c, const double *regions, int P, double min_side, double *out, int cap, int *n_out)
{
    int rc = check_geom(c);
    if (rc) return rc;
    if (P < 0 || (P && !regions) || !n_out || !(min_side > 0)) return fail(c, AZ_ERR_INVALID, "az_divide_region: bad arguments");
    if (P > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_divide_region: too many regions");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
    if (P) HIPCHK(c, hipMemcpyAsync(c->Z, regions, (size_t)P * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    if ((rc = set_count(c, &c->cnt->PZ[0], P)) != AZ_OK) return rc;
    azk_divide(s, &c->cnt->PZ[0], &c->cnt->CH[0], &c->cnt->err, c->maxR, c->maxCh, c->Z, min_side, c->choff, c->child,
               c->ckey, nullptr, nullptr, nullptr, 0, nullptr);
    azk_dedup_regions(s, c->ckey, &c->cnt->CH[0], c->maxCh, c->maxR, c->first, c->child, c->B[1], &c->cnt->P[1],
                      &c->cnt->err, nullptr, nullptr);
    HIPCHK(c, hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(AzCounts), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (c->h_cnt->err) return fail(c, AZ_ERR_CAPACITY, "az_divide_region: ctx capacity exceeded");
    const int n = c->h_cnt->P[1];
    *n_out = n;
    if (n > cap) return fail(c, AZ_ERR_CAPACITY, "az_divide_region: output cap too small");
    if (n) HIPCHK(c, hipMemcpy(out, c->B[1], (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return AZ_OK;
}

// the box-upload prologue of the entries that take P boxes: counters cleared, the boxes in B[0], P[0] = P
static int upload_boxes(az_ctx *c, const double *boxes, int P)
{
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
    if (P) HIPCHK(c, hipMemcpyAsync(c->B[0], boxes, (size_t)P * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    return set_count(c, &c->cnt->P[0], P);
}

// az_roi_dedup / az_roi_dedup_pyramid past their argument checks: one scale, or the pyramid `pyr`
static int roi_dedup(az_ctx *c, const double *boxes, int P, double scale, const AzPyrScales *pyr, double dedup,
                     int batch_size, float *rois_out, int32_t *index_out, int32_t *inv_index_out, int *n_unique)
{
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = upload_boxes(c, boxes, P);
    if (rc) return rc;
    azk_rois_dedup(s, c->B[0], &c->cnt->P[0], c->maxR, scale, pyr, (float)dedup, batch_size, c->rois, c->key, c->grp,
                   c->first, c->index, c->inv, c->urois, c->ubox, &c->cnt->U[0]);
    HIPCHK(c, hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(AzCounts), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const int U = c->h_cnt->U[0];
    *n_unique = U;
    if (P && rois_out) HIPCHK(c, hipMemcpy(rois_out, c->rois, (size_t)P * 5 * 4, hipMemcpyDeviceToHost));
    if (U && index_out) HIPCHK(c, hipMemcpy(index_out, c->index, (size_t)U * 4, hipMemcpyDeviceToHost));
    if (P && inv_index_out) HIPCHK(c, hipMemcpy(inv_index_out, c->inv, (size_t)P * 4, hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_roi_dedup(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size,
                 float *rois_out, int32_t *index_out, int32_t *inv_index_out, int *n_unique)
{
    int rc = check_geom(c);
    if (rc) return rc;
    if (P < 0 || (P && !boxes) || !n_unique || batch_size <= 0) return fail(c, AZ_ERR_INVALID, "az_roi_dedup: bad arguments");
    if (P > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_roi_dedup: too many regions");
    return roi_dedup(c, boxes, P, scale, nullptr, dedup, batch_size, rois_out, index_out, inv_index_out, n_unique);
}

int az_roi_dedup_pyramid(az_ctx *c, const double *boxes, int P, const double *scales, int S, double dedup, int batch_size,
                         float *rois_out, int32_t *index_out, int32_t *inv_index_out, int *n_unique)
{
    int rc = check_geom(c);
    if (rc) return rc;
    AzPyrScales sc;
    if ((rc = pyramid_args(c, scales, S, &sc, "az_roi_dedup_pyramid")) != AZ_OK) return rc;
    if (P < 0 || (P && !boxes) || !n_unique || batch_size <= 0)
        return fail(c, AZ_ERR_INVALID, "az_roi_dedup_pyramid: bad arguments");
    if (P > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_roi_dedup_pyramid: too many regions");
    return roi_dedup(c, boxes, P, 0.0, &sc, dedup, batch_size, rois_out, index_out, inv_index_out, n_unique);
}

static int stage_rois(az_ctx *c, const float *rois, int R)
{
    if (R < 0 || (R && !rois)) return fail(c, AZ_ERR_INVALID, "bad rois");
    if (R > c->maxR) return fail(c, AZ_ERR_CAPACITY, "too many rois");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), c->stream));
    if (R) HIPCHK(c, hipMemcpyAsync(c->urois, rois, (size_t)R * 5 * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ubox, 0, (size_t)(R > 0 ? R : 1) * 4 * sizeof(double), c->stream));
    return set_count(c, &c->cnt->U[0], R);
}

// az_roi_pool / az_roi_pool_pyramid past their argument checks: RoIPool of the staged rois from the context's map, or
// through the map table feats / feat_hw (roi column 0 indexes it)
static int roi_pool(az_ctx *c, int R, float *out, const float *const *feats, const int *feat_hw)
{
    azk_roi_pool(c->stream, c->feat, c->d, c->spatial_scale, c->urois, &c->cnt->U[0], c->maxR, c->pool5, nullptr, 0, 0,
                 0, 0, nullptr, feats, feat_hw);
    // the ABI returns Caffe's [R, C, 7, 7] flattening; HBM holds [R, 49, C]
    if (R) azk_permute_k(c->stream, c->pool5, c->part, R, c->d.C, 0);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (R) HIPCHK(c, hipMemcpy(out, c->part, (size_t)R * c->d.K6 * 4, hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_roi_pool(az_ctx *c, const float *rois, int R, float *out)
{
    int rc = check_ready(c, true);
    if (rc) return rc;
    if ((rc = stage_rois(c, rois, R)) != AZ_OK) return rc;
    if (!out) return fail(c, AZ_ERR_INVALID, "az_roi_pool: null output");
    return roi_pool(c, R, out, nullptr, nullptr);
}

int az_roi_pool_pyramid(az_ctx *c, const float *rois, int R, float *out)
{
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!c->pyr_S) return fail(c, AZ_ERR_STATE, "az_roi_pool_pyramid: no pyramid set (az_set_feature_pyramid_dev_nhwc)");
    if (R < 0 || (R && (!rois || !out))) return fail(c, AZ_ERR_INVALID, "az_roi_pool_pyramid: bad arguments");
    for (int r = 0; r < R; ++r) {        // (column 0 indexes the map table)
        const float lv = rois[5 * (size_t)r];
        if (!(lv >= 0.0f && lv < (float)c->pyr_S && lv == (float)(int)lv))
            return fail(c, AZ_ERR_INVALID, "az_roi_pool_pyramid: roi column 0 must be a level of the pyramid set");
    }
    if ((rc = stage_rois(c, rois, R)) != AZ_OK) return rc;
    return roi_pool(c, R, out, c->pyr_feats, c->pyr_hw);
}

int az_head_forward(az_ctx *c, const float *rois, int R, float *zoom_prob, float *adj_prob, float *adj_bbox)
{
    int rc = check_ready(c, true);
    if (rc) return rc;
    if ((rc = stage_rois(c, rois, R)) != AZ_OK) return rc;
    if (!(c->profiling & 4)) clear_events(c);
    prep_scale(c);
    // (the row count is known on the host here: many rows take the many-row GEMM, as a one-pass search does)
    launch_head(c, &c->cnt->U[0], 0, 1, 1, 0.0, c->zoom_u, c->score_u, c->delta_u, 0.0, false, 0, nullptr, nullptr, R);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (R && zoom_prob) HIPCHK(c, hipMemcpy(zoom_prob, c->zoom_u, (size_t)R * 4, hipMemcpyDeviceToHost));
    if (R && adj_prob) HIPCHK(c, hipMemcpy(adj_prob, c->score_u, (size_t)R * AZ_NSUB * 4, hipMemcpyDeviceToHost));
    if (R && adj_bbox) HIPCHK(c, hipMemcpy(adj_bbox, c->delta_u, (size_t)R * 4 * AZ_NSUB * 4, hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_decode_filter(az_ctx *c, const double *anchors, const float *deltas, const float *scores, int R,
                     int im_h, int im_w, double eps, double min_side, double *boxes_out, float *scores_out,
                     int cap, int *n_out)
{
    int rc = check_geom(c);
    if (rc) return rc;
    if (R < 0 || (R && (!anchors || !deltas || !scores)) || !n_out) return fail(c, AZ_ERR_INVALID, "az_decode_filter: bad arguments");
    if (R > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_decode_filter: too many regions");
    c->cand_n = -1;                              // Yall / Sall are reused below
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
    // stage: anchors -> ubox, deltas -> delta_u, scores -> score_s (scratch of R * 11 floats: Sout holds max_candidates,
    // which may be fewer); inv = identity
    std::vector<int> ident(R);
    for (int i = 0; i < R; ++i) ident[i] = i;
    if (R) {
        HIPCHK(c, hipMemcpyAsync(c->ubox, anchors, (size_t)R * 4 * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->delta_u, deltas, (size_t)R * 4 * AZ_NSUB * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->score_s, scores, (size_t)R * AZ_NSUB * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->inv, ident.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    }
    if ((rc = set_count(c, &c->cnt->P[0], R)) != AZ_OK) return rc;
    HIPCHK(c, hipMemsetAsync(c->zoom_u, 0, (size_t)(R > 0 ? R : 1) * 4, s));
    azk_decode_unit(s, c->ubox, c->delta_u, c->score_s, R, im_h, im_w, eps, c->pred_u, c->score_u);
    azk_flags_compact(s, c->cnt, 0, c->maxR, c->maxCand, c->ubox, c->inv, c->pred_u, c->score_u, c->zoom_u, 2.0,
                      min_side, 0, c->cflag, c->zflag, c->bc_c, c->bc_z, c->Yall, c->Sall, c->Z, c->zr);
    HIPCHK(c, hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(AzCounts), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const int n = c->h_cnt->NC[0];
    *n_out = n;
    if (n > cap) return fail(c, AZ_ERR_CAPACITY, "az_decode_filter: output cap too small");
    if (n && boxes_out) HIPCHK(c, hipMemcpy(boxes_out, c->Yall, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (n && scores_out) HIPCHK(c, hipMemcpy(scores_out, c->Sall, (size_t)n * 4, hipMemcpyDeviceToHost));
    // more kept candidates than the context holds: k_compact clamped the count (n == max_candidates, the first n kept
    // candidates are out) and raised the flag the search reports as AZ_ERR_CAPACITY -- so does the unit
    if (c->h_cnt->err & 2) return fail(c, AZ_ERR_CAPACITY, "az_decode_filter: candidate capacity exceeded (raise az_set_limits)");
    return AZ_OK;
}

// az_topk and az_topk_radix: `radix` keeps the chip-wide counting kernels out (no rank scratch), so the single-workgroup
// radix select takes every n.
static int topk_unit(az_ctx *c, const float *scores, int n, int k, int32_t *idx_out, int *n_out, bool radix, const char *who)
{
    int rc = check_geom(c);
    if (rc) return rc;
    if (n < 0 || (n && !scores) || k <= 0 || !idx_out || !n_out) return fail(c, AZ_ERR_INVALID, std::string(who) + ": bad arguments");
    if (n > c->maxCand || k > AZ_TOPK_MAX) return fail(c, AZ_ERR_CAPACITY, std::string(who) + ": n or k too large");
    c->cand_n = -1;                              // Sall is reused below
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
    if (n) HIPCHK(c, hipMemcpyAsync(c->Sall, scores, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if ((rc = set_count(c, &c->cnt->scratch[0], n)) != AZ_OK) return rc;
    azk_topk(s, c->Sall, &c->cnt->scratch[0], c->maxCand, k, c->sel_idx, &c->cnt->nsel, radix ? nullptr : c->rank_part);
    HIPCHK(c, hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(AzCounts), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const int m = c->h_cnt->nsel;
    *n_out = m;
    if (m) HIPCHK(c, hipMemcpy(idx_out, c->sel_idx, (size_t)m * 4, hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_topk(az_ctx *c, const float *scores, int n, int k, int32_t *idx_out, int *n_out)
{
    return topk_unit(c, scores, n, k, idx_out, n_out, false, "az_topk");
}

int az_topk_radix(az_ctx *c, const float *scores, int n, int k, int32_t *idx_out, int *n_out)
{
    return topk_unit(c, scores, n, k, idx_out, n_out, true, "az_topk_radix");
}

// --------------------------------------------------------------------------------------
// Fast R-CNN head on the shared conv map (lib/detect/test.py:259-318,432-445).
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

// the detection head on the `U` rois in ctx->urois / ctx->ubox
// (rows_bound: what the host knows about the row count -- the number of boxes before the 1/16 dedup)
// (feats / feat_hw / row_hw: the rows of several images, az_detect_batch -- RoIPool's map table, per-row image sizes)
// (skip: pool5 comes from the skip-connection front, az_skip.hip, instead of RoIPool of the context's map)
static void launch_det_head(az_ctx *c, const int *Uptr, int im_h, int im_w, double eps, int rows_bound,
                            const float *const *feats = nullptr, const int *feat_hw = nullptr, const int *row_hw = nullptr,
                            bool skip = false)
{
    AzHeadDims d = c->d;
    const int K6 = d.C * 49, NO = 5 * c->det_ncls;
    d.K6 = K6;
    // many rows (the reference's 300 proposals per image): fc6 / fc7 on the many-row GEMM, as int6 (same bits either way)
    const bool many_rows = rows_bound >= c->gemm12_min_rows;
    const bool terms = c->gemm_parts && c->det_fc6.Wp;             // (16-bit-term modes: fc6, 86 % of this head's FLOPs, as int6)
    if (terms && c->gemm_parts == 2)
        azk_feat_scale(c->stream, c->feat, (long long)d.C * d.H * d.W, c->dgscale, c->det_fc6.w_scale);
    if (skip) skip_front_launch(c, Uptr, rows_bound);
    else
    { Timed t(c, "det_roi_pool", 0);
      azk_roi_pool(c->stream, c->feat, d, c->spatial_scale, c->urois, Uptr, c->maxR, c->pool5, terms ? c->pool5p : nullptr,
                   terms ? azk_act_plane_elems(c->maxR, K6) : 0, terms ? c->gemm_parts : 0, 0, 0,
                   (terms && c->gemm_parts == 2) ? c->dgscale : nullptr, feats, feat_hw); }
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
      azk_det_epilogue(c->stream, c->dpart, AZK_TAIL_SPLIT, c->det_ncls, c->dbt, c->ubox, Uptr, c->maxR, im_h, im_w,
                       eps, c->dprob_u, c->ddelta_u, c->dpred_u, row_hw); }
}

static int check_det(az_ctx *c)
{
    if (!c) return AZ_ERR_INVALID;
    if (!c->det_loaded) return fail(c, AZ_ERR_STATE, "az_load_det_head has not been called");
    if (!c->feat) return fail(c, AZ_ERR_STATE, "no feature map set");
    return AZ_OK;
}

int az_det_forward(az_ctx *c, const float *rois, int R, float *cls_prob, float *bbox_pred)
{
    int rc = check_det(c);
    if (rc) return rc;
    if ((rc = stage_rois(c, rois, R)) != AZ_OK) return rc;
    if (!(c->profiling & 4)) clear_events(c);
    launch_det_head(c, &c->cnt->U[0], 1, 1, 0.0, R);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    const size_t nc = (size_t)c->det_ncls;
    if (R && cls_prob) HIPCHK(c, hipMemcpy(cls_prob, c->dprob_u, (size_t)R * nc * 4, hipMemcpyDeviceToHost));
    if (R && bbox_pred) HIPCHK(c, hipMemcpy(bbox_pred, c->ddelta_u, (size_t)R * 4 * nc * 4, hipMemcpyDeviceToHost));
    return AZ_OK;
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

// az_detect / az_detect_pyramid past their argument checks: projection + dedup (one scale, or the pyramid `pyr`), the
// head with RoIPool from the context's map or through the map table feats / feat_hw, the un-dedup gather, the download
static int detect(az_ctx *c, const double *boxes, int P, double scale, const AzPyrScales *pyr, double dedup,
                  int batch_size, int im_h, int im_w, double eps, const float *const *feats, const int *feat_hw,
                  float *scores_out, double *boxes_out, bool skip = false)
{
    if (P == 0) return AZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (!(c->profiling & 4)) clear_events(c);
    int rc = upload_boxes(c, boxes, P);
    if (rc) return rc;
    azk_rois_dedup(s, c->B[0], &c->cnt->P[0], c->maxR, scale, pyr, (float)dedup, batch_size, c->rois, c->key, c->grp,
                   c->first, c->index, c->inv, c->urois, c->ubox, &c->cnt->U[0]);
    launch_det_head(c, &c->cnt->U[0], im_h, im_w, eps, P, feats, feat_hw, nullptr, skip);
    azk_det_gather(s, &c->cnt->P[0], c->inv, c->det_ncls, c->dprob_u, c->dpred_u, c->dprob, c->dpred);
    return fetch_dets(c, P, scores_out, boxes_out);
}

int az_detect(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h,
              int im_w, double eps, float *scores_out, double *boxes_out)
{
    int rc = check_det(c);
    if (rc) return rc;
    if (P < 0 || (P && !boxes) || batch_size <= 0 || !(scale > 0)) return fail(c, AZ_ERR_INVALID, "az_detect: bad arguments");
    if (P > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_detect: too many boxes");
    return detect(c, boxes, P, scale, nullptr, dedup, batch_size, im_h, im_w, eps, nullptr, nullptr, scores_out, boxes_out);
}

// The skip-connection detector (az_skip.hip): az_detect / az_det_forward / az_roi_pool with the front in RoIPool's place.
int az_detect_skip(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h,
                   int im_w, double eps, float *scores_out, double *boxes_out)
{
    int rc = skip_check(c, "az_detect_skip", true);
    if (rc) return rc;
    if (P < 0 || (P && !boxes) || batch_size <= 0 || !(scale > 0)) return fail(c, AZ_ERR_INVALID, "az_detect_skip: bad arguments");
    if (P > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_detect_skip: too many boxes");
    return detect(c, boxes, P, scale, nullptr, dedup, batch_size, im_h, im_w, eps, nullptr, nullptr, scores_out, boxes_out, true);
}

// az_detect_iter / az_detect_iter_skip past their argument checks.  Round 1 is detect()'s launch sequence; every further
// round is k_iter_select (az_iterloc.hip: the sources, their boxes into B[0], the device row count) + the same projection,
// dedup and head pass + k_iter_take (the class column through inv, so dprob / dpred keep round 1's rows until the one
// download at the end).  The extras of all rounds live in scratch slot 0, round r at row r * max_rows.
// The 4-byte row count of a round is read back (AzEnv::iterloc_sync, the default): the next launches are sized by it and
// an empty round ends the loop; without the read-back every round is enqueued at max_rows rows and the host waits once.
static int detect_iter(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h, int im_w,
                       double eps, int rounds, double min_score, int max_rows, float *scores_out, double *boxes_out,
                       int32_t *ex_cls, int32_t *ex_src, float *ex_score, double *ex_box, int32_t *ex_count, bool skip)
{
    const int NX = rounds - 1;
    for (int r = 0; r < NX; ++r) ex_count[r] = 0;
    if (P == 0) return AZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t rows = (size_t)NX * max_rows, o_box = 256, o_score = o_box + rows * 4 * sizeof(double),
                 o_cls = o_score + rows * sizeof(float), o_src = o_cls + rows * sizeof(int);
    int rc;
    if (NX && (rc = scratch_grow(c, 0, o_src + rows * sizeof(int))) != AZ_OK) return rc;
    unsigned char *ar = c->scratch[0].as<unsigned char>();
    int *d_cnt = (int *)ar;                                   // [NX] (<= 7 ints)
    double *d_box = (double *)(ar + o_box);
    float *d_score = (float *)(ar + o_score);
    int *d_cls = (int *)(ar + o_cls), *d_src = (int *)(ar + o_src);
    if (!(c->profiling & 4)) clear_events(c);
    if ((rc = upload_boxes(c, boxes, P)) != AZ_OK) return rc;
    if (NX) HIPCHK(c, hipMemsetAsync(d_cnt, 0, 256, s));
    azk_rois_dedup(s, c->B[0], &c->cnt->P[0], c->maxR, scale, nullptr, (float)dedup, batch_size, c->rois, c->key, c->grp,
                   c->first, c->index, c->inv, c->urois, c->ubox, &c->cnt->U[0]);
    launch_det_head(c, &c->cnt->U[0], im_h, im_w, eps, P, nullptr, nullptr, nullptr, skip);
    azk_det_gather(s, &c->cnt->P[0], c->inv, c->det_ncls, c->dprob_u, c->dpred_u, c->dprob, c->dpred);
    int32_t n_host[8] = {0};
    bool counted = true;                                      // n_host holds every enqueued round's count
    for (int r = 0; r < NX; ++r) {
        const size_t o = (size_t)r * max_rows, op = r ? o - max_rows : 0;
        { Timed t(c, "iter_select", r + 1);
          azk_iter_select(s, c->dprob, c->dpred, P, c->det_ncls, r ? d_cnt + r - 1 : nullptr, d_score + op, d_box + 4 * op,
                          d_cls + op, (float)min_score, max_rows, c->B[0], d_cls + o, d_src + o, d_cnt + r, &c->cnt->P[0],
                          &c->cnt->U[0]); }
        int bound = max_rows;
        if (c->env.iterloc_sync) {
            HIPCHK(c, hipMemcpyAsync(&c->h_cnt->scratch[0], d_cnt + r, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            n_host[r] = bound = c->h_cnt->scratch[0];
            if (bound == 0) break;
        } else counted = false;
        azk_rois_dedup(s, c->B[0], &c->cnt->P[0], c->maxR, scale, nullptr, (float)dedup, batch_size, c->rois, c->key,
                       c->grp, c->first, c->index, c->inv, c->urois, c->ubox, &c->cnt->U[0]);
        launch_det_head(c, &c->cnt->U[0], im_h, im_w, eps, bound, nullptr, nullptr, nullptr, skip);
        { Timed t(c, "iter_take", r + 1);
          azk_iter_take(s, d_cnt + r, max_rows, c->inv, d_cls + o, c->det_ncls, c->dprob_u, c->dpred_u, d_score + o,
                        d_box + 4 * o); }
    }
    if ((rc = fetch_dets(c, P, scores_out, boxes_out)) != AZ_OK) return rc;
    if (!counted) HIPCHK(c, hipMemcpy(n_host, d_cnt, (size_t)NX * sizeof(int), hipMemcpyDeviceToHost));
    size_t at = 0;
    for (int r = 0; r < NX; ++r) {
        const size_t n = (size_t)n_host[r], o = (size_t)r * max_rows;
        ex_count[r] = n_host[r];
        if (!n) continue;
        HIPCHK(c, hipMemcpy(ex_cls + at, d_cls + o, n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(ex_src + at, d_src + o, n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(ex_score + at, d_score + o, n * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(ex_box + 4 * at, d_box + 4 * o, n * 4 * sizeof(double), hipMemcpyDeviceToHost));
        at += n;
    }
    return AZ_OK;
}

static int detect_iter_args(az_ctx *c, const char *who, const double *boxes, int P, double scale, int batch_size, int rounds,
                            int max_rows, const int32_t *ex_cls, const int32_t *ex_src, const float *ex_score,
                            const double *ex_box, const int32_t *ex_count)
{
    const std::string w(who);
    if (P < 0 || (P && !boxes) || batch_size <= 0 || !(scale > 0)) return fail(c, AZ_ERR_INVALID, w + ": bad arguments");
    if (rounds < 1 || rounds > AZ_ITER_LOC_MAX_ROUNDS) return fail(c, AZ_ERR_INVALID, w + ": 1 <= rounds <= AZ_ITER_LOC_MAX_ROUNDS");
    if (max_rows < 1 || max_rows > AZ_TOPK_MAX) return fail(c, AZ_ERR_INVALID, w + ": 1 <= max_rows <= 4096");
    if (rounds > 1 && (!ex_cls || !ex_src || !ex_score || !ex_box || !ex_count))
        return fail(c, AZ_ERR_INVALID, w + ": null extras pointer with rounds > 1");
    if (P > c->maxR) return fail(c, AZ_ERR_CAPACITY, w + ": too many boxes");
    if (max_rows > c->maxR) return fail(c, AZ_ERR_CAPACITY, w + ": max_rows above the region capacity");
    return AZ_OK;
}

int az_detect_iter(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h, int im_w,
                   double eps, int rounds, double min_score, int max_rows, float *scores_out, double *boxes_out,
                   int32_t *ex_cls, int32_t *ex_src, float *ex_score, double *ex_box, int32_t *ex_count)
{
    int rc = check_det(c);
    if (rc) return rc;
    if ((rc = detect_iter_args(c, "az_detect_iter", boxes, P, scale, batch_size, rounds, max_rows, ex_cls, ex_src, ex_score,
                               ex_box, ex_count)) != AZ_OK) return rc;
    return detect_iter(c, boxes, P, scale, dedup, batch_size, im_h, im_w, eps, rounds, min_score, max_rows, scores_out,
                       boxes_out, ex_cls, ex_src, ex_score, ex_box, ex_count, false);
}

int az_detect_iter_skip(az_ctx *c, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h, int im_w,
                        double eps, int rounds, double min_score, int max_rows, float *scores_out, double *boxes_out,
                        int32_t *ex_cls, int32_t *ex_src, float *ex_score, double *ex_box, int32_t *ex_count)
{
    int rc = skip_check(c, "az_detect_iter_skip", true);
    if (rc) return rc;
    if ((rc = detect_iter_args(c, "az_detect_iter_skip", boxes, P, scale, batch_size, rounds, max_rows, ex_cls, ex_src,
                               ex_score, ex_box, ex_count)) != AZ_OK) return rc;
    return detect_iter(c, boxes, P, scale, dedup, batch_size, im_h, im_w, eps, rounds, min_score, max_rows, scores_out,
                       boxes_out, ex_cls, ex_src, ex_score, ex_box, ex_count, true);
}

int az_det_forward_skip(az_ctx *c, const float *rois, int R, float *cls_prob, float *bbox_pred)
{
    int rc = skip_check(c, "az_det_forward_skip", true);
    if (rc) return rc;
    if (R > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_det_forward_skip: too many rois");
    if ((rc = stage_rois(c, rois, R)) != AZ_OK) return rc;
    if (!(c->profiling & 4)) clear_events(c);
    launch_det_head(c, &c->cnt->U[0], 1, 1, 0.0, R, nullptr, nullptr, nullptr, true);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    const size_t nc = (size_t)c->det_ncls;
    if (R && cls_prob) HIPCHK(c, hipMemcpy(cls_prob, c->dprob_u, (size_t)R * nc * 4, hipMemcpyDeviceToHost));
    if (R && bbox_pred) HIPCHK(c, hipMemcpy(bbox_pred, c->ddelta_u, (size_t)R * 4 * nc * 4, hipMemcpyDeviceToHost));
    return AZ_OK;
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

// _frcnn_forward over an image pyramid: az_detect with the pyramid projection and RoIPool through the map table (each
// roi reads the map of its level); decode and clip in original image pixels as before.
int az_detect_pyramid(az_ctx *c, const double *boxes, int P, const double *scales, int S, double dedup, int batch_size,
                      int im_h, int im_w, double eps, float *scores_out, double *boxes_out)
{
    int rc = check_det(c);
    if (rc) return rc;
    AzPyrScales sc;
    if ((rc = pyramid_args(c, scales, S, &sc, "az_detect_pyramid")) != AZ_OK) return rc;
    if (P < 0 || (P && !boxes) || batch_size <= 0) return fail(c, AZ_ERR_INVALID, "az_detect_pyramid: bad arguments");
    if (c->pyr_S != S)
        return fail(c, AZ_ERR_STATE, "az_detect_pyramid: no pyramid of that many maps set (az_set_feature_pyramid_dev_nhwc)");
    if (P > c->maxR) return fail(c, AZ_ERR_CAPACITY, "az_detect_pyramid: too many boxes");
    return detect(c, boxes, P, 0.0, &sc, dedup, batch_size, im_h, im_w, eps, c->pyr_feats, c->pyr_hw, scores_out,
                  boxes_out);
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
    const AzDetSeg *ds = (const AzDetSeg *)c->dseg_dev;
    double *dB = (double *)(c->dseg_dev + DET_SEG_HDR);
    // (device addresses of the table fields)
    const float *const *d_feats = (const float *const *)(c->dseg_dev + offsetof(AzDetSeg, feats));
    const int *d_feat_hw = (const int *)(c->dseg_dev + offsetof(AzDetSeg, feat_hw));
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
        { Timed t(c, "det_rois_dedup", 0);
          azk_rois_dedup(s, dB, ds, hs->n, c->maxR, (float)dedup, batch_size, c->rois, c->key, c->grp, c->first, c->index,
                         c->inv, c->urois, c->ubox, &c->cnt->U[0], c->drow_hw); }
        launch_det_head(c, &c->cnt->U[0], 1, 1, eps, P, d_feats, d_feat_hw, c->drow_hw);
        azk_det_gather(s, d_off + hs->n, c->inv, c->det_ncls, c->dprob_u, c->dpred_u, c->dprob, c->dpred);
        const int rc = fetch_dets(c, P, scores_out + (size_t)box_off[i0] * nc, boxes_out + (size_t)box_off[i0] * nc * 4);
        if (rc) return rc;
        i0 = i1;
    }
    return AZ_OK;
}

// --------------------------------------------------------------------------------------
// Tuner (lib/detect/tune.py): anchor history and the global k-th largest zoom score.
int az_last_anchors(az_ctx *c, double *regions_out, float *zoom_out, int cap, int *n_out)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!n_out) return AZ_ERR_INVALID;
    if (!(c->last.reserved & 4) || !c->hisB)
        return fail(c, AZ_ERR_STATE, "az_last_anchors: the last az_propose was not a tuner search (reserved bit 2)");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->his_n < 0)
        return fail(c, AZ_ERR_STATE, "az_last_anchors: the history is gone (the search failed, or a later tuner search has been launched)");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int n = c->his_n;
    *n_out = n;
    if (n > cap) return fail(c, AZ_ERR_CAPACITY, "az_last_anchors: cap too small");
    if (regions_out) HIPCHK(c, hipMemcpy(regions_out, c->hisB, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (zoom_out) HIPCHK(c, hipMemcpy(zoom_out, c->hisZ, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_tune_begin(az_ctx *c, long long capacity)
{
    if (!c || capacity <= 0) return fail(c, AZ_ERR_INVALID, "az_tune_begin: bad capacity");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (capacity > c->pool_alloc) {
        c->pool = c->pool_tmp = nullptr; c->pool_cap = c->pool_alloc = 0;
        HIPCHK(c, reserve_group({{&c->pool_own[0], (size_t)capacity * sizeof(float)}, {&c->pool_own[1], (size_t)capacity * sizeof(float)}}));
        c->pool = c->pool_own[0].as<float>(); c->pool_tmp = c->pool_own[1].as<float>(); c->pool_alloc = capacity;
    }
    c->pool_cap = capacity;                  // (a smaller pool than the last one keeps the allocation, not the capacity)
    if (!c->pool_n) {
        HIPCHK(c, reserve_group({{&c->pool_own[2], 4 * sizeof(unsigned long long)}, {&c->pool_own[3], 256 * sizeof(unsigned long long)}}));
        c->pool_n = c->pool_own[2].as<unsigned long long>(); c->pool_hist = c->pool_own[3].as<unsigned long long>();
    }
    HIPCHK(c, hipMemsetAsync(c->pool_n, 0, 4 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pool_bad = false;
    return AZ_OK;
}

int az_tune_end(az_ctx *c)
{
    if (!c) return AZ_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pool_own[0].reset(); c->pool_own[1].reset();
    c->pool = c->pool_tmp = nullptr;
    c->pool_cap = c->pool_alloc = 0;
    c->pool_bad = false;
    return AZ_OK;
}

static int pool_size(az_ctx *c, long long *n, long long *dropped)
{
    if (!c->pool) return fail(c, AZ_ERR_STATE, "az_tune_begin has not been called");
    if (c->pool_bad)
        return fail(c, AZ_ERR_CAPACITY, "az_tune: a tuner search that fed the score pool failed, the pool is incomplete; az_tune_begin again");
    unsigned long long h[2];
    HIPCHK(c, hipMemcpyAsync(h, c->pool_n, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n = (long long)h[0];
    *dropped = (long long)h[1];
    return AZ_OK;
}

int az_tune_push(az_ctx *c, const float *scores, long long n)
{
    if (!c || n < 0 || (n && !scores)) return fail(c, AZ_ERR_INVALID, "az_tune_push: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    long long have, dropped;
    int rc = pool_size(c, &have, &dropped);
    if (rc) return rc;
    if (have + n > c->pool_cap) return fail(c, AZ_ERR_CAPACITY, "az_tune_push: pool capacity exceeded");
    if (n) HIPCHK(c, hipMemcpyAsync(c->pool + have, scores, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const unsigned long long nn = (unsigned long long)(have + n);
    HIPCHK(c, hipMemcpyAsync(c->pool_n, &nn, sizeof(nn), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AZ_OK;
}

// MSB-first radix select over order-preserving keys: the key of the k-th largest score.
static int pool_kth_key(az_ctx *c, long long n, long long k, unsigned int *key_out)
{
    unsigned int prefix = 0;
    long long want = k;                       // rank (1-based, from the top) inside the current bucket
    unsigned long long h[256];
    for (int shift = 24; shift >= 0; shift -= 8) {
        HIPCHK(c, hipMemsetAsync(c->pool_hist, 0, sizeof(h), c->stream));
        azk_pool_hist(c->stream, c->pool, n, prefix, shift, c->pool_hist);
        HIPCHK(c, hipMemcpyAsync(h, c->pool_hist, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        int b = 255;
        for (; b > 0; --b) {
            if ((long long)h[b] >= want) break;
            want -= (long long)h[b];
        }
        prefix |= (unsigned int)b << shift;
    }
    *key_out = prefix;
    return AZ_OK;
}

static float key_to_float(unsigned int k)
{
    const unsigned int u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

int az_tune_kth_largest(az_ctx *c, long long k, float *value_out, long long *n_total)
{
    if (!c || k <= 0 || !value_out) return fail(c, AZ_ERR_INVALID, "az_tune_kth_largest: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    long long n, dropped;
    int rc = pool_size(c, &n, &dropped);
    if (rc) return rc;
    if (n_total) *n_total = n;
    if (dropped) return fail(c, AZ_ERR_CAPACITY, "az_tune: score pool overflowed; raise az_tune_begin's capacity");
    if (n <= k) { *value_out = -INFINITY; return AZ_OK; }     // the heap of tune.py:343-350 never overflowed
    unsigned int key;
    if ((rc = pool_kth_key(c, n, k, &key)) != AZ_OK) return rc;
    *value_out = key_to_float(key);
    return AZ_OK;
}

int az_tune_top(az_ctx *c, long long k, float *scores_out, long long cap, long long *n_out)
{
    if (!c || k <= 0 || !n_out) return fail(c, AZ_ERR_INVALID, "az_tune_top: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    long long n, dropped;
    int rc = pool_size(c, &n, &dropped);
    if (rc) return rc;
    if (dropped) return fail(c, AZ_ERR_CAPACITY, "az_tune: score pool overflowed; raise az_tune_begin's capacity");
    unsigned int key = 0;
    if (n > k && (rc = pool_kth_key(c, n, k, &key)) != AZ_OK) return rc;
    HIPCHK(c, hipMemsetAsync(&c->pool_n[2], 0, sizeof(unsigned long long), c->stream));
    azk_pool_keep(c->stream, c->pool, n, key, c->pool_tmp, &c->pool_n[2]);
    unsigned long long m = 0;
    HIPCHK(c, hipMemcpyAsync(&m, &c->pool_n[2], sizeof(m), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_out = (long long)m;
    if ((long long)m > cap) return fail(c, AZ_ERR_CAPACITY, "az_tune_top: cap too small");
    if (m && scores_out) HIPCHK(c, hipMemcpy(scores_out, c->pool_tmp, (size_t)m * sizeof(float), hipMemcpyDeviceToHost));
    return AZ_OK;
}

// --------------------------------------------------------------------------------------
// Recall evaluation (lib/datasets/imdb.py:120-159) and utils.cython_bbox.bbox_overlaps.
int az_bbox_overlaps(az_ctx *c, const double *boxes, int N, const double *query, int K, double *overlaps_out)
{
    if (!c || N < 0 || K < 0 || ((N && !boxes) || (K && !query)) || (N && K && !overlaps_out))
        return fail(c, AZ_ERR_INVALID, "az_bbox_overlaps: bad arguments");
    if (N == 0 || K == 0) return AZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = scratch_grow(c, 0, (size_t)N * 4 * sizeof(double))) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 1, (size_t)K * 4 * sizeof(double))) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 2, (size_t)N * K * sizeof(double))) != AZ_OK) return rc;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->scratch[0].p, boxes, (size_t)N * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->scratch[1].p, query, (size_t)K * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    azk_bbox_overlaps(s, (const double *)c->scratch[0].p, N, (const double *)c->scratch[1].p, K, (double *)c->scratch[2].p);
    HIPCHK(c, hipMemcpyAsync(overlaps_out, c->scratch[2].p, (size_t)N * K * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return AZ_OK;
}

int az_recall_match(az_ctx *c, int n_images, const double *boxes, const int32_t *box_off, const double *gt,
                    const int32_t *gt_off, double *gt_overlaps_out)
{
    if (!c || n_images < 0 || (n_images && (!box_off || !gt_off)))
        return fail(c, AZ_ERR_INVALID, "az_recall_match: bad arguments");
    if (n_images == 0) return AZ_OK;
    const int NB = box_off[n_images], NG = gt_off[n_images];
    std::vector<long long> ov_off((size_t)n_images + 1, 0);
    for (int i = 0; i < n_images; ++i) {
        const long long n = box_off[i + 1] - box_off[i], k = gt_off[i + 1] - gt_off[i];
        if (n < 0 || k < 0) return fail(c, AZ_ERR_INVALID, "az_recall_match: offsets must ascend");
        if (n == 0 && k > 0)
            return fail(c, AZ_ERR_INVALID, "az_recall_match: an image without boxes (imdb.py:128-129 skips those)");
        ov_off[i + 1] = ov_off[i] + n * k;
    }
    if (NG == 0) return AZ_OK;
    if (!boxes || !gt || !gt_overlaps_out) return fail(c, AZ_ERR_INVALID, "az_recall_match: NULL array");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t offb = ((size_t)n_images + 1) * sizeof(int32_t);
    if ((rc = scratch_grow(c, 0, (size_t)NB * 4 * sizeof(double))) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 1, (size_t)NG * 4 * sizeof(double))) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 2, (size_t)ov_off[n_images] * sizeof(double) + 8)) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 3, offb)) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 4, offb)) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 5, ((size_t)n_images + 1) * sizeof(long long))) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 6, (size_t)NG * sizeof(double))) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 7, (size_t)n_images * sizeof(int))) != AZ_OK) return rc;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->scratch[0].p, boxes, (size_t)NB * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->scratch[1].p, gt, (size_t)NG * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->scratch[3].p, box_off, offb, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->scratch[4].p, gt_off, offb, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->scratch[5].p, ov_off.data(), ((size_t)n_images + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->scratch[7].p, 0, (size_t)n_images * sizeof(int), s));
    azk_recall_match(s, n_images, (const double *)c->scratch[0].p, (const int *)c->scratch[3].p, (const double *)c->scratch[1].p,
                     (const int *)c->scratch[4].p, (const long long *)c->scratch[5].p, (double *)c->scratch[2].p, (double *)c->scratch[6].p,
                     (int *)c->scratch[7].p);
    std::vector<int> bad((size_t)n_images);
    HIPCHK(c, hipMemcpyAsync(gt_overlaps_out, c->scratch[6].p, (size_t)NG * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(bad.data(), c->scratch[7].p, (size_t)n_images * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));     // ov_off / bad live on this frame
    for (int i = 0; i < n_images; ++i)
        if (bad[i])
            return fail(c, AZ_ERR_INVALID,
                        "az_recall_match: image " + std::to_string(i) +
                            " has more ground-truth boxes than candidates (assert gt_ovr >= 0, imdb.py:139)");
    return AZ_OK;
}

// --------------------------------------------------------------------------------------
// Image front-end (_get_image_blob, lib/detect/test.py:27-59).
int az_image_blob_size(int h, int w, double scale, int *oh, int *ow)
{
    if (h <= 0 || w <= 0 || !(scale > 0) || !oh || !ow) return AZ_ERR_INVALID;
    *oh = (int)std::nearbyint((double)h * scale);      // cv2: saturate_cast<int>(rows * fy), ties to even
    *ow = (int)std::nearbyint((double)w * scale);
    return (*oh > 0 && *ow > 0) ? AZ_OK : AZ_ERR_INVALID;
}

static int image_blob_common(az_ctx *c, const uint8_t *im, int h, int w, const float *means, double scale,
                             float *out, bool out_is_dev, int oh, int ow)
{
    int eh, ew;
    if (!c || !im || !means || !out || az_image_blob_size(h, w, scale, &eh, &ew) != AZ_OK || eh != oh || ew != ow)
        return fail(c, AZ_ERR_INVALID, "az_image_blob: bad arguments (output size must come from az_image_blob_size)");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    const size_t nin = (size_t)h * w * 3, nout = (size_t)oh * ow * 3;
    if ((rc = scratch_grow(c, 0, nin)) != AZ_OK) return rc;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->scratch[0].p, im, nin, hipMemcpyHostToDevice, s));
    float *dst = out;
    if (!out_is_dev) {
        if ((rc = scratch_grow(c, 1, nout * sizeof(float))) != AZ_OK) return rc;
        dst = (float *)c->scratch[1].p;
    }
    azk_image_blob(s, (const unsigned char *)c->scratch[0].p, h, w, means, 1.0 / scale, 1.0 / scale, oh, ow, dst);
    if (!out_is_dev) HIPCHK(c, hipMemcpyAsync(out, dst, nout * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return AZ_OK;
}

int az_image_blob_host(az_ctx *c, const uint8_t *im, int h, int w, const float *means, double scale, float *blob_out,
                       int oh, int ow)
{
    return image_blob_common(c, im, h, w, means, scale, blob_out, false, oh, ow);
}

int az_image_blob_dev(az_ctx *c, const uint8_t *im, int h, int w, const float *means, double scale, float *blob_dev,
                      int oh, int ow)
{
    return image_blob_common(c, im, h, w, means, scale, blob_dev, true, oh, ow);
}


int az_image_blob_dev_on(az_ctx *c, const uint8_t *im, int h, int w, const float *means, double scale, float *blob_dev,
                         int oh, int ow, void *stream)
{
    int eh, ew;
    if (!c || !im || !means || !blob_dev || az_image_blob_size(h, w, scale, &eh, &ew) != AZ_OK || eh != oh || ew != ow)
        return fail(c, AZ_ERR_INVALID, "az_image_blob_dev_on: bad arguments (output size must come from az_image_blob_size)");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t nin = (size_t)h * w * 3;
    if (nin > c->io_cap) {
        // (larger images: nothing may still be reading the old slots)
        for (auto &q : c->io) HIPCHK(c, hipEventSynchronize(q.ev));
        c->io.clear();
        c->io_cap = nin + nin / 4 + 256;
        c->io_turn = 0;
    }
    auto add_slot = [&](size_t at) {
        az_ctx::IoSlot q;
        if (q.host.reserve(c->io_cap) != hipSuccess || q.dev.reserve(c->io_cap) != hipSuccess || q.ev.create(hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            return false;                      // (q's owners release whatever it got)
        }
        c->io.insert(c->io.begin() + (long)at, std::move(q));
        return true;
    };
    while (c->io.size() < 2)
        if (!add_slot(c->io.size())) return fail(c, AZ_ERR_HIP, "az_image_blob_dev_on: upload slots");
    if (c->io_turn >= (int)c->io.size()) c->io_turn = 0;
    // the slot in turn holds the oldest upload: done long ago in a loop that fetches what it launches; still QUEUED when the
    // caller enqueues a whole batch behind the previous batch's search -- then a fresh slot takes this image (it goes in
    // front of the busy one: the ring stays oldest-first) rather than the host waiting for the GPU
    if (hipEventQuery(c->io[c->io_turn].ev) == hipErrorNotReady && (int)c->io.size() < az_ctx::IO_SLOTS_MAX)
        (void)add_slot((size_t)c->io_turn);
    (void)hipGetLastError();
    az_ctx::IoSlot &q = c->io[c->io_turn];
    c->io_turn = (c->io_turn + 1) % (int)c->io.size();
    HIPCHK(c, hipEventSynchronize(q.ev));                   // (a fresh slot's event was never recorded: returns at once)
    std::memcpy(q.host.p, im, nin);                         // the caller's array may go away as soon as this returns
    HIPCHK(c, hipMemcpyAsync(q.dev.p, q.host.p, nin, hipMemcpyHostToDevice, s));
    azk_image_blob(s, q.dev.as<unsigned char>(), h, w, means, 1.0 / scale, 1.0 / scale, oh, ow, blob_dev);
    HIPCHK(c, hipEventRecord(q.ev, s));
    HIPCHK(c, hipGetLastError());
    return AZ_OK;
}


}  // extern "C"
