// az_units.hip -- the C ABI's unit entry points (one stage of the path at a time: host in, host out, same kernels), the
// zoom-threshold tuner, recall evaluation and the image front-end.  (The detection head's entries: az_detect.hip.)
#include "az_ctx.h"

int upload_boxes(az_ctx *c, const double *boxes, int P)
{
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
    if (P) HIPCHK(c, hipMemcpyAsync(c->B[0], boxes, (size_t)P * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    return set_count(c, &c->cnt->P[0], P);
}

int stage_rois(az_ctx *c, const float *rois, int R)
{
    if (R < 0 || (R && !rois)) return fail(c, AZ_ERR_INVALID, "bad rois");
    if (R > c->maxR) return fail(c, AZ_ERR_CAPACITY, "too many rois");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), c->stream));
    if (R) HIPCHK(c, hipMemcpyAsync(c->urois, rois, (size_t)R * 5 * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ubox, 0, (size_t)(R > 0 ? R : 1) * 4 * sizeof(double), c->stream));
    return set_count(c, &c->cnt->U[0], R);
}

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
