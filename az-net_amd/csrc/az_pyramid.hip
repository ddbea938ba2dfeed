// az_pyramid.hip -- multi-scale test pyramids (cfg.TEST.SCALES with several entries): roi projection into the pyramid +
// feature-space dedup (lib/detect/test.py:61-97,210-218), the pyramid map set and the pyramid search.  The search is the
// plain level loop of az_search.hip with this file's projection and RoIPool through the map table (az_ctx.h: pyr_now);
// the detection entries live beside their single-scale twins in az_units.hip.  Built with -ffp-contract=off: the level
// choice and the projection round once per operation, in the reference's order.
#include "az_ctx.h"
#include "az_geom_dev.h"

namespace {

constexpr int TB = 256;

// _project_im_rois (test.py:73-97) + _get_rois_blob (:61-71) + the dedup hash (:212-214) of one box.  Level: the first
// minimum over s of |w * h * s^2 - 224^2| (np.argmin), in f64; roi = f32(box * s[level]), column 0 = f32(level); the key
// of np.round(roi * DEDUP_BOXES) . [1, 1e3, 1e6, 1e9, 1e12] -- roi_and_key's plus rint(level * dedup) with weight 1
// (0 for every level at 1/16 up to level 7).  S == 1 (the reference's else branch, level 0): roi_and_key's bits.
__device__ __forceinline__ long long pyramid_roi_and_key(const double *box, const AzPyrScales &sc, float dedup, float *roi5,
                                                         int r)
{
    int lv = 0;
    double s = sc.s[0];
    if (sc.S > 1) {
        const double w = box[2] - box[0] + 1.0, h = box[3] - box[1] + 1.0;
        const double area = w * h;
        double best = 0.0;
#pragma unroll
        for (int i = 0; i < AZ_PYRAMID_MAX; ++i) {
            if (i >= sc.S) break;
            const double d = fabs(area * (sc.s[i] * sc.s[i]) - 224.0 * 224.0);
            if (i == 0 || d < best) { best = d; lv = i; s = sc.s[i]; }
        }
    }
    const float L = (float)lv;
    roi5[0] = L;
    long long h = (long long)rintf(L * dedup), mult = 1000;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float x = (float)(box[c] * s);
        roi5[1 + c] = x;
        h += (long long)rintf(x * dedup) * mult;
        mult *= 1000;
    }
    return dedup > 0.0f ? h : (long long)r;
}

// k_first_rois with the pyramid key: one wave per box stores its roi / key / chunk id and flags whether it is the first
// of its key within its BATCH_SIZE chunk (np.unique's return_index); k_dedup_rois (azk_dedup_slots) orders the rest.
__global__ void k_pyramid_rois(const double *__restrict__ B, const int *Pptr, AzPyrScales sc, float dedup, int batch,
                               float *rois, long long *key, int *grp, unsigned char *first)
{
    const int P = *Pptr;
    const int lane = lane_id();
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < P; i += nwaves) {
        float roi5[5];
        const long long ki = pyramid_roi_and_key(B + 4 * (size_t)i, sc, dedup, roi5, i);
        const int gi = i / batch;
        if (lane == 0) { key[i] = ki; grp[i] = gi; }
        if (lane < 5) rois[5 * (size_t)i + lane] = roi5[lane];
        bool dup = false;
        for (int j0 = gi * batch; j0 < i; j0 += 64) {  // only the same chunk can hold a duplicate
            const int j = j0 + lane;
            if (j < i) {
                float r5[5];
                dup |= (pyramid_roi_and_key(B + 4 * (size_t)j, sc, dedup, r5, j) == ki);
            }
            if (__any(dup)) break;
        }
        const bool any_dup = __any(dup);               // vote with all lanes active
        if (lane == 0) first[i] = any_dup ? 0 : 1;
    }
}

inline int grid_for(int cap, int per) { int g = (cap + per - 1) / per; return g < 1 ? 1 : (g > 2048 ? 2048 : g); }

}  // namespace

void azk_pyramid_rois_dedup(hipStream_t s, const double *B, const int *Pptr, int cap, const AzPyrScales &sc, float dedup,
                            int batch, float *rois, long long *key, int *grp, unsigned char *first, int *index, int *inv,
                            float *urois, double *ubox, int *Uptr)
{
    hipLaunchKernelGGL(k_pyramid_rois, dim3(grid_for(cap, TB / 64)), dim3(TB), 0, s, B, Pptr, sc, dedup, batch, rois, key,
                       grp, first);
    azk_dedup_slots(s, key, grp, Pptr, cap, first, rois, B, index, inv, urois, ubox, Uptr);
}

int pyramid_args(az_ctx *c, const double *scales, int S, AzPyrScales *sc, const char *who)
{
    if (S < 1 || S > AZ_PYRAMID_MAX || !scales)
        return fail(c, AZ_ERR_INVALID, std::string(who) + ": the pyramid must have 1 to AZ_PYRAMID_MAX (8) scales");
    *sc = AzPyrScales{};
    sc->S = S;
    for (int i = 0; i < S; ++i) {
        if (!(scales[i] > 0.0) || !std::isfinite(scales[i]))
            return fail(c, AZ_ERR_INVALID, std::string(who) + ": every scale must be positive and finite");
        sc->s[i] = scales[i];
    }
    if (c->gemm_parts == 2 || c->gemm_parts == 3)
        return fail(c, AZ_ERR_STATE, std::string(who) + ": fp32 only (the 16-bit-term GEMM modes are not supported)");
    return AZ_OK;
}

extern "C" {

int az_set_feature_pyramid_dev_nhwc(az_ctx *c, const float *const *maps, int S, int C, int H, int W)
{
    if (!c) return AZ_ERR_INVALID;
    // (an AZ head, a detection head or both: a detection-only context -- HipFrcnnNet -- pools from the pyramid too)
    if (!c->head_loaded && !c->det_loaded)
        return fail(c, AZ_ERR_STATE, "az_set_feature_pyramid_dev_nhwc: load a head (az_load_head / az_load_det_head) first");
    join_s2(c);
    if (S < 1 || S > AZ_PYRAMID_MAX || !maps)
        return fail(c, AZ_ERR_INVALID, "az_set_feature_pyramid_dev_nhwc: the pyramid must have 1 to AZ_PYRAMID_MAX (8) maps");
    for (int i = 0; i < S; ++i)
        if (!maps[i]) return fail(c, AZ_ERR_INVALID, "az_set_feature_pyramid_dev_nhwc: null map");
    if (C != c->d.C || H <= 0 || W <= 0)
        return fail(c, AZ_ERR_INVALID, "az_set_feature_pyramid_dev_nhwc: channel count must match the loaded head");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->pyr_feats) {
        HIPCHK(c, hipMalloc((void **)&c->pyr_feats, AZ_PYRAMID_MAX * sizeof(const float *)));
        HIPCHK(c, hipMalloc((void **)&c->pyr_hw, AZ_PYRAMID_MAX * 2 * sizeof(int)));
    }
    const float *tab[AZ_PYRAMID_MAX] = {};
    int hw[2 * AZ_PYRAMID_MAX] = {};
    for (int i = 0; i < S; ++i) { tab[i] = maps[i]; hw[2 * i] = H; hw[2 * i + 1] = W; }
    // (whatever the context still has queued may read the previous table)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->pyr_feats, tab, sizeof(tab), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->pyr_hw, hw, sizeof(hw), hipMemcpyHostToDevice));
    c->pyr_S = S;
    c->feat = maps[0];                 // (level 0 is also the context's single map, as az_set_feature_map_dev_nhwc sets it)
    c->d.H = H; c->d.W = W;
    return AZ_OK;
}

int az_propose_pyramid(az_ctx *c, const az_params *p, const double *scales, int S, double *boxes_out, float *scores_out,
                       int cap, int *n_out, az_stats *st)
{
    if (!c) return AZ_ERR_INVALID;
    AzPyrScales sc;
    int rc = pyramid_args(c, scales, S, &sc, "az_propose_pyramid");
    if (rc) return rc;
    if (!p || !boxes_out || !n_out || cap < 0) return fail(c, AZ_ERR_INVALID, "az_propose_pyramid: bad arguments");
    if (c->pyr_S != S)
        return fail(c, AZ_ERR_STATE, "az_propose_pyramid: no pyramid of that many maps set (az_set_feature_pyramid_dev_nhwc)");
    // the plain level loop: one projection + dedup and one head pass per level, nothing speculated or planned from the
    // image shape (those forms assume one map and one scale)
    az_params q = *p;
    q.scale = sc.s[0];
    q.reserved |= AZ_P_NO_SPECULATION | AZ_P_UNFUSED_FIRST_LEVELS | AZ_P_UNFUSED_LEVELS | AZ_P_LEVEL_LOOP_AT_TZ0 |
                  AZ_P_NO_PAIR_ROWS | AZ_P_NO_WHOLE_TREE | AZ_P_NO_EARLY_END;
    q.reserved &= ~(AZ_P_PAIR_ROWS_ALWAYS | AZ_P_WHOLE_TREE_ALWAYS | AZ_P_CLOSURE_ROWS);
    c->pyr_sc = sc;
    c->pyr_now = 1;
    rc = az_propose(c, &q, boxes_out, scores_out, cap, n_out, st);
    c->pyr_now = 0;
    return rc;
}

}  // extern "C"
