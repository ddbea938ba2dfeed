// az_pyramid.hip -- multi-scale test pyramids (cfg.TEST.SCALES with several entries): the pyramid's arguments, its map
// set and the pyramid search.  The search is the plain level loop of az_search.hip with the pyramid projection of
// k_first_rois (az_geom.hip, pyramid_roi_and_key in az_geom_dev.h) and RoIPool through the map table (az_ctx.h: pyr_now);
// the detection entries share their bodies with their single-scale twins in az_units.hip and az_detect.hip.
#include "az_ctx.h"

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
        HIPCHK(c, reserve_group({{&c->pyr_own[0], AZ_PYRAMID_MAX * sizeof(const float *)}, {&c->pyr_own[1], AZ_PYRAMID_MAX * 2 * sizeof(int)}}));
        c->pyr_feats = c->pyr_own[0].as<const float *>(); c->pyr_hw = c->pyr_own[1].as<int>();
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
