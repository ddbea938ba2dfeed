// az_search.hip -- one search: the level loop (or the one-pass plan) as one stream-ordered launch sequence (optionally a
// hipGraph) in the form az_plan.hip picked, on what az_shape.hip prepared; collecting a result -- including running a
// search again in another form; staging its record.
#include "az_search.h"

static inline hipStream_t geom_stream(const az_ctx *c) { return c->gs ? c->gs : c->stream; }   // (az_ctx.h: two stages)

// Final selection (test.py:392-400): top-k by score, or everything with score >= Tc.
static void enqueue_select(az_ctx *c, const az_params *p, int nlev, int k)
{
    hipStream_t s = geom_stream(c);
    Timed t(c, "select", nlev);
    if (p->fixed_num)
        azk_topk_full(s, c->Sall, &c->cnt->ytot[nlev], c->maxCand, k, c->sel_idx, &c->cnt->nsel, c->Yall,
                      c->Sall, (double *)((unsigned char *)c->cnt + RES_HDR),
                      (float *)((unsigned char *)c->cnt + RES_HDR + (size_t)k * 32),
                      (p->reserved & 8) ? nullptr : c->rank_part);
    else
        azk_thresh_select_full(s, c->Sall, &c->cnt->ytot[nlev], c->maxCand, p->Tc, c->maxCand, c->sel_idx,
                               &c->cnt->nsel, c->Yall, c->Sall, c->Yout, c->Sout);
}

static int enqueue_static(az_ctx *c, const az_params *p, int nlev, int k)
{
    const auto &q = *c->plan;
    launch_head(c, q.meta, -1, p->im_h, p->im_w, p->eps, c->zoom_u, c->score_u, c->delta_u, p->min_side, true,
                q.coop, q.urois, q.ubox, q.Utot, true);
    { Timed t(c, "static_candidates", nlev - 1);
      AzStaticArgs a;
      a.cnt = c->cnt; a.reg_u = q.reg_u; a.cand_src = q.cand_src; a.key_u = c->key_u; a.pred_u = c->pred_u;
      a.score_u = c->score_u;
      a.zoom_u = c->zoom_u; a.Yall = c->Yall; a.Sall = c->Sall; a.Tz = p->Tz;
      a.nlev = nlev; a.Utot = q.Utot; a.capCand = c->maxCand;
      for (int l = 0; l <= nlev; ++l) a.roff[l] = q.roff[l];
      for (int l = 0; l < nlev; ++l) { a.U[l] = q.U[l]; a.CH[l] = q.CH[l]; }
      a.k = k; a.Yout = (double *)((unsigned char *)c->cnt + RES_HDR);
      a.Sout = (float *)((unsigned char *)c->cnt + RES_HDR + (size_t)k * 32);
      // fixed proposal count: the same launch ranks the candidates and writes the top k (params.reserved bit 3
      // keeps the separate selection kernels, for tests)
      if (p->fixed_num && !(p->reserved & 8) && azk_static_select(geom_stream(c), a)) return AZ_OK;
      azk_static_candidates(geom_stream(c), a); }
    enqueue_select(c, p, nlev, k);
    return AZ_OK;
}

// --------------------------------------------------------------------------------------
// Everything az_propose enqueues on the ctx stream (no host synchronisation, no host-dependent sizes:
// every count is read on the device), so the same sequence can also be captured into a hipGraph.
static int enqueue_search(az_ctx *c, const az_params *p, int K, int nlev, int k, bool tune)
{
    hipStream_t s = c->stream;

    // Speculative evaluation of levels 1-3.  The root is always divided (test.py:383-384), so
    // level 2's regions are known up front, and level 3's regions are a subset of the children
    // of ALL level-2 regions.  These few dozen rows cost one pass over the 411 MB int6 weights
    // instead of three (each of those levels is weight-streaming-bound).  Head outputs are a
    // fixed function of the roi, so the levels below just look their rows up: bit-identical
    // results.  (params.reserved bit 0 turns this off.)
    const SearchPlan plan = plan_search(c, p, nlev, tune);
    const int n_spec = plan.n_spec;
    const bool fused = plan.fused, fused_lv = plan.fused_lv, defer_root = plan.defer_root;
    if (tune && !c->hisB) {
        c->capHis = 2 * c->maxR;
        HIPCHK(c, reserve_group({{&c->his_own[0], (size_t)c->capHis * 4 * sizeof(double)}, {&c->his_own[1], (size_t)c->capHis * sizeof(float)}}));
        c->hisB = c->his_own[0].as<double>(); c->hisZ = c->his_own[1].as<float>();
    }
    if (!fused) azk_init_root(s, c->cnt, c->B[0], p->im_h, p->im_w);       // also zeroes the counters
    if (fused) {
        // (the pre-pass -- B1, all children of B1, the rois of the speculative rows -- depends on the image shape
        //  only: az_propose_launch ran it for this shape, k_spec_levels restores its counters)
    } else if (n_spec) {
        Timed t(c, "spec_geometry", -1);
        // children of the root -> B1 (with _sift_dup), exactly what level 1's divide will produce
        azk_divide(s, &c->cnt->P[0], &c->cnt->scratch[3], &c->cnt->err, c->maxR, c->maxCh, c->B[0], p->min_side,
                   c->choff, c->child, c->ckey, nullptr, nullptr, nullptr, 0, nullptr);
        azk_dedup_regions(s, c->ckey, &c->cnt->scratch[3], c->maxCh, c->maxR, c->first, c->child, c->B[1],
                          &c->cnt->specP1, &c->cnt->err, nullptr, nullptr);
        // children of ALL of B1, before _sift_dup; their offsets identify (parent, child) later
        azk_divide(s, &c->cnt->specP1, &c->cnt->specCH, &c->cnt->err, c->maxR, c->maxCh, c->B[1], p->min_side,
                   c->choff_all, c->child, c->ckey, nullptr, nullptr, nullptr, 0, nullptr);
        azk_spec_rois(s, c->B[0], c->B[1], c->child, c->cnt, c->maxR, p->scale, c->urois);
    }
    const bool full = plan.full != 0;
    const az_ctx::StaticPlan::FullSet *fp = full ? &c->plan->fs[plan.full - 1] : nullptr;
    // the head outputs of the speculative / whole-tree pass (three stages: two sets used in turn, az_ctx.h)
    float *zs = c->zoom_s, *ss = c->score_s, *ds = c->delta_s;
    if (full && c->three_now) {
        c->out_par ^= 1;
        if (c->out_par) { zs = c->zoom_s2; ss = c->score_s2; ds = c->delta_s2; }
    }
    // inv_index of level l (two buffers by level parity: k_level_geom's candidate-copy workgroup reads level l's while
    // its chain workgroup writes level l+1's)
    auto INV = [&](int l) { return (l & 1) ? c->inv_odd : c->inv; };
    // (whole-tree speculation: the *_v sets alternate by level -- a level's geometry kernel reads its own set while it
    //  writes the next level's)
    auto Vp = [&](int l) { return (full && (l & 1)) ? c->pred_w : c->pred_v; };
    auto Vs = [&](int l) { return (full && (l & 1)) ? c->score_w : c->score_v; };
    auto Vz = [&](int l) { return (full && (l & 1)) ? c->zoom_w : c->zoom_v; };
    auto Vk = [&](int l) { return (full && (l & 1)) ? c->keep_w : c->keep_v; };
    auto Vy = [&](int l) { return (full && (l & 1)) ? c->key_w : c->key_v; };
    if (full)
        // the search's ONE head pass: the unique rois of the image shape's full tree (+ the speculative rows the plan
        // lacks), the root last; outputs by row in zoom_s / score_s / delta_s
    {
        launch_head(c, fp->full_meta, -1, p->im_h, p->im_w, p->eps, zs, ss, ds, 0.0, false, 1,
                    fp->full_urois, fp->full_ubox, fp->Ufull);
        s = geom_stream(c);            // (two stages: everything behind the one head pass goes where its int7 went)
    }
    else if (fused && plan.cut == 2 && !defer_root)
        // early end before the third level: the first 1 + P1 rows of S = [root ; B1 ; children of all of B1]
        launch_head(c, c->spec_U[0] + 1, -1, p->im_h, p->im_w, p->eps, zs, ss, ds, 0.0, false,
                    0, c->spec_urois[0], nullptr, 1 + c->spc[0].P1);
    else if (fused)
        launch_head(c, c->spec_U[defer_root ? 1 : 0], -1, p->im_h, p->im_w, p->eps, zs, ss, ds, 0.0, false,
                    0, c->spec_urois[defer_root ? 1 : 0], nullptr, c->spc[defer_root ? 1 : 0].U);
    else if (n_spec)
        launch_head(c, &c->cnt->specU, -1, p->im_h, p->im_w, p->eps, zs, ss, ds);
    if (fused) {
        Timed t(c, "spec_levels", 0);
        AzFusedArgs a;
        a.cnt = c->cnt;
        a.B[0] = c->B[0]; a.B[1] = c->B[1]; a.srcB[0] = c->srcB[0]; a.srcB[1] = c->srcB[1];
        a.index = c->index; a.inv = INV(n_spec); a.zr = c->zr; a.choff = c->choff; a.csrc = c->csrc;
        const int dslot = defer_root ? 1 : 0;
        a.choff_all = c->spec_choff[dslot]; a.specB1 = c->specB1[dslot];
        a.reset = 1; a.specP1 = c->spc[dslot].P1; a.specCH = c->spc[dslot].CH; a.specU = c->spc[dslot].U;
        a.ubox = c->ubox; a.pred_u = c->pred_u; a.Yall = c->Yall; a.Z = c->Z; a.child = c->child;
        a.zoom_u = c->zoom_u; a.score_u = c->score_u; a.delta_u = c->delta_u; a.Sall = c->Sall;
        a.zoom_s = zs; a.score_s = ss; a.delta_s = ds;
        a.scale = p->scale; a.Tz = p->Tz; a.min_side = p->min_side; a.eps = p->eps; a.dedup = (float)p->dedup;
        a.batch = p->batch_size; a.im_h = p->im_h; a.im_w = p->im_w; a.nlev = nlev; a.n_fused = n_spec;
        a.capR = c->maxR; a.capCh = c->maxCh; a.capCand = c->maxCand;
        a.rois = c->rois; a.urois = c->urois; a.next_dedup = fused_lv ? 1 : 0; a.defer_root = defer_root ? 1 : 0;
        a.cut_next = (plan.cut && plan.cut <= n_spec) ? 1 : 0;
        a.cut_short = (plan.cut == 2 && !defer_root) ? 1 : 0;
        a.spec_next = (plan.pair_mask >> n_spec) & 1; a.choff_next = c->choff_pair; a.crow = c->crow;
        a.spatial_scale = c->spatial_scale;
        a.row_map = full ? fp->spec_map : nullptr; a.root_row = full ? fp->Ufull - 1 : 0;
        a.stab = full ? fp->htab : nullptr; a.stabT = full ? fp->hT : 0;
        a.pred_v = Vp(n_spec); a.score_v = Vs(n_spec); a.zoom_v = Vz(n_spec); a.keep_v = Vk(n_spec); a.key_v = Vy(n_spec);
        azk_spec_levels(s, a);
    }
    bool have_v = full;               // this level's head outputs were looked up among the previous pass's rows (*_v arrays)
    const int nlev_run = plan.cut ? plan.cut : nlev;     // (early end: the levels from plan.cut on are not enqueued)
    for (int l = fused ? n_spec : 0; l < nlev_run; ++l) {
        const int cur = l & 1;
        const int *Pptr = &c->cnt->P[l];
        int *Uptr = &c->cnt->U[l];
        // (the last level's copy + top-k stay chip-wide; from plan.lv_limit on the levels outgrow the fused kernel)
        const bool lv_here = fused_lv && l + 1 < nlev && l < plan.lv_limit;
        const bool pair_here = !full && fused_lv && ((plan.pair_mask >> l) & 1) && !have_v;   // this pass carries level l+1's rows
        if (lv_here) {
            // this level's rois were projected and deduplicated by the previous geometry kernel, which also left the
            // pass's row count (its unique rois + pair-speculation rows + the deferred root's) in cnt->PR[l]
            if (!have_v)
                launch_head(c, &c->cnt->PR[l], l, p->im_h, p->im_w, p->eps, c->zoom_u, c->score_u,
                            c->delta_u, p->min_side, true, (defer_root && l == n_spec) ? 1 : 0, nullptr, nullptr,
                            many_rows_expected(c, l));
            Timed t(c, "level_geom", l);
            AzLevelArgs a;
            a.cnt = c->cnt; a.level = l; a.nlev = nlev;
            a.cut_next = (plan.cut == l + 1) ? 1 : 0;
            a.B = c->B[cur]; a.Bnext = c->B[cur ^ 1];
            a.pred_u = have_v ? Vp(l) : c->pred_u; a.score_u = have_v ? Vs(l) : c->score_u;
            a.zoom_u = have_v ? Vz(l) : c->zoom_u; a.keep_u = have_v ? Vk(l) : c->keep_u; a.Uptr = Uptr;
            a.urois = c->urois; a.index = c->index; a.inv = INV(l); a.inv_next = INV(l + 1); a.ubox = c->ubox;
            a.Yall = c->Yall; a.Sall = c->Sall;
            a.scale = p->scale; a.Tz = p->Tz; a.min_side = p->min_side; a.dedup = (float)p->dedup;
            a.batch = p->batch_size; a.capR = c->maxR; a.capCh = c->maxCh; a.capCand = c->maxCand;
            a.force_root = 1; a.root_row = (defer_root && l == n_spec && !have_v) ? 1 : 0;
            a.lookup_next = full ? 2 : (pair_here ? 1 : 0);
            a.spec_next = (!full && !pair_here && ((plan.pair_mask >> (l + 1)) & 1)) ? 1 : 0;
            a.delta_u = full ? ds : c->delta_u; a.choff_all = c->choff_pair; a.choff_next = c->choff_pair; a.crow = c->crow;
            a.stab = full ? fp->htab : nullptr; a.stabT = full ? fp->hT : 0; a.root_row_full = full ? fp->Ufull - 1 : 0;
            a.score_all = ss; a.zoom_all = zs;
            a.pred_v = Vp(l + 1); a.score_v = Vs(l + 1); a.zoom_v = Vz(l + 1); a.keep_v = Vk(l + 1); a.key_v = Vy(l + 1);
            a.im_h = p->im_h; a.im_w = p->im_w; a.eps = p->eps; a.spatial_scale = c->spatial_scale;
            azk_level_geom(s, a);
            have_v = full || pair_here;
            continue;
        }
        if (!fused_lv || l > plan.lv_limit) {   // (otherwise the fused predecessor -- spec_levels or level_geom -- has done this already)
          Timed t(c, "rois_dedup", l);
          // (a pyramid search, az_propose_pyramid, always takes this plain level loop)
          azk_rois_dedup(s, c->B[cur], Pptr, c->maxR, p->scale, c->pyr_now ? &c->pyr_sc : nullptr, (float)p->dedup,
                         p->batch_size, c->rois, c->key, c->grp, c->first, c->index, INV(l), c->urois, c->ubox, Uptr); }
        // The last level of a default search with a fixed proposal count: its candidates, its counters and the final
        // top-k come from ONE launch (az_static.hip: k_final_select) instead of k_flags, k_compact, k_rank_count and
        // k_rank_scatter; the tail kernel emits the selection keys.  (params.reserved bits 1 / 3 keep the separate
        // kernels: same bits.)
        const bool final_fused = fused && !tune && l + 1 == nlev && l >= n_spec && p->fixed_num && !(p->reserved & 8);
        if (full && !have_v && l >= n_spec) {
            // whole-tree speculation, a level on the multi-launch kernels: its outputs by window lookup, chip-wide
            Timed t(c, "full_lookup", l);
            azk_full_lookup(s, Uptr, c->urois, c->ubox, fp->htab, fp->hT, fp->Ufull - 1, c->spatial_scale, ds, ss,
                            zs, p->im_h, p->im_w, p->eps, p->min_side, Vp(l), Vs(l), Vz(l), Vk(l), Vy(l), &c->cnt->err);
            have_v = true;
        }
        if (l < n_spec) {
            Timed t(c, "spec_lookup", l);
            azk_spec_lookup(s, l, Uptr, c->index, c->srcB[cur], c->ubox, zs, ss, ds,
                            p->im_h, p->im_w, p->eps, c->zoom_u, c->score_u, c->delta_u, c->pred_u);
        } else if (!have_v) {
            launch_head(c, (fused_lv && l <= plan.lv_limit) ? &c->cnt->PR[l] : Uptr, l, p->im_h, p->im_w, p->eps, c->zoom_u, c->score_u, c->delta_u,
                        p->min_side, final_fused, 0, nullptr, nullptr, many_rows_expected(c, l), final_fused);
        }
        if (final_fused) {
            Timed t(c, "final_select", l);
            AzFinalArgs a;
            a.cnt = c->cnt; a.level = l; a.inv = INV(l); a.key_u = have_v ? Vy(l) : c->key_u;
            a.pred_u = have_v ? Vp(l) : c->pred_u;
            a.score_u = have_v ? Vs(l) : c->score_u; a.zoom_u = have_v ? Vz(l) : c->zoom_u;
            a.Yall = c->Yall; a.Sall = c->Sall; a.Tz = p->Tz;
            a.force_root = (l == 0) ? 1 : 0; a.capCand = c->maxCand; a.k = k;
            a.Yout = (double *)((unsigned char *)c->cnt + RES_HDR);
            a.Sout = (float *)((unsigned char *)c->cnt + RES_HDR + (size_t)k * 32);
            azk_final_select(s, a);
            return AZ_OK;
        }
        if (tune) {
            Timed t(c, "record_anchors", l);
            azk_record_anchors(s, c->cnt, l, c->maxR, c->capHis, c->B[cur], INV(l), c->zoom_u, c->hisB, c->hisZ,
                               &c->cnt->nhis, &c->cnt->err);
        }
        { Timed t(c, "flags_compact", l);
          azk_flags_compact(s, c->cnt, l, c->maxR, c->maxCand, c->B[cur], INV(l), have_v ? Vp(l) : c->pred_u,
                            have_v ? Vs(l) : c->score_u,
                            have_v ? Vz(l) : c->zoom_u, (tune && l == 0) ? 0.0 : p->Tz, p->min_side, l == 0 && !tune, c->cflag,
                            c->zflag, c->bc_c, c->bc_z, c->Yall, c->Sall, c->Z, c->zr); }
        if (l + 1 < nlev) {      // the reference also divides after the last level but never uses it
            const bool track = (n_spec && l == 1);       // level-3 regions remember their speculative row
            { Timed t(c, "divide", l);
              azk_divide(s, &c->cnt->PZ[l], &c->cnt->CH[l], &c->cnt->err, c->maxR, c->maxCh, c->Z, p->min_side,
                         c->choff, c->child, c->ckey, track ? c->choff_all : nullptr, c->zr, &c->cnt->specP1, 1,
                         track ? c->csrc : nullptr); }
            { Timed t(c, "sift_dup", l);
              azk_dedup_regions(s, c->ckey, &c->cnt->CH[l], c->maxCh, c->maxR, c->first, c->child,
                                c->B[cur ^ 1], &c->cnt->P[l + 1], &c->cnt->err, track ? c->csrc : nullptr,
                                c->srcB[cur ^ 1]); }
        }
        have_v = false;           // (a level on the multi-launch kernels never looks the next one's outputs up)
    }
    enqueue_select(c, p, nlev_run, k);
    if (tune && c->pool) {
        Timed t(c, "pool_append", nlev);
        azk_pool_append(s, c->hisZ, &c->cnt->nhis, c->capHis, c->pool, c->pool_n, c->pool_cap);
    }
    return AZ_OK;
}

static int launch_impl_body(az_ctx *c, const az_params *p);

// One search enqueued on THIS context's stream (the public az_propose_launch picks the lane first).
int launch_impl(az_ctx *c, const az_params *p)
{
    const int rc = launch_impl_body(c, p);
    if (rc && c) c->part7_wait = true;            // (it may have taken a buffer of the int7 slab ring: launch_head)
    // a batch slot on the owner's spare head set: the next slot to take the set waits for what this one enqueued (whatever
    // became of the launch -- a failed one may have enqueued its first kernels)
    if (c && c->head_shared && c->owner && c->owner->spare.ev) {
        if (hipEventRecord(c->owner->spare.ev, c->stream) == hipSuccess) c->owner->spare.ev_live = true;
        else { (void)hipGetLastError(); c->async_err = 1; }
    }
    return rc;
}

static int launch_impl_body(az_ctx *c, const az_params *p)
{
    int rc = check_ready(c, true, false);          // (whether `stream` waits for the second stream is decided below)
    if (rc) return rc;
    if (!p || p->im_h <= 0 || p->im_w <= 0 || !(p->scale > 0) || p->batch_size <= 0 || !(p->min_side > 0))
        return fail(c, AZ_ERR_INVALID, "az_propose: bad parameters");
    const int K = num_levels(p->im_h, p->im_w, p->min_side);
    // The tuner's variant of the search (lib/detect/tune.py:256-316, params.reserved bit 2) runs
    // `for k in xrange(K)` -- one level more than test.py:373 --, applies Tz from the second level
    // on (the first compares against 0), never forces the root, and keeps the anchor history Bhis.
    const bool tune = (p->reserved & 4) != 0;
    const int nlev = tune ? K : K - 1;
    if (nlev < 1)
        return fail(c, AZ_ERR_INVALID,
                    "az_propose: image too small for one search level (the reference's loop at "
                    "lib/detect/test.py:373 would not execute)");
    if (nlev > AZ_MAX_LEVELS) return fail(c, AZ_ERR_CAPACITY, "az_propose: too many levels");
    int k = p->num_proposals;
    if (p->fixed_num) {
        if (k <= 0) return fail(c, AZ_ERR_INVALID, "az_propose: num_proposals must be positive");
        if (k > AZ_TOPK_MAX) return fail(c, AZ_ERR_CAPACITY, "az_propose: num_proposals > 4096");
    }
    if ((int)c->pend.size() >= az_ctx::AZ_QUEUE_MAX)
        return fail(c, AZ_ERR_STATE, "az_propose_launch: three searches are already queued on this lane, fetch one first");
    if (!c->head_bufs && (rc = ensure_lane_head(c)) != AZ_OK) return rc;   // (a batch slot searching on its own for the first time)
    if (c->head_shared && c->owner && c->owner->spare.ev_live)             // (... behind the slot that had the spare set before it)
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->owner->spare.ev, 0));
    if (!c->pend.empty() && !(p->fixed_num && c->pend.back().copied))
        return fail(c, AZ_ERR_STATE, "az_propose_launch: queueing a search behind another needs a fixed proposal count for both");
    HIPCHK(c, hipSetDevice(c->device));
    if (!(c->profiling & 4)) clear_events(c);
    c->cand_n = -1;
    if (tune) c->his_n = -1;                       // (hisB / hisZ are one buffer per context: this search writes them)
    if (c->cal.state == 0 && (rc = calibrate_passes(c)) != AZ_OK) return rc;
    hint_load(c, p->im_h, p->im_w, nlev);          // what this shape's last search looked like (decides the form below)
    bool stat = static_wanted(c, p, tune);
    if (stat) {
        if ((rc = ensure_static_plan(c, p, nlev)) != AZ_OK) return rc;
        stat = static_plan_matches(c, p, nlev);          // (a tree that outgrows the plan buffers: level loop)
    }
    c->last_static = stat ? 1 : 0;
    c->full_now = 0;
    if (!stat && (rc = full_prepare(c, p, nlev, tune)) != AZ_OK) return rc;
    c->last_full = !stat ? plan_search(c, p, nlev, tune).full : 0;
    if (!stat && (rc = ensure_spec_cache(c, p, plan_search(c, p, nlev, tune))) != AZ_OK) return rc;
    c->last_defer = (!stat && plan_search(c, p, nlev, tune).defer_root) ? 1 : 0;
    c->last_pair_mask = stat ? 0 : plan_search(c, p, nlev, tune).pair_mask;
    c->last_cut = stat ? 0 : plan_search(c, p, nlev, tune).cut;
    hipStream_t s = c->stream;
    // Stages on streams of their own (az_ctx.h): a search of ONE head pass whose rows do not depend on its own geometry, on a
    // context that runs its searches on ONE lane -- measured (round 5, 600x1000 at Tz = 0): one lane 1.20 -> 1.15-1.17 ms per
    // image (the next image's RoIPool + int6 no longer wait for this one's heads and three single-workgroup geometry kernels);
    // with two lanes the lanes already give that overlap and the split only makes the steps burstier (1.119 -> 1.122 ms), so
    // it is left off there.  AZ_TWO_STAGE=0: never; 2: on two lanes as well; 4: two stages, never three (measurements).
    const int two_stage = c->no_stage_streams ? 0 : c->env.two_stage;
    const bool one_lane = !c->owner && c->lanes == 1;
    c->split_now = (two_stage && (one_lane || two_stage == 2) && (stat || c->last_full) && p->fixed_num && !c->use_graphs &&
                    !tune && !Timed::trace() && !c->head_shared) ? 1 : 0;
    if (c->split_now && !c->stream2) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        bool ok = c->stream2.create(hipStreamNonBlocking, lo) == hipSuccess;
        for (Event *e : {&c->ev_h6, &c->ev_i7, &c->ev_s2}) ok = ok && e->create(hipEventDisableTiming) == hipSuccess;
        ok = ok && c->stream3.create(hipStreamNonBlocking, lo) == hipSuccess;
        for (Event *e : {&c->ev_tail, &c->ev_s3, &c->ev_geo[0], &c->ev_geo[1]}) ok = ok && e->create(hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            c->split_now = 0; c->no_stage_streams = true;          // (this device / runtime does not give the extra streams: one stage)
        }
    }
    // three stages for the whole-tree / closure form (AZ_TWO_STAGE=4: two stages there as well: measurements)
    c->three_now = (c->split_now && !stat && c->last_full && two_stage != 4) ? 1 : 0;
    // (a two-stage search's second stage works in the buffers a three-stage search's geometry may still be using)
    if (c->split_now && !c->three_now && c->s3_live && hipStreamWaitEvent(c->stream2, c->ev_s3, 0) != hipSuccess) c->async_err = 1;
    if (!c->split_now) join_s2(c);                       // every kernel of this search goes to `stream`, into the per-search buffers
    c->gs = nullptr; c->ts = nullptr; c->async_err = 0;
    auto enqueue = [&]() { c->npass = 0; prep_scale(c); return stat ? enqueue_static(c, p, nlev, k) : enqueue_search(c, p, K, nlev, k, tune); };
    // az_set_graphs / AZ_GRAPH=1: capture the launch sequence once per (parameters, feature map) and replay it
    // as a hipGraph.  Every size is read on the device, so the sequence never changes for given parameters.
    if (c->use_graphs && !c->profiling && !(tune && c->pool) && !c->pyr_now) {
        // key = the fields themselves (never the struct's bytes: padding is the caller's garbage)
        std::string key;
        auto put = [&key](const void *v, size_t n) { key.append((const char *)v, n); };
        put(&p->im_h, sizeof p->im_h); put(&p->im_w, sizeof p->im_w); put(&p->scale, sizeof p->scale);
        put(&p->Tz, sizeof p->Tz); put(&p->Tc, sizeof p->Tc); put(&p->dedup, sizeof p->dedup);
        put(&p->eps, sizeof p->eps); put(&p->min_side, sizeof p->min_side); put(&p->batch_size, sizeof p->batch_size);
        put(&p->num_proposals, sizeof p->num_proposals); put(&p->fixed_num, sizeof p->fixed_num);
        put(&p->reserved, sizeof p->reserved);
        const void *fp = c->feat;
        key.append((const char *)&fp, sizeof(fp));
        key.append((const char *)&c->d, sizeof(c->d));
        key.append((const char *)&c->nofuse_h, sizeof(int));
        key.append((const char *)&c->nofuse_w, sizeof(int));
        key.append((const char *)&c->nofuse_lv_h, sizeof(int));
        key.append((const char *)&c->nofuse_lv_w, sizeof(int));
        { const int lim = plan_search(c, p, nlev, tune).lv_limit; key.append((const char *)&lim, sizeof(int)); }
        key.append((const char *)&c->last_static, sizeof(int));
        key.append((const char *)&c->last_pair_mask, sizeof(int));
        key.append((const char *)&c->last_defer, sizeof(int));
        key.append((const char *)&c->last_full, sizeof(int));
        key.append((const char *)&c->last_cut, sizeof(int));
        for (int l = 0; l < nlev; ++l) { const int mr = many_rows_expected(c, l); key.append((const char *)&mr, sizeof(int)); }
        const void *pp = (stat || c->last_full) ? (const void *)c->plan : nullptr;
        key.append((const char *)&pp, sizeof(pp));
        auto it = c->graphs.find(key);
        if (it == c->graphs.end()) {
            // (the first search of a shape also runs once un-captured: one-time attribute calls happen there)
            if ((rc = enqueue()) != AZ_OK) return rc;
            HIPCHK(c, hipStreamSynchronize(s));
            hipGraph_t g = nullptr;
            hipGraphExec_t ge = nullptr;
            HIPCHK(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            rc = enqueue();
            // (whatever enqueue() returned, the capture ends here: the stream must never be left capturing)
            const hipError_t ec = hipStreamEndCapture(s, &g);
            if (rc || ec != hipSuccess) {
                if (g) hipGraphDestroy(g);
                (void)hipGetLastError();
                return rc ? rc : fail(c, AZ_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
            }
            const hipError_t ei = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
            hipGraphDestroy(g);
            if (ei != hipSuccess) return fail(c, AZ_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
            az_ctx::GraphEntry ent;
            ent.exec = ge; ent.npass = c->npass;
            std::memcpy(ent.pass_src, c->pass_src, sizeof(ent.pass_src));
            std::memcpy(ent.pass_lv, c->pass_lv, sizeof(ent.pass_lv));
            it = c->graphs.emplace(key, ent).first;
        }
        c->npass = it->second.npass;
        std::memcpy(c->pass_src, it->second.pass_src, sizeof(c->pass_src));
        std::memcpy(c->pass_lv, it->second.pass_lv, sizeof(c->pass_lv));
        HIPCHK(c, hipGraphLaunch(it->second.exec, s));
    } else {
        if ((rc = enqueue()) != AZ_OK) return rc;
    }
    HIPCHK(c, hipGetLastError());
    if (c->async_err) { c->gs = nullptr; c->ts = nullptr; c->split_now = 0; c->three_now = 0; return fail(c, AZ_ERR_HIP, "az_propose: a stream / event call of the two-stage search failed"); }
    s = geom_stream(c);                                  // where the search ends: its result copy follows there
    az_ctx::PendingSearch q;
    q.p = *p; q.nlev = nlev; q.is_static = c->last_static; q.defer = c->last_defer; q.pair_mask = c->last_pair_mask;
    q.full = c->last_full;
    q.cut = c->last_cut;
    q.pyr = c->pyr_now;
    q.pooled = tune && c->pool;
    q.npass = c->npass;
    q.feat = c->feat; q.fH = c->d.H; q.fW = c->d.W; q.feat_gen = c->feat_gen;
    q.feat_is_copy = c->feat && (c->feat == c->feat_owned[0] || c->feat == c->feat_owned[1] || c->feat == c->feat_owned[2]);
    std::memcpy(q.pass_src, c->pass_src, sizeof(q.pass_src));
    std::memcpy(q.pass_lv, c->pass_lv, sizeof(q.pass_lv));
    for (q.slot = 0; q.slot < 3 && c->slot_busy[q.slot]; ++q.slot) { }
    if (q.slot >= 3) return fail(c, AZ_ERR_STATE, "az_propose_launch: no free result slot");
    if (p->fixed_num) {
        // the result block follows the search's kernels in stream order: whatever is enqueued next (the next image's
        // search, a unit call) finds it already on its way to the host
        HIPCHK(c, hipMemcpyAsync(c->h_res[q.slot], c->cnt, RES_HDR + (size_t)k * 36, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(c->ev_res[q.slot], s));
        q.copied = true;
    }
    q.last_s = s;
    c->last_s = s;
    if (c->gs) { HIPCHK(c, hipEventRecord(c->ev_s2, c->stream2)); c->s2_live = true; }
    if (c->gs && c->gs == c->stream3) {
        HIPCHK(c, hipEventRecord(c->ev_s3, c->stream3));
        HIPCHK(c, hipEventRecord(c->ev_geo[c->out_par], c->stream3));
        c->s3_live = true; c->g_live[c->out_par] = true;
    }
    c->gs = nullptr; c->ts = nullptr; c->split_now = 0; c->three_now = 0;
    c->slot_busy[q.slot] = true;
    c->pend.push_back(q);
    return AZ_OK;
}

// Collect the result of the search at position `idx` of the pending queue (0 = the oldest; a fallback rerun sits at
// the back) and remove it from the queue.
int fetch_entry(az_ctx *c, size_t idx, double *boxes_out, float *scores_out, int cap, int *n_out, az_stats *st)
{
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const az_ctx::PendingSearch q = c->pend[idx];
    const int nlev = q.nlev;
    // With a fixed proposal count the output size is bounded up front: one batched D2H (enqueued by the launch), one wait.
    const int want = q.p.fixed_num ? q.p.num_proposals : -1;
    int rc;
    const double *hY = nullptr;
    const float *hS = nullptr;
    unsigned char *blk = c->h_res[q.slot];
    auto drop = [&]() { c->pend.erase(c->pend.begin() + (long)idx); c->slot_busy[q.slot] = false; };
    if (q.copied) {
        const hipError_t e = hipEventSynchronize(c->ev_res[q.slot]);
        if (e != hipSuccess) { drop(); return fail(c, AZ_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(e)); }
        hY = (const double *)(blk + RES_HDR);
        hS = (const float *)(blk + RES_HDR + (size_t)want * 32);
    } else {
        // (variable proposal count: nothing is queued behind this search)
        drop();
        HIPCHK(c, hipMemcpyAsync(blk, c->cnt, sizeof(AzCounts), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        int n = ((const AzCounts *)blk)->nsel;
        if (n > c->maxCand) n = c->maxCand;
        if ((rc = ensure_host(c, n > 0 ? n : 1)) != AZ_OK) return rc;
        if (n > 0) {
            HIPCHK(c, hipMemcpyAsync(c->h_Y, c->Yout, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipMemcpyAsync(c->h_S, c->Sout, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        hY = c->h_Y;              // (ensure_host may have moved them)
        hS = c->h_S;
    }
    if (q.copied) drop();
    c->last = q.p;
    c->his_n = -1;                                 // (until this fetch has succeeded)
    const AzCounts &h = *(const AzCounts *)blk;
    if (st) {
        std::memset(st, 0, sizeof(*st));
        st->n_levels = nlev;
        st->n_candidates = h.ytot[q.cut ? q.cut : nlev];
        st->spec_rows = h.specU;
        st->root_deferred = q.defer;
        st->static_plan = q.is_static;
        st->search_form = q.batch ? 5 : (q.is_static ? 4 : (q.full == 2 ? 3 : (q.full == 1 ? 2 : (q.pair_mask ? 1 : 0))));
        st->n_reruns = q.reruns;
        const int *hc = reinterpret_cast<const int *>(&h);
        for (int i = 0; i < q.npass && i < AZ_MAX_LEVELS; ++i) {
            const int r = q.pass_src[i] >= 0 ? hc[q.pass_src[i]] : -q.pass_src[i] - 1;
            if (r <= 0) continue;
            // the tree levels whose rois the pass evaluated
            const int lv = q.pass_lv[i];
            const bool spec3 = nlev >= 3 && !(q.p.reserved & (1 | 4));         // (plan_search: n_spec == 3)
            int mask;
            if (lv < 0) {
                if (q.is_static || q.full) mask = (1 << nlev) - 1;
                else if (q.batch) mask = 3;                                    // (the root and its children)
                else mask = (q.cut == 2 ? 3 : 7) & ~(q.defer ? 1 : 0);
            } else {
                mask = 1 << lv;
                if ((q.pair_mask >> lv) & 1) mask |= 1 << (lv + 1);
                if (q.defer && spec3 && lv == 3) mask |= 1;
            }
            st->pass_levels[st->n_passes] = mask;
            st->pass_rows[st->n_passes++] = r;
        }
        for (int l = 0; l < nlev; ++l) {
            st->level_regions[l] = h.P[l];
            st->level_unique[l] = h.U[l];
            st->level_zoomed[l] = h.PZ[l];
            st->num_eval += h.P[l];
            if (h.P[l] > 0) st->depth = (q.p.reserved & 4) ? l : l + 1;   // tune.py counts k from 0
        }
    }
    // A search that has to be run again in another form is launched now (behind whatever is queued), its record staged
    // where the failed run's was, and collected from the back of the queue.
    auto rerun = [&](az_params p2) {
        const int err = h.err;
        (void)err;
        // (a queue that is full cannot take the rerun: the caller queued ahead, so the oldest other search is collected
        //  only after this one -- make room by running this rerun with the queue drained)
        if ((int)c->pend.size() >= az_ctx::AZ_QUEUE_MAX) return fail(c, AZ_ERR_STATE, "az_propose_fetch: no room to rerun a search in another form");
        // the rerun reads THIS search's map (a later one may have been handed over since)
        if (q.feat_is_copy && q.feat_gen != c->feat_gen)
            return fail(c, AZ_ERR_STATE, "az_propose_fetch: the queued search has to be rerun but its feature map copy was reallocated");
        const float *cur_feat = c->feat;
        const int cur_H = c->d.H, cur_W = c->d.W;
        c->feat = q.feat; c->d.H = q.fH; c->d.W = q.fW;
        int rc2 = launch_impl(c, &p2);
        c->feat = cur_feat; c->d.H = cur_H; c->d.W = cur_W;
        if (rc2) return rc2;
        c->pend.back().feat = q.feat; c->pend.back().fH = q.fH; c->pend.back().fW = q.fW;
        c->pend.back().reruns = q.reruns + 1;
        ++c->n_rerun_total;
        if (q.stage_dst && (rc2 = stage_impl(c, q.stage_dst, q.stage_cap)) != AZ_OK) return rc2;
        return fetch_entry(c, c->pend.size() - 1, boxes_out, scores_out, cap, n_out, st);
    };
    if (q.batch && c->batch_set)
        for (int l = 0; l < nlev; ++l) c->batch_set->rows_acc[l] += (l < 2) ? (l == 0 ? h.specU : 0) : h.PR[l];
    if ((h.err & 2048) && q.batch) {
        // a level of the batch held more rois than the head's buffers take rows: every image of it runs again on its own
        az_params p2 = q.p;
        return rerun(p2);
    }
    if ((h.err & 32) && q.is_static) {
        // a zoom score of the tree is not >= Tz (NaN): the one-pass plan's premise fails for this image -> level loop
        az_params p2 = q.p;
        p2.reserved |= 32;
        return rerun(p2);
    }
    if ((h.err & 64) && !(q.p.reserved & 64)) {
        // the pair-speculation rows of a level outgrew the tables: this image shape runs without them from now on
        if (c->nopair.size() >= 32) c->nopair.erase(c->nopair.begin());
        c->nopair.emplace_back(q.p.im_h, q.p.im_w);
        az_params p2 = q.p;
        p2.reserved = (p2.reserved | 64) & ~128;
        return rerun(p2);
    }
    if ((h.err & 1024) && q.cut) {
        // the search was enqueued up to level q.cut only (the previous search of the shape ended there) and this tree goes
        // on: run it in full (its result enters the history below as a search that did not end early)
        az_params p2 = q.p;
        p2.reserved |= 4096;
        return rerun(p2);
    }
    if ((h.err & 256) && !(q.p.reserved & 256)) {
        // the whole-tree pass did not hold a window this search needed (a _sift_dup survivor other than the full tree's):
        // repeat it level by level; its history then says "pruned tree" and the next search of the shape goes that way at once
        if (c->env.full_debug) fprintf(stderr, "az: whole-tree pass missed a window (%dx%d, err %d)\n", q.p.im_h, q.p.im_w, h.err);
        az_params p2 = q.p;
        p2.reserved = (p2.reserved | 256) & ~512;
        return rerun(p2);
    }
    if ((h.err & 8) && !(q.p.reserved & 2)) {
        // a fused level outgrew its LDS tables: rerun with the multi-launch kernels and remember
        // the image shape so that later calls skip the fused attempt -- first only for the levels after the
        // speculative ones (az_level.hip: also level 3 past batch_size at the hand-over); for everything when levels 1-3
        // themselves outgrew k_spec_levels (it says so in scratch[5]: ONE rerun, not one per kernel given up)
        const bool lv_was_on = !(q.p.reserved & 16) &&
                               !(q.p.im_h == c->nofuse_lv_h && q.p.im_w == c->nofuse_lv_w);
        az_params p2 = q.p;
        // scratch[5]: l + 1 from k_level_geom at level l; 0 from the hand-over of k_spec_levels (level 3 past batch_size);
        // -1 from k_spec_levels when one of levels 1-3 outgrew its own tables (only the multi-launch form fits then)
        const int ovf = h.scratch[5] - 1;          // the level whose k_level_geom overflowed (< 0: none did)
        const bool spec_ovf = h.scratch[5] < 0;
        bool limited = false;
        if (lv_was_on && ovf > 3) {
            // a level behind the first fused one: the levels before it keep their fused kernels
            for (auto &e : c->lv_limits)
                if (e.h == q.p.im_h && e.w == q.p.im_w) { if (ovf < e.limit) { e.limit = ovf; limited = true; } }
            bool known = false;
            for (const auto &e : c->lv_limits) known = known || (e.h == q.p.im_h && e.w == q.p.im_w);
            if (!known) {
                if (c->lv_limits.size() >= 32) c->lv_limits.erase(c->lv_limits.begin());
                c->lv_limits.push_back({q.p.im_h, q.p.im_w, ovf});
                limited = true;
            }
        }
        if (limited) { }
        else if (lv_was_on && !spec_ovf) { c->nofuse_lv_h = q.p.im_h; c->nofuse_lv_w = q.p.im_w; p2.reserved |= 16; }
        else { c->nofuse_h = q.p.im_h; c->nofuse_w = q.p.im_w; p2.reserved |= 2; }
        return rerun(p2);
    }
    // (a failed tuner search has appended an incomplete history to the score pool -- past capHis its rows were never
    //  written: the pool answers nothing until the next az_tune_begin)
    if (h.err && q.pooled) c->pool_bad = true;
    if (h.err)
        return fail(c, AZ_ERR_CAPACITY,
                    std::string("az_propose: ctx capacity exceeded (flags ") + std::to_string(h.err) +
                        "): raise az_set_limits");
    if (!q.is_static && !(q.p.reserved & 4) && !q.pyr) {
        hint_load(c, q.p.im_h, q.p.im_w, nlev);           // (the shape's records: a search of another shape may have been launched since)
        if (c->hint_n > 0) {                              // the records move down by one, the oldest drops out
            for (int r = az_ctx::HINT_K - 2; r > 0; --r) c->hint_old[r] = c->hint_old[r - 1];
            std::memcpy(c->hint_old[0].rows, c->hint_rows, sizeof(c->hint_rows)); std::memcpy(c->hint_old[0].P, c->hint_P, sizeof(c->hint_P));
            std::memcpy(c->hint_old[0].PZ, c->hint_PZ, sizeof(c->hint_PZ)); std::memcpy(c->hint_old[0].U, c->hint_U, sizeof(c->hint_U));
            std::memcpy(c->hint_old[0].SPN, c->hint_SPN, sizeof(c->hint_SPN));
        }
        c->hint_n = c->hint_n < az_ctx::HINT_K ? c->hint_n + 1 : az_ctx::HINT_K;
        bool walked_full = true;
        for (int l = 0; walked_full && l + 1 < nlev; ++l) walked_full = h.P[l] > 0 && h.PZ[l] == h.P[l];
        c->hint_full_streak = walked_full ? c->hint_full_streak + 1 : 0;
        for (int l = 0; l < AZ_MAX_LEVELS; ++l) {
            const bool in = l < nlev;
            // rows of the pass at that level (fused level loop: PR; multi-launch forms: the level's unique rois)
            c->hint_rows[l] = in ? (h.PR[l] > 0 ? h.PR[l] : (((q.pair_mask >> (l > 0 ? l - 1 : 0)) & 1) && l > 0 ? 0 : h.U[l])) : 0;
            c->hint_P[l] = in ? h.P[l] : 0;
            c->hint_PZ[l] = in ? h.PZ[l] : 0;
            c->hint_U[l] = in ? h.U[l] : 0;
            c->hint_SPN[l] = (in && ((q.pair_mask >> l) & 1)) ? h.SPN[l] : -1;
        }
        c->hint_h = q.p.im_h; c->hint_w = q.p.im_w; c->hint_nlev = nlev;
        hint_store(c);
        int first_empty = 15;
        for (int l = 1; l < nlev && l < 15; ++l)
            if (h.P[l] == 0) { first_empty = l; break; }
        c->early_hist = (c->early_hist << 4) | (unsigned)first_empty;
        if (c->n_hist < 1000000) ++c->n_hist;
    }
    const int n = h.nsel;
    // (the candidate list stays readable only while no later search has been queued: it would be overwriting it)
    c->cand_n = c->pend.empty() ? h.ytot[q.cut ? q.cut : nlev] : -1;
    // (likewise the anchor history: a tuner search queued behind this one writes the same hisB / hisZ)
    bool his_live = true;
    for (const auto &e : c->pend) his_live = his_live && !(e.p.reserved & 4);
    c->his_n = his_live ? h.nhis : -1;
    if (st) st->n_proposals = n;
    *n_out = n;
    if (n > cap) return fail(c, AZ_ERR_CAPACITY, "az_propose: output capacity too small");
    std::memcpy(boxes_out, hY, (size_t)n * 4 * sizeof(double));
    if (scores_out) std::memcpy(scores_out, hS, (size_t)n * sizeof(float));
    return AZ_OK;
}

int stage_impl(az_ctx *c, void *dst_dev, size_t cap_bytes)
{
    if (!c || c->pend.empty()) return fail(c, AZ_ERR_STATE, "az_propose_stage_result_dev without az_propose_launch");
    az_ctx::PendingSearch &q = c->pend.back();
    if (!q.p.fixed_num) return fail(c, AZ_ERR_STATE, "az_propose_stage_result_dev: fixed proposal count only");
    const size_t bytes = RES_HDR + (size_t)q.p.num_proposals * 36;
    if (!dst_dev || cap_bytes < bytes) return fail(c, AZ_ERR_INVALID, "az_propose_stage_result_dev: destination too small");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t ls = q.last_s ? q.last_s : c->stream;
    HIPCHK(c, hipMemcpyAsync(dst_dev, c->cnt, bytes, hipMemcpyDeviceToDevice, ls));
    // az_propose_fetch waits for the slot's event: recorded again HERE, behind the staging copy, so that "the record is
    // staged when az_propose_fetch returns" holds (the launch recorded it behind the host copy only)
    if (q.copied) HIPCHK(c, hipEventRecord(c->ev_res[q.slot], ls));
    if (ls == c->stream2 && c->stream2) HIPCHK(c, hipEventRecord(c->ev_s2, c->stream2));
    if (ls == c->stream3 && c->stream3) HIPCHK(c, hipEventRecord(c->ev_s3, c->stream3));
    q.stage_dst = dst_dev; q.stage_cap = cap_bytes;
    return AZ_OK;
}
