// az_shape.hip -- what a search prepares per image shape, outside any graph capture: the cached speculative pre-pass, the
// one-pass plan of a Tz <= 0 tree (LRU cache), and the whole-tree / closure row sets built on top of it.
#include "az_search.h"

constexpr unsigned AZ_TAB_ROOT_HOST = 0x1FFFu;      // (az_geom_dev.h: AZ_TAB_ROOT)

// The speculative pre-pass (B1 = divide_region(root), all children of B1, the rois of the speculative rows) is a
// function of the image shape alone: run once per shape, outside any graph capture, its outputs kept in
// dedicated buffers and its three counters on the host; k_spec_levels restores them for every search.
int ensure_spec_cache(az_ctx *c, const az_params *p, const SearchPlan &q)
{
    if (!q.fused) return AZ_OK;
    const int defer = q.defer_root ? 1 : 0;
    auto &k = c->spc[defer];
    if (k.h == p->im_h && k.w == p->im_w && k.scale == p->scale && k.min_side == p->min_side)
        return AZ_OK;
    auto use = [&](az_ctx::SpecEntry &e) {
        c->spec_urois[defer] = e.urois; c->specB1[defer] = e.B1; c->spec_choff[defer] = e.choff; c->spec_U[defer] = e.Udev;
        k.h = e.h; k.w = e.w; k.scale = e.scale; k.min_side = e.min_side; k.P1 = e.P1; k.CH = e.CH; k.U = e.U;
        e.use = ++c->spec_clock;
    };
    for (auto &e : c->spec_store)
        if (e.h == p->im_h && e.w == p->im_w && e.defer == defer && e.scale == p->scale && e.min_side == p->min_side) {
            use(e);
            return AZ_OK;
        }
    join_s2(c);                        // (the pre-pass works in the per-search buffers)
    hipStream_t s = c->stream;
    azk_spec_prepass(s, c->cnt, c->B[0], c->spec_scr_B1[defer], c->child, c->spec_scr_choff[defer], c->spec_scr_urois[defer],
                     p->scale, p->min_side, c->maxR, c->maxCh, p->im_h, p->im_w, defer);
    HIPCHK(c, hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(AzCounts), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (c->h_cnt->err) {               // the speculative rows outgrow the context: take the multi-launch path
        c->nofuse_h = p->im_h; c->nofuse_w = p->im_w;
        k.h = -1;
        return AZ_OK;
    }
    az_ctx::SpecEntry e;
    e.h = p->im_h; e.w = p->im_w; e.defer = defer; e.scale = p->scale; e.min_side = p->min_side;
    e.P1 = c->h_cnt->specP1; e.CH = c->h_cnt->specCH; e.U = c->h_cnt->specU;
    if (reserve_group({{&e.own[0], (size_t)(e.U + 1) * 5 * sizeof(float)}, {&e.own[1], (size_t)(e.P1 + 1) * 4 * sizeof(double)},
                       {&e.own[2], (size_t)(e.P1 + 1) * sizeof(int)}, {&e.own[3], 16}}) != hipSuccess)
        return fail(c, AZ_ERR_HIP, "hipMalloc failed for a speculative pre-pass entry");
    e.urois = e.own[0].as<float>(); e.B1 = e.own[1].as<double>(); e.choff = e.own[2].as<int>(); e.Udev = e.own[3].as<int>();
    HIPCHK(c, hipMemcpyAsync(e.urois, c->spec_scr_urois[defer], (size_t)e.U * 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(e.B1, c->spec_scr_B1[defer], (size_t)e.P1 * 4 * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(e.choff, c->spec_scr_choff[defer], (size_t)e.P1 * sizeof(int), hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(e.Udev, &c->cnt->specU, sizeof(int), hipMemcpyDeviceToDevice, s));
    const int rows_short = (defer ? 0 : 1) + e.P1;        // the pass without the third level's rows (early end: plan.cut == 2)
    HIPCHK(c, hipMemcpyAsync(e.Udev + 1, &rows_short, sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (c->spec_store.size() >= 128) {
        // drop the least recently used entry; captured launch sequences may hold its pointers: drop those too
        size_t lru = 0;
        for (size_t i = 1; i < c->spec_store.size(); ++i) if (c->spec_store[i].use < c->spec_store[lru].use) lru = i;
        for (auto &g : c->graphs) hipGraphExecDestroy(g.second.exec);
        c->graphs.clear();
        auto &d = c->spec_store[lru];
        for (int i = 0; i < 2; ++i) if (c->spec_urois[i] == d.urois) { c->spc[i].h = -1; }
        c->spec_store.erase(c->spec_store.begin() + (long)lru);
    }
    c->spec_store.push_back(std::move(e));
    use(c->spec_store.back());
    return AZ_OK;
}

bool plan_is_for(const az_ctx::StaticPlan &k, const az_params *p, int nlev)
{
    return k.h == p->im_h && k.w == p->im_w && k.scale == p->scale && k.min_side == p->min_side &&
           k.dedup == p->dedup && k.batch == p->batch_size && k.nlev == nlev;
}

bool static_plan_matches(const az_ctx *c, const az_params *p, int nlev)
{
    return c->plan && plan_is_for(*c->plan, p, nlev);
}

// All levels' regions with every region zoomed: the level loop's own geometry kernels (roi projection + dedup,
// divide_region + _sift_dup), run once per image shape, outside any graph capture.
int ensure_static_plan(az_ctx *c, const az_params *p, int nlev)
{
    for (auto *q : c->plans)
        if (plan_is_for(*q, p, nlev)) { c->plan = q; q->last_use = ++c->plan_clock; return AZ_OK; }
    c->plan = nullptr;
    join_s2(c);                        // (the plan is built in the per-search buffers)
    hipStream_t s = c->stream;
    auto give_up = [&]() {
        if (c->nostatic.size() >= 32) c->nostatic.erase(c->nostatic.begin());
        c->nostatic.emplace_back(p->im_h, p->im_w);
        return (int)AZ_OK;
    };
    az_ctx::StaticPlan k;      // (owns its five device buffers: freed on every exit but the one that moves it into the cache)
    // Two passes over the tree: sizes first, then placement.  Rows of the one head pass: levels 2, 3, ... in order, the
    // root last (RoIPool treats that one whole-image roi cooperatively: a workgroup per bin instead of a wave.
    // Deepest level first with levels 1-3 cooperative was measured too: 26.2 us against 24.5).
    int uoff[AZ_MAX_LEVELS] = {0};
    int roff = 0;
    for (int pass = 0; pass < 2; ++pass) {
        azk_init_root(s, c->cnt, c->B[0], p->im_h, p->im_w);
        roff = 0;
        for (int l = 0; l < nlev; ++l) {
            const int cur = l & 1;
            azk_rois_dedup(s, c->B[cur], &c->cnt->P[l], c->maxR, p->scale, nullptr, (float)p->dedup, p->batch_size,
                           c->rois, c->key, c->grp, c->first, c->index, c->inv, c->urois, c->ubox, &c->cnt->U[l]);
            if (l + 1 < nlev) {
                azk_divide(s, &c->cnt->P[l], &c->cnt->CH[l], &c->cnt->err, c->maxR, c->maxCh, c->B[cur], p->min_side,
                           c->choff, c->child, c->ckey, nullptr, nullptr, nullptr, 0, nullptr);
                azk_dedup_regions(s, c->ckey, &c->cnt->CH[l], c->maxCh, c->maxR, c->first, c->child, c->B[cur ^ 1],
                                  &c->cnt->P[l + 1], &c->cnt->err, nullptr, nullptr);
            }
            if (pass == 0) {
                HIPCHK(c, hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(AzCounts), hipMemcpyDeviceToHost, s));
                HIPCHK(c, hipStreamSynchronize(s));
                if (c->h_cnt->err) return give_up();
                k.roff[l] = roff; k.U[l] = c->h_cnt->U[l]; k.CH[l] = (l + 1 < nlev) ? c->h_cnt->CH[l] : 0;
                roff += c->h_cnt->P[l];
                if (l == 0 && (c->h_cnt->P[0] != 1 || k.U[0] != 1)) return give_up();
            } else {
                const int P = k.roff[l + 1] - k.roff[l], U = k.U[l];
                if (P > 0) {
                    HIPCHK(c, hipMemcpyAsync(k.urois + (size_t)uoff[l] * 5, c->urois, (size_t)U * 5 * sizeof(float),
                                             hipMemcpyDeviceToDevice, s));
                    HIPCHK(c, hipMemcpyAsync(k.ubox + (size_t)uoff[l] * 4, c->ubox, (size_t)U * 4 * sizeof(double),
                                             hipMemcpyDeviceToDevice, s));
                    azk_plan_rows(s, c->inv, &c->cnt->P[l], c->maxR, k.roff[l], uoff[l], k.reg_u);
                }
            }
        }
        if (pass == 0) {
            k.roff[nlev] = roff;
            int tot = 0;
            for (int l = 1; l < nlev; ++l) { uoff[l] = tot; tot += k.U[l]; }
            uoff[0] = tot;
            k.Utot = tot + 1;
            if (k.Utot > c->maxR || roff > c->maxR) return give_up();
            k.coop = 1;
            // exact-size buffers of this shape's plan
            if (k.own.alloc(&k.urois, (size_t)k.Utot * 5) != hipSuccess || k.own.alloc(&k.ubox, (size_t)k.Utot * 4) != hipSuccess ||
                k.own.alloc(&k.reg_u, (size_t)roff) != hipSuccess || k.own.alloc(&k.cand_src, (size_t)roff * AZ_NSUB) != hipSuccess ||
                k.own.alloc(&k.meta, 4) != hipSuccess)
                return fail(c, AZ_ERR_HIP, "hipMalloc failed for a static plan");
        }
    }
    if (hipMemcpyAsync(k.meta, &k.Utot, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess ||
        (azk_plan_cands(s, k.reg_u, k.roff[nlev], k.cand_src), hipStreamSynchronize(s)) != hipSuccess)
        return fail(c, AZ_ERR_HIP, "static plan: copy failed");
    k.h = p->im_h; k.w = p->im_w; k.scale = p->scale; k.min_side = p->min_side; k.dedup = p->dedup;
    k.batch = p->batch_size; k.nlev = nlev;
    k.last_use = ++c->plan_clock;
    if (c->plan_cache_max < 1) c->plan_cache_max = 1;
    if ((int)c->plans.size() >= c->plan_cache_max) {
        // drop the least recently used shape; captured launch sequences may hold its pointers: drop those too
        size_t lru = 0;
        for (size_t i = 1; i < c->plans.size(); ++i) if (c->plans[i]->last_use < c->plans[lru]->last_use) lru = i;
        for (auto &g : c->graphs) hipGraphExecDestroy(g.second.exec);
        c->graphs.clear();
        delete c->plans[lru];
        c->plans.erase(c->plans.begin() + (long)lru);
    }
    c->plans.push_back(new az_ctx::StaticPlan(std::move(k)));
    c->plan = c->plans.back();
    return AZ_OK;
}

// Whole-tree speculation: should this search evaluate, in ONE head pass, a shape-static superset of the rows its tree can
// need and find every level's outputs by window lookup?  Two supersets (StaticPlan::fs): the unique rois of the shape's FULL
// tree (fewest rows; right only if the tree turns out full -- a pruned tree may keep another _sift_dup survivor, err bit
// 256 -> the search is repeated level by level) and the CLOSURE over all survivor choices (~12 % more rows at 600x1000;
// right for every tree).  It pays when the tree is dense: the level-by-level forms stream the int6 weights once per pass
// and pay each pass's fixed cost (RoIPool, reduce, int7, heads, a geometry kernel), the whole-tree pass pays the rows the
// tree does not have.  The decision is by ROW COUNTS: what the shape's previous search would have cost in the
// level-by-level form the context would pick for it (pair_plan) against one pass of the superset's rows, with the pass
// costs measured on this device (pass_us).  A full-tree history takes the tree rows, anything else the closure.
// Builds what the form needs (the shape's plan, the non-deferred speculative pre-pass, the window table, the row map)
// outside any graph capture; sets c->full_now.  params.reserved bit 8: never; bit 9: whenever the shape allows (tests) --
// the tree rows, or with bit 10 the closure; AZ_FULL_SPEC=0 / 2 / 3 likewise (3 = closure whenever possible).
static int build_full_set(az_ctx *c, const az_params *p, int nlev, int variant)
{
    az_ctx::StaticPlan &k = *c->plan;
    az_ctx::StaticPlan::FullSet &f = k.fs[variant];
    const auto &sp = c->spc[0];
    join_s2(c);
    hipStream_t s = c->stream;
    f.own.release();                               // (what an earlier attempt that ended in an error left behind)
    auto give_up = [&]() {
        (void)hipGetLastError();
        f = az_ctx::StaticPlan::FullSet();
        f.full_state = -1;
        return (int)AZ_OK;
    };
    if (sp.U > 64) return give_up();
    const int root = k.Utot - 1;                   // the plan's last row
    int base_rows = 0;                             // rows of the pass before the extra rows
    struct Tmp { float *all = nullptr; int *newrow = nullptr; DevList own; } tmp;
    int N = 0;
    if (variant == 1) {
        // every region any pruning can produce, level by level (no _sift_dup: whichever duplicate survives is among them)
        const int capAll = (int)AZ_TAB_ROOT_HOST - 2;
        if (tmp.own.alloc(&tmp.all, (size_t)capAll * 5) != hipSuccess || tmp.own.alloc(&tmp.newrow, (size_t)capAll) != hipSuccess)
            return give_up();
        const double rootb[4] = {0.0, 0.0, p->im_w - 1.0, p->im_h - 1.0};           // test.py:355
        HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
        HIPCHK(c, hipMemcpyAsync(c->Z, rootb, sizeof(rootb), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipStreamSynchronize(s));                                          // (`rootb` lives on this frame)
        int n_cur = 1;
        for (int l = 0; l < nlev; ++l) {
            if (N + n_cur > capAll) return give_up();
            azk_closure_rois(s, c->Z, n_cur, p->scale, tmp.all + (size_t)N * 5);
            N += n_cur;
            if (l + 1 == nlev) break;
            int rc = set_count(c, &c->cnt->PZ[0], n_cur);
            if (rc) return rc;
            azk_divide(s, &c->cnt->PZ[0], &c->cnt->CH[0], &c->cnt->err, c->maxR, c->maxCh, c->Z, p->min_side, c->choff,
                       c->child, c->ckey, nullptr, nullptr, nullptr, 0, nullptr);
            HIPCHK(c, hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(AzCounts), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            const int n_next = c->h_cnt->CH[0];
            if (c->h_cnt->err || n_next > c->maxR) {
                HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
                return give_up();
            }
            if (n_next == 0) break;
            HIPCHK(c, hipMemcpyAsync(c->Z, c->child, (size_t)n_next * 4 * sizeof(double), hipMemcpyDeviceToDevice, s));
            n_cur = n_next;
        }
    }
    const int cap = (variant == 1 ? N : k.Utot) + sp.U + 1;
    unsigned T = 64; while (T < 2u * (unsigned)cap) T <<= 1;
    if (cap > c->maxR || cap >= (int)AZ_TAB_ROOT_HOST ||
        f.own.alloc(&f.htab, (size_t)T) != hipSuccess || f.own.alloc(&f.spec_map, (size_t)sp.U) != hipSuccess ||
        f.own.alloc(&f.full_meta, 4) != hipSuccess || f.own.alloc(&f.full_urois, (size_t)cap * 5) != hipSuccess ||
        f.own.alloc(&f.full_ubox, (size_t)cap * 4) != hipSuccess)
        return give_up();
    f.hT = T;
    HIPCHK(c, hipMemsetAsync(f.full_meta, 0, 16, s));
    int h[4] = {0, 0, 0, 0};
    if (variant == 1) {
        azk_full_tab_build(s, tmp.all, N, 0, c->spatial_scale, f.htab, T, f.full_meta + 2);
        azk_closure_compact(s, tmp.all, N, c->spatial_scale, f.htab, T, tmp.newrow, f.full_urois, f.full_ubox, f.full_meta + 3,
                            f.full_meta + 2);
        HIPCHK(c, hipMemcpyAsync(h, f.full_meta, 16, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (h[2]) return give_up();
        base_rows = h[3];
    } else {
        HIPCHK(c, hipMemcpyAsync(f.full_urois, k.urois, (size_t)root * 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(f.full_ubox, k.ubox, (size_t)root * 4 * sizeof(double), hipMemcpyDeviceToDevice, s));
        azk_full_tab_build(s, k.urois, k.Utot, root, c->spatial_scale, f.htab, T, f.full_meta + 2);
        base_rows = root;
    }
    // every row of the speculative layout (levels 1-3) -> its row in this pass; windows the rows above lack become extra rows
    azk_full_map(s, c->spec_urois[0], sp.U, c->spatial_scale, f.htab, T, base_rows, cap, f.full_urois, f.full_ubox, f.spec_map,
                 f.full_meta + 1, f.full_meta + 2);
    HIPCHK(c, hipMemcpyAsync(h, f.full_meta, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (h[2] || (variant == 1 && h[1] != 0)) return give_up();       // (the closure holds every speculative row by construction)
    f.Ufull = base_rows + h[1] + 1;
    // the root: the pass's last row (RoIPool treats the tail of a launch cooperatively)
    HIPCHK(c, hipMemcpyAsync(f.full_urois + (size_t)(f.Ufull - 1) * 5, k.urois + (size_t)root * 5, 5 * sizeof(float),
                             hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(f.full_ubox + (size_t)(f.Ufull - 1) * 4, k.ubox + (size_t)root * 4, 4 * sizeof(double),
                             hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(f.full_meta, &f.Ufull, sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    f.full_state = 1;
    if (c->env.full_debug) fprintf(stderr, "az: whole-tree rows for (%dx%d), %s: %d (full tree %d, closure regions %d)\n",
                                         p->im_h, p->im_w, variant ? "closure" : "tree", f.Ufull, k.Utot, N);
    return AZ_OK;
}

int full_prepare(az_ctx *c, const az_params *p, int nlev, bool tune)
{
    c->full_now = 0;
    if (tune || (p->reserved & (1 | 2 | 16 | 256)) || !p->fixed_num) return AZ_OK;
    const bool forced = (p->reserved & 512) || c->env.full_spec >= 2;
    if (!forced && c->env.full_spec == 0) return AZ_OK;
    const SearchPlan q0 = plan_search(c, p, nlev, tune);        // (full_now is 0: the other form's plan)
    if (!(q0.fused && q0.fused_lv && q0.n_spec == 3 && q0.lv_limit >= q0.n_spec && nlev > q0.n_spec)) return AZ_OK;
    const bool have_hist = c->hint_h == p->im_h && c->hint_w == p->im_w && c->hint_nlev == nlev && c->hint_n > 0;
    // the last TWO searches of this shape walked the FULL tree (every region zoomed at every level but the last)?  One full
    // tree in a stream of different images says little about the next, and a tree-rows pass that misses a window costs a
    // second search; a context that keeps seeing full trees (Tz <= 0, or a threshold every region passes) gets there at its
    // third search.
    const bool full_hist = have_hist && c->hint_full_streak >= 2;
    if (!forced && !have_hist) return AZ_OK;
    int variant = forced ? (((p->reserved & 1024) || c->env.full_spec == 3) ? 1 : 0) : (full_hist ? 0 : 1);
    int rc;
    if ((rc = ensure_static_plan(c, p, nlev)) != AZ_OK) return rc;
    if (!static_plan_matches(c, p, nlev)) return AZ_OK;
    az_ctx::StaticPlan &k = *c->plan;
    if (k.fs[variant].full_state < 0) return AZ_OK;
    double now = 0.0;
    if (!forced) {
        // cheapest the superset can be: the full tree's rows.  Not worth building anything if even that loses.
        // (expected over the shape's recorded trees)
        const int specU = c->spc[q0.defer_root ? 1 : 0].h == p->im_h ? c->spc[q0.defer_root ? 1 : 0].U : 48;
        // (the tree-rows pass presumes the tree is full again: priced against the full trees of the streak)
        const int nrec = variant == 0 ? (c->hint_full_streak < c->hint_n ? c->hint_full_streak : c->hint_n) : c->hint_n;
        for (int r = 0; r < nrec; ++r) now += level_forms_cost(c, hint_rec(c, r), nlev, q0.n_spec, specU, q0.pair_mask);
        now /= nrec;
        const double best = pass_us(c, k.Utot) + PASS_OVERHEAD_US + LOOKUP_US * (nlev - q0.n_spec);
        if (!(best + 10.0 < now)) return AZ_OK;
    }
    // the non-deferred layout of the speculative rows (the root is row 0 there; here it maps to the pass's last row)
    SearchPlan q1 = q0; q1.defer_root = false;
    if ((rc = ensure_spec_cache(c, p, q1)) != AZ_OK) return rc;
    const auto &sp = c->spc[0];
    if (!(sp.h == p->im_h && sp.w == p->im_w && sp.scale == p->scale && sp.min_side == p->min_side)) return AZ_OK;
    if (k.fs[variant].full_state == 0 && (rc = build_full_set(c, p, nlev, variant)) != AZ_OK) return rc;
    if (k.fs[variant].full_state != 1) return AZ_OK;
    if (!forced) {
        const double full = pass_us(c, k.fs[variant].Ufull) + PASS_OVERHEAD_US + LOOKUP_US * (nlev - q0.n_spec);
        if (!(full + 10.0 < now)) return AZ_OK;
    }
    c->full_now = variant + 1;
    if (c->env.full_debug) fprintf(stderr, "az: whole-tree pass on (%dx%d): %d rows (%s; plan %d)\n", p->im_h, p->im_w,
                                         k.fs[variant].Ufull, variant ? "closure" : "tree rows", k.Utot);
    return AZ_OK;
}

