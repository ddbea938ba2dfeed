// az_plan.hip -- which form a search takes: the head-pass cost model (measured on the device), the history of an image
// shape's last searches, and the planner that picks speculative levels, fused kernels, deferred root, pair rows, the
// whole-tree pass and the early end from them.
#include "az_search.h"

// Cost of one head pass (RoIPool, int6, reduce, int7, heads) at `rows` rois, in us: measured on this device at a few row
// counts the first time the context launches a search (calibrate_passes) and interpolated; until then (or with
// AZ_PASS_CAL=0) the figures of the round-3 profiles: weight-streaming bound up to ~40 rows, then ~1.4 us per row.
// What a level costs besides its head pass (its geometry kernel and the kernel boundaries) is GEOM_US; a window lookup
// stage LOOKUP_US.
double pass_us(const az_ctx *c, double rows)
{
    const auto &k = c->cal;
    if (k.state == 1 && k.n >= 2) {
        if (rows <= k.rows[0]) return k.us[0];
        for (int i = 1; i < k.n; ++i)
            if (rows <= k.rows[i] || i == k.n - 1)
                return k.us[i - 1] + (k.us[i] - k.us[i - 1]) * (rows - k.rows[i - 1]) / (double)(k.rows[i] - k.rows[i - 1]);
    }
    // (int6 on the 16-bit matrix cores, az_set_gemm_mode 2 / 3: a row costs a fraction of that, a launch somewhat more.
    //  Measured: two terms 100-113 us at 48 rows, 365 us at 670; three terms 125 us and 630 us -- int6 alone)
    double t;
    if (c->gemm_parts == 2) { t = 85.0 + 0.42 * rows; t = t < 100.0 ? 100.0 : t; }
    else if (c->gemm_parts == 3) { t = 110.0 + 0.78 * rows; t = t < 130.0 ? 130.0 : t; }
    else { t = 60.0 + 1.4 * rows; t = t < 92.0 ? 92.0 : t; }
    return t + 50.0;
}

// Measure pass_us on this device: whole head passes over synthetic rois (a grid of ~64-px boxes on the current map) at a
// few row counts, HIP events on the ctx stream, best of three each; ~10 ms, once per context, outside any capture and with
// no search queued.  The forms' costs differ by tens of us per image and boxes of one pool differ by 5-10 %: literals tuned
// on one box pick the wrong form on another.  AZ_PASS_CAL=0 keeps the literals.
int calibrate_passes(az_ctx *c)
{
    auto &k = c->cal;
    if (k.state != 0) return AZ_OK;
    if (!c->env.pass_cal) { k.state = -1; return AZ_OK; }
    if (!c->feat || !c->pend.empty() || c->d.H <= 0 || c->d.W <= 0) return AZ_OK;       // (next time)
    join_s2(c);
    k.state = -1;                                                                      // (any failure below: literals)
    hipStream_t s = c->stream;
    const int sizes[] = {48, 112, 176, 352, 704, 1408};
    int nsz = 0;
    for (int v : sizes) if (v + 1 < c->maxR) ++nsz;
    if (nsz < 2) return AZ_OK;
    const int maxrows = sizes[nsz - 1];
    {   // rois: boxes of ~4 x 4 map cells walking over the map (what the deep levels look like)
        std::vector<float> r((size_t)maxrows * 5);
        const float fw = (float)c->d.W / c->spatial_scale, fh = (float)c->d.H / c->spatial_scale;
        for (int i = 0; i < maxrows; ++i) {
            const float x = fmodf(37.0f * i, fw > 80.f ? fw - 72.f : 1.f), y = fmodf(53.0f * i, fh > 80.f ? fh - 72.f : 1.f);
            r[5 * (size_t)i] = 0.f; r[5 * (size_t)i + 1] = x; r[5 * (size_t)i + 2] = y;
            r[5 * (size_t)i + 3] = x + 63.f; r[5 * (size_t)i + 4] = y + 63.f;
        }
        HIPCHK(c, hipMemcpyAsync(c->urois, r.data(), r.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    Event ea, eb;
    if (ea.create(hipEventDefault) != hipSuccess || eb.create(hipEventDefault) != hipSuccess) {
        (void)hipGetLastError();
        return AZ_OK;
    }
    const int prof = c->profiling;
    c->profiling = 0;
    c->cand_n = -1;
    bool ok = true;
    for (int i = 0; i < nsz && ok; ++i) {
        HIPCHK(c, hipMemsetAsync(c->cnt, 0, sizeof(AzCounts), s));
        ok = set_count(c, &c->cnt->U[0], sizes[i]) == AZ_OK;
        double best = 1e30;
        for (int rep = 0; rep < 4 && ok; ++rep) {
            prep_scale(c);
            ok = hipEventRecord(ea, s) == hipSuccess;
            launch_head(c, &c->cnt->U[0], 0, 1, 1, 0.0, c->zoom_u, c->score_u, c->delta_u, 0.0, false, 0, nullptr, nullptr, sizes[i]);
            ok = ok && hipEventRecord(eb, s) == hipSuccess && hipEventSynchronize(eb) == hipSuccess;
            float ms = 0.f;
            ok = ok && hipEventElapsedTime(&ms, ea, eb) == hipSuccess;
            if (rep > 0 && ms * 1e3 < best) best = ms * 1e3;
        }
        k.rows[i] = sizes[i]; k.us[i] = best;
    }
    c->profiling = prof;
    c->npass = 0;
    (void)hipGetLastError();
    if (!ok) return AZ_OK;
    for (int i = 1; i < nsz; ++i) if (!(k.us[i] > k.us[i - 1])) k.us[i] = k.us[i - 1] + 1.0;    // (monotone)
    k.n = nsz;
    k.state = 1;
    if (c->env.full_debug) {
        fprintf(stderr, "az: head-pass cost on this device (rows: us):");
        for (int i = 0; i < nsz; ++i) fprintf(stderr, " %d: %.1f", k.rows[i], k.us[i]);
        fprintf(stderr, "\n");
    }
    return AZ_OK;
}

// Pair speculation: the head pass of level l also evaluates one row per distinct RoIPool window among ALL children of
// its regions, so that level l+1 needs no pass of its own (az_level.hip).  Worth it when most regions zoom: the extra
// rows are then few more than level l+1 would have forwarded anyway, and a whole pass (one stream of the 411 MB int6
// weights for small levels, the reduce / int7 / heads / geometry chain always) disappears.  The decision comes from
// the previous search of this context on the same image shape (what a dataset run looks like); without history
// nothing is speculated.  params.reserved bit 6 / AZ_PAIR_SPEC=0: never; bit 7 / AZ_PAIR_SPEC=2: at every eligible
// level (tests).  Results are bit-identical either way.
// The records of the shape's history: r = 0 the last search (the hint_* fields), r = 1.. the ones before it.
HintView hint_rec(const az_ctx *c, int r)
{
    if (r == 0) return {c->hint_rows, c->hint_P, c->hint_PZ, c->hint_U, c->hint_SPN};
    const auto &o = c->hint_old[r - 1];
    return {o.rows, o.P, o.PZ, o.U, o.SPN};
}
constexpr double EMPTY_LEVEL_US = 35.0;    // an enqueued level whose row count turns out to be zero: five launches + a geometry kernel that leave at once

// rows a pair-speculating pass of level l carries for level l+1, for one recorded tree: what it carried then, else level l+1's
// unique rois scaled by parents / zoomed parents, else (the tree ended at level l) ~4.5 windows per region
static double pair_rows(const HintView &v, int l)
{
    if (v.SPN[l] >= 0) return (double)v.SPN[l];
    if (v.U[l + 1] > 0) return (double)v.U[l + 1] * v.P[l] / (v.PZ[l] > 0 ? v.PZ[l] : 1);
    return 4.5 * v.P[l];
}

static int pair_plan(az_ctx *c, const az_params *p, int nlev, int n_spec, bool fused_lv, int lv_limit)
{
    if (!fused_lv || (p->reserved & 64) || c->env.pair_spec == 0) return 0;
    for (const auto &hw : c->nopair)
        if (hw.first == p->im_h && hw.second == p->im_w) return 0;
    const bool force = (p->reserved & 128) || c->env.pair_spec == 2;
    const bool hist = c->hint_h == p->im_h && c->hint_w == p->im_w && c->hint_nlev == nlev && c->hint_n > 0;
    int mask = 0;
    for (int l = n_spec; l + 1 < nlev && l < lv_limit; ++l) {      // (the lookup runs in level l's fused geometry kernel)
        bool want = force;
        if (!want && hist) {
            // expected cost over the shape's recorded trees that reached level l (the others pay nothing here either way)
            double with = 0.0, without = 0.0;
            int n = 0;
            bool fits = true;
            for (int r = 0; r < c->hint_n; ++r) {
                const HintView v = hint_rec(c, r);
                if (v.P[l] <= 0) continue;
                const double S = pair_rows(v, l);
                with += pass_us(c, v.U[l] + S) + PASS_OVERHEAD_US + LOOKUP_US;
                without += pass_us(c, v.U[l]) + PASS_OVERHEAD_US +
                           (v.U[l + 1] > 0 ? pass_us(c, v.U[l + 1]) + PASS_OVERHEAD_US : EMPTY_LEVEL_US);
                fits = fits && v.U[l] + S + 2 < c->maxR;
                ++n;
            }
            want = n > 0 && with < without && fits;
        }
        if (want) { mask |= 1 << l; ++l; }          // level l+1 is looked up: it has no pass to carry rows
    }
    return mask;
}

SearchPlan plan_search(az_ctx *c, const az_params *p, int nlev, bool tune)
{
    SearchPlan q;
    q.n_spec = (nlev >= 3 && !(p->reserved & 1) && !tune) ? 3 : 0;
    // The geometry of those three levels is a few dozen elements per stage: by default it runs
    // inside single-workgroup kernels (az_fused.hip) instead of ~40 tiny launches.
    // (params.reserved bit 1 keeps the multi-launch form; same bits, for tests.)
    q.fused = q.n_spec && !(p->reserved & 2) && !(p->im_h == c->nofuse_h && p->im_w == c->nofuse_w);
    // Levels after the speculative ones: one single-workgroup kernel per mid-tree level (az_level.hip) instead of
    // ten launches (params.reserved bit 4 keeps the multi-launch form; same bits).
    q.fused_lv = q.fused && nlev > q.n_spec && !(p->reserved & 16) &&
                 !(p->im_h == c->nofuse_lv_h && p->im_w == c->nofuse_lv_w);
    // The root's row (zoom forced, candidates only needed by the final selection) moves from the speculative
    // pass to the first fused level's head pass: 48 rows = 1.5 strips instead of 49 = 2 for a 600x1000 image
    // (same bits either way).  That level must be a mid-tree one.
    q.defer_root = q.fused_lv && q.n_spec == 3 && nlev >= q.n_spec + 2;
    // ... and must exist: a tree that ends before it would pay a whole head pass for the root's one row (measured: a
    // [1, 8, 0, 0, 0] tree 0.43 ms deferred against 0.32).  The previous search of this image shape tells.
    if (q.defer_root && c->hint_h == p->im_h && c->hint_w == p->im_w && c->hint_nlev == nlev && c->hint_P[q.n_spec] == 0)
        q.defer_root = false;
    // (round 5: a stream of different images -- deferring gains 16 us when the tree reaches that level and costs a whole
    //  one-row head pass, ~110 us, when it does not: only when every one of the context's last four searches got there)
    if (q.defer_root && c->n_hist < 4) q.defer_root = false;
    for (int i = 0; i < 4 && q.defer_root; ++i)
        if ((int)((c->early_hist >> (4 * i)) & 15u) <= q.n_spec) q.defer_root = false;
    q.lv_limit = AZ_MAX_LEVELS + 1;
    for (const auto &e : c->lv_limits)
        if (e.h == p->im_h && e.w == p->im_w) q.lv_limit = e.limit;
    q.pair_mask = pair_plan(c, p, nlev, q.n_spec, q.fused_lv, q.lv_limit);
    // whole-tree speculation (decided and prepared by az_propose_launch: full_prepare): one head pass over the rows of
    // the image shape's full tree, every level's outputs by window lookup -- no deferred root, no pair rows
    q.full = (c->full_now && q.fused && q.fused_lv && q.n_spec == 3 && q.lv_limit >= q.n_spec && c->plan &&
              c->plan->fs[c->full_now - 1].full_state == 1 && plan_is_for(*c->plan, p, nlev)) ? c->full_now : 0;
    if (q.full) { q.defer_root = false; q.pair_mask = 0; }
    // early end: recent searches of this context had no regions from level `cut` on (a level the fused kernels hand over
    // to: the one before it carries the check).  Two rules, by what a miss costs (round 5; az_ctx.h: early_hist):
    //   cut == 2 (the tree is the root and its children): a hit saves the third level's 40 rows and two empty levels
    //            (~70 us of ~170), a miss wastes the 9-row pass (~100 us) -- taken when at least 7 of the context's last 8
    //            searches ended there, whatever the very last one did;
    //   cut >= 3: a miss repeats a search that has already run most of its passes -- taken only when the last four all
    //            ended at or before that level.
    q.cut = 0;
    if (!(p->reserved & 4096) && !q.full && !tune && q.fused && q.fused_lv) {
        auto ended_by = [&](int i, int l) { return (int)((c->early_hist >> (4 * i)) & 15u) <= l; };
        if (q.n_spec == 3 && nlev > 2) {
            int n2 = 0;
            for (int i = 0; i < 8; ++i) n2 += ended_by(i, 2) ? 1 : 0;
            if (n2 >= 7) q.cut = 2;
        }
        for (int l = q.n_spec; !q.cut && l < nlev; ++l) {
            bool all = true;
            for (int i = 0; i < 4 && all; ++i) all = ended_by(i, l);
            if (all) q.cut = l;
        }
        if (q.cut > q.n_spec && q.cut - 1 >= q.lv_limit) q.cut = 0;      // (the level before it runs on the multi-launch kernels)
        if (q.cut && q.cut < q.n_spec && q.defer_root) q.defer_root = false;   // (a deferred root needs level 4 to exist)
    }
    return q;
}

// The history of an image shape's last level-loop search: into / out of the context's working fields.
void hint_load(az_ctx *c, int h, int w, int nlev)
{
    if (c->hint_h == h && c->hint_w == w && c->hint_nlev == nlev) return;
    for (auto &e : c->hints)
        if (e.h == h && e.w == w && e.nlev == nlev) {
            std::memcpy(c->hint_rows, e.rows, sizeof(e.rows)); std::memcpy(c->hint_P, e.P, sizeof(e.P));
            std::memcpy(c->hint_PZ, e.PZ, sizeof(e.PZ)); std::memcpy(c->hint_U, e.U, sizeof(e.U));
            std::memcpy(c->hint_SPN, e.SPN, sizeof(e.SPN));
            std::memcpy(c->hint_old, e.old, sizeof(e.old)); c->hint_n = e.n; c->hint_full_streak = e.full_streak;
            c->hint_h = h; c->hint_w = w; c->hint_nlev = nlev;
            e.use = ++c->hint_clock;
            return;
        }
    c->hint_h = -1; c->hint_w = -1; c->hint_nlev = 0;          // no search of this shape seen (yet)
    c->hint_n = 0; c->hint_full_streak = 0;
    std::memset(c->hint_rows, 0, sizeof(c->hint_rows));
}

void hint_store(az_ctx *c)
{
    if (c->hint_h < 0) return;
    az_ctx::ShapeHint *slot = nullptr;
    for (auto &e : c->hints) if (e.h == c->hint_h && e.w == c->hint_w && e.nlev == c->hint_nlev) slot = &e;
    if (!slot) {
        if (c->hints.size() >= 64) {
            size_t lru = 0;
            for (size_t i = 1; i < c->hints.size(); ++i) if (c->hints[i].use < c->hints[lru].use) lru = i;
            c->hints.erase(c->hints.begin() + (long)lru);
        }
        c->hints.emplace_back();
        slot = &c->hints.back();
        slot->h = c->hint_h; slot->w = c->hint_w; slot->nlev = c->hint_nlev;
    }
    std::memcpy(slot->rows, c->hint_rows, sizeof(slot->rows)); std::memcpy(slot->P, c->hint_P, sizeof(slot->P));
    std::memcpy(slot->PZ, c->hint_PZ, sizeof(slot->PZ)); std::memcpy(slot->U, c->hint_U, sizeof(slot->U));
    std::memcpy(slot->SPN, c->hint_SPN, sizeof(slot->SPN));
    std::memcpy(slot->old, c->hint_old, sizeof(slot->old)); slot->n = c->hint_n; slot->full_streak = c->hint_full_streak;
    slot->use = ++c->hint_clock;
}

// What the level-by-level form the context would pick for this shape (pair_plan on the same history) costs for ONE of the
// shape's recorded trees, in us.
double level_forms_cost(az_ctx *c, const HintView &v, int nlev, int n_spec, int specU, int pair_mask)
{
    double t = pass_us(c, specU) + PASS_OVERHEAD_US;
    for (int l = n_spec; l < nlev; ++l) {
        if (v.U[l] <= 0) {              // the tree had ended: the level's pass is enqueued all the same and finds no rows
            t += EMPTY_LEVEL_US;
            if ((pair_mask >> l) & 1) ++l;
            continue;
        }
        if ((pair_mask >> l) & 1) {
            t += pass_us(c, v.U[l] + pair_rows(v, l)) + PASS_OVERHEAD_US + LOOKUP_US;
            ++l;
        } else
            t += pass_us(c, v.U[l]) + PASS_OVERHEAD_US;
    }
    return t;
}

// ---- Tz <= 0: the tree is known before any score is (az_static.hip) -----------------------------------------------
// (params.reserved bits 0, 1, 2, 4 ask for one of the level-loop forms; bit 5 / AZ_STATIC_TREE=0 turn the plan off)
bool static_wanted(az_ctx *c, const az_params *p, bool tune)
{
    if (tune || !(p->Tz <= 0.0) || (p->reserved & (1 | 2 | 16 | 32)) || !c->env.static_tree) return false;
    for (const auto &hw : c->nostatic)
        if (hw.first == p->im_h && hw.second == p->im_w) return false;
    return true;
}

// In the level loop only the device knows a level's row count.  If the previous search on this context forwarded many
// rois at level l, the next one probably does too: its int6 is then sent to both GEMM kernels (rows_hint -1, see
// launch_head).  A wrong guess costs an idle launch, never a result.
int many_rows_expected(const az_ctx *c, int l)
{
    // (hint rows: rows of the PASS at that level, speculative rows included; the mean over the shape's recorded searches)
    if (l < 0 || l >= AZ_MAX_LEVELS || c->gemm12_min_rows == 0x7fffffff || c->hint_n <= 0) return 0;
    long sum = 0;
    for (int r = 0; r < c->hint_n; ++r) sum += hint_rec(c, r).rows[l];
    return sum >= (long)c->gemm12_dual_rows * c->hint_n ? -1 : 0;
}
