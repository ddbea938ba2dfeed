// az_search.h -- what the translation units of a search share (internal): az_plan.hip (which form a search takes),
// az_shape.hip (what is prepared per image shape), az_search.hip (enqueue / launch / fetch of one search) and the host
// side of az_batch.hip (a batch of images in lockstep).
#pragma once
#include "az_ctx.h"

// Which form of the search a call takes.
struct SearchPlan { int n_spec; bool fused, fused_lv, defer_root; int pair_mask; int lv_limit; int full; /* 0 / 1 tree rows / 2 closure */
                    int cut; /* > 0: nothing is enqueued from this level on (the tree is expected to end before it) */ };
struct HintView { const int *rows, *P, *PZ, *U, *SPN; };   // one record of a shape's history (az_plan.hip: hint_rec)
constexpr double PASS_OVERHEAD_US = 40.0, LOOKUP_US = 8.0;     // (PASS_OVERHEAD_US: the level's geometry kernel + boundaries)

// ---- az_plan.hip --------------------------------------------------------------------------------------------------------
double pass_us(const az_ctx *c, double rows);
int calibrate_passes(az_ctx *c);
HintView hint_rec(const az_ctx *c, int r);
void hint_load(az_ctx *c, int h, int w, int nlev);
void hint_store(az_ctx *c);
SearchPlan plan_search(az_ctx *c, const az_params *p, int nlev, bool tune);
double level_forms_cost(az_ctx *c, const HintView &v, int nlev, int n_spec, int specU, int pair_mask);
bool static_wanted(az_ctx *c, const az_params *p, bool tune);
int many_rows_expected(const az_ctx *c, int l);
// ---- az_shape.hip -------------------------------------------------------------------------------------------------------
int ensure_spec_cache(az_ctx *c, const az_params *p, const SearchPlan &q);
bool plan_is_for(const az_ctx::StaticPlan &k, const az_params *p, int nlev);
bool static_plan_matches(const az_ctx *c, const az_params *p, int nlev);
int ensure_static_plan(az_ctx *c, const az_params *p, int nlev);
int full_prepare(az_ctx *c, const az_params *p, int nlev, bool tune);
