// az_ctx.h -- the context behind the C ABI (include/aznet_hip.h) and the declarations of what its translation units share:
// az_ctx.hip (the shared host helpers), az_capi.hip (lifecycle, head, maps, lanes, public launch / fetch, measurement,
// exchange), az_plan.hip / az_shape.hip / az_search.hip / az_batch.hip (the forms of a search: cost model and planner,
// per-shape caches, launch sequence and collecting a result, lockstep batches; az_search.h), az_units.hip (unit entry points,
// tuner, recall, front-end), az_detect.hip (the detection head: loaders, one pass, the az_detect* entries), az_nms.hip (NMS).  Only what must be visible at the call site has a body here.
// Who owns what: az_res.h.  Every allocation, pinned block, event and stream below is held by an owner (DevList, Buf, Event,
// Stream, EventPool) that releases it when the context is deleted; the raw pointers beside them are views.
#pragma once
#include "az_dev.h"
#include "az_res.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <vector>

#define AZ_VERSION_STR "aznet_hip 0.1 (gfx950)"

struct AzEventRec { std::string name; int level; hipEvent_t a, b; int slot; /* >= 0: an in-kernel span (a, b unused) */ };

constexpr size_t RES_HDR = 1024;    // AzCounts, padded, at the head of the result block
static_assert(sizeof(AzCounts) <= RES_HDR, "AzCounts outgrew its slot");

// The environment switches (measurements and A/B tests only; none changes a result): read once per context by
// az_create (az_read_env, the library's one getenv site), lanes and batch slots take their owner's table.
struct AzEnv {
    bool graph = false;        // AZ_GRAPH=1: hipGraph replay (the default az_set_graphs starts from)
    bool trace = false;        // AZ_TRACE=1: announce and wait for every launch group (debugging; process-wide, Timed::trace)
    bool full_debug = false;   // AZ_FULL_DEBUG (set): says on stderr when the whole-tree pass is taken or repeated, what the head-pass calibration measured, and when a batch is not taken in lockstep
    bool pass_cal = true;      // AZ_PASS_CAL=0: built-in head-pass costs instead of the first-launch measurement
    int plan_cache = 64;       // AZ_PLAN_CACHE=<n>: shapes kept in the plan cache (64)
    int gemm12_min = 161;      // AZ_GEMM12_MIN=<rows>: row count from which host-known launches take k_fc_splitk12 (161; 0 = never, held as INT_MAX)
    bool static_tree = true;   // AZ_STATIC_TREE=0: level loop also for Tz <= 0
    int pair_spec = 1;         // AZ_PAIR_SPEC=0|2: pair speculation never / whenever possible (1: by the context's history)
    int full_spec = 1;         // AZ_FULL_SPEC=0|2|3: whole-tree speculation never / whenever possible / the closure whenever possible (1: by history)
    int two_stage = 1;         // AZ_TWO_STAGE=0|2|4: one-pass searches never staged / staged on two lanes as well / two stages, never three
    bool iterloc_sync = true;  // AZ_ITERLOC_SYNC=0: az_detect_iter reads no round's row count back (every round enqueued at max_rows rows, one wait)
};

inline AzEnv az_read_env()
{
    AzEnv v;
    auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
    v.graph = num("AZ_GRAPH", 0) != 0; v.trace = num("AZ_TRACE", 0) != 0; v.full_debug = getenv("AZ_FULL_DEBUG") != nullptr;
    v.pass_cal = num("AZ_PASS_CAL", 1) != 0; v.static_tree = num("AZ_STATIC_TREE", 1) != 0;
    if (num("AZ_PLAN_CACHE", 0) > 0) v.plan_cache = num("AZ_PLAN_CACHE", 0);
    if (getenv("AZ_GEMM12_MIN")) v.gemm12_min = num("AZ_GEMM12_MIN", 0) > 0 ? num("AZ_GEMM12_MIN", 0) : 0x7fffffff;
    v.pair_spec = num("AZ_PAIR_SPEC", 1); v.full_spec = num("AZ_FULL_SPEC", 1); v.two_stage = num("AZ_TWO_STAGE", 1);
    v.iterloc_sync = num("AZ_ITERLOC_SYNC", 1) != 0;
    return v;
}

// One InnerProduct layer of a head as its forward path reads it (fc_layer_forward): how it is stored and split.  Views, not
// owners: the buffers are in the head's DevList (fc_layer_load), so a lane takes a layer by copying the record.
struct FcLayer {
    int N = 0, K = 0;                   // outputs, inputs
    int S = 1;                          // K chunks of the full-rank GEMM
    int r = 0, SL = 0;                  // truncated SVD: rank (0: the layer at full rank) and the L stage's K chunks
    float *W = nullptr;                 // full rank: [N, K], tiled (azk_tile_weights)
    float *L = nullptr, *U = nullptr;   // rank r: L [r, K] tiled like W, U [N, r] row-major (az_lowrank.hip)
    float *b = nullptr, *zero = nullptr;   // bias [N]; [>= r] zeros, the bias that makes the L stage's azk_fc_reduce a plain slab sum
    unsigned short *Wp = nullptr;       // 16-bit-term modes: the weight planes (null: the layer stays on the fp32 GEMM)
    float w_scale = 0.f;                // ... and the power-of-two scale of their fp16 terms
    int lead() const { return r ? r : N; }      // rows of the [., K] matrix the first GEMM reads (W or L)
    size_t slab_elems(size_t rows) const { return (size_t)(r ? SL : S) * rows * lead(); }   // that GEMM's split-K slabs
};

struct az_ctx {
    int device = 0;
    AzEnv env;
    // (declared first, so destroyed last: the streams outlive every event and buffer used on them)
    Stream stream, stream2, stream3, comm_stream;
    std::string err;
    int maxR = 16384, maxCand = 16384 * AZ_NSUB, maxCh = 65536;
    bool head_loaded = false;
    AzHeadDims d{};
    // int6 on the 16-bit matrix cores (az_set_gemm_mode): 0 = off (fp32 MFMA everywhere), 2 = two fp16 terms of
    // x * 2^k / 3 MFMAs per product (~2^-21), 3 = three bf16 terms / 6 MFMAs (every fp32 value exactly)
    int gemm_parts = 0;
    unsigned short *pool5p = nullptr;
    float *gscale = nullptr;            // two-term (fp16) mode: {pool5 scale of this map, 1 / (sx * sw), scratch, scratch}
    float spatial_scale = 0.0625f;                 // test_fc.prototxt:22
    // weights (HBM).  int6 is an FcLayer (full rank: az_load_head; truncated SVD: az_load_head_lowrank); t6 [maxR][fc6.r], its
    // L stage's rows, belongs to the head buffer set: every lane has its own.  int7 (W7, b7, S7) is no FcLayer: its slab
    // sum lives in azk_tail, so it has no reduce launch of its own and does not go through fc_layer_forward
    FcLayer fc6;
    int S7 = 1;
    float *W7 = nullptr, *b7 = nullptr, *Wt = nullptr, *bt = nullptr;
    float *t6 = nullptr;
    // feature map
    const float *feat = nullptr;        // channel-last copy of the current map (what RoIPool reads)
    // [H][W][C] copies of NCHW maps, three of them used in turn (two until round 5): the map of a search that is still queued (and might have to
    // be run again in another form) survives the hand-over of the next image's map
    static constexpr int NFEAT = 3;      // (one per search a lane may have queued: AZ_QUEUE_MAX)
    static constexpr int AZ_QUEUE_MAX = 3;
    float *feat_owned[NFEAT] = {nullptr, nullptr, nullptr};
    int feat_turn = 0;
    unsigned feat_gen = 0;              // bumped when the copies are reallocated
    float *feat_stage = nullptr;        // NCHW staging for host uploads
    Buf feat_own[NFEAT + 1];            // (owners of feat_owned[] and feat_stage)
    size_t feat_owned_elems = 0;
    // image pyramid (az_pyramid.hip): S borrowed channel-last maps of one padded size and the device table RoIPool reads
    // them through (roi column 0 = level); pyr_now: a pyramid search / detection is being enqueued
    int pyr_S = 0, pyr_now = 0;
    const float **pyr_feats = nullptr;  // [AZ_PYRAMID_MAX] (device)
    int *pyr_hw = nullptr;              // [AZ_PYRAMID_MAX][2] (device)
    Buf pyr_own[2];
    AzPyrScales pyr_sc{};               // the scales of the pyramid search being enqueued
    // level-loop buffers (HBM)
    AzCounts *cnt = nullptr;
    double *B[2] = {nullptr, nullptr};
    float *rois = nullptr, *urois = nullptr;
    long long *key = nullptr, *ckey = nullptr;
    int *grp = nullptr, *index = nullptr, *inv = nullptr, *choff = nullptr, *bc_c = nullptr, *bc_z = nullptr;
    // inv_index of the ODD levels of a search (even levels and the unit entry points: `inv`): a level's fused geometry
    // kernel writes the next level's inv_index while its second workgroup may still be reading this level's
    int *inv_odd = nullptr;
    unsigned char *first = nullptr, *cflag = nullptr, *zflag = nullptr, *keep_u = nullptr;
    double *ubox = nullptr, *pred_u = nullptr, *Yall = nullptr, *Z = nullptr, *child = nullptr, *Yout = nullptr;
    float *pool5 = nullptr, *part = nullptr, *h6 = nullptr, *h7 = nullptr;
    float *zoom_u = nullptr, *score_u = nullptr, *delta_u = nullptr, *Sall = nullptr, *Sout = nullptr;
    int *sel_idx = nullptr, *rank_part = nullptr;
    // speculative levels 1-3: provenance of zoomed regions / children / regions, head outputs of the pass
    int *zr = nullptr, *csrc = nullptr, *choff_all = nullptr, *srcB[2] = {nullptr, nullptr};
    float *zoom_s = nullptr, *score_s = nullptr, *delta_s = nullptr;
    // the speculative pre-pass depends on the image shape only: its outputs are kept per shape (one entry)
    // (two entries: with the root's row in the pass [0] / deferred to level 4's pass [1] -- a context whose images
    //  alternate between trees that reach level 4 and trees that do not keeps both)
    float *spec_urois[2] = {nullptr, nullptr};
    double *specB1[2] = {nullptr, nullptr};
    int *spec_choff[2] = {nullptr, nullptr}, *spec_U[2] = {nullptr, nullptr};
    struct SpecCache { int h = -1, w = -1; double scale = 0, min_side = 0; int P1 = 0, CH = 0, U = 0; } spc[2];
    // the pre-pass writes into the scratch buffers; its result is kept per image shape in exact-size buffers (a dataset
    // mixes shapes: a shape seen before costs neither the pre-pass nor its host synchronisation) and spec_urois / specB1 /
    // spec_choff / spec_U[defer] POINT at the entry of the shape in use
    float *spec_scr_urois[2] = {nullptr, nullptr};
    double *spec_scr_B1[2] = {nullptr, nullptr};
    int *spec_scr_choff[2] = {nullptr, nullptr};
    struct SpecEntry { int h = -1, w = -1, defer = 0; double scale = 0, min_side = 0; int P1 = 0, CH = 0, U = 0;
                       float *urois = nullptr; double *B1 = nullptr; int *choff = nullptr, *Udev = nullptr; Buf own[4];
                       unsigned long long use = 0; };
    std::vector<SpecEntry> spec_store;
    unsigned long long spec_clock = 0;
    // Tz <= 0: the whole tree is a function of the image shape (az_static.hip); its rois / anchors / region -> row
    // map are kept per shape in exact-size HBM buffers (~100 B per roi: 70 KB for a 600x1000 image), least recently
    // used shapes are dropped beyond AZ_PLAN_CACHE entries; the per-level sizes stay on the host
    struct StaticPlan {
        int h = -1, w = -1, nlev = 0, batch = 0, Utot = 0, coop = 1;
        double scale = 0, min_side = 0, dedup = 0;
        int roff[AZ_MAX_LEVELS + 1] = {0}, U[AZ_MAX_LEVELS] = {0}, CH[AZ_MAX_LEVELS] = {0};
        float *urois = nullptr;
        double *ubox = nullptr;
        int *reg_u = nullptr, *cand_src = nullptr, *meta = nullptr;
        DevList own;                          // (what the five views above point into)
        unsigned long long last_use = 0;
        // whole-tree speculation (SearchPlan::full): window table over the pass's rows, the speculative rows' map, the
        // pass's rois.  Two row sets per shape:
        //   fs[0] "tree":    the plan's non-root rows (the unique rois of the FULL tree) ++ extra rows (speculative rows
        //                    whose window the plan lacks) ++ the root.  Serves a search whose tree is the full tree; a
        //                    pruned tree may keep another _sift_dup survivor (same 10-px hash, other window) -> err bit 256.
        //   fs[1] "closure": one row per distinct RoIPool window among ALL regions any pruning can produce -- level l+1 =
        //                    every child of every region of level l, no _sift_dup (whichever duplicate survives is among
        //                    them) -- ++ the root.  Serves every Tz; never misses.
        struct FullSet {
            unsigned long long *htab = nullptr; unsigned hT = 0;
            int *spec_map = nullptr, *full_meta = nullptr;
            float *full_urois = nullptr; double *full_ubox = nullptr;
            DevList own;
            int Ufull = 0, full_state = 0;    // 0: not built, 1: ready, -1: cannot be used for this shape
        } fs[2];
    };
    std::vector<StaticPlan *> plans;
    StaticPlan *plan = nullptr;               // the plan of the search being launched / in flight
    unsigned long long plan_clock = 0;
    int plan_cache_max = 64;
    unsigned *key_u = nullptr;                // selection keys of the decoded boxes (tail kernel), [row][11]
    std::vector<std::pair<int, int>> nostatic; // image shapes whose trees outgrew the plan buffers (a few; oldest dropped)
    int last_static = 0;
    int hint_rows[AZ_MAX_LEVELS] = {0};       // rows of the head pass launched at each level in the last fetched level-loop search (kernel choice)
    // the last fetched level-loop search, per level: regions, zoomed regions, unique rois, pair-speculation rows (-1: none)
    int hint_P[AZ_MAX_LEVELS] = {0}, hint_PZ[AZ_MAX_LEVELS] = {0}, hint_U[AZ_MAX_LEVELS] = {0}, hint_SPN[AZ_MAX_LEVELS] = {0};
    int hint_h = -1, hint_w = -1, hint_nlev = 0;
    // ... kept per image shape (a dataset mixes a few dozen shapes: each keeps the history of ITS last search; the fields
    // above are the entry of the shape being launched / last fetched)
    // (round 5) A dataset is a stream of DIFFERENT images: the tree of the previous image is one sample of what the next one
    // looks like, not a prediction of it.  Each shape keeps its last HINT_K level-loop searches (newest = the hint_* fields
    // above, then hint_old[0..]); the choices that cost little when wrong and gain little when right are made on the
    // EXPECTED cost over those (pair_plan, full_prepare), the ones that cost a second search when wrong need a streak
    // (tree rows of the whole-tree pass: the last two searches of the shape both walked the full tree).
    static constexpr int HINT_K = 4;
    struct HintRec { int rows[AZ_MAX_LEVELS], P[AZ_MAX_LEVELS], PZ[AZ_MAX_LEVELS], U[AZ_MAX_LEVELS], SPN[AZ_MAX_LEVELS]; };
    HintRec hint_old[HINT_K - 1];
    int hint_n = 0;                           // records held for the shape in the working fields (0: none, 1: hint_* only, ...)
    int hint_full_streak = 0;                 // consecutive searches of the shape, up to the last, that walked the FULL tree
    struct ShapeHint { int h, w, nlev; int rows[AZ_MAX_LEVELS], P[AZ_MAX_LEVELS], PZ[AZ_MAX_LEVELS], U[AZ_MAX_LEVELS], SPN[AZ_MAX_LEVELS];
                       HintRec old[HINT_K - 1]; int n, full_streak;
                       unsigned long long use; };
    std::vector<ShapeHint> hints;
    unsigned long long hint_clock = 0;
    std::vector<std::pair<int, int>> nopair;  // image shapes whose pair-speculation rows outgrew the tables
    int full_now = 0;                         // the search being launched takes the whole-tree pass: 1 = tree rows, 2 = closure
    int last_full = 0;
    // the closure's rows of the shape last looked at by the cost model (0: not built): what the one pass would cost
    int n_rerun_total = 0;                    // searches this context has had to run twice (any reason) since it was created
    // Two lanes (az_set_lanes): a second stream with its own per-search buffers (`twin`, an az_ctx of its own that shares
    // this context's head weights) takes every other queued search, so that consecutive images overlap on the GPU -- one
    // image's single-workgroup geometry kernels and its small head kernels run beside the other image's GEMM.
    // Two stages (round 5).  A search whose ONE head pass does not depend on its own geometry -- the whole-tree / closure
    // pass, the one-pass plan: its rows are a function of the image shape -- is enqueued on two streams: stage 1 = RoIPool +
    // int6 + slab sum on `stream`, stage 2 = int7 + heads + every geometry kernel + the selection + the result copy on
    // `stream2`, behind an event.  The next search's stage 1 then does not queue behind this one's single-workgroup geometry
    // kernels (which cannot get a CU while a lane's int6 holds them all), and this one's MFMA-bound int7 may run beside the
    // next int6's HBM-bound neighbours (the other image's slab sum and RoIPool) instead of in a slot of its own.
    //   h6 (slab sum -> int7) is the one buffer both stages touch: ev_h6 orders int7 behind the slab sum, ev_i7 the NEXT
    //   slab sum behind this int7; int7's slabs live in `part7`, not in `part`.
    //   ev_s2 = everything enqueued on stream2 so far: whatever is not stage 1 of another two-stage search (a search in
    //   another form, a plan builder, a unit entry point) makes `stream` wait for it first (join_s2).
    //   The whole-tree / closure form goes one step further (three stages): its geometry kernels + selection + result copy
    //   run on a THIRD stream behind the heads (ev_tail).  They are single-workgroup kernels that get a CU only between two
    //   int6 launches; on the second stream they held the NEXT search's int7 back for ~70 us.  The head outputs they read
    //   (zoom_s / score_s / delta_s) exist twice, used in turn (out_par); ev_geo[p] = the geometry that read set p is done.
    Event ev_tail, ev_s3, ev_geo[2];
    bool s3_live = false, g_live[2] = {false, false};
    int out_par = 0, three_now = 0;
    float *zoom_s2 = nullptr, *score_s2 = nullptr, *delta_s2 = nullptr;
    hipStream_t gs = nullptr;                 // while a search is being enqueued: where the kernels behind its head pass go (nullptr: `stream`)
    hipStream_t ts = nullptr;                 // ... and where profiling events are recorded (nullptr: `stream`)
    hipStream_t last_s = nullptr;             // the stream the search launched last ends on
    Event ev_h6, ev_i7, ev_s2;
    bool i7_live = false, s2_live = false;
    int split_now = 0, async_err = 0;
    bool no_stage_streams = false;            // this device / runtime did not give the extra streams: every search in one stage
    float *part7 = nullptr;                   // int7's split-K slabs [S7][maxR][n7]
    // Staged searches write int7's slabs into THREE buffers in turn (ring[0] = part7): the heads of search i - 3 -- the last
    // reader of the buffer search i writes -- ran before that search was fetched, and a lane never holds more than
    // AZ_QUEUE_MAX = 3 unfetched searches, so int7 needs no event wait for the previous search's heads any more (each wait on
    // the main stream is a ~6 us bubble between two chip-wide kernels).  No room for the two extra buffers: one buffer + the wait.
    static_assert(AZ_QUEUE_MAX <= 3, "the int7 slab ring has one buffer per search a lane may hold unfetched");
    float *part7_ring[3] = {nullptr, nullptr, nullptr};
    int part7_turn = 0;
    bool part7_no_room = false, part7_wait = false;   // no memory for the two extra buffers; a launch failed after taking one: the next staged search waits for ev_s2
    az_ctx *twin = nullptr, *owner = nullptr;
    // A batch of images searched in lockstep (az_batch_launch; az_batch.hip: batch_launch_impl).  Held by the
    // lane whose head buffers the batch's passes run in (the context, or its twin for every other batch when two lanes are
    // on); every image of the batch has a SLOT: an az_ctx of its own for the tree (regions, counters, candidates, result
    // slots, history), created without head buffers -- it gets them if one of its searches ever has to be run again alone.
    struct Batch {
        std::vector<az_ctx *> slots;
        int *off = nullptr;                   // device: AzGatherArgs::off_out of the pass being enqueued, [AZ_BATCH_MAX + 2]
        float *rois_cat = nullptr;            // the pass's rois / anchors / map table
        double *ubox_cat = nullptr;
        const float **feats = nullptr;
        int *feat_hw = nullptr, *row_hw = nullptr;   // every image's map size [AZ_BATCH_MAX][2]; every row's image size [maxR][2]
        unsigned char *args_dev = nullptr, *args_host = nullptr;   // the geometry kernels' arguments, one block per image and launch
        size_t args_cap = 0;
        // (owners: off .. row_hw, the args pair, the result pair)
        Buf own[6], args_own[2] = {Buf::DEVICE, Buf::PINNED}, res_own[2] = {Buf::DEVICE, Buf::PINNED};
        // the images' result blocks (counters + selected boxes and scores) lie side by side, on the device and in pinned host
        // memory: ONE device-to-host copy per batch (eight copies of 12 KB cost 75 us of stream time, one of 95 KB ~10)
        unsigned char *res_dev = nullptr, *res_host = nullptr;
        int n_live = 0, next_fetch = 0;       // images of the batch in flight; the one az_batch_fetch returns next
        bool lockstep = false;                // false: the batch's images were launched one after the other on their slots
        int rows_hint[AZ_MAX_LEVELS] = {0};   // rows of the passes of the last fetched batch (which int6 kernel takes a level)
        int rows_acc[AZ_MAX_LEVELS] = {0};
        int hint_n = 0;                       // images of the batch rows_hint was taken from (0: none yet)
    } bsets[2];                               // two sets per lane, used in turn: the host enqueues a lane's next batch while its
                                              // current one runs (same stream: the two do not interleave on the GPU)
    int bset_turn = 0;
    std::deque<int> batch_order;              // (owner) lane | set << 1 of the batches in flight, oldest first
    int batch_next = 0;
    bool head_bufs = true;                    // false: a batch slot that has not needed pool5 / slabs / h6 / h7 yet
    // A batch slot that searches on its own (its batch's pass overflowed, its shape is not taken in lockstep) does not get a
    // head set of its own -- at max_regions 16384 and the VGG16 dims that is ~8.5 GB, times 32 slots, times two sets per
    // lane -- but takes the OWNER's one spare set in turn: `ev` (recorded behind each such search) orders the next user's
    // stream behind the previous one.  The searches were chip-wide one after the other anyway.
    struct HeadSet {                          // (views; alloc_head_set, az_capi.hip)
        float *pool5 = nullptr, *part = nullptr, *h6 = nullptr, *h7 = nullptr, *part7 = nullptr, *gscale = nullptr, *t6 = nullptr;
        unsigned short *pool5p = nullptr;
    };
    struct SpareHead : HeadSet {
        bool ready = false, ev_live = false;     // (the buffers are in the owner's `allocs`)
        Event ev;
    } spare;                                  // (owner)
    bool head_shared = false;                 // (a batch slot) pool5 / part / h6 / h7 / part7 are the owner's spare set
    Batch *batch_set = nullptr;               // (a batch slot) the batch set it belongs to
    // (a batch slot) its counters / result block and its first host result slot are views into the lane's arenas
    // (Batch::res_dev / res_host); the slot's own blocks stay with their owners and are freed with it
    int lanes = 1, lane_next = 0, last_fetch_lane = 0;
    std::deque<int> lane_order;               // lanes of the searches launched through the public entry points, oldest first
    Event ev_hand;                            // (in a twin) orders the lane behind the owner's stream when it reads the owner's map
    // (in a twin) recorded behind the lane's private copy of an owner-held map: the owner's stream waits for it before it
    // writes its channel-last copies again (the lane may still be busy with an earlier search when the owner is handed
    // the map after next)
    Event ev_copy;
    bool ev_copy_live = false;
    void *comm = nullptr;                     // ncclComm_t of az_rccl_init
    int comm_ranks = 0, comm_rank = 0;
    // the collective runs on a stream of its own, behind events of the lanes: in a lane's stream it would hold that lane's
    // next search back until the collective's kernel finds free CUs, i.e. until the OTHER lane's GEMM is done
    Event comm_ev[2];
    // cost of one head pass (RoIPool + int6 + reduce + int7 + heads) at a few row counts, measured on THIS device with HIP
    // events the first time a search is launched (calibrate_passes): what the choice between the search forms goes by
    struct PassCal { int state = 0; int n = 0; int rows[6] = {0}; double us[6] = {0}; bool pinned = false; } cal;   // state 0: not yet, 1: measured, -1: off; pinned: the caller's table (az_set_pass_costs)
    double *pred_w = nullptr; float *score_w = nullptr, *zoom_w = nullptr; unsigned char *keep_w = nullptr; unsigned *key_w = nullptr;   // second *_v set
    int last_pair_mask = 0;                   // levels whose head pass carried pair-speculation rows (search in flight / last)
    // pair speculation: all-children offsets / child -> row of the level whose pass carries the rows; looked-up outputs
    int *choff_pair = nullptr, *crow = nullptr;
    double *pred_v = nullptr;
    float *score_v = nullptr, *zoom_v = nullptr;
    unsigned char *keep_v = nullptr;
    unsigned *key_v = nullptr;
    int gemm12_min_rows = 161;                // rows from which a host-known launch takes az_head12.hip (AzEnv::gemm12_min;
                                              // measured crossover with k_fc_splitk: 160 rows)
    int gemm12_dual_rows = 161;               // ... and from which a launch whose row count only the device knows takes it, going by the previous search
    // Fast R-CNN head on the shared map (az_load_det_head)
    bool det_loaded = false;
    int det_ncls = 0;
    DevList allocs_det;
    // fc6 / fc7 (full rank: az_load_det_head; either or both as a truncated SVD: az_load_det_head_lowrank) and the tail.
    // The L stages' output rows dlr_t [maxR][max r] and their zero bias dlr_zero [max r] serve both layers (both records'
    // `zero` point at dlr_zero).  16-bit-term modes: det_fc6.Wp set = fc6 on the same kernel as int6, with -- two fp16
    // terms -- its own {pool5 scale, 1 / (sx * sw)} pair in dgscale
    FcLayer det_fc6, det_fc7;
    float *dWt = nullptr, *dbt = nullptr, *dlr_t = nullptr, *dlr_zero = nullptr, *dgscale = nullptr;
    float *dh6 = nullptr, *dh7 = nullptr, *dpart = nullptr, *dprob_u = nullptr, *ddelta_u = nullptr, *dprob = nullptr;
    double *dpred_u = nullptr, *dpred = nullptr;
    // the skip-connection front of the detection head (az_skip.hip: az_load_skip_front): up to AZ_SKIP_MAX_SRC borrowed
    // channel-last maps, each pooled 7x7 and normalised across its channels, concatenated [rows][sumC] in `cat`
    // (AZ_SKIP_CHUNK rois at a time) and folded to the head's C channels by a 1x1 convolution straight into pool5
    struct SkipFront {
        bool loaded = false, maps_set = false;
        int n = 0, C[AZ_SKIP_MAX_SRC] = {0, 0, 0}, sumC = 0, Cout = 0;
        float scale[AZ_SKIP_MAX_SRC] = {0.f, 0.f, 0.f};
        double gain = 1000.0, eps = 1e-10;       // scale5 (test_fc.prototxt of the skip model); the GRN layers' eps
        float *Wp = nullptr, *bp = nullptr, *cat = nullptr;
        DevList own;
        const float *maps[AZ_SKIP_MAX_SRC] = {nullptr, nullptr, nullptr};
        int H[AZ_SKIP_MAX_SRC] = {0, 0, 0}, W[AZ_SKIP_MAX_SRC] = {0, 0, 0};
    } skip;
    // az_detect_batch: one pass's AzDetSeg + boxes (pinned staging and its device copy), per-row image sizes
    unsigned char *dseg_host = nullptr, *dseg_dev = nullptr;
    Buf dseg_own{Buf::PINNED};
    int *drow_hw = nullptr;
    // nms scratch (grown on demand)
    int nms_cap = 0;
    float *nms_dets = nullptr, *nms_sdets = nullptr;
    int *nms_order = nullptr;
    unsigned long long *nms_mask = nullptr;
    int *nms_rank = nullptr;            // [nms_cap] rank scratch of k_nms_rank_count: zero between calls
    long long *nms_keep = nullptr;
    Buf nms_own[6];                     // (dets, sdets, order, mask, rank, keep: grown together, nms_cap boxes)
    // the host-mapped result blocks of az_nms's small case, of its general case (keep list + count) and of az_nms_batched
    Buf h_nms_own{Buf::MAPPED}, h_nmsg_own{Buf::MAPPED}, h_nmsb_own{Buf::MAPPED}, nms_done_own;
    int *nms_done = nullptr; int nms_seq = 0;    // az_nms_batched's count of finished workgroups (device) and its launch number
    unsigned nms_tag = 0;               // sequence number carried by every word an NMS kernel writes to host-mapped memory
    // Soft-NMS / box voting scratch (az_postproc.hip; grown on demand): pp_box_cap boxes, pp_grp_cap groups
    int pp_box_cap = 0, pp_grp_cap = 0;
    Buf pp_box_own[4];                  // (dets [.][5] f32, keep i64, scores f32, voted boxes [.][4] f32: grown together)
    Buf pp_grp_own[3];                  // (offsets [. + 1], the launch's group list, counts: grown together)
    // tuner (az_eval.hip): anchor history of the last search, score pool over an image set
    double *hisB = nullptr;
    float *hisZ = nullptr;
    int capHis = 0;
    float *pool = nullptr, *pool_tmp = nullptr;
    unsigned long long *pool_n = nullptr, *pool_hist = nullptr;      // [2], [256]
    long long pool_cap = 0, pool_alloc = 0;      // floats the open pool takes (az_tune_begin's capacity); floats allocated
    bool pool_bad = false;              // a tuner search that appended to the pool failed: refused until the next az_tune_begin
    Buf his_own[2], pool_own[4];        // (hisB, hisZ; pool, pool_tmp, pool_n, pool_hist)
    // grow-on-demand scratch of the evaluation / front-end entry points
    // (slots 0-7: whatever the entry point wants; 8, 9, 10: the arenas of az_voc_eval, az_coco_eval, az_diag_eval)
    Buf scratch[11];
    // front-end on a caller's stream (az_image_blob_dev_on): two pinned host slots and two device slots for the uint8 image,
    // used in turn; a slot's event says its last upload + kernel are done
    // upload slots of az_image_blob_dev_on (pinned host + device staging + "slot free" event).  Two to start with; a slot
    // whose previous upload is still queued on the GPU (a lockstep batch's uploads wait behind the previous batch's search)
    // makes the ring GROW, up to IO_SLOTS_MAX, instead of making the host wait.
    static constexpr int IO_SLOTS_MAX = 40;
    struct IoSlot { Buf host{Buf::PINNED}, dev; Event ev; };
    std::vector<IoSlot> io;
    size_t io_cap = 0;
    int io_turn = 0;
    // pinned host staging
    AzCounts *h_cnt = nullptr;
    double *h_Y = nullptr;
    float *h_S = nullptr;
    int h_cap = 0;
    Buf h_cnt_own{Buf::PINNED}, h_own[2] = {Buf::PINNED, Buf::PINNED};      // (h_cnt; h_Y, h_S: grown together, h_cap rows)
    // Searches launched and not yet fetched, oldest first (at most two: the host may enqueue the next image's launch
    // sequence while the GPU still works on the current one -- same stream, so the searches never overlap on the GPU).
    // With a fixed proposal count the result block's device-to-host copy is enqueued right behind the search's kernels,
    // into a pinned slot of its own; az_propose_fetch then only waits for that copy's event.
    struct PendingSearch {
        az_params p{};
        int nlev = 0, is_static = 0, defer = 0, pair_mask = 0, npass = 0, full = 0, reruns = 0;
        int cut = 0;                        // > 0: the search was enqueued up to (not including) this level
        int pyr = 0;                        // a pyramid search (az_propose_pyramid): kept out of the shape's history
        int pass_src[AZ_MAX_LEVELS + 2] = {0};
        int pass_lv[AZ_MAX_LEVELS + 2] = {0};   // the `level` each head pass was launched for (-1: speculative / whole-tree / one-pass)
        void *stage_dst = nullptr;          // az_propose_stage_result_dev target
        size_t stage_cap = 0;
        int slot = 0;
        hipStream_t last_s = nullptr;       // the stream the search's last kernels and its result copy are on
        bool copied = false;                // result block already on its way to h_res[slot]
        bool pooled = false;                // a tuner search that appended its anchors' scores to the score pool
        const float *feat = nullptr;        // the map the search reads (a rerun in another form needs it again)
        int fH = 0, fW = 0;
        unsigned feat_gen = 0;
        bool feat_is_copy = false;          // `feat` is one of the ctx's own channel-last copies (gone if they are reallocated)
        int batch = 0;                      // 1: an image of a lockstep batch (az_batch_launch)
    };
    std::deque<PendingSearch> pend;
    unsigned char *h_res[3] = {nullptr, nullptr, nullptr};
    Buf h_res_own[3] = {Buf::PINNED, Buf::PINNED, Buf::PINNED};
    Event ev_res[3];
    bool slot_busy[3] = {false, false, false};
    // parameters of the last FETCHED search
    az_params last{};
    int nofuse_h = -1, nofuse_w = -1;   // image shape for which the fused levels 1-3 overflowed
    int nofuse_lv_h = -1, nofuse_lv_w = -1;   // ... for which the first level after the speculative ones outgrew the fused level kernel
    // image shapes whose level `limit` (> the first fused level) outgrew the fused level kernel: the levels before it stay
    // on it, the step from level `limit` on runs on the multi-launch kernels
    struct LvLimit { int h, w, limit; };
    std::vector<LvLimit> lv_limits;
    struct GraphEntry { hipGraphExec_t exec; int npass; int pass_src[AZ_MAX_LEVELS + 2]; int pass_lv[AZ_MAX_LEVELS + 2]; };
    std::map<std::string, GraphEntry> graphs;        // captured launch sequences (az_set_graphs)
    int use_graphs = 0;                              // az_set_graphs (az_create: AzEnv::graph)
    int last_defer = 0;
    // Early end: a tree whose previous search of the shape had no regions from some level on is enqueued only up to that
    // level (the passes and geometry kernels of an empty level cost ~35 us each, a fifth of a sparse search); the last
    // geometry kernel checks -- regions after all set err bit 1024 and az_propose_fetch runs the search again in full
    // (params.reserved bit 12: never).  A miss costs more than a hit saves (a second search against two
    // empty levels), so the cut is taken only when the context's last FOUR level-loop searches all ended at or before the
    // level in question: early_hist holds the first empty level of the last eight (4 bits each, 15 = none).
    int last_cut = 0;
    unsigned early_hist = 0xFFFFFFFFu;
    int n_hist = 0;                     // level-loop searches this context has recorded in early_hist (saturating)
    // head passes of the search being enqueued / last launched: where each one's row count lives
    // (>= 0: int index into AzCounts; < 0: -(rows + 1), a count the host knows)
    int npass = 0;
    int pass_src[AZ_MAX_LEVELS + 2] = {0};
    int pass_lv[AZ_MAX_LEVELS + 2] = {0};
    int his_n = 0;                      // rows of the anchor history of the last fetched tuner search still in hisB / hisZ
                                        // (-1: a later tuner search is overwriting them, or the search failed)
    int cand_n = -1;                    // candidates of the last fetched search still in Yall/Sall (-1: overwritten)
    // profiling
    int profiling = 0;
    int event_errors = 0;              // hipEvent* calls that failed while profiling
    std::vector<AzEventRec> events;
    // profiling bit 3: the fc GEMM launches time THEMSELVES (AzSpan: first workgroup in, last workgroup out on the 100 MHz
    // clock) into slots of this ring -- exact also when another lane's kernels delay the launch, and free of the ~7 us of
    // stream time an event pair costs
    unsigned long long *span_ring = nullptr;
    Buf span_own;
    int span_next = 0;
    static constexpr int SPAN_SLOTS = 32768;
    EventPool event_pool;              // recycled events
    DevList allocs;                    // head-sized buffers (az_load_head)
    DevList allocs_geom;               // geometry buffers (first use)
    std::vector<az_solver *> solvers;  // trainers created on this context (az_solver.hip), freed with it
    std::vector<az_det_solver *> det_solvers;  // the detection net's trainers (az_det_solver.hip), freed with it
    bool geom_ready = false;
};

inline int fail(az_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(c, call)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail((c), AZ_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// One allocation of n elements (+ the list's slack) into `list`, a view of it in *p; the context's error set on failure.
template <typename T>
int dalloc(az_ctx *c, DevList &list, T **p, size_t n)
{
    const hipError_t e = list.alloc(p, n);
    if (e == hipSuccess) return AZ_OK;
    return fail(c, AZ_ERR_HIP, (&list == &c->allocs_det ? "hipMalloc: " : alloc_what(n * sizeof(T)) + ": ") +
                                   hipGetErrorString(e));
}
// ... member `p` of the context `c`, from inside a function that has `rc` and names the list it fills `list`
#define AZ_A(p, n) if ((rc = dalloc(c, list, &c->p, (n))) != AZ_OK) return rc

// Profiling modes (az_set_profiling): bit 0 = time the GEMM launches only, bit 1 = time every
// launch group, bit 2 = keep events across az_propose calls (read them once at the end).
struct Timed {
    az_ctx *c; bool on; hipEvent_t a{}, b{}; const char *name; int level;
    // (events are recycled through c->event_pool: creating one costs about as much as recording it)
    // AZ_TRACE=1 (debugging): every launch group is announced on stderr and waited for, so a faulting kernel is the one
    // named last
    static bool trace() { static const bool t = az_read_env().trace; return t; }
    Timed(az_ctx *c_, const char *n, int l, int cls = 2) : c(c_), name(n), level(l)
    {
        if (trace()) { fprintf(stderr, "az[%p]: %s L%d ...", (void *)c_, n, l); fflush(stderr); }
        on = (c_->profiling & 2) || ((c_->profiling & 1) && cls == 1);
        if (!on) return;
        // a failed event call drops this measurement (and is reported by az_last_kernel_times), never the search
        if (!c->event_pool.grab(&a)) { on = false; ++c->event_errors; return; }
        if (!c->event_pool.grab(&b)) { c->event_pool.put(a); on = false; ++c->event_errors; return; }
        if (hipEventRecord(a, c->ts ? c->ts : c->stream) != hipSuccess) { c->event_pool.put(a); c->event_pool.put(b); on = false; ++c->event_errors; }
    }
    ~Timed()
    {
        if (trace()) { const hipError_t e = hipStreamSynchronize(c->ts ? c->ts : c->stream); fprintf(stderr, " %s\n", e == hipSuccess ? "ok" : hipGetErrorString(e)); }
        if (!on) return;
        if (hipEventRecord(b, c->ts ? c->ts : c->stream) != hipSuccess) { c->event_pool.put(a); c->event_pool.put(b); ++c->event_errors; return; }
        c->events.push_back({name, level, a, b, -1});
    }
};

// ---- az_ctx.hip ---------------------------------------------------------------------------------------------------------
int ensure_geom(az_ctx *c);               // the buffers that depend only on the context's limits, at first use
void clear_events(az_ctx *c);             // the profiling records dropped, their events back in the pool
int num_levels(int h, int w, double min_side);      // K of lib/detect/test.py:365-368
int ensure_host(az_ctx *c, int cap);      // the pinned staging h_Y / h_S grown to `cap` rows
int set_count(az_ctx *c, int *dptr, int v);         // one device int set on the context's stream
void prep_scale(az_ctx *c);               // two-term (fp16) mode: the scale of this map's pool5 terms, once per search
// one fp32 fc layer's split-K GEMM on the many-row kernel (a layer that fits it, `many_rows`, the kernel not disabled) or not
void fc_gemm_fp32(const az_ctx *c, hipStream_t s, const float *x, int ldx, const float *W, const int *Mptr, int N, int K, int S,
                  float *part, bool many_rows, unsigned long long *ts = nullptr);
// the power of two that brings max |w| of n weights into [2^14, 2^15): the scale of the two-term mode's fp16 weight terms
float fc_weight_scale(const float *w, size_t n);
// One fc layer `f` (N, K, S, r, SL set by the caller) loaded, in two steps: a head's loader allocates its layers first and its
// pass buffers, one of which stages the upload, behind them (the order of a head's allocations shows in the time of a
// one-image az_detect_batch of the full-size head: 0.698 -> 0.710 ms with the weights allocated last, MI355X).
// fc_layer_alloc: W, or L and U of a truncated SVD, the bias and `parts` 16-bit weight planes (0: none), into `list`.
// fc_layer_load: the [f.lead(), K] matrix -- W, or `L`, whose U factor `W` then is -- uploaded (permC > 0: through `stage`, its
// Caffe-order columns bin-permuted for permC channels) into the row-major temporary `tmp`, split into the weight planes
// (f.Wp set: c->gemm_parts of them) and tiled; c->stream waited for; U (row-major as it is) and the bias copied.
int fc_layer_alloc(az_ctx *c, DevList &list, FcLayer &f, int parts);
int fc_layer_load(az_ctx *c, FcLayer &f, const float *L, const float *W, const float *b, int permC, float *stage, float *tmp);
// the buffers of one pass through a layer: x [*Mptr][K] (xp: its 16-bit planes, xp_stride elements each, with the two-term
// mode's scale block gscale), the split-K slabs, the L stage's rows t [maxR][r], y [*Mptr][N]
struct FcWork { const float *x; const unsigned short *xp; size_t xp_stride; float *part, *t, *y; const float *gscale; };
struct FcNames { const char *gemm, *reduce, *L, *L_reduce, *U; };      // profiling labels of the launches
// y = relu(x . W^T + b) on stream s, one of three ways.  16-bit-term mode (c->gemm_parts and f.Wp): azk_fc_gemm_terms + the
// slab sum with bias and ReLU.  fp32 at full rank: fc_gemm_fp32 (ts: its self-timing span, no event pair then) + the same
// slab sum.  Truncated SVD (f.r): the L stage on fc_gemm_fp32 (f.SL chunks), the linear slab sum into w.t (f.zero),
// then the U stage with bias and ReLU in one launch (az_lowrank.hip).  timed = false: no launch is recorded (a batch's pass)
void fc_layer_forward(az_ctx *c, hipStream_t s, const FcLayer &f, const FcWork &w, const int *Mptr, bool many_rows,
                      const FcNames &names, int level, unsigned long long *ts = nullptr, bool timed = true);
// one head pass; rows_hint: the row count where the host knows it, -1: many rows at this level in the last search
void launch_head(az_ctx *c, const int *Uptr, int level, int im_h, int im_w, double eps, float *zoom, float *score,
                 float *delta, double min_side = 0.0, bool keep_flags = false, int coop_tail = 0,
                 const float *urois = nullptr, const double *ubox = nullptr, int rows_hint = 0, bool keys = false);
int scratch_grow(az_ctx *c, int i, size_t bytes);   // scratch slot i of the evaluation entry points, at least `bytes`
void join_s2(az_ctx *c);                  // `stream` behind everything enqueued on the second and third streams
int check_geom(az_ctx *c);                // what a geometry entry point starts with: join_s2 + ensure_geom
int check_ready(az_ctx *c, bool need_feat, bool join = true);     // ... a head entry point: the head loaded (a map set)
// ---- az_units.hip (shared with az_detect.hip) ---------------------------------------------------------------------------
// the prologue of the entries that take P boxes: counters cleared, the boxes in B[0], P[0] = P
int upload_boxes(az_ctx *c, const double *boxes, int P);
// ... of those that take R rois [R][5]: checked ("bad rois" / "too many rois"), counters cleared, the rois in urois, ubox zeroed, U[0] = R
int stage_rois(az_ctx *c, const float *rois, int R);
// ---- az_search.hip ------------------------------------------------------------------------------------------------------
// one search enqueued on THIS context's stream / its result collected (idx: position in c->pend) / its record staged
int launch_impl(az_ctx *c, const az_params *p);
int fetch_entry(az_ctx *c, size_t idx, double *boxes_out, float *scores_out, int cap, int *n_out, az_stats *st);
int stage_impl(az_ctx *c, void *dst_dev, size_t cap_bytes);
// ---- az_pyramid.hip ------------------------------------------------------------------------------------------------------
// the scales of a pyramid entry checked (S in [1, AZ_PYRAMID_MAX], every scale positive and finite, fp32 GEMM mode) and
// packed; the context's error set on failure (`who`: the entry's name)
int pyramid_args(az_ctx *c, const double *scales, int S, AzPyrScales *sc, const char *who);
// ---- az_batch.hip --------------------------------------------------------------------------------------------------------
// n images (one shape or several, the same number of levels) in lockstep on lane L (whose head buffers the passes use), image b
// on slots[b] with parameters params[b] and map maps[b] of Hs[b] x Ws[b] cells;
// AZ_ERR_STATE + *not_taken = 1: this shape / these settings do not take the lockstep form (nothing enqueued)
int batch_launch_impl(az_ctx *L, az_ctx::Batch &B, int n, az_ctx **slots, const az_params *params /* [n] */, const float *const *maps,
                      const int *Hs, const int *Ws, int *not_taken);
// ---- az_voc.hip (shared with az_coco.hip) ------------------------------------------------------------------------------
// Stable LSD radix ranking of D detections by (-score, input order), segment s = class * n_images + image owning
// [det_off[s], det_off[s+1]) (device arrays): *by_seg lists every segment's detections in rank order, *by_class every
// class's.  Scratch: key [D], seg [D], perm[4] [D] each, hist [hist_n], sums [sums_n] (rank_scratch_sizes); D > 0.
struct RankScratch {
    unsigned long long *key;
    unsigned *seg, *perm[4], *hist, *sums;
};
void rank_scratch_sizes(int D, size_t *hist_n, size_t *sums_n);
void rank_by_score(hipStream_t s, int D, long long S, int n_images, int n_classes, const double *score, const int *det_off,
                   const RankScratch &r, const unsigned **by_seg, const unsigned **by_class);
// ---- az_solver.hip -------------------------------------------------------------------------------------------------------
void az_solver_free_all(az_ctx *c);       // az_destroy: the trainers still alive
// ---- az_det_solver.hip ---------------------------------------------------------------------------------------------------
void az_det_solver_free_all(az_ctx *c);
// ---- az_skip.hip --------------------------------------------------------------------------------------------------------
// what every skip entry refuses before it enqueues anything (`who`: the entry's name); need_maps: the maps must be set
int skip_check(az_ctx *c, const char *who, bool need_maps);
// what a front's description must satisfy (sources, channel counts, scales, gain, eps), for the inference front, the trainer's
// and the unit entry alike; *sumC_out: the channels in all
int skip_front_check(az_ctx *c, const std::string &who, int n_src, const int *Cs, const float *scales, double gain, double eps,
                     long long *sumC_out);
// the front on the rois in c->urois (row count *Uptr, at most rows_bound): pool5 [U][49][Cout] as the head's fc6 reads it
void skip_front_launch(az_ctx *c, const int *Uptr, int rows_bound);
int skip_pool_unit(az_ctx *c, int R, int normalise, float *out);      // az_skip_pool past its checks, the rois staged
// ---- az_nms.hip ---------------------------------------------------------------------------------------------------------
unsigned nms_next_tag(az_ctx *c);         // the sequence number the next NMS call's host-mapped result words carry
// the context's NMS scratch grown to n boxes, as az_nms grows it (`who`: the entry's name in the error)
int nms_reserve(az_ctx *c, int n, const char *who);
// greedy NMS of n_groups groups of records [x1, y1, x2, y2, score] that are on the device already, with the kernels of
// az_nms_batched / az_nms (k_nms_small for groups of up to 256 boxes, all in one launch; azk_nms on the context's scratch for
// larger ones); off: the groups' offsets on the host, goff_dev: the same on the device.  Enqueues only.
int nms_groups_dev(az_ctx *c, const float *dets_dev, const int32_t *off, const int *goff_dev, int *gsel_dev, std::vector<int> &small,
                   int n_groups, double thresh, long long *keep_dev, int *nkeep_dev, const char *who);
// ---- az_capi.hip --------------------------------------------------------------------------------------------------------
int set_feature_map_common(az_ctx *c, const float *src, bool src_is_host, int C, int H, int W, bool wait = true);
int ensure_lane_head(az_ctx *t);          // the head buffers of a lane / batch slot created without them
