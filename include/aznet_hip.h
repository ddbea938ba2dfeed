/*
 * aznet_hip.h -- C ABI of libaznet_hip.so: the MI355X (gfx950) implementation of
 * AZ-Net's adjacency-and-zoom region-proposal search.
 *
 * The reference (luyongxi/az-net) has no C API: its native surface is three Cython
 * modules plus pycaffe.  Each entry point below names the reference interface it
 * replaces (paths relative to the upstream tree).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns AZ_OK (0) or a negative az_status; az_last_error(ctx)
 *     gives a message for the last failure on that context.  No exceptions and no
 *     C++ types cross the boundary.
 *   - all pointers are HOST pointers unless the parameter says "dev"; outputs are
 *     caller-allocated with an explicit capacity and an out-count.
 *   - one az_ctx per GPU; a ctx is not thread-safe, distinct ctxs are independent.
 *   - calls are synchronous for the caller; inside they are stream-ordered HIP work
 *     with a single host synchronisation at the end (az_propose: none inside the
 *     level loop).
 *   - boxes are (x1, y1, x2, y2) float64 in ORIGINAL image pixels, as in
 *     lib/detect/test.py:346-414; rois are (batch, x1, y1, x2, y2) float32 in scaled
 *     image pixels, as in lib/detect/test.py:61-71.
 */
#ifndef AZNET_HIP_H
#define AZNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct az_ctx az_ctx;

typedef enum {
    AZ_OK = 0,
    AZ_ERR_INVALID = -1,      /* bad argument (NULL, negative size, shape mismatch) */
    AZ_ERR_HIP = -2,          /* a HIP runtime call failed; see az_last_error       */
    AZ_ERR_CAPACITY = -3,     /* a level / candidate list outgrew the ctx limits or `cap` */
    AZ_ERR_STATE = -4,        /* head or feature map not loaded                      */
    AZ_ERR_NO_DEVICE = -5     /* no usable gfx950 device: there is NO CPU fallback   */
} az_status;

#define AZ_MAX_LEVELS 16
#define AZ_NUM_SUBREG 11      /* len(cfg.SEAR.SUBREGION), lib/detect/config.py:149-155 */
#define AZ_BATCH_MAX 32        /* images az_batch_launch searches in lockstep */

/* Search parameters = the cfg keys lib/detect/test.py reads on this path. */
typedef struct {
    int32_t im_h, im_w;       /* original image size (im.shape[0:2])                  */
    double  scale;            /* im_scale of the single test scale (test.py:45-50)     */
    double  Tz;               /* cfg.SEAR.Tz  (config.py:272-280); compared in double  */
    double  Tc;               /* cfg.SEAR.Tc  (config.py:171), used when !fixed_num    */
    double  dedup;            /* cfg.DEDUP_BOXES = 1/16 (config.py:206); <= 0: no dedup
                                 (test.py:211 `if cfg.DEDUP_BOXES > 0:`): every region forwarded */
    double  eps;              /* cfg.EPS = 1e-14 (config.py:216)                       */
    double  min_side;         /* cfg.SEAR.MIN_SIDE = 10 (config.py:186)                */
    int32_t batch_size;       /* cfg.SEAR.BATCH_SIZE (config.py:189): dedup chunk size */
    int32_t num_proposals;    /* cfg.SEAR.NUM_PROPOSALS (config.py:133, 279)           */
    int32_t fixed_num;        /* cfg.SEAR.FIXED_PROPOSAL_NUM (config.py:172)           */
    int32_t reserved;         /* flags; bit 0: evaluate levels 1-3 one by one (no speculation);
                                 bit 1: keep their geometry as separate launches (same bits);
                                 bit 2: the tuner's variant of the search (lib/detect/tune.py:
                                 256-316): K levels instead of K-1, Tz applied from the second
                                 level on, root not forced, anchor history kept (az_last_anchors);
                                 bit 3: final top-k by the single-workgroup radix select instead of
                                 the chip-wide counting kernels (same result; for tests);
                                 bit 4: keep the geometry of the levels after the speculative ones as
                                 separate launches instead of one kernel per level (same bits);
                                 bit 5: with Tz <= 0 still walk the tree level by level (by default such a
                                 search -- every finite zoom score passes `zoom >= Tz`, test.py:386, so the
                                 tree depends on the image shape only -- forwards the rois of ALL levels in
                                 ONE head pass; same bits);
                                 bit 6: no pair speculation; bit 7: pair speculation at every eligible level (by
                                 default the context decides from its previous search whether the head pass of a
                                 level also evaluates the rois of ALL children of its regions, a superset of the next
                                 level's, which then needs no pass of its own; same bits in all three);
                                 bit 8: no whole-tree speculation; bit 9: whole-tree speculation whenever the image
                                 shape allows (by default the context decides from the row counts of its previous
                                 search of the shape: a dense tree's ONE head pass evaluates a shape-static superset
                                 of its rows and every level finds its outputs by RoIPool window -- after a full tree
                                 the full tree's unique rois, where a search that needs a window the pass lacks is
                                 repeated level by level; otherwise the closure rows, which hold every region any
                                 pruning can produce; same bits in all three);
                                 bit 10: with bit 9, the closure rows instead of the full tree's;
                                 bit 12: no early end (by default, when the context's previous search of the image shape
                                 had no regions from some level on AND its last four searches all ended there or earlier,
                                 a search is enqueued only up to that level -- an empty level still costs its launches,
                                 ~35 us -- and is run again in full if this tree goes on; same bits)                 */
} az_params;

/* The bits of az_params.reserved by name.  A caller that just wants the search passes 0.  AZ_P_TUNE is the ONLY bit that
 * changes a result (it selects the tuner's variant of the search, lib/detect/tune.py:256-316); every other bit picks among
 * forms of the same search that give the same bits -- they exist for the parity tests (each form against the plain level
 * loop) and for A/B measurements, and the context's own choice (all bits 0) is what bench.py and the tools run. */
enum {
    AZ_P_NO_SPECULATION      = 1,     /* levels 1-3 one head pass each                                  */
    AZ_P_UNFUSED_FIRST_LEVELS = 2,    /* their geometry as separate launches                            */
    AZ_P_TUNE                = 4,     /* the tuner's variant (K levels, no forced root, anchor history) */
    AZ_P_RADIX_SELECT        = 8,     /* final top-k by the single-workgroup radix select               */
    AZ_P_UNFUSED_LEVELS      = 16,    /* geometry of the later levels as separate launches              */
    AZ_P_LEVEL_LOOP_AT_TZ0   = 32,    /* no one-pass plan for Tz <= 0                                   */
    AZ_P_NO_PAIR_ROWS        = 64,    /* never carry the next level's rows in a pass                    */
    AZ_P_PAIR_ROWS_ALWAYS    = 128,   /* ... at every eligible level                                    */
    AZ_P_NO_WHOLE_TREE       = 256,   /* never the whole-tree / closure pass                            */
    AZ_P_WHOLE_TREE_ALWAYS   = 512,   /* ... whenever the image shape allows                            */
    AZ_P_CLOSURE_ROWS        = 1024,  /* with AZ_P_WHOLE_TREE_ALWAYS: the closure rows                  */
    AZ_P_NO_EARLY_END        = 4096   /* enqueue every level whatever the last search of the shape did  */
};

/* What the reference prints per image (test.py:408-409) plus per-level sizes. */
typedef struct {
    int32_t n_proposals;
    int32_t num_eval;                     /* sum of B.shape[0] over levels (test.py:378) */
    int32_t depth;                        /* last k of the level loop                    */
    int32_t n_levels;                     /* K - 1                                       */
    int32_t n_candidates;                 /* len(aScores) before selection               */
    int32_t level_regions[AZ_MAX_LEVELS]; /* B.shape[0] per level                        */
    int32_t level_unique[AZ_MAX_LEVELS];  /* rois actually forwarded (after 1/16 dedup)  */
    int32_t level_zoomed[AZ_MAX_LEVELS];  /* len(indZ)                                   */
    int32_t spec_rows;                    /* rois forwarded by the speculative pass that serves
                                             levels 1-3 in one launch (0: levels ran one by one) */
    int32_t root_deferred;                /* 1: the root's row rode on level 4's head pass instead
                                             (spec_rows excludes it, level 4 evaluated one more row) */
    int32_t static_plan;                  /* 1: Tz <= 0, all levels went through one head pass of
                                             spec_rows rois (params.reserved bit 5 turns this off)  */
    int32_t n_passes;                     /* head passes (RoIPool -> int6 -> int7 -> heads) the search made */
    int32_t pass_rows[AZ_MAX_LEVELS];     /* rois each of them evaluated (speculative rows included); a search in
                                             its whole-tree form: ONE pass of the image shape's full tree
                                             (pass_rows[0] > spec_rows, static_plan = 0)                   */
    int32_t search_form;                  /* the form the search took (all forms give the same bits): 0 level by level, one
                                             head pass per level (levels 1-3 in one speculative pass); 1 some passes also
                                             carried the next level's rows (pair speculation); 2 ONE pass over the unique rois
                                             of the image shape's full tree; 3 ONE pass over the closure rows (every region any
                                             pruning of the shape's tree can produce); 4 the Tz <= 0 one-pass plan; 5 level by
                                             level in lockstep with the other images of its batch (az_batch_launch: the root and
                                             its children in the first pass, then one pass per level, shared by the batch)      */
    int32_t n_reruns;                     /* times this search had to be run again in another form before it gave this
                                             result (0 normally; e.g. a whole-tree pass over the full tree's rows that lacked
                                             a window the pruned tree needed)                                               */
    int32_t pass_levels[AZ_MAX_LEVELS];   /* per head pass (as pass_rows): bit l set = the pass evaluated the rois of tree level
                                             l + 1 (its own level, the next one's when it carried pair-speculation rows, levels
                                             1-3 for the speculative pass, every level for a whole-tree / one-pass form) --
                                             what a floor that charges ONE weight stream per pass needs (bench.py)           */
} az_stats;

/* ---- lifecycle ----------------------------------------------------------------- */
const char *az_version(void);
/* Layout check for bindings: sizeof(az_params) in the low 16 bits, sizeof(az_stats) in the next 16 (a caller built against
 * another header would hand az_propose_fetch a block of the wrong size -- every fetch clears sizeof(az_stats) bytes -- so a
 * binding compares this with its own structs when it loads the library; lib/aznet_hip/ffi.py does).  Nothing in the reference
 * corresponds: its Cython modules are compiled against their caller. */
int az_abi_sizes(void);
/* Replaces caffe.set_mode_gpu(); caffe.set_device(id) (tools/prop_az.py:88-89). */
int az_create(int device, az_ctx **out);
int az_destroy(az_ctx *ctx);
const char *az_last_error(const az_ctx *ctx);
/* Optional, before az_load_head: per-level region capacity (default 16384) and total
 * candidate capacity (default 16384*11).  Buffers are sized once, for 288 GB of HBM. */
int az_set_limits(az_ctx *ctx, int max_regions, int max_candidates);

/* Optional, before az_load_head.  How int6 (95 % of the head's FLOPs) is evaluated:
 *   0 (default)  fp32 MFMA (v_mfma_f32_32x32x2_f32), bitwise an fmaf chain;
 *   2            fp32 operands as TWO fp16 terms (x * 2^k = x0 + x1, 22 mantissa bits; 2^k brings the largest
 *                |weight| resp. the largest |feature-map value| of the image to [2^14, 2^15), so nothing overflows and
 *                the scaling is exact), three fp16 MFMAs per product (x0*w1 + x1*w0 + x0*w0) with fp32 accumulation:
 *                products good to ~2^-21; the head's outputs are as close to an f64 evaluation as mode 0's
 *                (measured: tests/test_gpu_gemm_modes.py), at 3/16 of the matrix-pipe cost;
 *   3            fp32 operands as THREE bf16 terms (24 mantissa bits: every fp32 value exactly), six bf16 MFMAs per
 *                product (all cross terms of order <= 2), fp32 accumulation: nothing of fp32's precision or range is
 *                given up; 6/16 of the matrix-pipe cost.  (Operands must be finite and below bf16's largest value,
 *                3.39e38: the terms of an inf are (inf, inf - inf), i.e. NaN where fp32 arithmetic gives +-inf.)
 * In modes 2 and 3 every launch, whatever its row count, uses the same per-row arithmetic (a roi's bits do not
 * depend on its batch), and int6 is the only layer that changes.  Any other value is AZ_ERR_INVALID. */
int az_set_gemm_mode(az_ctx *ctx, int parts);

/* Replaces caffe.Net(test_fc.prototxt, caffemodel) (tools/prop_az.py:95-96): the AZ head
 * models/Pascal/VGG16/az-net/test_fc.prototxt:14-232.  Weights are Caffe InnerProduct
 * blobs, row-major [out, in]; they are copied (and re-tiled) into HBM.
 *   W6 [n6, C*49] b6 [n6] | W71 [n71, n6] b71 | W72 [n72, n6] b72
 *   Was [11, n71] bas | Wab [44, n71] bab | Wz [1, n72] bz
 * Sizes: C, n6, n71 and n72 are positive multiples of 4, and n71 + n72 <= 3072 (the tail kernel stages four rows of
 * int7_1 | int7_2, zero-padded to a multiple of 256, in a 64 KB LDS tile).  Anything else is AZ_ERR_INVALID and leaves the
 * head loaded before in place.  The number of K chunks of a layer is fixed by its K alone (1, 2, 8, 16 from K = 512, 2048,
 * 16384), never by the row count: a roi's bits do not depend on its batch at any size (tests/test_gpu_head_sizes.py). */
int az_load_head(az_ctx *ctx, int C, int n6, int n71, int n72,
                 const float *W6, const float *b6, const float *W71, const float *b71,
                 const float *W72, const float *b72, const float *Was, const float *bas,
                 const float *Wab, const float *bab, const float *Wz, const float *bz);
/* The same head with int6 compressed by truncated SVD (Fast R-CNN, section 4.4; opt-in, not in the reference tree; the
 * detection head's twin is az_load_det_head_lowrank below).  int6, y = relu(W6 x + b6), runs as t = L6 x with L6 =
 * diag(s[:r6]) Vt[:r6] [r6, C*49] (linear: no bias, no ReLU: int6_L) and y = relu(U6 t + b6) with U6 = U[:, :r6] [n6, r6]
 * (int6_U), all fp32, Caffe [out, in] layout; int7_1, int7_2, adj_score, adj_bbox and zoom_score stay as they are.
 * r6 is a multiple of 4 with 4 <= r6 <= min(n6, C*49, AZ_LOWRANK_MAX); that and every size rule of az_load_head:
 * AZ_ERR_INVALID.  On a context in a 16-bit-term GEMM mode (az_set_gemm_mode 2 | 3) the call is AZ_ERR_STATE (and
 * az_set_gemm_mode is refused once any AZ head is loaded).  A refused call leaves the head loaded before in place and
 * answering.  az_load_head replaces a low-rank head and the reverse; either drops the lanes, batch slots and captured
 * graphs built on the head before.  Every form of the search and az_head_forward then run, in int6's place and on the
 * same stream, three launches: fc6_L (the split-K GEMM with az_az_lowrank_split(C*49, r6) chunks, on the many-row kernel
 * where int6 would have been), fc6_L_reduce (a linear slab sum) and fc6_U (the whole K = r6 in one launch, bias and ReLU in
 * registers: az_lowrank.hip's k_lowrank_gemm) -- those are the profiling names; the self-timing span (az_set_profiling bit 3) stays with the full head's
 * fc6_gemm.  No stage's order of summation depends on the row count.  This is a different model from the full head: its
 * zoom scores move, so thresholds tuned on the full net (thresh.pkl) have to be tuned again on the compressed one. */
int az_load_head_lowrank(az_ctx *ctx, int C, int n6, int n71, int n72, int r6, const float *L6, const float *U6,
                         const float *b6, const float *W71, const float *b71, const float *W72, const float *b72,
                         const float *Was, const float *bas, const float *Wab, const float *bab, const float *Wz,
                         const float *bz);
/* The number of K chunks of the AZ head's L stage [., K] x [K, r] (host arithmetic, ctx-free): a function of (K, r) alone.
 * Among the splits that keep the many-row GEMM eligible (whole 128-wide n-tiles of r, nt = r / 128; at least 256 (n-tile,
 * chunk) groups; chunks of exactly K / S in whole K steps of 32, at least two steps each) the one with the least
 * 4 ceil(nt S / 256) (K / S) + nt S -- the longest workgroup's K depth on that kernel's 256 workgroups against the slab
 * traffic, weighted as measured; ties: the smaller S: 56 at (25088, 1024).  Where none exists:
 * az_lowrank_split(K, r), on the plain split-K kernel.  K or r not positive: AZ_ERR_INVALID. */
int az_az_lowrank_split(int K, int r);

/* Replaces feeding `conv5_3` to net['fc'] (lib/detect/test.py:229-236).  The map (NCHW f32,
 * batch 1) is transposed once into ctx-owned HBM in the channel-last layout RoIPool reads;
 * the call returns after that copy, so the source may be reused or freed afterwards.
 * _dev: device pointer, e.g. a torch tensor's data_ptr(); the producer's stream must have
 *       finished writing it before the call.
 * _host: host array. */
int az_set_feature_map_dev(az_ctx *ctx, const float *dev_ptr, int C, int H, int W);
int az_set_feature_map_host(az_ctx *ctx, const float *host_ptr, int C, int H, int W);
/* As _dev, without the closing synchronisation: the transpose is only enqueued on the ctx stream,
 * so handing over the next image's map costs no host round trip.  The source must stay valid (and
 * unmodified) until the next az_propose_fetch / az_propose on this ctx returns. */
int az_set_feature_map_dev_async(az_ctx *ctx, const float *dev_ptr, int C, int H, int W);
/* A map that is already channel-last in HBM ([H][W][C], e.g. a torch.channels_last conv5_3): borrowed as is, no
 * transpose and no copy.  It must stay valid and unmodified while searches use it. */
int az_set_feature_map_dev_nhwc(az_ctx *ctx, const float *dev_ptr, int C, int H, int W);

/* ---- the hot path --------------------------------------------------------------- */
/* Replaces im_propose (lib/detect/test.py:346-414) given the cached conv5_3: the whole
 * level loop (roi projection + 1/16 dedup, RoIPool, fc head, sigmoid, box decode, clip,
 * MIN_SIDE filter, zoom select, divide_region + _sift_dup, final top-K / Tc select) runs
 * on the GPU.  boxes_out [cap,4] f64, scores_out [cap] f32 (may be NULL). */
int az_propose(az_ctx *ctx, const az_params *p, double *boxes_out, float *scores_out,
               int cap, int *n_out, az_stats *stats);
/* Same search split in two so the caller can overlap other GPU work (the next image's
 * backbone): _launch enqueues everything and returns, _fetch waits and copies out. */
int az_propose_launch(az_ctx *ctx, const az_params *p);
/* az_set_feature_map_dev_async (channels_last = 0: NCHW source) or az_set_feature_map_dev_nhwc (1) followed by
 * az_propose_launch, in one call: one host round trip per image. */
int az_propose_launch_on(az_ctx *ctx, const az_params *p, const float *dev_map, int C, int H, int W,
                         int channels_last);
int az_propose_fetch(az_ctx *ctx, double *boxes_out, float *scores_out, int cap, int *n_out,
                     az_stats *stats);
/* Two lanes (default 1).  With 2, the searches launched through az_propose_launch(_on) take turns between the context's
 * stream and a second stream with per-search buffers of its own (the head's weights are shared): while one image's GEMM holds
 * the matrix cores, the other image's single-workgroup geometry kernels and small head kernels run beside it, so a loop that
 * keeps two searches queued gets consecutive images OVERLAPPED on the GPU (~6 % more images per second at 600x1000).  Results,
 * order of az_propose_fetch (oldest first) and every other call are unchanged; a lane queues up to three searches; the
 * synchronous az_propose, the tuner's variant and variable proposal counts stay on the first lane.  Costs the second lane's
 * buffers (pool5, split-K slabs, geometry: ~1.5 GB at max_regions 4096).  Call with nothing queued.
 * az_next_stream: the hipStream_t the NEXT az_propose_launch(_on) will run on (make it wait for the map's producer there);
 * az_last_stream: the one the most recently launched search runs on (record "search done" events there). */
int az_set_lanes(az_ctx *ctx, int lanes);
void *az_next_stream(az_ctx *ctx);
void *az_last_stream(az_ctx *ctx);
/* A batch of images of ONE shape searched in lockstep -- the images of consecutive iterations of the dataset loop
 * (lib/detect/test.py:508-513), each with its own tree, but every level's rois of ALL of them forwarded in ONE head pass
 * (the reference's roi blob carries Caffe's batch index in column 0, test.py:93-97; there it is always 0).  At a tuned
 * threshold a level of one image is a few dozen rois: passes that are weight streams for one image become matrix work for
 * eight, and the latency chain between two passes (slab sum, int7, heads, geometry kernel) is paid once per level, not once
 * per level and image.  Every image's result is what az_propose gives for it alone, bit for bit (stats: search_form 5).
 *   maps: n device pointers to channel-last maps [H][W][C] (az_set_feature_map_dev_nhwc's layout), valid and unmodified
 *   until the batch's last az_batch_fetch; p: fixed proposal count, not the tuner's variant; 1 <= n <= AZ_BATCH_MAX.
 * The search is level by level for every image (root + its children in the first pass); an image whose tree outgrows a
 * fused kernel's tables, or a batch whose level outgrows max_regions rows, is run again on its own by az_batch_fetch (a
 * batch that would not fit, going by the rows per image of the context's last batch, is enqueued in parts that do).
 * Shapes / settings the lockstep form does not take (fewer than three levels, params.reserved bits 0 / 1 / 4, int6 on the
 * 16-bit matrix cores) are searched one image after the other, same results.  az_batch_fetch returns the images of the
 * OLDEST unfetched batch, i = 0 .. n-1 in order.  Two batches per lane may be in flight (a lane's two run one after the other
 * on its stream: the host enqueues the next while the GPU works on the current one; with az_set_lanes(ctx, 2) four).
 * Uses max_regions-sized geometry buffers per image slot (~25 KB per region), allocated at the first batch. */
int az_batch_launch(az_ctx *ctx, int n, const az_params *p, const float *const *maps_nhwc_dev, int C, int H, int W);
/* The same for images of SEVERAL shapes (a dataset mixes them: VOC has 500x375, 375x500, 500x333 ...): params[b] and the map
 * size H[b] x W[b] are image b's; every image keeps its own pre-pass, RoIPool clamps to its own map and its boxes are clipped
 * to its own size, the head passes are shared as before.  The trees may differ in depth (K of lib/detect/test.py:365-368):
 * the batch runs as many level passes as its deepest tree has, an image's last level gets its final selection where the
 * others go on.  The images of a batch share num_proposals, eps, min_side and the flags, and each has at least three levels
 * (>= 80 px on the short side at MIN_SIDE 10); otherwise they are searched one by one (same results). */
int az_batch_launch_shapes(az_ctx *ctx, int n, const az_params *params, const float *const *maps_nhwc_dev, int C,
                           const int *H, const int *W);
int az_batch_fetch(az_ctx *ctx, int i, double *boxes_out, float *scores_out, int cap, int *n_out, az_stats *stats);
/* All images of the oldest unfetched batch (those not yet fetched one by one) in ONE call: image i's boxes at
 * boxes_out + i * cap * 4, scores at scores_out + i * cap (may be NULL), count in n_out[i] (-1: that image failed), statistics
 * in stats[i] (may be NULL); returns the first error, the other images are collected all the same. */
int az_batch_fetch_all(az_ctx *ctx, double *boxes_out, float *scores_out, int cap, int *n_out, az_stats *stats);
/* the hipStream_t the NEXT az_batch_launch runs on: make it wait for the maps' producers there */
void *az_batch_next_stream(az_ctx *ctx);
/* az_propose_stage_result_dev for the batch launched last (call it right behind az_batch_launch): image i's record to
 * dst_dev + i * pitch_bytes, complete when az_batch_fetch(i) returns -- one strided device-to-device copy for the batch. */
int az_batch_stage_results_dev(az_ctx *ctx, void *dst_dev, size_t pitch_bytes, size_t cap_bytes);
/* Multi-GPU exchange of proposals (image-sharded ranks, one all-gather of fixed-size
 * records; the reference itself is single-process).  A fixed-count search (params.fixed_num) leaves
 * its result in HBM as ONE record of az_result_record_layout(k) bytes: int32 n at n_offset,
 * boxes f64 [k][4] at boxes_offset, scores f32 [k] at scores_offset (rows >= n undefined).
 * az_propose_stage_result_dev, called between az_propose_launch and az_propose_fetch, enqueues a
 * device-to-device copy of that record to dst_dev (e.g. a slot of the RCCL send buffer) on the ctx
 * stream; it is complete when az_propose_fetch returns.  No host hop for the exchanged data. */
int az_result_record_layout(int num_proposals, size_t *bytes, size_t *n_offset, size_t *boxes_offset,
                            size_t *scores_offset);
int az_propose_stage_result_dev(az_ctx *ctx, void *dst_dev, size_t cap_bytes);
/* The exchange itself as ONE ncclAllGather over RCCL / xGMI, no framework in between: every rank
 * contributes `bytes_per_rank` bytes at send_dev (its staged records, padding rows included) and receives all ranks' blocks
 * in rank order at recv_dev (nranks * bytes_per_rank bytes).  It runs on a stream of the context's own
 * (az_comm_stream: a hipStream_t; make it wait for whoever wrote padding rows, make readers of recv_dev wait for it),
 * device-ordered behind everything both lanes have queued when the call is made -- so it may be issued right behind the
 * batch's last az_propose_launch -- and holds neither lane back.  RCCL is bound at run time to the librccl.so the process
 * already holds (PyTorch-ROCm's), else ROCm's.  az_rccl_unique_id: 128 bytes made on rank 0 and handed to every rank by
 * the launcher's own means (a file, torch.distributed's store, MPI); az_rccl_init: collective over the nranks processes,
 * one per GPU.  The reference is single-process: this replaces nothing there. */
int az_rccl_unique_id(void *id_out, size_t cap);
int az_rccl_init(az_ctx *ctx, const void *id, size_t id_bytes, int nranks, int rank);
int az_gather_records(az_ctx *ctx, const void *send_dev, void *recv_dev, size_t bytes_per_rank);
int az_rccl_destroy(az_ctx *ctx);
void *az_comm_stream(az_ctx *ctx);
/* All candidates of the last az_propose, before selection (Y / aScores of test.py:380-381). */
int az_last_candidates(az_ctx *ctx, double *boxes_out, float *scores_out, int cap, int *n_out);

/* ---- unit entry points (the same kernels, one stage at a time) --------------------- */
/* utils.cython_div.divide_region(regions f64[P,4], min_height) (lib/utils/div.pyx:15-76). */
int az_divide_region(az_ctx *ctx, const double *regions, int P, double min_side,
                     double *out, int cap, int *n_out);
/* utils.cython_div._sift_dup (lib/utils/div.pyx:78-89). */
int az_sift_dup(az_ctx *ctx, const double *regions, int C, double min_side,
                double *out, int cap, int *n_out);
/* _get_rois_blob + the feature-space dedup of lib/detect/test.py:61-97,210-218 for one
 * level.  rois_out [P,5] f32 (all rois, before dedup), index_out [P] (first n_unique
 * valid), inv_index_out [P]. */
int az_roi_dedup(az_ctx *ctx, const double *boxes, int P, double scale, double dedup,
                 int batch_size, float *rois_out, int32_t *index_out, int32_t *inv_index_out,
                 int *n_unique);
/* Caffe ROIPooling 7x7 @ spatial_scale (test_fc.prototxt:14-25) over the current
 * feature map.  out [R, C*49] f32. */
int az_roi_pool(az_ctx *ctx, const float *rois, int R, float *out);
/* net['fc'].forward(rois=...) (lib/detect/test.py:235-242): zoom_prob [R,1],
 * adj_prob [R,11], adj_bbox [R,44], all f32.  Any output may be NULL. */
int az_head_forward(az_ctx *ctx, const float *rois, int R, float *zoom_prob, float *adj_prob,
                    float *adj_bbox);
/* _bbox_pred + _clip_boxes + _unwrap_adj_pred (lib/detect/test.py:106-151,171-187) for R
 * regions: anchors [R,4] f64, deltas [R,44] f32, scores [R,11] f32 -> kept boxes/scores in
 * r*11+s order.  More kept candidates than the context's max_candidates: AZ_ERR_CAPACITY, with
 * *n_out = max_candidates and the first max_candidates kept candidates written (cap permitting). */
int az_decode_filter(az_ctx *ctx, const double *anchors, const float *deltas, const float *scores,
                     int R, int im_h, int im_w, double eps, double min_side,
                     double *boxes_out, float *scores_out, int cap, int *n_out);
/* Final selection of lib/detect/test.py:393-401: indices of the top-k scores, descending
 * (ties: lower index first). */
int az_topk(az_ctx *ctx, const float *scores, int n, int k, int32_t *idx_out, int *n_out);
/* az_topk by the single-workgroup radix select at every n (az_topk hands n <= 65536 to the chip-wide counting
 * kernels): same arguments, same result. */
int az_topk_radix(az_ctx *ctx, const float *scores, int n, int k, int32_t *idx_out, int *n_out);
/* utils.cython_nms.nms(dets f32[N,5], thresh) (lib/utils/nms.pyx:17-68): kept original
 * indices in descending-score order.  The reference's call site is apply_nms
 * (lib/detect/test.py:467-484); it is NOT on the proposal path.  Equal scores: the higher original index first.  NaN
 * scores are outside the stated behaviour (unspecified order; here and in az_nms_batched). */
int az_nms(az_ctx *ctx, const float *dets, int n, double thresh, int64_t *keep, int *n_keep);
/* The call site itself, apply_nms (lib/detect/test.py:467-484): one nms per class per image, i.e.
 * many small independent problems.  Group g owns dets[offsets[g] .. offsets[g+1]) (rows of 5 f32);
 * keep[offsets[g] ..] receives its kept group-local indices (descending score), n_keep[g] their
 * number.  Groups of <= 256 boxes share one launch (a workgroup each). */
int az_nms_batched(az_ctx *ctx, const float *dets, const int32_t *offsets, int n_groups, double thresh,
                   int64_t *keep, int32_t *n_keep);

/* ---- Soft-NMS and box voting (not in the reference; opt-in behind cfg.TEST.NMS_METHOD / BBOX_VOTE) ---------------------------- */
/* Two test-time refinements of apply_nms's step: Soft-NMS (Bodla et al., ICCV 2017) decays the scores of overlapping
 * detections instead of deleting them; box voting (Gidaris & Komodakis, ICCV 2015) replaces each surviving box by the
 * score-weighted mean of the group's boxes that overlap it.  Groups, offsets and the keep / n_keep layout are az_nms_batched's:
 * group g owns the rows dets[offsets[g] .. offsets[g+1]) of [x1, y1, x2, y2, score] float32, a group of n rows.
 *   IoU of rows i and j is az_nms's float32 arithmetic, one rounding per operation (the library is built without
 *   contraction):  area = (x2 - x1 + 1) * (y2 - y1 + 1);  w = max(0, min(x2_i, x2_j) - max(x1_i, x1_j) + 1), h likewise;
 *   inter = w * h;  den = (area_i + area_j) - inter;  ovr = inter / den.
 * az_soft_nms_batched.  Every box starts alive with its input score.  Rounds repeat while a box is alive: the alive box of
 * highest CURRENT score is picked (equal scores: the higher original index, az_nms's rule), emitted with that score and
 * leaves the pool; every other alive box j gets s_j = s_j * w_j in float32 with
 *     AZ_NMS_HARD      w = (double)ovr >= thresh ? 0 : 1
 *     AZ_NMS_LINEAR    w = (double)ovr >= thresh ? 1 - ovr : 1
 *     AZ_NMS_GAUSSIAN  w = expf(-(ovr * ovr) / (float)sigma)          (thresh unused)
 * and is dropped, without being emitted, when (double)s_j < min_score.  The comparison with thresh is `>=`, as in az_nms (the
 * Soft-NMS paper's code uses `>`).  keep[offsets[g] ..] receives the picked group-local indices in pick order,
 * scores_out[offsets[g] ..] their scores at the moment they were picked, n_keep[g] their number.  AZ_NMS_HARD with min_score in
 * (0, smallest positive input score] returns az_nms's keep list exactly; with min_score = 0 a suppressed box stays in the
 * pool with score 0 and is emitted later.  Stated domain: finite scores >= 0; anything else is unspecified, as NaN is for
 * az_nms -- but whatever the values, a group ends after at most n rounds and no index leaves [0, n).
 * Groups of 1 .. 256 boxes share one launch (k_soft_nms_small: a workgroup per group, a box per thread), groups of 257 ..
 * 4096 another (k_soft_nms_large: a workgroup per group, four boxes per thread); a group of more than 4096 boxes is
 * AZ_ERR_CAPACITY (4096 is az_topk's largest k: no image of the pipeline exceeds it).
 * az_box_vote_batched.  dets are the groups' ORIGINAL rows, keep / n_keep a keep list per group in az_nms_batched's layout
 * (from az_nms_batched or az_soft_nms_batched).  For each kept box k the voters are all rows j of its group with
 * (double)ovr(k, j) >= vote_thresh (the box itself among them); in float64 and in ascending j:  sw += s_j;  sc[q] += s_j *
 * b_j[q]  (s_j the rows' original scores; the product of two float32 values is exact in float64); the voted coordinate is
 * (float)(sc[q] / sw), and with sw == 0 the box stays as it was.  boxes_out [total][4]: row offsets[g] + k receives the
 * voted box of group g's k-th kept box; scores are not touched.  One thread walks one kept box's voters in index order, so
 * the same call gives the same bits.
 * Both: AZ_ERR_INVALID, before anything is enqueued and with the outputs untouched, for a method outside the three
 * constants, sigma <= 0 (or not finite) with AZ_NMS_GAUSSIAN, a negative (or NaN) min_score, a NaN thresh (hard, linear) / vote_thresh,
 * offsets that do not start at 0 or decrease, an n_keep[g] outside [0, n], a keep index outside its group, a NULL array that
 * is needed; AZ_ERR_CAPACITY likewise for a group of more than 4096 boxes.  Empty groups and n_groups == 0 are fine.
 * Device scratch is kept in the context and grown on demand. */
#define AZ_NMS_HARD 0
#define AZ_NMS_LINEAR 1
#define AZ_NMS_GAUSSIAN 2
#define AZ_SOFT_NMS_MAX 4096   /* boxes per group */
int az_soft_nms_batched(az_ctx *ctx, const float *dets, const int32_t *offsets, int n_groups, int method,
                        double thresh, double sigma, double min_score,
                        int64_t *keep, float *scores_out, int32_t *n_keep);
int az_box_vote_batched(az_ctx *ctx, const float *dets, const int32_t *offsets, int n_groups,
                        const int64_t *keep, const int32_t *n_keep, double vote_thresh, float *boxes_out);

/* ---- Fast R-CNN head on the shared conv map (BASELINE config 3) ---------------------- */
/* Replaces caffe.Net(frcnn/test_fc.prototxt, caffemodel) (tools/test_shared.py): the detection
 * head models/Pascal/VGG16/frcnn/test_fc.prototxt:14-145 -- fc6 [n6, C*49], fc7 [n7, n6],
 * cls_score [ncls, n7] (+Softmax), bbox_pred [4*ncls, n7]; Caffe [out, in] layout.  2 <= ncls <= 256 (VOC: 21;
 * COCO, models/COCO/VGG16/frcnn/test_fc.prototxt:97-135: 81).
 * Sizes: C, n6 and n7 are positive multiples of 4 (n7 has no upper limit: this head's tail is a GEMM); with an AZ head
 * loaded, C must be that head's.  Anything else is AZ_ERR_INVALID and leaves the detection head loaded before in place. */
int az_load_det_head(az_ctx *ctx, int C, int n6, int n7, int ncls, const float *W6, const float *b6,
                     const float *W7, const float *b7, const float *Wc, const float *bc,
                     const float *Wb, const float *bb);
/* The same head with fc6 and / or fc7 compressed by truncated SVD (Fast R-CNN, section 4.4; opt-in, not in the reference
 * tree).  A layer y = relu(W x + b) of rank r is two products: t = L x with L = diag(s[:r]) Vt[:r] [r, in] (linear: no
 * bias, no ReLU: the paper's fc6_L / fc7_L), then y = relu(U t + b) with U = U[:, :r] [out, r] (fc6_U / fc7_U), all fp32,
 * Caffe [out, in] layout.  r6 / r7 == 0 leaves that layer at full rank: its L is NULL and its U holds the full weight
 * ([n6, C*49] resp. [n7, n6]); otherwise the rank is a multiple of 4 with 4 <= r <= min(out, in, AZ_LOWRANK_MAX) and L
 * is not NULL.  cls_score and bbox_pred are untouched.  Sizes and refusals otherwise as az_load_det_head: AZ_ERR_INVALID,
 * with the head loaded before left in place.  In the 16-bit-term GEMM modes a head with a compressed layer is refused
 * (AZ_ERR_STATE, the head loaded before left in place; it does not run at full rank), and az_set_gemm_mode(2 | 3)
 * with one loaded is AZ_ERR_STATE.  A later az_load_det_head replaces a low-rank head, and the reverse.  Every entry that runs
 * the detection head (az_det_forward, az_detect, az_detect_batch, az_detect_pyramid, az_detect_skip,
 * az_det_forward_skip) then runs the compressed layers: the L stage on the split-K GEMM with az_lowrank_split(in, r)
 * chunks and a linear slab sum, the U stage in one launch over the whole K = r with bias and ReLU applied in registers
 * (az_lowrank.hip).  Neither stage's order of summation depends on the row count: a roi's bits do not depend on which
 * rois share the launch.  The profiling names are det_fc6_L, det_fc6_L_reduce, det_fc6_U (likewise fc7).  The
 * trainers keep full-rank weights of their own.  This is a different model from the full head: U L only approximates W. */
#define AZ_LOWRANK_MAX 2048    /* largest rank = largest K of the U stage */
int az_load_det_head_lowrank(az_ctx *ctx, int C, int n6, int n7, int ncls, int r6, int r7, const float *L6,
                             const float *U6, const float *b6, const float *L7, const float *U7, const float *b7,
                             const float *Wc, const float *bc, const float *Wb, const float *bb);
/* The U-stage kernel alone (tests): Y [M, N] = act(X [M, K] . W [N, K]^T + b [N]), host arrays, act = ReLU if relu != 0.
 * Each element's K terms are added by one fp32 fmaf chain in an order fixed by K, then the bias.  N and K are positive
 * multiples of 4 and K <= AZ_LOWRANK_MAX, 0 <= M; anything else is AZ_ERR_INVALID, M above the region capacity
 * AZ_ERR_CAPACITY, both before any device work.  M == 0 is a no-op (AZ_OK, Y untouched, pointers not read).  The launch
 * reads M from device memory, as the head's launches do, and the device copy of Y carries 64 pre-filled rows behind row M: if
 * the kernel changed one of them the call returns AZ_ERR_HIP. */
int az_lowrank_gemm_unit(az_ctx *ctx, const float *X, const float *W, const float *b, int M, int N, int K, int relu,
                         float *Y);
/* The number of K chunks of an L stage [., K] x [K, r] (host arithmetic, ctx-free): a function of (K, r) alone -- the
 * number of chunks is part of a row's bits.  K or r not positive: AZ_ERR_INVALID. */
int az_lowrank_split(int K, int r);
/* frcnn_net['fc'].forward(rois=..., conv5_3=...) (lib/detect/test.py:302-307): cls_prob [R,ncls],
 * bbox_pred [R,4*ncls], f32. */
int az_det_forward(az_ctx *ctx, const float *rois, int R, float *cls_prob, float *bbox_pred);
/* _frcnn_forward (lib/detect/test.py:259-318) for the proposals `boxes` [P,4] f64 of one image:
 * roi projection + 1/16 dedup per batch_size chunk, head, _bbox_pred + _clip_boxes of every
 * class, un-dedup.  scores_out [P,ncls] f32, boxes_out [P,4*ncls] f64. */
int az_detect(az_ctx *ctx, const double *boxes, int P, double scale, double dedup, int batch_size,
              int im_h, int im_w, double eps, float *scores_out, double *boxes_out);
/* _frcnn_forward (lib/detect/test.py:259-318) for n images at once, as test_net (:541-668) runs it
 * over saved proposals: image i has its own channel-last map maps_nhwc_dev[i] [Hs[i]][Ws[i]][C]
 * (device memory, C = the detection head's), proposals boxes[box_off[i] .. box_off[i+1]) ([.,4] f64),
 * scale scales[i] and size im_hw[2i], im_hw[2i+1].  Rows [box_off[i], box_off[i+1]) of scores_out
 * [box_off[n],ncls] f32 / boxes_out [box_off[n],4*ncls] f64 are bit for bit what az_detect returns
 * for image i alone with its map set: the 1/16 dedup and its batch_size chunks are per image, and
 * the head runs over the unique rows of all images in one pass.  Images without boxes contribute
 * nothing (their map may be NULL).  1 <= n <= AZ_BATCH_MAX; a batch with more boxes than the
 * region capacity is run in several passes split at image boundaries; one image with more boxes
 * than that is AZ_ERR_CAPACITY.  fp32 only: AZ_ERR_STATE in the 16-bit-term GEMM modes.  Every
 * argument error is reported before anything is enqueued. */
int az_detect_batch(az_ctx *ctx, int n, const float *const *maps_nhwc_dev, int C, const int32_t *Hs,
                    const int32_t *Ws, const double *boxes, const int32_t *box_off, const double *scales,
                    const int32_t *im_hw, double dedup, int batch_size, double eps, float *scores_out,
                    double *boxes_out);

/* ---- multi-scale test pyramids (cfg.TEST.SCALES with several entries) ------------------------ */
/* _get_image_blob (lib/detect/test.py:27-59) stacks every scale's image in ONE zero-padded blob, so the backbone gives
 * S conv5_3 maps of one padded size; _project_im_rois (:73-97) sends each roi to the level whose scaled area is closest
 * to 224 x 224, and roi column 0 holds that level.  Every entry below refuses a bad argument before any device work:
 * S outside [1, AZ_PYRAMID_MAX], a scale that is not positive and finite, a pyramid of another S than the one set, the
 * 16-bit-term GEMM modes (AZ_ERR_STATE).  S == 1 gives the bits of the single-scale entries.  The level is the FIRST
 * minimum (equal scales: the first of them); a box whose area is infinite or NaN takes level 0, as np.argmin does on
 * distances that are all inf / all NaN (its roi is then not finite: use dedup <= 0 with such boxes). */
#define AZ_PYRAMID_MAX 8
/* S channel-last maps [H][W][C] (device memory, all of one size: the padded blob's conv5_3), borrowed as
 * az_set_feature_map_dev_nhwc borrows one; level 0 also becomes the context's single map. */
int az_set_feature_pyramid_dev_nhwc(az_ctx *ctx, const float *const *maps_nhwc_dev, int S, int C, int H, int W);
/* _get_rois_blob with a pyramid + the feature-space dedup of one chunked level (test.py:61-97,210-218): rois_out [P,5]
 * f32 (column 0 = level, before dedup), index_out [P] (first n_unique valid), inv_index_out [P]. */
int az_roi_dedup_pyramid(az_ctx *ctx, const double *boxes, int P, const double *scales, int S, double dedup,
                         int batch_size, float *rois_out, int32_t *index_out, int32_t *inv_index_out, int *n_unique);
/* RoIPool over the pyramid set: each roi [R,5] reads the map of its level (column 0, an integer in [0, S)) and
 * clamps to that map's padded size.  out [R, C*49] f32 (Caffe's flattening). */
int az_roi_pool_pyramid(az_ctx *ctx, const float *rois, int R, float *out);
/* im_propose / tune.im_propose (params.reserved bit 2) over the pyramid set: the plain level loop, each level's regions
 * projected into the pyramid; the speculative, whole-tree, one-pass, fused, pair-row, early-end and graph forms are never
 * taken.  Synchronous, on the context's first lane; az_last_candidates and az_last_anchors answer for it as for
 * az_propose.  scales [S] as _get_image_blob returns them (p->scale is ignored). */
int az_propose_pyramid(az_ctx *ctx, const az_params *p, const double *scales, int S, double *boxes_out,
                       float *scores_out, int cap, int *n_out, az_stats *stats);
/* az_detect over the pyramid set: projection + dedup as az_roi_dedup_pyramid, RoIPool on each roi's level, the
 * detection head, decode + clip in original image pixels, un-dedup. */
int az_detect_pyramid(az_ctx *ctx, const double *boxes, int P, const double *scales, int S, double dedup,
                      int batch_size, int im_h, int im_w, double eps, float *scores_out, double *boxes_out);

/* ---- the skip-connection detector (models/COCO/VGG16_skip/frcnn/test_fc.prototxt, experiments/cfgs/voc_skip.yml) ---- */
/* A front in place of the detection head's RoIPool: every roi is pooled 7x7 from up to three maps (conv3_3, conv4_3,
 * conv5_3: cfg.SEAR.FRCNN_CONV), each block normalised across its channels, the blocks concatenated, scaled and folded
 * to the head's C channels by a 1x1 convolution + ReLU; fc6 ... cls_prob / bbox_pred run unchanged on the result.
 * Inference, one image per call, fp32 only.  Every entry below refuses, before any device work: the 16-bit-term GEMM
 * modes and a context whose pyramid was set after the skip maps (AZ_ERR_STATE), more rois than the region capacity (AZ_ERR_CAPACITY), a missing
 * detection head / front / map set (AZ_ERR_STATE). */
#define AZ_SKIP_MAX_SRC 3
#define AZ_SKIP_MAX_SUMC 4096   /* channels of all sources together */
#define AZ_SKIP_CHUNK 128       /* rois per pass of the front: the concatenated rows are held for this many at a time */
/* roi_pool3/4/5 + roi_norm3/4/5 + concat5 + scale5 + conv_pool5 + relu_pool (test_fc.prototxt of the skip model):
 * source i has Cs[i] channels (a positive multiple of 4) and ROIPooling spatial_scale spatial_scales[i]; the GRN layers
 * compute y[c] = x[c] / sqrt(sum_c x[c]^2 + eps) per roi, bin and source (their eps: 1e-10 by default; an all-zero
 * vector gives zeros); `gain` is scale5's factor (1000); Wp [Cout][sum Cs] and bp [Cout] are conv_pool5's blobs.  Cout
 * must be the loaded detection head's C (AZ_ERR_INVALID); without a detection head: AZ_ERR_STATE.  On any error the
 * front loaded before stays in place. */
int az_load_skip_front(az_ctx *ctx, int n_src, const int *Cs, const float *spatial_scales, double gain, double eps,
                       int Cout, const float *Wp, const float *bp);
/* The blobs _frcnn_forward hands the skip net, forward_kwargs[name] = conv[name] for name in cfg.SEAR.FRCNN_CONV
 * (lib/detect/test.py:300-304): n_src channel-last maps [Hs[i]][Ws[i]][Cs[i]] (device memory), borrowed as
 * az_set_feature_map_dev_nhwc borrows one.  Channel counts must be the loaded front's (AZ_ERR_INVALID).  The last map
 * also becomes the context's ordinary map when it has the heads' channel count.  A pyramid set the context held
 * (az_set_feature_pyramid_dev_nhwc) is dropped: set it again before the next pyramid entry; a pyramid set AFTER these
 * maps makes the skip entries refuse (AZ_ERR_STATE) until the maps are set again. */
int az_set_skip_maps_dev_nhwc(az_ctx *ctx, int n_src, const float *const *maps_nhwc_dev, const int *Cs, const int *Hs,
                              const int *Ws);
/* _frcnn_forward (lib/detect/test.py:259-318) with the skip net: az_detect's contract and outputs, the head's RoIPool
 * replaced by the front on the maps of az_set_skip_maps_dev_nhwc. */
int az_detect_skip(az_ctx *ctx, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h,
                   int im_w, double eps, float *scores_out, double *boxes_out);
/* Iterative box localisation (not in the reference; Gidaris & Komodakis, ICCV 2015): az_detect, then up to rounds - 1
 * further head passes whose proposals are the class boxes of the pass before that score well.  Round 1 is az_detect on
 * `boxes`: scores_out [P,ncls] f32 / boxes_out [P,4*ncls] f64 carry its bits.  The sources of round 2 are the pairs (row
 * i, class j >= 1) with scores[i][j] >= (float)min_score (an f32 comparison), in ascending f = (j - 1) * P + i; more than
 * max_rows of them: the max_rows with the highest score are kept, ties to the lower f (az_topk's rule), still in ascending
 * f.  Their boxes boxes_out[i][4j .. 4j+3] are the next pass's proposals, treated as az_detect treats `boxes` (projection,
 * 1/16 dedup per batch_size chunk, un-dedup, decode, clip); of new row e, which came from class j, only column j is kept.
 * Each later round selects among the extras of the round before alone (same threshold and cap, f = the position in that
 * round's list); a round without sources ends the loop.  The extras of all rounds come out round after round without
 * gaps, ex_count[r] of them for round r + 2 (ex_count [rounds-1]): ex_cls (the class), ex_src (the proposal row for round
 * 2, later the position in the previous round's list), ex_score f32, ex_box [.,4] f64.  The caller sizes the four lists to
 * (rounds - 1) * max_rows rows.  Boxes and scores stay on the device between rounds; by default the 4-byte row count of
 * each round is read back (AZ_ITERLOC_SYNC=0: not even that).  1 <= rounds <= AZ_ITER_LOC_MAX_ROUNDS, 1 <= max_rows <=
 * 4096 (AZ_ERR_INVALID), max_rows or P above the region capacity: AZ_ERR_CAPACITY, a NULL extras pointer with rounds > 1:
 * AZ_ERR_INVALID, otherwise az_detect's checks; every refusal comes before any device work and leaves the outputs
 * untouched.  P == 0: AZ_OK, all counts 0.  rounds == 1: az_detect (the extras pointers are not read).  One image, one
 * scale: there is no pyramid and no batch form of this entry. */
#define AZ_ITER_LOC_MAX_ROUNDS 8
int az_detect_iter(az_ctx *ctx, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h, int im_w,
                   double eps, int rounds, double min_score, int max_rows, float *scores_out, double *boxes_out,
                   int32_t *ex_cls, int32_t *ex_src, float *ex_score, double *ex_box, int32_t *ex_count);
/* az_detect_iter with the skip net: the front of az_detect_skip in RoIPool's place in every round; its refusals too. */
int az_detect_iter_skip(az_ctx *ctx, const double *boxes, int P, double scale, double dedup, int batch_size, int im_h,
                        int im_w, double eps, int rounds, double min_score, int max_rows, float *scores_out,
                        double *boxes_out, int32_t *ex_cls, int32_t *ex_src, float *ex_score, double *ex_box,
                        int32_t *ex_count);
/* frcnn_net['fc'].forward(rois=..., conv3_3=..., conv4_3=..., conv5_3=...) (lib/detect/test.py:302-307) of the skip
 * net: az_det_forward's twin. */
int az_det_forward_skip(az_ctx *ctx, const float *rois, int R, float *cls_prob, float *bbox_pred);
/* Unit entries.  az_skip_pool: the blobs concat5 (normalise = 0: before roi_norm*, the raw ROIPooling maxima;
 * normalise = 1: after scale5) as rows [R*49][sum Cs], row = roi * 49 + ph * 7 + pw.  az_skip_conv: conv_pool5 +
 * relu_pool of `rows` such rows given by the host, out [rows][Cout]. */
int az_skip_pool(az_ctx *ctx, const float *rois, int R, int normalise, float *out);
int az_skip_conv(az_ctx *ctx, const float *cat_host, int rows, float *out);

/* ---- zoom-threshold tuner (lib/detect/tune.py, tools/set_thresh.py) ------------------- */
/* `Bhis` of the tuner's im_propose (tune.py:303, returned at :316) for the last az_propose run
 * with params.reserved bit 2: every region evaluated, level-major, with its zoom score.
 * regions_out [cap,4] f64, zoom_out [cap] f32; either may be NULL.
 * The history is ONE buffer per context: from the moment a later tuner search is launched (az_propose_launch queues
 * them: they have a fixed proposal count) it is being overwritten, so between the fetch of a tuner search and the fetch
 * of a tuner search queued behind it az_last_anchors returns AZ_ERR_STATE, as az_last_candidates does for the candidate
 * list; after that fetch it answers for the later search.  A plain search queued behind leaves the history alone.  A
 * tuner search whose fetch failed (a history past 2 * max_regions rows is AZ_ERR_CAPACITY, raise az_set_limits) has no
 * history either: AZ_ERR_STATE.
 * Thresholds compare as `(double)zoom >= Tz` in every form of the search, which is the reference's comparison: its zoom
 * scores are float64 by the time `np.where(zoom >= Tz)` sees them (test.py:198,253: an hstack onto np.zeros((0,))).  A
 * Tz that float32 does not hold (a hand-written 0.35) therefore drops a region whose float32 score is float32(0.35), in
 * the reference and here alike; a tuned threshold is a widened float32 and meets no such case. */
int az_last_anchors(az_ctx *ctx, double *regions_out, float *zoom_out, int cap, int *n_out);
/* tune_thresh (tune.py:318-366) keeps the num_images*ANCHORS_PER_IMG largest zoom scores of a
 * whole image set in a heap and returns the smallest of them.  Here the scores stay in HBM:
 * between az_tune_begin and az_tune_end every tuner-variant az_propose appends its anchors' zoom
 * scores to a device pool of `capacity` floats (no host round trip), and az_tune_kth_largest
 * radix-selects the k-th largest: -inf when the pool holds <= k scores, exactly as the heap
 * never overflowing leaves `thresh = -np.inf` (tune.py:326,347-350).
 * The n <= k rule: with n pooled scores az_tune_kth_largest gives -inf for n <= k and the k-th largest (ties counted,
 * -0.0 below +0.0) for n > k; az_tune_top gives all n for n <= k, else every score >= the k-th largest, which is more
 * than k scores when the k-th ties.  k <= 0 is AZ_ERR_INVALID.  Scores may be any float but NaN: denormals, either zero
 * and +-inf order as values.  NaN scores are outside the contract (the key order ranks them above +inf; the
 * reference's heap is undefined on them), and so is the heap's habit of never pushing a -inf score (`scores > thresh`
 * at thresh = -inf): zoom scores are sigmoid outputs.
 * The pool takes `capacity` floats, whatever an earlier az_tune_begin allocated; az_tune_begin empties it.  A push past
 * the capacity is AZ_ERR_CAPACITY and changes nothing; searches that append past it are counted on the device and
 * az_tune_kth_largest / az_tune_top then return AZ_ERR_CAPACITY ("raise az_tune_begin's capacity", n_total = capacity).
 * After a tuner search that appended to the pool has FAILED (its fetch returned an error: its history, hence what it
 * appended, is incomplete) az_tune_kth_largest, az_tune_top and az_tune_push return AZ_ERR_CAPACITY until the next
 * az_tune_begin: the pool never answers over an incomplete set.  Without az_tune_begin, or after az_tune_end, the three
 * return AZ_ERR_STATE. */
int az_tune_begin(az_ctx *ctx, long long capacity);
int az_tune_end(az_ctx *ctx);
int az_tune_kth_largest(az_ctx *ctx, long long k, float *value_out, long long *n_total);
/* Multi-GPU merge: every pooled score >= the k-th largest (all of them when the pool holds
 * <= k), unordered; rank 0 pushes the gathered lists into its own pool and selects again. */
int az_tune_top(az_ctx *ctx, long long k, float *scores_out, long long cap, long long *n_out);
int az_tune_push(az_ctx *ctx, const float *scores, long long n);

/* ---- recall evaluation (lib/datasets/imdb.py:120-159) ----------------------------------- */
/* utils.cython_bbox.bbox_overlaps(boxes f64[N,4], query_boxes f64[K,4]) -> f64[N,K]
 * (lib/utils/bbox.pyx:132-172). */
int az_bbox_overlaps(az_ctx *ctx, const double *boxes, int N, const double *query, int K,
                     double *overlaps_out);
/* The matching loop of imdb.evaluate_recall (imdb.py:124-147) for n_images images at once:
 * image i owns boxes[box_off[i]:box_off[i+1]] and gt[gt_off[i]:gt_off[i+1]] (f64 [.,4]); per
 * image, repeatedly take the best remaining (box, gt) pair, record its overlap, retire both.
 * gt_overlaps_out [gt_off[n_images]] in image order, then pick order.  Images without boxes
 * must be left out by the caller (imdb.py:128-129); fewer boxes than gt boxes in an image is
 * AZ_ERR_INVALID (the reference's `assert(gt_ovr >= 0)` fires there). */
int az_recall_match(az_ctx *ctx, int n_images, const double *boxes, const int32_t *box_off,
                    const double *gt, const int32_t *gt_off, double *gt_overlaps_out);

/* ---- detection evaluation (imdb.evaluate_detections, lib/datasets/pascal_voc.py:147-190) -- */
/* What the reference hands to MATLAB: the VOCdevkit's VOCevaldet.m per class plus the wrapper's
 * xVOCap.m (VOCdevkit-matlab-wrapper/voc_eval.m), restated in DESIGN §1b, for n_classes x n_images
 * segments, class-major: segment s = c*n_images + i owns det[det_off[s]:det_off[s+1]] (file order:
 * the results file's values, boxes 1-based) and gt[gt_off[s]:gt_off[s+1]] (1-based, with the XML's
 * difficult flag).  Per class: MATLAB's stable sort of -confidence, the greedy match at
 * ovmax >= min_overlap (a difficult box: neither TP nor FP), rec = tp/npos, prec = tp/(fp+tp),
 * ap = 11-point AP (metric_07, the VOC2007 devkit) or the area AP (2010+ devkits), ap_auc = xVOCap.
 * match_out [D] in input order: 1 TP, -1 FP, 0 ignored; rec_out / prec_out [D] in each class's
 * rank order at that class's offset det_off[c*n_images]; any of the three may be NULL.
 * Malformed offsets are AZ_ERR_INVALID and n_classes*n_images past int32 is AZ_ERR_CAPACITY, both
 * before any device work.  Device scratch is kept in the context. */
int az_voc_eval(az_ctx *ctx, int n_classes, int n_images,
                const double *det_box, const double *det_conf, const int32_t *det_off,
                const double *gt_box, const uint8_t *gt_difficult, const int32_t *gt_off,
                double min_overlap, int metric_07,
                int8_t *match_out, double *rec_out, double *prec_out,
                int64_t *npos_out, double *ap_out, double *ap_auc_out);
/* Unit entry (tests): the ranking that az_voc_eval and az_coco_eval share, alone, on host arrays.  For the D = det_off[S]
 * scores of n_classes x n_images class-major segments: by_seg_out [D] lists the detections segment by segment, by_class_out
 * [D] class by class, each group by (-score, input order) with NaN last and -0 equal to +0.  Offsets are validated as
 * az_voc_eval validates them (same codes); D = 0 returns AZ_OK and touches nothing. */
int az_rank_unit(az_ctx *ctx, int n_classes, int n_images, const double *score, const int32_t *det_off,
                 uint32_t *by_seg_out, uint32_t *by_class_out);

/* ---- detection evaluation (imdb.evaluate_detections, lib/datasets/coco.py:_do_coco_eval) ----------- */
/* What the reference hands to pycocotools: COCOeval's evaluate + accumulate + summarize with iouType 'bbox' (the
 * COCO detection metric), restated in DESIGN §1c, for n_classes x n_images segments, class-major: segment
 * s = k*n_images + i (k-th of the ground truth's sorted category ids, i-th of its sorted image ids) owns
 * det[det_off[s]:det_off[s+1]] (file order: [x, y, w, h] and score, as the results file holds them; loadRes's
 * area w*h and iscrowd 0 are implied) and gt[gt_off[s]:gt_off[s+1]] ([x, y, w, h], the annotation's own area field,
 * iscrowd; ignore = iscrowd).  Per segment: the first 100 detections by stable -score, f64 box IoU (maskApi.c bbIou,
 * a crowd box's union the detection's area), evaluateImg's greedy match at iouThrs = linspace(.5, .95, 10) for the
 * area ranges all / small / medium / large (0, 32^2, 96^2, 1e10); per (class, area, maxDets in {1, 10, 100})
 * accumulate's cumulative TP / FP, recall and the precision envelope at recThrs = linspace(0, 1, 101).
 * precision_out [10, 101, n_classes, 4, 3] and recall_out [10, n_classes, 4, 3] (-1: no ground truth that counts;
 * either may be NULL); stats_out [12]: summarize's AP, AP50, AP75, AP small / medium / large, AR1, AR10, AR100,
 * AR small / medium / large (NumPy's mean of the entries > -1, or -1).  dt_match_out [4, 10, D] int32 / dt_ignore_out
 * [4, 10, D] int8, both or neither, in input order per (area, threshold): the matched box's position in its segment's
 * ground truth (-1: none) and dtIgnore (-1 for both: past the segment's first 100, not evaluated).
 * Malformed offsets are AZ_ERR_INVALID and n_classes*n_images past int32 is AZ_ERR_CAPACITY, both before any device
 * work.  Device scratch is kept in the context. */
int az_coco_eval(az_ctx *ctx, int n_classes, int n_images,
                 const double *det_box, const double *det_score, const int32_t *det_off,
                 const double *gt_box, const double *gt_area, const uint8_t *gt_crowd, const int32_t *gt_off,
                 double *precision_out, double *recall_out, double *stats_out,
                 int32_t *dt_match_out, int8_t *dt_ignore_out);

/* ---- proposal diagnosis (what lib/detect/tune.py:368-419 records AZ_results.mat for) --------------------------- */
/* The offline analysis of a proposal run, restated in DESIGN §4, "Proposal diagnosis", for n_images images in one call.  Image i owns
 * anchors[anc_off[i]:anc_off[i+1]] (f64 [.,4]: the search's anchor history `Bhis`, tune.py:299) with the zoom score
 * (f32) and the search level (int32, 0 = the root level) of each, gt[gt_off[i]:gt_off[i+1]] (f64 [.,4]) and
 * props[prop_off[i]:prop_off[i+1]] (f64 [.,4], in rank order as the search returns them, tune.py:309-311); n_anchors,
 * n_gt, n_props are the row counts the offsets must end at.  cuts[n_cuts] (n_cuts <= 16): ascending proposal budgets;
 * area_edges[2]: an object is small below area_edges[0], medium below area_edges[1], else large, by
 * area = (x2-x1+1)*(y2-y1+1).  Every output may be NULL:
 *   anchor_label_out [A] u8      _compute_zoom_labels of the anchor against its image's objects (roidb.py:313-341,
 *                                lib/utils/bbox.pyx:20-60) at max_area_ratio = emb_reg_thresh, min_obj = emb_obj_thresh
 *   level_table_out [AZ_MAX_LEVELS][4] i64   per level: anchors, zoomed, labelled, zoomed and labelled; zoomed is
 *                                (double)zoom >= (level == 0 ? 0.0 : tz) (tune.py:282, 296, 306)
 *   gt_best_iou_out [G] f64 / gt_best_rank_out [G] i32   the largest bbox_overlaps IoU (bbox.pyx:132-172) of the object
 *                                with its image's proposals and the rank of its first maximum; 0.0 / -1 without proposals
 *   gt_first_hit_out [G] i32     the smallest rank with IoU >= iou_thresh, or -1
 *   gt_deepest_level_out [G] i32 the largest level of an anchor of the image that holds the object (iw > 0, ih > 0,
 *                                iw*ih / (gt_area + 1e-14) >= emb_obj_thresh: bbox.pyx:48-58 without the area-ratio gate), or -1
 *   recall_table_out [n_cuts + 1][4] i64   row c: objects with 0 <= first_hit < cuts[c]; the last row: all objects;
 *                                columns all / small / medium / large
 *   kernel_ms_out [1] f32        device time of the two launches (two events around them)
 * Malformed offsets (negative, descending, or not ending at the row counts), a level outside [0, AZ_MAX_LEVELS),
 * descending cuts or n_cuts > 16 are AZ_ERR_INVALID and row counts past int32 AZ_ERR_CAPACITY, both before any device
 * work and with the outputs untouched.  Device scratch is kept in the context. */
int az_diag_eval(az_ctx *ctx, int n_images,
                 const double *anchors, const float *zoom, const int32_t *level, const int32_t *anc_off, long long n_anchors,
                 const double *gt, const int32_t *gt_off, long long n_gt,
                 const double *props, const int32_t *prop_off, long long n_props,
                 double tz, double emb_reg_thresh, double emb_obj_thresh, double iou_thresh,
                 const int32_t *cuts, int n_cuts, const double *area_edges,
                 uint8_t *anchor_label_out, int64_t *level_table_out, double *gt_best_iou_out, int32_t *gt_best_rank_out,
                 int32_t *gt_first_hit_out, int32_t *gt_deepest_level_out, int64_t *recall_table_out, float *kernel_ms_out);

/* ---- detection diagnosis (Hoiem et al., ECCV 2012; TIDE, Bolya et al., ECCV 2020) ------------------------------- */
/* Why a VOC evaluation's AP is what it is, restated in DESIGN §4, "Detection diagnosis", in one call over a whole set.
 * The segments, the ranking (stable -confidence per class) and the overlap are az_voc_eval's.  New inputs: bg_overlap
 * (Hoiem's 0.1), class_group[n_classes] (int32; NULL: every class is its own group), cuts[n_cuts] (f64, finite, ascending,
 * n_cuts <= 16).  Per detection d of segment (c, i), in input order; every output may be NULL:
 *   ov_same_out [D] f64 / arg_same_out [D] i32     the largest overlap with the segment's boxes (difficult ones too; pairs
 *                                with iw > 0 and ih > 0 only; the first maximum) and that box's position in the segment;
 *                                0.0 / -1 where nothing overlaps
 *   ov_other_out [D] f64 / other_class_out [D] i32 the same over image i's boxes of every class c' != c, the first maximum
 *                                in (class, position) order, and that box's class
 *   type_out [D] i8              the first that fits, in each class's rank order:
 *                                0 IGN  ov_same >= min_overlap and the box is difficult
 *                                1 TP   ... not difficult and unclaimed: the box is claimed (gt_claim = d)
 *                                2 DUP  ... not difficult and claimed already
 *                                3 LOC  ov_same >= bg_overlap
 *                                4 SIM  ov_other >= bg_overlap and class_group[c] == class_group[other_class]
 *                                5 OTH  ov_other >= bg_overlap, another group
 *                                6 BG   anything else
 *                                TP / IGN / the rest are az_voc_eval's match 1 / 0 / -1
 *   loc_fixed_out [D] u8         TIDE's rule, after the segment's matching: a LOC row, in rank order, is fixed when its
 *                                arg_same box is not difficult, no detection claimed it (a lower-ranked TP counts) and no
 *                                higher-ranked LOC row was fixed onto it
 *   gt_claim_out [G] i32         the input index of the detection that claimed the box, or -1
 * Per class:
 *   type_table_out [n_classes][7] i64   the count of each type
 *   miss_out [n_classes] i64     non-difficult boxes that nothing claimed;  npos_out [n_classes] i64: non-difficult boxes
 *   fp_at_out [n_classes][n_cuts][7] i64   the types of the class's first min(floor(cuts[k] * (double)npos), its
 *                                detections) detections in rank order
 *   ap_fix_out [n_classes][8] f64   the class's AP by k_voc_class's arithmetic (11-point with metric_07, else the area)
 *                                under 0 plain; 1 DUP rows removed (neither TP nor FP); 2 LOC rows: the fixed ones TP, the
 *                                others removed; 3 SIM / 4 OTH / 5 BG removed; 6 missed objects removed (npos = the TP
 *                                count; no TP: NaN under the area metric); 7 all of these (npos = TP + fixed rows)
 *   kernel_ms_out [1] f32        device time of the launches (two events around them)
 * Offsets are validated as az_voc_eval validates them (same codes); a NaN threshold, bg_overlap < 0,
 * bg_overlap > min_overlap, n_cuts > 16 and negative, NaN, infinite or descending cuts are AZ_ERR_INVALID; all before any device
 * work and with the outputs untouched.  After AZ_ERR_HIP the per-detection and per-box outputs are undefined (the
 * per-class tables are written only on success).  D = 0 and G = 0 are valid.  Device scratch is kept in the context (the slot
 * az_voc_eval uses: the two never overlap). */
int az_det_diag_eval(az_ctx *ctx, int n_classes, int n_images,
                     const double *det_box, const double *det_conf, const int32_t *det_off,
                     const double *gt_box, const uint8_t *gt_difficult, const int32_t *gt_off,
                     double min_overlap, double bg_overlap, int metric_07,
                     const int32_t *class_group, const double *cuts, int n_cuts,
                     int8_t *type_out, double *ov_same_out, int32_t *arg_same_out,
                     double *ov_other_out, int32_t *other_class_out, uint8_t *loc_fixed_out,
                     int32_t *gt_claim_out, int64_t *type_table_out, int64_t *miss_out,
                     int64_t *fp_at_out, int64_t *npos_out, double *ap_fix_out, float *kernel_ms_out);

/* The same diagnosis under the COCO protocol, restated in DESIGN §4, "Detection diagnosis, COCO protocol": why
 * az_coco_eval's AP@[.5:.95] is what it is.  The inputs are az_coco_eval's (class-major (category, image) segments, xywh
 * f64 boxes, det_score, gt_area, gt_crowd) plus bg_overlap and class_group[n_classes] (int32; NULL: every class is its
 * own group).  Fixed settings: area range ALL, maxDets 100, each of the ten thresholds thr = linspace(.5, .95, 10); the
 * per-area-range diagnosis (AP small / medium / large with fixes) and the cut table of az_det_diag_eval (fp_at) are out of
 * scope.  The ranking, the IoU (maskApi's bbIou) and the matching are az_coco_eval's, instruction for instruction.  A box
 * COUNTS when it is not a crowd box and its area field lies in [0, 1e10] (COCOeval's gtIgnore = 0 in area range all);
 * wherever "non-crowd" is said below, such boxes are meant.  Every output may be NULL.
 * Per detection d of segment (k, i), in input order, among the segment's first 100 by stable -score (past them: 0.0 / -1):
 *   ov_same_out [D] f64 / arg_same_out [D] i32     the largest IoU with the segment's non-crowd boxes (pairs with w > 0 and
 *                                h > 0 only; the first maximum in position order) and that box's position in the segment;
 *                                0.0 / -1 where nothing overlaps.  They do not depend on the threshold
 *   ov_other_out [D] f64 / other_class_out [D] i32 the same over image i's non-crowd boxes of every other category, the
 *                                first maximum in (category, position) order, and that box's category
 *   type_out [10][D] i8          per threshold t the first rule that fits:
 *                                -1      past the segment's first 100: not evaluated (as dt_match_out's -1)
 *                                0 IGN   evaluateImg matched it to a crowd box, or it is unmatched and its area w*h lies
 *                                        outside [0, 1e10]: exactly az_coco_eval's dtIgnore for area range all
 *                                1 TP    evaluateImg matched it to a non-crowd box m: gt_claim[t][m] = d; m is
 *                                        az_coco_eval's dt_match_out[0][t][d]
 *                                2 DUP   unmatched and ov_same >= thr[t] (every such box is taken already)
 *                                3 LOC   unmatched and ov_same >= bg_overlap
 *                                4 SIM   unmatched, ov_other >= bg_overlap, class_group[k] == class_group[other_class]
 *                                5 OTH   unmatched, ov_other >= bg_overlap, another group
 *                                6 BG    anything else
 *   loc_fixed_out [10][D] u8     TIDE's rule, after the segment's matching at t: a LOC row, in rank order, is fixed when
 *                                no detection claimed its arg_same box at t (a lower-ranked TP counts) and no higher-ranked
 *                                LOC row was fixed onto that box at t
 * Per box:   gt_claim_out [10][G] i32   the input index of the detection that claimed the box at t, or -1 (crowd boxes: -1)
 * Per class: npos_out [K] i64           non-crowd boxes
 *            type_table_out [K][10][7] i64   the count of each type at t
 *            miss_out [K][10] i64       non-crowd boxes unclaimed at t
 * The curves: prec_fix_out [8][10][101][K] f64 / recall_fix_out [8][10][K] f64 -- accumulate's interpolated precision at
 * recThrs = linspace(0, 1, 101) and its final recall for (k, area all, maxDets 100), in k_coco_acc's arithmetic
 * (np.spacing(1) in the precision, the envelope, searchsorted(.., 'left'), -1 where the variant's npig is 0), under
 *   0 plain (az_coco_eval's precision[:, :, :, 0, 2]);  1 DUP rows ignored;  2 fixed LOC rows count as TP, the other LOC rows
 *   are ignored;  3 SIM / 4 OTH / 5 BG rows ignored;  6 missed objects removed (npig = the TP count at t);  7 all of
 *   these (npig = TP + fixed rows at t).
 * The means (AP, AP50, AP75 per variant) are summarize's np.mean(s[s > -1]) and are taken by the caller.
 *   kernel_ms_out [1] f32        device time of the launches (two events around them)
 * Offsets are validated as az_coco_eval validates them (same codes); a NaN or negative bg_overlap or bg_overlap > 0.5 is
 * AZ_ERR_INVALID; all before any device work and with the outputs untouched.  After AZ_ERR_HIP the per-detection and
 * per-box outputs are undefined (the tables and curves are written only on success).  D = 0 and G = 0 are valid.  Device
 * scratch is kept in the context (the slot az_coco_eval uses: calls are synchronous, the two never overlap). */
int az_coco_diag_eval(az_ctx *ctx, int n_classes, int n_images,
                      const double *det_box, const double *det_score, const int32_t *det_off,
                      const double *gt_box, const double *gt_area, const uint8_t *gt_crowd, const int32_t *gt_off,
                      double bg_overlap, const int32_t *class_group,
                      double *ov_same_out, int32_t *arg_same_out, double *ov_other_out, int32_t *other_class_out,
                      int8_t *type_out, uint8_t *loc_fixed_out, int32_t *gt_claim_out,
                      int64_t *npos_out, int64_t *type_table_out, int64_t *miss_out,
                      double *prec_fix_out, double *recall_fix_out, float *kernel_ms_out);

/* ---- image front-end (_get_image_blob, lib/detect/test.py:27-59) ------------------------- */
/* uint8 BGR HWC image (host) -> float32 [3, oh, ow] blob: subtract cfg.PIXEL_MEANS, then
 * cv2.resize(fx=fy=scale, INTER_LINEAR) semantics on f32 (half-pixel centres, edge clamp,
 * horizontal pass then vertical pass).  oh/ow must come from az_image_blob_size
 * (cv2's dsize = round-half-even(dim * scale)).  _dev writes to a device pointer (e.g. the
 * torch tensor the backbone reads), _host to a host array. */
int az_image_blob_size(int h, int w, double scale, int *oh, int *ow);
int az_image_blob_host(az_ctx *ctx, const uint8_t *im, int h, int w, const float *means,
                       double scale, float *blob_out, int oh, int ow);
int az_image_blob_dev(az_ctx *ctx, const uint8_t *im, int h, int w, const float *means,
                      double scale, float *blob_dev, int oh, int ow);

/* As az_image_blob_dev, as ONE step of a pipelined harness: the upload and the kernel are only enqueued -- on `stream`
 * (a hipStream_t, e.g. the stream the backbone runs on; NULL: the ctx stream -- the DEFAULT stream, whose handle is also 0, is
 * passed as hipStreamLegacy, (hipStream_t)1) -- and the call returns; `im` is copied to
 * pinned staging before that, so the caller's array may be reused at once.  Whatever is enqueued on `stream` afterwards
 * (the backbone) finds the blob complete; nothing else is synchronised. */
int az_image_blob_dev_on(az_ctx *ctx, const uint8_t *im, int h, int w, const float *means, double scale,
                         float *blob_dev, int oh, int ow, void *stream);

/* ---- backbone epilogues (context-free; `stream`: a hipStream_t, NULL = the default stream) -------------------- */
/* What follows a VGG16 convolution (models/Pascal/VGG16/az-net/test.prototxt:16-384: Convolution with bias, ReLU in
 * place; Pooling MAX 2x2 / 2, Caffe's ceil mode) in ONE pass over the convolution's output, which PyTorch-ROCm produces
 * without the bias (F.conv2d(x, w, None)): y = max(y + bias[c], 0) in place -- channels_last != 0: y is [hw][C] (C % 4 == 0,
 * 16-byte aligned), else [C][hw].  PyTorch's own bias add and ReLU are two element-wise launches over the same bytes;
 * same fp32 operations, same bits. */
int az_bias_relu(void *stream, float *y, const float *bias, int C, long long hw, int channels_last);
/* The same followed by the 2x2 / 2 max-pool: y [H][W][C] (channels_last != 0: C % 4 == 0, 16-byte aligned) or [C][H][W]
 * -> out [ceil(H/2)][ceil(W/2)][C] / [C][ceil(H/2)][ceil(W/2)]; the last window row / column is clipped by the map's edge
 * (ceil mode).  out = max over the window of max(y + bias, 0), computed as max(max(y) + bias, 0): the same bits (rounding
 * is monotonic). */
int az_bias_relu_pool(void *stream, const float *y, const float *bias, float *out, int C, int H, int W, int channels_last);

/* ---- training data layer (lib/az_data_layer/roidb.py) -------------------------------------------- */
#define AZ_TRAIN_MAX_REGIONS 16   /* rows of cfg.TRAIN.ADDREGIONS / cfg.SEAR.SUBREGION a call may carry */
/* The cfg keys the training kernels read: SEAR.MIN_SIDE, SEAR.TRAIN_REP, SEAR.ZOOM_ERR_PROB, SEAR.EMB_OBJ_THRESH,
 * SEAR.EMB_REG_THRESH, SEAR.ADJ_THRESH, EPS, TRAIN.ADDREGIONS, SEAR.SUBREGION (lib/detect/config.py:91-195). */
typedef struct {
    double min_side, zoom_err_prob, emb_obj_thresh, emb_reg_thresh, adj_thresh, eps;
    int32_t train_rep, n_addregions, n_subregion, reserved;
    double addregions[AZ_TRAIN_MAX_REGIONS][4];
    double subregion[AZ_TRAIN_MAX_REGIONS][4];
} az_train_params;

/* _compute_zoom_labels (roidb.py:313-341 over bbox_zoom_labels, lib/utils/bbox.pyx:20-60): labels_out[r] = 1 when
 * some object n has area(gt_n) / (area(roi_r) + 1e-14) <= max_area_ratio and intersection / (area(gt_n) + 1e-14)
 * >= min_obj.  rois f64 [R,4], gt f64 [N,4] (N = 0: all 0). */
int az_zoom_labels(az_ctx *ctx, const double *rois, int R, const double *gt, int N, double max_area_ratio,
                   double min_obj, uint8_t *labels_out);
/* _compute_ex_rois (roidb.py:230-299) for n_images images in ONE launch: image i has sizes[i] = (h, w) and the objects
 * gt[gt_off[i]:gt_off[i+1]] (f64 [.,4]).  Per image, train_rep zoom searches from the addregions roots over
 * int(log2(min(h, w) / min_side) + 1) levels -- zoom labels, `err = noise <= zoom_err_prob` on the next |B| doubles of
 * `noise`, divide_region of the regions with label XOR err -- then every object's n_subregion super-regions
 * (roidb.py:270-289), clipped to the image, sides >= min_side kept, in the reference's order.  The images consume ONE
 * stream: image i + 1 starts where image i stopped (the position lives on the device).
 * ex_boxes_out f32 [cap,4] (the f64 box rounded once, roidb.py:65), zoom_out [cap], ex_off_out [n_images + 1],
 * noise_used_out [n_images].  AZ_ERR_CAPACITY, and nothing in the outputs, when `noise` runs out (needed_out[0] = the
 * doubles needed at the level that ran out; how many more the rest needs depends on the noise itself) or the regions
 * outgrow `cap` (needed_out[1] = their exact number), or a level holds more than 4096 children before the dedup
 * (needed_out both zero: no larger buffer helps); AZ_ERR_INVALID when a child's _sift_dup hash
 * round(box / min_side) . [1, 1e3, 1e6, 1e9] leaves [0, 2^40), i.e. y2 / min_side reaches 1100 or the sum is negative.
 * needed_out [2] is zero otherwise.  After either error the context is usable as before. */
int az_train_ex_rois(az_ctx *ctx, const az_train_params *p, int n_images, const int32_t *sizes, const double *gt,
                     const int32_t *gt_off, const double *noise, long long n_noise, float *ex_boxes_out,
                     uint8_t *zoom_out, int32_t *ex_off_out, int cap, long long *noise_used_out, long long *needed_out);
/* _compute_targets (roidb.py:146-227) for n_images images: image i owns ex_boxes[ex_off[i]:ex_off[i+1]] and
 * gt[gt_off[i]:gt_off[i+1]], both the roidb's f32, widened to f64.  Per example region k with max IoU >= adj_thresh:
 * the sub-regions (x2 - x1, y2 - y1) * subregion + (x1, y1), their IoU with every object, the objects whose IoU with
 * sub-region 0 is below adj_thresh retired, then min(n_subregion, objects left) rounds of: the first maximum in
 * row-major order (a maximum of 0 still matches), one row (dx, dy, dw, dh, k within its image, sub-region,
 * IoU(region, object)), that sub-region and object retired.  targets_out f64 [cap,7] ordered by image, k, round;
 * tgt_off_out [n_images + 1].  AZ_ERR_CAPACITY with tgt_off_out filled (tgt_off_out[n_images] = rows needed) and no
 * rows written when cap is too small; AZ_ERR_CAPACITY before any launch (tgt_off_out[n_images] left 0) when an image's
 * n_subregion x objects f64 matrix exceeds 128 KB of LDS: 1489 objects at 11 sub-regions, 1024 at 16. */
int az_train_adj_targets(az_ctx *ctx, const az_train_params *p, int n_images, const float *ex_boxes,
                         const int32_t *ex_off, const float *gt, const int32_t *gt_off, double *targets_out,
                         int32_t *tgt_off_out, int cap);
/* roidb.py:110-134 over T target rows: per sub-region (column 5) counts + eps, sums and squared sums of columns 0-3
 * in a fixed two-level order (the same bits on every run), means = sums / counts, stds = sqrt(sq / counts - means^2)
 * -> means_out / stds_out [n_sub * 4]; normalise_in_place != 0: every row's columns 0-3 -> (x - mean) / std.  A row
 * belongs to sub-region c when column 5 == c exactly (roidb.py:119, 132): rows with any other value there (negative,
 * >= n_sub, not an integer) enter no statistic and are not normalised.  1 <= n_sub <= AZ_TRAIN_MAX_REGIONS, else
 * AZ_ERR_INVALID.  An absent sub-region has nan statistics at eps 0, a sub-region of identical rows std 0 and nan rows,
 * as NumPy has them. */
int az_train_target_stats(az_ctx *ctx, int n_sub, double eps, double *targets, long long T, double *means_out,
                          double *stds_out, int normalise_in_place);

/* ---- AZ-net training from conv5_3 on (models/Pascal/VGG16/az-net/train.prototxt, lib/detect/train_az.py) ------------------ */
/* Replaces caffe.SGDSolver(solver_prototxt) and solver.step(1) (train_az.py:41,106) for everything behind conv5_3: the layers
 * roi_pool5 (ROIPooling 7x7, 1/16) -> int6 -> {int7_1 -> adj_score, adj_bbox; int7_2 -> zoom_score} (InnerProduct, ReLU and
 * Dropout in place on int6 / int7_1 / int7_2), loss_zoom and loss_adj (SigmoidCrossEntropyLoss), loss_bbox (SmoothL1Loss with
 * adj_targets and adj_loss_weights), all with loss_weight 1 and normalised by the roi rows R.  The convolutions stay with the
 * caller (PyTorch-ROCm autograd): the step returns d loss / d conv5_3.  A trainer belongs to its az_ctx (az_destroy frees the
 * trainers still alive), runs on the ctx stream and is synchronous like every other call.  It holds fp32 master weights in
 * Caffe layout ([out][in]; roi_pool5 flattened c * 49 + p), one gradient and one momentum history per parameter, and the
 * activations of one step for up to max_rois rows.  The twelve parameters are always in az_load_head's order:
 *   W6 b6 W71 b71 W72 b72 Was bas Wab bab Wz bz.
 * fp32 throughout, GEMMs on v_mfma_f32_32x32x2_f32; no floating-point atomics and no scheduling-dependent order in any
 * reduction: the same step from the same state gives the same bits. */
typedef struct az_solver az_solver;
/* net.params as Caffe's fillers leave them (train.prototxt: gaussian std 1e-4, 1e-4, 1e-3, 1e-2, 1e-3, 1e-2 for int6, int7_1,
 * int7_2, adj_score, adj_bbox, zoom_score; biases 0), drawn from the generator below with `seed` (Box-Muller on the two 24-bit
 * halves of element e's word under layer id 16 + parameter index; Caffe's own RNG stream is not reproduced); history zero.
 * lr_mult / decay_mult start at 1 / 1 for weights and 2 / 0 for biases, the dropout ratios at 0.5.  C, n6 multiples of 4. */
int az_solver_create(az_ctx *ctx, int C, int n6, int n71, int n72, int max_rois, uint64_t seed, az_solver **out);
int az_solver_destroy(az_solver *s);
/* solver.net.copy_from(pretrained_model) (train_az.py:45) / net.params[...].data reads (train_az.py:56-61,71-80): host arrays
 * in Caffe layout; a NULL array is skipped. */
int az_solver_load(az_solver *s, const float *W6, const float *b6, const float *W71, const float *b71, const float *W72,
                   const float *b72, const float *Was, const float *bas, const float *Wab, const float *bab, const float *Wz,
                   const float *bz);
int az_solver_read(az_solver *s, float *W6, float *b6, float *W71, float *b71, float *W72, float *b72, float *Was, float *bas,
                   float *Wab, float *bab, float *Wz, float *bz);
/* param { lr_mult decay_mult } of the six layers ([12], parameter order) and dropout_ratio of int6, int7_1, int7_2 ([3], each
 * in [0, 1)) as train.prototxt states them; a NULL array keeps the current values. */
int az_solver_set_hyper(az_solver *s, const float *lr_mult, const float *decay_mult, const float *dropout_ratio);
/* net.forward() + net.backward() of one minibatch (Caffe Solver::Step before the update).  conv_dev: conv5_3 of N images on the
 * device, [N][C][H][W] (channels_last = 0) or [N][H][W][C] (1); rois [R][5] (batch index, x1, y1, x2, y2 in network-input
 * pixels), adj_labels [R][11], adj_targets [R][44], adj_loss_weights [R][44], zoom_labels [R]: host arrays, the blobs of
 * lib/az_data_layer/layer.py.  losses_out [3] = loss_zoom, loss_adj, loss_bbox; sumsq_out = the sum of squares of the twelve
 * parameter gradients (which stay on the device for az_solver_update); dmap_dev (may be NULL): d loss / d conv5_3, written over
 * a caller-owned device buffer of conv_dev's shape and layout.
 *   ROIPooling: az_roi_pool's arithmetic per roi on image batch_index, arg-max = first maximum in (h, w) scan order; backward:
 *     every pooled gradient to its arg-max cell (a gather over the rois in row order), empty bins send nothing.
 *   InnerProduct: y = x W^T + b; dx = dy W, dW = dy^T x, db = column sums in row order.  ReLU passes where its output is > 0.
 *   SigmoidCrossEntropyLoss: -1/R sum(x (t - [x >= 0]) - log(1 + exp(x - 2 x [x >= 0]))), dx = (sigmoid(x) - t) / R, t in [0, 1].
 *   SmoothL1Loss: d = w (x - t), f = 0.5 d^2 if |d| < 1 else |d| - 0.5, sum f / R; dx = w (d if |d| < 1 else sign d) / R.
 *   Dropout (ratio p, layer id L = 0 / 1 / 2 for int6 / int7_1 / int7_2, element e = row * width + column), all in uint64
 *   arithmetic modulo 2^64:
 *       mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *       key = mix(mix(mix(seed + 0x9E3779B97F4A7C15) + iteration) + L)
 *       keep(e) = (mix(key + 0x9E3779B97F4A7C15 * (e + 1)) >> 40) >= floor(p * 2^24);   y = keep ? x * (1 / (1 - p)) : 0
 *   with p the float32 of az_solver_set_hyper (0.3 is 0.300000012: floor(p * 2^24) = 5033165, not 5033164), p * 2^24 exact
 *   in double and 1 / (1 - p) in float32; p = 0: no mask is drawn, written or read.
 *   (Caffe's own RNG stream is not reproduced.)  The backward uses the same mask and scale.
 * Bad arguments (NULL arrays, R outside [1, max_rois], a batch index outside [0, N)) return AZ_ERR_INVALID before anything is
 * written. */
int az_solver_step(az_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                   const float *adj_labels, const float *adj_targets, const float *adj_loss_weights, const float *zoom_labels,
                   uint64_t seed, long long iteration, float *losses_out, double *sumsq_out, float *dmap_dev);
/* SGDSolver::ComputeUpdateValue + Net::Update for the head's parameters with the gradients of the last az_solver_step: per
 * element, one rounding per operation, g = clip_scale * g; g = g + (weight_decay * decay_mult) * w;
 * hist = momentum * hist + (rate * lr_mult) * g; w = w - hist.  The caller computes rate (lr_policy) and clip_scale
 * (clip_gradients / the L2 norm of ALL learnable gradients when that exceeds clip_gradients, else 1). */
int az_solver_update(az_solver *s, double rate, double momentum, double weight_decay, double clip_scale);
/* The same arithmetic on raw device pointers (n floats each; rate and decay already multiplied by the blob's lr_mult /
 * decay_mult): what the convolution parameters PyTorch owns are updated with. */
int az_sgd_update(az_ctx *ctx, float *w_dev, const float *g_dev, float *hist_dev, long long n, double rate, double momentum,
                  double decay, double clip_scale);
/* net.forward() in Caffe's TEST phase (dropout = identity) on the trainer's current weights: the raw zoom_score [R],
 * adj_score [R][11], adj_bbox [R][44] (host; any may be NULL). */
int az_solver_forward_test(az_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                           float *zoom_score, float *adj_score, float *adj_bbox);
/* net.blobs[...].data / .diff and net.params[...].diff of the last pass, for tests: pool5, argmax (int32: h * W + w in the roi's
 * map, -1 for an empty bin), pre6 / pre71 / pre72 (pre-activations), a6 / a71 / a72, mask6 / mask71 / mask72 (uint8),
 * adj_score, adj_bbox, zoom_score, d_adj_score, d_adj_bbox, d_zoom_score, d_pre6, d_pre71, d_pre72, d_pool5, and per parameter
 * P of the twelve: g_P (gradient), h_P (history), w_P (value).  out == NULL: only the size. */
int az_solver_fetch(az_solver *s, const char *name, void *out, long long cap_bytes, long long *bytes_out);
/* One product of the trainer's GEMM kernel on host arrays, for tests: d [M][N] = form 0: a [M][K] b[N][K]^T (forward);
 * 1: a [M][K] b [K][N] (dx); 2: a [K][M]^T b [K][N] (dW). */
int az_solver_gemm_unit(az_ctx *ctx, int form, const float *a, const float *b, float *d, int M, int N, int K);

/* ---- training precision (not in the reference; opt-in, default AZ_TRAIN_FP32) ---------------------------------------------- */
/* AZ_TRAIN_BF16: every matrix product of the trainer (all layers: forward, dx, dW; with a skip front attached also
 * conv_pool5's three) rounds BOTH operands to bf16, round to nearest even, as they are staged on chip, multiplies them on
 * the 16-bit matrix cores and sums in fp32.  Weights, activations, gradients and history stay fp32 in memory; pooling,
 * bias / ReLU / dropout, column sums, losses, the gradient norm, GRN and the update are unchanged.  May be called between
 * steps; the mode is read when a product is launched and nothing else is stored, so switching back leaves no trace.  Any
 * other value: AZ_ERR_INVALID, state unchanged.  fp32 denormal operands are outside the stated behaviour. */
#define AZ_TRAIN_FP32 0
#define AZ_TRAIN_BF16 1
int az_solver_set_precision(az_solver *s, int precision);
/* az_solver_gemm_unit in the given precision. */
int az_solver_gemm_unit_prec(az_ctx *ctx, int form, int precision, const float *a, const float *b, float *d, int M, int N, int K);

/* ---- detection-net training: the box-regression targets (lib/roi_data_layer/roidb.py) ------------------------------------ */
/* _compute_targets (roidb.py:149-207) for n_images images in ONE launch (a thread per example box, no host wait inside):
 * image i owns ex_boxes[ex_off[i]:ex_off[i+1]] (f32 [.,4] as the roidb stores them, widened to f64 as the reference's
 * astype(float) does) and the objects gt[gt_off[i]:gt_off[i+1]] (f32 [.,4]) with gt_labels (int32).  Per example box: the
 * maximum IoU over the image's objects (bbox_overlaps' arithmetic, f64) and the FIRST maximum's object.  Where the maximum is
 * >= bbox_thresh the row is [label, dx, dy, dw, dh] rounded to f32, in the reference's order: widths and heights + eps, the
 * centres from those, max(1, .) afterwards, dx = (tcx - pcx) / pw, dw = log(tw / pw); elsewhere the row is zero.
 * targets_out f32 [E][5], max_overlaps_out f64 [E].  An image without objects: zero rows and max_overlaps = the float32 of
 * bg_thresh_lo (roidb.py:160-163). */
int az_det_targets(az_ctx *ctx, int n_images, const float *ex_boxes, const int32_t *ex_off, const float *gt,
                   const int32_t *gt_labels, const int32_t *gt_off, double bbox_thresh, double bg_thresh_lo, double eps,
                   float *targets_out, double *max_overlaps_out);
/* roidb.py:119-145 over the set: targets f32 [E][5] (rows of image i: ex_off[i]:ex_off[i+1]).  Per image and class
 * 1 .. num_classes - 1 the float32 sums of t and of t * t (the square rounded to float32) over the rows with that label, in
 * row order (NumPy's axis-0 sum of a float32 array); those added into float64 across the images in image order, counts
 * starting at eps; means = sums / counts, stds = sqrt(squared sums / counts - means^2); class 0 keeps mean 0, std 0.
 * normalise_in_place != 0: every labelled row t = f32(f64(t) - mean), then t = f32(f64(t) / std); a std of 0 divides by 0 as
 * the reference does.  counts_out f64 [num_classes] (may be NULL), means_out / stds_out f64 [num_classes][4].  No atomics:
 * two runs give the same bits. */
int az_det_target_stats(az_ctx *ctx, int n_images, float *targets, const int32_t *ex_off, int num_classes, double eps,
                        int normalise_in_place, double *counts_out, double *means_out, double *stds_out);

/* ---- detection-net training from conv5_3 on (models/Pascal/VGG16/frcnn/train.prototxt, lib/detect/train_det.py) ----------- */
/* Replaces caffe.SGDSolver(solver_prototxt) and solver.step(1) (train_det.py:40,105) for everything behind conv5_3: roi_pool5
 * (ROIPooling 7x7, 1/16) -> fc6 -> fc7 (InnerProduct, ReLU, Dropout in place) -> {cls_score [num_classes], bbox_pred
 * [4 num_classes]}, loss_cls (SoftmaxWithLoss on labels) and loss_bbox (SmoothL1Loss with bbox_targets and bbox_loss_weights),
 * both with loss_weight 1 and normalised by the roi rows R.  Everything else is as az_solver states it: the convolutions stay
 * with the caller, fp32 master weights in Caffe layout, one gradient and one history per parameter, the same kernels, the same
 * fixed orders (the same step from the same state gives the same bits), synchronous calls on the ctx stream, freed with the
 * ctx.  The eight parameters are always in this order:  W6 b6 W7 b7 Wc bc Wb bb  (fc6, fc7, cls_score, bbox_pred). */
typedef struct az_det_solver az_det_solver;
/* The fillers of train.prototxt: gaussian std 0.01 for cls_score, 0.001 for bbox_pred; fc6 / fc7 come from the pretrained
 * model (az_det_solver_load) and start at gaussian std 0.005 without one; biases 0; history 0; drawn as az_solver_create
 * draws.  lr_mult / decay_mult start at 1 / 1 (weights) and 2 / 0 (biases), the two dropout ratios at 0.5.
 * C, n6, n7 positive multiples of 4 (what az_load_det_head accepts), 2 <= num_classes <= 256, 1 <= max_rois <= 4096. */
int az_det_solver_create(az_ctx *ctx, int C, int n6, int n7, int num_classes, int max_rois, uint64_t seed, az_det_solver **out);
int az_det_solver_destroy(az_det_solver *s);
/* solver.net.copy_from(pretrained_model) (train_det.py:44) / net.params[...].data reads and writes (train_det.py:49-54,70-96):
 * host arrays in Caffe layout; a NULL array is skipped. */
int az_det_solver_load(az_det_solver *s, const float *W6, const float *b6, const float *W7, const float *b7, const float *Wc,
                       const float *bc, const float *Wb, const float *bb);
int az_det_solver_read(az_det_solver *s, float *W6, float *b6, float *W7, float *b7, float *Wc, float *bc, float *Wb, float *bb);
/* param { lr_mult decay_mult } of the four layers ([8], parameter order) and dropout_ratio of fc6, fc7 ([2], each in [0, 1));
 * a NULL array keeps the current values. */
int az_det_solver_set_hyper(az_det_solver *s, const float *lr_mult, const float *decay_mult, const float *dropout_ratio);
/* AZ_TRAIN_FP32 / AZ_TRAIN_BF16, as az_solver_set_precision; covers az_det_solver_step_skip's conv_pool5 products as well. */
int az_det_solver_set_precision(az_det_solver *s, int precision);
/* net.forward() + net.backward() of one minibatch.  conv_dev, N, H, W, channels_last, rois [R][5], seed, iteration, sumsq_out
 * and dmap_dev as in az_solver_step (dropout layer ids: 0 = fc6, 1 = fc7); labels [R] (float, whole numbers in
 * [0, num_classes)), bbox_targets [R][4 num_classes], bbox_loss_weights [R][4 num_classes]: host arrays, the blobs of
 * lib/roi_data_layer/layer.py.  losses_out [2] = loss_cls, loss_bbox.
 *   SoftmaxWithLoss: p = exp(x - max x) / sum exp(x - max x) per row; loss = -1/R sum log(max(p[label], FLT_MIN));
 *     dx = (p - onehot(label)) / R.
 * A label outside [0, num_classes) (or any other bad argument) returns AZ_ERR_INVALID before anything is enqueued. */
int az_det_solver_step(az_det_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                       const float *labels, const float *bbox_targets, const float *bbox_loss_weights, uint64_t seed,
                       long long iteration, float *losses_out, double *sumsq_out, float *dmap_dev);
/* az_solver_update's arithmetic on the eight parameters with the gradients of the last az_det_solver_step. */
int az_det_solver_update(az_det_solver *s, double rate, double momentum, double weight_decay, double clip_scale);
/* net.forward() in the TEST phase (dropout = identity; models/Pascal/VGG16/frcnn/test.prototxt) on the trainer's current
 * weights: cls_prob [R][num_classes] (softmax) and the raw bbox_pred [R][4 num_classes] (host; either may be NULL). */
int az_det_solver_forward_test(az_det_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois,
                               int R, float *cls_prob, float *bbox_pred);
/* Saved tensors of the last pass, for tests: pool5, argmax, pre6, a6, mask6, pre7, a7, mask7 (uint8), cls_score, cls_prob,
 * bbox_pred, d_cls_score, d_bbox_pred, d_pre7, d_pre6, d_pool5, and per parameter P of the eight g_P, h_P, w_P.
 * out == NULL: only the size. */
int az_det_solver_fetch(az_det_solver *s, const char *name, void *out, long long cap_bytes, long long *bytes_out);

/* ---- training the skip-connection detector (models/COCO/VGG16_skip/frcnn/finetune/train.prototxt, frozen/train.prototxt) ---- */
/* The trainer above with the skip front in place of roi_pool5: roi_pool3 / roi_pool4 / roi_pool5 (ROIPooling 7x7 of conv3_3,
 * conv4_3, conv5_3, each at its own spatial_scale), roi_norm3/4/5 (GRN, as az_load_skip_front states it), concat5, scale5
 * (Power, scale = gain) and conv_pool5 + relu_pool (1x1 Convolution sum Cs -> C with bias, xavier filler); fc6 .. loss_cls /
 * loss_bbox behind it are az_det_solver_step's.  Same argument checks as az_load_skip_front; Cout is the trainer's C.
 * Allocates cat, arg-max, d_cat and d_raw ([max_rois * 49][sum Cs], 4 bytes each: the backward needs them whole) and the
 * parameters Wp [C][sum Cs] (uniform in +-sqrt(3 / sum Cs) from `seed`, drawn on the device) and bp [C] (0) with gradient
 * and history; lr_mult / decay_mult 1 / 1 and 2 / 0.  max_rois * 49 * sum Cs must fit in 31 bits (AZ_ERR_INVALID).  One front
 * per trainer (a second attach: AZ_ERR_STATE).  An error leaves the trainer as it was; a trainer without a front, and
 * az_det_solver_step on one with a front, compute exactly what they did before. */
int az_det_solver_attach_skip(az_det_solver *s, int n_src, const int *Cs, const float *spatial_scales, double gain, double eps,
                              uint64_t seed);
/* net.params['conv_pool5'][0 / 1].data (train_det.py:44,70-96): host Wp [C][sum Cs], bp [C]; a NULL array is skipped. */
int az_det_solver_load_skip(az_det_solver *s, const float *Wp, const float *bp);
int az_det_solver_read_skip(az_det_solver *s, float *Wp, float *bp);
/* param { lr_mult decay_mult } of conv_pool5 ([2]: weight, bias); a NULL array keeps the current values. */
int az_det_solver_set_skip_hyper(az_det_solver *s, const float *lr_mult, const float *decay_mult);
/* net.forward() + net.backward() of one minibatch of the skip train net.  maps_dev[i]: device map [N][Cs[i]][Hs[i]][Ws[i]]
 * (all NCHW or all channels-last); Cs must be the attached front's; rois [R][5] with the image index in column 0; the other
 * arguments as az_det_solver_step.  dmaps_dev: NULL, or n_src device buffers of the maps' shapes and memory format that
 * receive d loss / d map; a NULL entry gives no gradient for that source; wholly NULL: the backward stops at conv_pool5's
 * parameters.  sumsq_out: the sum of squares of all ten gradients (the head's eight, then Wp, bp).  The backward:
 *   d_y[(r,p)][j] = d_pool5[r][j*49+p] where pool5 > 0;  g_Wp = d_y^T cat;  g_bp = column sums;  d_cat = d_y Wp;
 *   GRN + scale, per (row, source): d_raw[c] = f (d_cat[c] - x[c] (sum_c x[c] d_cat[c]) / (ss + eps)), f = gain / sqrt(ss + eps),
 *     0 where ss + eps == 0;  ROIPooling backward: each d_raw to its arg-max cell (the first maximum in row-major window
 *     order), gathered per map cell over the rois in row order and the bins in bin order.
 * No floating-point atomics: the same step from the same state gives the same bits.  Refused before anything is enqueued: no
 * attached front (AZ_ERR_STATE); another n_src or other channel counts, a null map, a roi naming an image >= N, a bad label
 * (AZ_ERR_INVALID). */
int az_det_solver_step_skip(az_det_solver *s, int n_src, const int *Cs, const void *const *maps_dev, const int *Hs, const int *Ws,
                            int N, int channels_last, const float *rois, int R, const float *labels, const float *bbox_targets,
                            const float *bbox_loss_weights, uint64_t seed, long long iteration, float *losses_out,
                            double *sumsq_out, void *const *dmaps_dev);
/* net.forward() of the skip net in the TEST phase on the trainer's current weights (az_det_solver_forward_test's twin). */
int az_det_solver_forward_test_skip(az_det_solver *s, int n_src, const int *Cs, const void *const *maps_dev, const int *Hs,
                                    const int *Ws, int N, int channels_last, const float *rois, int R, float *cls_prob,
                                    float *bbox_pred);
/* az_det_solver_update also updates Wp / bp when the last gradients came from az_det_solver_step_skip.  az_det_solver_fetch
 * also knows, once a front is attached: cat, skip_argmax (int32), d_cat, d_raw ([R*49][sum Cs]), skip_factor (f64
 * [R*49][n_src]), d_y ([R*49][C]), g_Wp, g_bp, h_Wp, h_bp, w_Wp, w_bp.  d_cat and d_raw exist only behind a step that was asked
 * for a map gradient (otherwise AZ_ERR_STATE). */
/* Unit entry (tests): roi_pool3/4/5 forward with arg-max on host maps [N][Cs[i]][Hs[i]][Ws[i]] (or channels-last) and host
 * rois, then the ROIPooling backward gather of the host d_raw [R*49][sum Cs].  pooled_out (the raw maxima) and argmax_out are
 * [R*49][sum Cs]; dmaps_out[i] has map i's shape; any output (and d_raw with dmaps_out) may be NULL. */
int az_skip_pool_bwd_unit(az_ctx *ctx, int n_src, const int *Cs, const float *spatial_scales, const float *const *maps_host,
                          const int *Hs, const int *Ws, int N, int channels_last, const float *rois, int R,
                          const float *d_raw_host, float *pooled_out, int32_t *argmax_out, float *const *dmaps_out);

/* ---- online hard-example mining (Shrivastava et al., CVPR 2016; not in the reference) ------------------------------------------ */
/* One call mines one minibatch: the TEST-phase forward of az_det_solver_forward_test (dropout = identity, the trainer's
 * current precision) over all R pool rows, one loss per row, per image greedy NMS over the rows with the loss as score, and
 * the first per_image survivors of every image.  Nothing but the selection leaves the device.
 *   rois [R][5] as az_det_solver_step takes them; column 0 (the image index) must not decrease: image i owns the rows that
 *     name it (possibly none).  labels [R]: whole numbers in [0, num_classes).  targets [R][4]: the normalised deltas of each
 *     row's own class (ignored where the label is 0); NULL: no box term (TRAIN.BBOX_REG off).
 *   loss_r = cls_r + bbox_r in float32:
 *     cls_r = -logf(max(p[label], FLT_MIN)), p = exp(x - max x) / sum exp(x - max x) as az_det_solver_step computes it;
 *     bbox_r = ((f0 + f1) + f2) + f3 for label > 0, f_q = 0.5 d d if |d| < 1 else |d| - 0.5, d = bbox_pred[r][4 label + q] -
 *     targets[r][q] (SmoothL1Loss with weight 1, not divided by R); 0 for label 0.
 *   Selection, per image: az_nms's kernels, arithmetic and order on the records [x1, y1, x2, y2, loss_r] (the rois' float32
 *     columns 1..4) with nms_thresh: rows visited by descending loss, of equal losses the higher index first; a row is dropped
 *     when its IoU with a kept row is >= nms_thresh (so nms_thresh > 1 keeps every row).  sel_out [N * per_image] receives,
 *     image by image and packed, the first min(per_image, kept) kept rows as indices into the R rows; n_sel_out [N] their
 *     numbers.  row_loss_out [R] (may be NULL): the losses.
 * Afterwards the trainer is as after az_det_solver_forward_test (an az_det_solver_update without a new step is refused);
 * parameter gradients, history and the accumulate flag are untouched, so mining between two accumulating steps is safe.
 * az_det_solver_fetch also knows mine_loss, mine_loss_cls, mine_loss_bbox (f32 [R]), mine_keep (int32 [R]: image i's whole keep
 * list, before the cut at per_image, from its first row on; -1 behind it) and mine_nkeep (int32 [N]).
 * AZ_ERR_INVALID before anything is enqueued: what az_det_solver_forward_test refuses, a null labels / sel_out / n_sel_out,
 * per_image < 1, nms_thresh negative or not finite, a label that is no class, a decreasing image index.  AZ_ERR_STATE:
 * az_det_solver_mine on a trainer with a skip front, az_det_solver_mine_skip on one without.  A row whose loss, or whose sum of
 * exponentials, is not finite (a NaN score, which the FLT_MIN clamp would turn into a finite loss; found after the pass through a
 * device flag): AZ_ERR_INVALID, sel_out and n_sel_out untouched.  The same call from the same
 * state gives the same bits. */
int az_det_solver_mine(az_det_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                       const float *labels, const float *targets, double nms_thresh, int per_image, int32_t *sel_out,
                       int32_t *n_sel_out, float *row_loss_out);
/* The same behind the skip front (az_det_solver_forward_test_skip's forward). */
int az_det_solver_mine_skip(az_det_solver *s, int n_src, const int *Cs, const void *const *maps_dev, const int *Hs, const int *Ws,
                            int N, int channels_last, const float *rois, int R, const float *labels, const float *targets,
                            double nms_thresh, int per_image, int32_t *sel_out, int32_t *n_sel_out, float *row_loss_out);

/* ---- gradient accumulation and the solver's state between two iterations (all three trainers, both precisions) ------------ */
/* Caffe's iter_size (Solver::Step: `for (int i = 0; i < param_.iter_size(); ++i) loss += net_->ForwardBackward();` after one
 * ClearParamDiffs, then SGDSolver::ApplyUpdate: ClipGradients on the summed diffs, then Normalize scales them by
 * 1 / iter_size, then Regularize and ComputeUpdateValue).  on = 0 (the default): a step overwrites the parameter gradients,
 * with the launches and arguments it always had.  on = 1: every following *_step / *_step_skip ADDS its parameter gradients
 * to what the trainer holds, per element  g = g_old + g_step  with one float32 add, where g_step has the bits the same step
 * writes with the flag off: a split-K product is out[e] + (its slabs in slab order), an unsplit one *d + v, a bias gradient
 * the rows summed in row order and then added once; conv_pool5's Wp / bp included.  The gradients are zero after create, so
 * accumulating from the first step on gives 0 + g_step.  d conv5_3 and the skip front's map gradients stay those of the one
 * step (the caller's autograd accumulates in the convolutions' .grad).  sumsq_out is over the gradient buffers as they
 * stand, i.e. of the accumulated gradient: what ClipGradients looks at.  The caller divides by iter_size through
 * *_update's clip_scale.  *_update and *_forward_test leave the flag alone.  Any other value: AZ_ERR_INVALID, flag unchanged. */
int az_solver_set_accumulate(az_solver *s, int on);
int az_det_solver_set_accumulate(az_det_solver *s, int on);
/* SGDSolver::RestoreSolverStateFrom*: the momentum history (history_[i]) of every parameter from host arrays, in the order
 * and layout of *_load / *_load_skip; a NULL array keeps what the trainer holds.  Reading it back is *_fetch("h_<name>").
 * Gradients and the "a step has run" state are untouched (an update still needs a step before it).  Without an attached
 * front az_det_solver_load_skip_history returns AZ_ERR_STATE. */
int az_solver_load_history(az_solver *s, const float *W6, const float *b6, const float *W71, const float *b71, const float *W72,
                           const float *b72, const float *Was, const float *bas, const float *Wab, const float *bab,
                           const float *Wz, const float *bz);
int az_det_solver_load_history(az_det_solver *s, const float *W6, const float *b6, const float *W7, const float *b7,
                               const float *Wc, const float *bc, const float *Wb, const float *bb);
int az_det_solver_load_skip_history(az_det_solver *s, const float *Wp, const float *bp);

/* ---- measurement ------------------------------------------------------------------ */
/* HIP-event timing (events on the ctx stream) of the launches made by az_propose /
 * az_head_forward.  mode bits: 1 = time only the fc GEMM launches, 2 = time every launch
 * group, 4 = keep accumulating across calls until read (otherwise each call starts afresh);
 * 8 = the fp32 fc GEMM launches time THEMSELVES instead (first workgroup in to last workgroup out on the GPU's constant
 * 100 MHz clock, written by the kernels: no event pair on the stream -- an event pair costs ~7 us of stream time and, with
 * two lanes, also spans the time a launch waits for the other lane's GEMM to release the CUs); 32768 launches per call of
 * az_set_profiling, which resets them; 16 (with 8, after a call with 8) = forget the spans recorded so far without
 * touching the GPU -- no stream synchronisation, no copy: what to call right in front of a region to be timed;
 * 0 = off.  names_out: `cap` slots of 32 chars. */
int az_set_profiling(az_ctx *ctx, int mode);
int az_last_kernel_times(az_ctx *ctx, char *names_out, float *ms_out, int32_t *level_out,
                         int cap, int *n_out);
/* Replay az_propose's launch sequence as a hipGraph (captured once per parameter set and feature map;
 * every size is read on the device, so the sequence is fixed).  Same results; the GPU time does not
 * change, the host time inside az_propose_launch drops from ~110 us to ~17 us.  Default: the
 * AZ_GRAPH environment variable (off).  Ignored while kernel timing (az_set_profiling) is on. */
int az_set_graphs(az_ctx *ctx, int on);
/* What the context chooses between the forms of a search by (level by level / pair speculation / one whole-tree pass;
 * all give the same bits): the cost in us of ONE head pass (RoIPool + int6 + reduce + int7 + heads) at a few row counts,
 * ascending, linearly interpolated.  By default the context measures the table on its device the first time a search is
 * launched (~10 ms, HIP events); az_set_pass_costs pins it (n >= 2; tests, or a deployment that has measured its boxes),
 * n = 0 returns to measuring.  az_get_pass_costs reads the table in use (n_out = 0: none yet). */
int az_set_pass_costs(az_ctx *ctx, int n, const int32_t *rows, const double *us);
int az_get_pass_costs(az_ctx *ctx, int32_t *rows_out, double *us_out, int cap, int *n_out);
/* What this box sustains, for reading a roofline fraction apart from the box it was measured on: the fp32-input MFMA rate
 * (TFLOP/s) of a ~3 ms register-only v_mfma_f32_32x32x2_f32 loop on every SIMD, pseudo-random operands (the data-sheet
 * peak, 157.3 TFLOP/s, assumes 2.4 GHz; boxes hold 5-10 % less and differ among themselves), and the rate (TB/s, bytes
 * read + written) of a 1 GiB float4 copy through HBM.  ~40 ms; either output may be NULL.  Blocks until done. */
int az_measure_box(az_ctx *ctx, double *mfma_f32_tflops, double *copy_tb_per_s);
/* The HIP stream the ctx launches on (a hipStream_t). */
void *az_stream(az_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* AZNET_HIP_H */
