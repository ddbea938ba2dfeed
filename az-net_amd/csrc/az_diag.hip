// az_diag.hip -- the analysis AZ_results.mat was written for (lib/detect/tune.py:368-419 records prop_boxes, anchor_boxes
// and gt_boxes per image; the reference did the rest offline), for a whole image set in one call ("Proposal
// diagnosis"):
//   k_diag_anchor   one thread per anchor: its image by a bisection of anc_off, _compute_zoom_labels against that image's
//                   objects (az_zoom_label, bbox.pyx:20-60), zoomed = zoom >= (level 0 ? 0 : Tz) (tune.py:282, 296, 306);
//                   per level: anchors, zoomed, labelled, both -- counted in LDS, one 64-bit atomic per non-zero cell
//   k_diag_object   one wave per object, grid-striding: lanes over the image's proposals (bbox_overlaps, az_iou_f64) ->
//                   first maximum and first rank at iou_thresh by a wave reduction; lanes over the image's anchors ->
//                   deepest level that holds the object (bbox.pyx:48-58 without the area-ratio gate); lane 0 files the
//                   object under every budget it is hit within, by size -- LDS, then 64-bit atomics
// The tables are integer counts: the atomics' order does not show.  f64 throughout, -ffp-contract=off (Makefile).
#include "az_ctx.h"

namespace {

constexpr int DT = 256;               // threads of every workgroup here (4 waves)
constexpr int DIAG_MAX_CUTS = 16;

struct DiagCuts { int n; int v[DIAG_MAX_CUTS]; };

// last i in [0, n) with off[i] <= x (off[n] > x)
__device__ __forceinline__ int seg_of(const int *__restrict__ off, int n, int x)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(DT) k_diag_anchor(int A, int n_img, const double *__restrict__ anc,
                                                     const float *__restrict__ zoom, const int *__restrict__ level,
                                                     const int *__restrict__ anc_off, const double *__restrict__ gt,
                                                     const int *__restrict__ gt_off, double tz, double max_ratio,
                                                     double min_obj, unsigned char *__restrict__ label,
                                                     unsigned long long *__restrict__ table)
{
    __shared__ unsigned s_t[AZ_MAX_LEVELS * 4];
    if (threadIdx.x < AZ_MAX_LEVELS * 4) s_t[threadIdx.x] = 0;
    __syncthreads();
    const int a = blockIdx.x * DT + threadIdx.x;
    if (a < A) {
        const int img = seg_of(anc_off, n_img, a);
        const int g0 = gt_off[img], N = gt_off[img + 1] - g0;
        const bool lab = az_zoom_label(anc + 4 * (size_t)a, gt + 4 * (size_t)g0, N, max_ratio, min_obj);
        const int lv = level[a];
        const bool zm = (double)zoom[a] >= (lv == 0 ? 0.0 : tz);
        label[a] = lab ? 1 : 0;
        atomicAdd(&s_t[lv * 4 + 0], 1u);
        if (zm) atomicAdd(&s_t[lv * 4 + 1], 1u);
        if (lab) atomicAdd(&s_t[lv * 4 + 2], 1u);
        if (zm && lab) atomicAdd(&s_t[lv * 4 + 3], 1u);
    }
    __syncthreads();
    if (threadIdx.x < AZ_MAX_LEVELS * 4 && s_t[threadIdx.x])
        atomicAdd(&table[threadIdx.x], (unsigned long long)s_t[threadIdx.x]);
}

__global__ void __launch_bounds__(DT) k_diag_object(int G, int n_img, const double *__restrict__ gt,
                                                     const int *__restrict__ gt_off, const double *__restrict__ prop,
                                                     const int *__restrict__ prop_off, const double *__restrict__ anc,
                                                     const int *__restrict__ level, const int *__restrict__ anc_off,
                                                     double min_obj, double iou_thresh, DiagCuts cuts, double edge0,
                                                     double edge1, double *__restrict__ best_iou, int *__restrict__ best_rank,
                                                     int *__restrict__ first_hit, int *__restrict__ deepest,
                                                     unsigned long long *__restrict__ table)
{
    __shared__ unsigned s_t[(DIAG_MAX_CUTS + 1) * 4];
    if (threadIdx.x < (DIAG_MAX_CUTS + 1) * 4) s_t[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (AZ_WAVE - 1);
    const int nw = gridDim.x * (DT / AZ_WAVE);
    for (int g = blockIdx.x * (DT / AZ_WAVE) + threadIdx.x / AZ_WAVE; g < G; g += nw) {      // wave-uniform
        const int img = seg_of(gt_off, n_img, g);
        const double *q = gt + 4 * (size_t)g;
        const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        const double qb[4] = {q0, q1, q2, q3};
        const double gt_area = (q2 - q0 + 1.0) * (q3 - q1 + 1.0);
        // ---- proposals, in rank order -------------------------------------------------------------------------
        const int p0 = prop_off[img], n = prop_off[img + 1] - p0;
        double best = -INFINITY;
        int bj = 0x7fffffff, fh = 0x7fffffff;
        for (int j = lane; j < n; j += AZ_WAVE) {
            const double ov = az_iou_f64(prop + 4 * (size_t)(p0 + j), qb);
            if (ov > best) { best = ov; bj = j; }            // j ascends per lane: the first maximum is kept
            if (ov >= iou_thresh && j < fh) fh = j;
        }
        for (int o = AZ_WAVE / 2; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, AZ_WAVE);
            const int oj = __shfl_xor(bj, o, AZ_WAVE), of = __shfl_xor(fh, o, AZ_WAVE);
            if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
            if (of < fh) fh = of;
        }
        if (bj == 0x7fffffff) { best = 0.0; bj = -1; }       // no proposals
        if (fh == 0x7fffffff) fh = -1;
        // ---- anchors: the deepest level that holds the object -------------------------------------------------
        const int a0 = anc_off[img], m = anc_off[img + 1] - a0;
        int deep = -1;
        for (int j = lane; j < m; j += AZ_WAVE) {
            const double *r = anc + 4 * (size_t)(a0 + j);
            const double iw = (r[2] < q2 ? r[2] : q2) - (r[0] > q0 ? r[0] : q0) + 1.0;
            if (iw > 0.0) {
                const double ih = (r[3] < q3 ? r[3] : q3) - (r[1] > q1 ? r[1] : q1) + 1.0;
                if (ih > 0.0 && iw * ih / (gt_area + 1e-14) >= min_obj) {
                    const int lv = level[a0 + j];
                    if (lv > deep) deep = lv;
                }
            }
        }
        for (int o = AZ_WAVE / 2; o > 0; o >>= 1) {
            const int od = __shfl_xor(deep, o, AZ_WAVE);
            if (od > deep) deep = od;
        }
        if (lane == 0) {
            best_iou[g] = best; best_rank[g] = bj; first_hit[g] = fh; deepest[g] = deep;
            const int col = gt_area < edge0 ? 1 : (gt_area < edge1 ? 2 : 3);
            for (int c = 0; c < cuts.n; ++c)
                if (fh >= 0 && fh < cuts.v[c]) { atomicAdd(&s_t[c * 4], 1u); atomicAdd(&s_t[c * 4 + col], 1u); }
            atomicAdd(&s_t[cuts.n * 4], 1u);
            atomicAdd(&s_t[cuts.n * 4 + col], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < (cuts.n + 1) * 4 && s_t[threadIdx.x])
        atomicAdd(&table[threadIdx.x], (unsigned long long)s_t[threadIdx.x]);
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// 0 ok, 1 malformed: n + 1 non-negative, non-decreasing entries from 0 to `total`
int offsets_bad(const int32_t *off, int n, long long total)
{
    if (off[0] != 0) return 1;
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return 1;
    return (long long)off[n] != total;
}

}  // namespace

int az_diag_eval(az_ctx *c, int n_images, const double *anchors, const float *zoom, const int32_t *level,
                 const int32_t *anc_off, long long n_anchors, const double *gt, const int32_t *gt_off, long long n_gt,
                 const double *props, const int32_t *prop_off, long long n_props, double tz, double emb_reg_thresh,
                 double emb_obj_thresh, double iou_thresh, const int32_t *cuts, int n_cuts, const double *area_edges,
                 uint8_t *anchor_label_out, int64_t *level_table_out, double *gt_best_iou_out, int32_t *gt_best_rank_out,
                 int32_t *gt_first_hit_out, int32_t *gt_deepest_level_out, int64_t *recall_table_out, float *kernel_ms_out)
{
    if (!c || n_images < 0 || !anc_off || !gt_off || !prop_off || n_anchors < 0 || n_gt < 0 || n_props < 0 || n_cuts < 0 ||
        (n_cuts && !cuts) || !area_edges)
        return fail(c, AZ_ERR_INVALID, "az_diag_eval: bad arguments");
    if (n_cuts > DIAG_MAX_CUTS) return fail(c, AZ_ERR_INVALID, "az_diag_eval: at most 16 proposal budgets");
    for (int k = 1; k < n_cuts; ++k)
        if (cuts[k] < cuts[k - 1]) return fail(c, AZ_ERR_INVALID, "az_diag_eval: the proposal budgets must ascend");
    if (n_anchors > 0x7fffffffLL || n_gt > 0x7fffffffLL || n_props > 0x7fffffffLL)
        return fail(c, AZ_ERR_CAPACITY, "az_diag_eval: more rows than int32 offsets address");
    if (offsets_bad(anc_off, n_images, n_anchors) || offsets_bad(gt_off, n_images, n_gt) ||
        offsets_bad(prop_off, n_images, n_props))
        return fail(c, AZ_ERR_INVALID, "az_diag_eval: offsets must ascend from 0 to the row counts");
    const int A = (int)n_anchors, G = (int)n_gt, P = (int)n_props;
    if ((A && (!anchors || !zoom || !level)) || (G && !gt) || (P && !props))
        return fail(c, AZ_ERR_INVALID, "az_diag_eval: NULL array");
    for (int a = 0; a < A; ++a)
        if (level[a] < 0 || level[a] >= AZ_MAX_LEVELS)
            return fail(c, AZ_ERR_INVALID, "az_diag_eval: anchor " + std::to_string(a) + " has level " + std::to_string(level[a]) +
                                               " outside [0, AZ_MAX_LEVELS)");
    // one arena: inputs, offsets, per-anchor and per-object results, the two tables
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    const size_t o_anc = take((size_t)A * 32), o_zoom = take((size_t)A * 4), o_lev = take((size_t)A * 4);
    const size_t o_gt = take((size_t)G * 32), o_prop = take((size_t)P * 32);
    const size_t o_aoff = take(((size_t)n_images + 1) * 4), o_goff = take(((size_t)n_images + 1) * 4);
    const size_t o_poff = take(((size_t)n_images + 1) * 4);
    const size_t o_lab = take((size_t)A), o_iou = take((size_t)G * 8), o_rank = take((size_t)G * 4);
    const size_t o_hit = take((size_t)G * 4), o_deep = take((size_t)G * 4);
    const size_t n_lt = AZ_MAX_LEVELS * 4, n_rt = ((size_t)n_cuts + 1) * 4;
    const size_t o_tab = take((n_lt + n_rt) * 8);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = scratch_grow(c, 10, off)) != AZ_OK) return rc;
    char *B = (char *)c->scratch[10].p;
    hipStream_t s = c->stream;
    auto *d_anc = (double *)(B + o_anc), *d_gt = (double *)(B + o_gt), *d_prop = (double *)(B + o_prop);
    auto *d_zoom = (float *)(B + o_zoom);
    auto *d_lev = (int *)(B + o_lev), *d_aoff = (int *)(B + o_aoff), *d_goff = (int *)(B + o_goff), *d_poff = (int *)(B + o_poff);
    auto *d_lab = (unsigned char *)(B + o_lab);
    auto *d_iou = (double *)(B + o_iou);
    auto *d_rank = (int *)(B + o_rank), *d_hit = (int *)(B + o_hit), *d_deep = (int *)(B + o_deep);
    auto *d_lt = (unsigned long long *)(B + o_tab), *d_rt = d_lt + n_lt;
    if (A) {
        HIPCHK(c, hipMemcpyAsync(d_anc, anchors, (size_t)A * 32, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_zoom, zoom, (size_t)A * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_lev, level, (size_t)A * 4, hipMemcpyHostToDevice, s));
    }
    if (G) HIPCHK(c, hipMemcpyAsync(d_gt, gt, (size_t)G * 32, hipMemcpyHostToDevice, s));
    if (P) HIPCHK(c, hipMemcpyAsync(d_prop, props, (size_t)P * 32, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_aoff, anc_off, ((size_t)n_images + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_goff, gt_off, ((size_t)n_images + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_poff, prop_off, ((size_t)n_images + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(d_lt, 0, (n_lt + n_rt) * 8, s));
    Event e0, e1;
    if (kernel_ms_out) {
        HIPCHK(c, e0.create(hipEventDefault));
        if (e1.create(hipEventDefault) != hipSuccess) return fail(c, AZ_ERR_HIP, "az_diag_eval: hipEventCreate");
        hipEventRecord(e0, s);
    }
    if (A)
        hipLaunchKernelGGL(k_diag_anchor, dim3((A + DT - 1) / DT), dim3(DT), 0, s, A, n_images, (const double *)d_anc,
                           (const float *)d_zoom, (const int *)d_lev, (const int *)d_aoff, (const double *)d_gt,
                           (const int *)d_goff, tz, emb_reg_thresh, emb_obj_thresh, d_lab, d_lt);
    if (G) {
        DiagCuts dc;
        dc.n = n_cuts;
        for (int k = 0; k < DIAG_MAX_CUTS; ++k) dc.v[k] = k < n_cuts ? cuts[k] : 0;
        int nb = (G + (DT / AZ_WAVE) - 1) / (DT / AZ_WAVE);
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(k_diag_object, dim3(nb), dim3(DT), 0, s, G, n_images, (const double *)d_gt, (const int *)d_goff,
                           (const double *)d_prop, (const int *)d_poff, (const double *)d_anc, (const int *)d_lev,
                           (const int *)d_aoff, emb_obj_thresh, iou_thresh, dc, area_edges[0], area_edges[1], d_iou, d_rank,
                           d_hit, d_deep, d_rt);
    }
    if (kernel_ms_out) hipEventRecord(e1, s);
    int64_t lt[AZ_MAX_LEVELS * 4], rt[(DIAG_MAX_CUTS + 1) * 4];
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && A && anchor_label_out) e = hipMemcpyAsync(anchor_label_out, d_lab, (size_t)A, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && G && gt_best_iou_out) e = hipMemcpyAsync(gt_best_iou_out, d_iou, (size_t)G * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && G && gt_best_rank_out) e = hipMemcpyAsync(gt_best_rank_out, d_rank, (size_t)G * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && G && gt_first_hit_out) e = hipMemcpyAsync(gt_first_hit_out, d_hit, (size_t)G * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && G && gt_deepest_level_out) e = hipMemcpyAsync(gt_deepest_level_out, d_deep, (size_t)G * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(lt, d_lt, n_lt * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(rt, d_rt, n_rt * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    float ms = 0.f;
    if (e == hipSuccess && kernel_ms_out) e = hipEventElapsedTime(&ms, e0, e1);
    if (e != hipSuccess) return fail(c, AZ_ERR_HIP, std::string("az_diag_eval: ") + hipGetErrorString(e));
    // the tables reach the caller only once the whole call has succeeded
    if (level_table_out) memcpy(level_table_out, lt, sizeof(int64_t) * n_lt);
    if (recall_table_out) memcpy(recall_table_out, rt, sizeof(int64_t) * n_rt);
    if (kernel_ms_out) *kernel_ms_out = ms;
    return AZ_OK;
}
