// az_det_train.hip -- the detection net's box-regression targets (lib/roi_data_layer/roidb.py of the reference) on the GPU:
//   k_det_targets                        per example box: max IoU over its image's objects, the FIRST maximum's object, and where
//                                        that IoU reaches BBOX_THRESH the row [label, dx, dy, dw, dh]
//   k_det_stats_image / k_det_stats_set  per class counts, means and stds over the set
//   k_det_normalise                      (t - mean) / std in place
// f64 in the reference's operation order where the reference computes in f64, f32 where NumPy sums float32 arrays; compiled
// with -ffp-contract=off.  No atomics: every sum walks its rows (then the images) in index order, so two runs give the same
// bits, and those are NumPy's.
#include "az_ctx.h"

namespace {

__device__ __forceinline__ int image_of(const int *__restrict__ off, int n, int e)
{
    int lo = 0, hi = n - 1;                    // the last i with off[i] <= e (empty images share an offset with the next one)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// _compute_targets, one thread per example box of any image
__global__ void __launch_bounds__(256) k_det_targets(int n_images, int E, const float *__restrict__ ex, const int *__restrict__ ex_off,
                                                     const float *__restrict__ gt, const int *__restrict__ gt_lab,
                                                     const int *__restrict__ gt_off, double thresh, double bg_lo, double eps,
                                                     float *__restrict__ tgt, double *__restrict__ maxov)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int im = image_of(ex_off, n_images, e);
    const int g0 = gt_off[im], g1 = gt_off[im + 1];
    float *t = tgt + 5 * (size_t)e;
    t[0] = t[1] = t[2] = t[3] = t[4] = 0.0f;
    if (g1 <= g0) { maxov[e] = (double)(float)bg_lo; return; }        // (the reference's float32 array of BG_THRESH_LO)
    double b[4];
    for (int q = 0; q < 4; ++q) b[q] = (double)ex[4 * (size_t)e + q];
    double best = -1.0;
    int at = g0;
    for (int g = g0; g < g1; ++g) {
        double o[4];
        for (int q = 0; q < 4; ++q) o[q] = (double)gt[4 * (size_t)g + q];
        const double ov = az_iou_f64(b, o);
        if (ov > best) { best = ov; at = g; }                         // strict: the first maximum stays
    }
    maxov[e] = best;
    if (!(best >= thresh)) return;
    double o[4];
    for (int q = 0; q < 4; ++q) o[q] = (double)gt[4 * (size_t)at + q];
    double pw = b[2] - b[0] + eps, ph = b[3] - b[1] + eps;
    const double pcx = b[0] + 0.5 * pw, pcy = b[1] + 0.5 * ph;
    double tw = o[2] - o[0] + eps, th = o[3] - o[1] + eps;
    const double tcx = o[0] + 0.5 * tw, tcy = o[1] + 0.5 * th;
    pw = pw > 1.0 ? pw : 1.0; ph = ph > 1.0 ? ph : 1.0; tw = tw > 1.0 ? tw : 1.0; th = th > 1.0 ? th : 1.0;
    t[0] = (float)gt_lab[at];
    t[1] = (float)((tcx - pcx) / pw);
    t[2] = (float)((tcy - pcy) / ph);
    t[3] = (float)log(tw / pw);
    t[4] = (float)log(th / ph);
}

// per (image, class >= 1): the number of rows with that label and the float32 sums of t and of t * t (the square rounded to
// float32 first) over them in row order: what targets[cls_inds, 1:].sum(axis=0) and (targets[cls_inds, 1:] ** 2).sum(axis=0)
// give.  part [n_images][ncls][9]: count (as float bits of an int), 4 sums, 4 squared sums.
__global__ void __launch_bounds__(256) k_det_stats_image(int n_images, int ncls, const float *__restrict__ tgt,
                                                         const int *__restrict__ ex_off, float *__restrict__ part)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)n_images * ncls) return;
    const int im = (int)(id / ncls), cls = (int)(id % ncls);
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    int n = 0;
    if (cls >= 1)
        for (int e = ex_off[im]; e < ex_off[im + 1]; ++e) {
            const float *t = tgt + 5 * (size_t)e;
            if (t[0] != (float)cls) continue;
            ++n;
            for (int k = 0; k < 4; ++k) { const float v = t[1 + k]; const float vv = v * v; s[k] = s[k] + v; q[k] = q[k] + vv; }
        }
    float *p = part + 9 * (size_t)id;
    p[0] = __int_as_float(n);
    for (int k = 0; k < 4; ++k) { p[1 + k] = s[k]; p[5 + k] = q[k]; }
}

// per class: the per-image sums added into float64 in image order (images without a row of the class add nothing), counts
// from eps; means = sums / counts, stds = sqrt(sq / counts - means^2)
__global__ void __launch_bounds__(256) k_det_stats_set(int n_images, int ncls, const float *__restrict__ part, double eps,
                                                       double *__restrict__ counts, double *__restrict__ means,
                                                       double *__restrict__ stds)
{
    const int cls = blockIdx.x * 256 + threadIdx.x;
    if (cls >= ncls) return;
    double cnt = 0.0 + eps, s[4] = {0., 0., 0., 0.}, q[4] = {0., 0., 0., 0.};
    for (int im = 0; im < n_images; ++im) {
        const float *p = part + 9 * ((size_t)im * ncls + cls);
        const int n = __float_as_int(p[0]);
        if (n <= 0) continue;
        cnt += (double)n;
        for (int k = 0; k < 4; ++k) { s[k] += (double)p[1 + k]; q[k] += (double)p[5 + k]; }
    }
    counts[cls] = cnt;
    for (int k = 0; k < 4; ++k) {
        const double m = s[k] / cnt;
        means[4 * cls + k] = m;
        stds[4 * cls + k] = sqrt(q[k] / cnt - m * m);
    }
}

// targets[cls_inds, 1:] -= means[cls]; /= stds[cls] on a float32 array: each in float64, rounded to float32 in between.
// A std of 0 divides by 0 as the reference does.
__global__ void __launch_bounds__(256) k_det_normalise(int E, int ncls, float *__restrict__ tgt, const double *__restrict__ means,
                                                       const double *__restrict__ stds)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float *t = tgt + 5 * (size_t)e;
    const float lab = t[0];
    if (!(lab >= 1.0f && lab < (float)ncls)) return;
    const int cls = (int)lab;
    if ((float)cls != lab) return;
    for (int k = 0; k < 4; ++k) {
        const float c = (float)((double)t[1 + k] - means[4 * cls + k]);
        t[1 + k] = (float)((double)c / stds[4 * cls + k]);
    }
}

struct Arena {
    size_t total = 0;
    size_t add(size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; }
};

int offsets_ok(int n, const int32_t *off)
{
    if (off[0] != 0) return 0;
    for (int i = 0; i < n; ++i) if (off[i + 1] < off[i]) return 0;
    return 1;
}

}  // namespace

extern "C" {

int az_det_targets(az_ctx *c, int n_images, const float *ex_boxes, const int32_t *ex_off, const float *gt, const int32_t *gt_labels,
                   const int32_t *gt_off, double bbox_thresh, double bg_thresh_lo, double eps, float *targets_out,
                   double *max_overlaps_out)
{
    if (!c) return AZ_ERR_INVALID;
    if (n_images < 0 || (n_images && (!ex_off || !gt_off))) return fail(c, AZ_ERR_INVALID, "az_det_targets: bad arguments");
    if (n_images == 0) return AZ_OK;
    if (!offsets_ok(n_images, ex_off) || !offsets_ok(n_images, gt_off)) return fail(c, AZ_ERR_INVALID, "az_det_targets: offsets must ascend from 0");
    const int E = ex_off[n_images], NG = gt_off[n_images];
    if ((E && (!ex_boxes || !targets_out || !max_overlaps_out)) || (NG && (!gt || !gt_labels)))
        return fail(c, AZ_ERR_INVALID, "az_det_targets: NULL array");
    if (E == 0) return AZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    Arena ar;
    const size_t no = ((size_t)n_images + 1) * 4;
    const size_t o_ex = ar.add((size_t)E * 16), o_eo = ar.add(no), o_gt = ar.add((size_t)NG * 16 + 16), o_gl = ar.add((size_t)NG * 4 + 16),
                 o_go = ar.add(no), o_t = ar.add((size_t)E * 20), o_m = ar.add((size_t)E * 8);
    int rc;
    if ((rc = scratch_grow(c, 0, ar.total)) != AZ_OK) return rc;
    char *base = (char *)c->scratch[0].p;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(base + o_ex, ex_boxes, (size_t)E * 16, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(base + o_eo, ex_off, no, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(base + o_go, gt_off, no, hipMemcpyHostToDevice, s));
    if (NG) {
        HIPCHK(c, hipMemcpyAsync(base + o_gt, gt, (size_t)NG * 16, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(base + o_gl, gt_labels, (size_t)NG * 4, hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(k_det_targets, dim3((E + 255) / 256), dim3(256), 0, s, n_images, E, (const float *)(base + o_ex),
                       (const int *)(base + o_eo), (const float *)(base + o_gt), (const int *)(base + o_gl), (const int *)(base + o_go),
                       bbox_thresh, bg_thresh_lo, eps, (float *)(base + o_t), (double *)(base + o_m));
    HIPCHK(c, hipMemcpyAsync(targets_out, base + o_t, (size_t)E * 20, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(max_overlaps_out, base + o_m, (size_t)E * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    return AZ_OK;
}

int az_det_target_stats(az_ctx *c, int n_images, float *targets, const int32_t *ex_off, int num_classes, double eps,
                        int normalise_in_place, double *counts_out, double *means_out, double *stds_out)
{
    if (!c) return AZ_ERR_INVALID;
    if (n_images < 1 || !ex_off || num_classes < 2 || num_classes > 4096 || !means_out || !stds_out)
        return fail(c, AZ_ERR_INVALID, "az_det_target_stats: bad arguments");
    if (!offsets_ok(n_images, ex_off)) return fail(c, AZ_ERR_INVALID, "az_det_target_stats: offsets must ascend from 0");
    const int E = ex_off[n_images];
    if (E && !targets) return fail(c, AZ_ERR_INVALID, "az_det_target_stats: NULL targets");
    HIPCHK(c, hipSetDevice(c->device));
    Arena ar;
    const size_t no = ((size_t)n_images + 1) * 4, cells = (size_t)n_images * num_classes;
    const size_t o_t = ar.add((size_t)E * 20 + 16), o_eo = ar.add(no), o_p = ar.add(cells * 36), o_c = ar.add((size_t)num_classes * 8),
                 o_m = ar.add((size_t)num_classes * 32), o_s = ar.add((size_t)num_classes * 32);
    int rc;
    if ((rc = scratch_grow(c, 0, ar.total)) != AZ_OK) return rc;
    char *base = (char *)c->scratch[0].p;
    hipStream_t s = c->stream;
    if (E) HIPCHK(c, hipMemcpyAsync(base + o_t, targets, (size_t)E * 20, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(base + o_eo, ex_off, no, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_det_stats_image, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, n_images, num_classes,
                       (const float *)(base + o_t), (const int *)(base + o_eo), (float *)(base + o_p));
    hipLaunchKernelGGL(k_det_stats_set, dim3((num_classes + 255) / 256), dim3(256), 0, s, n_images, num_classes, (const float *)(base + o_p),
                       eps, (double *)(base + o_c), (double *)(base + o_m), (double *)(base + o_s));
    if (E && normalise_in_place)
        hipLaunchKernelGGL(k_det_normalise, dim3((E + 255) / 256), dim3(256), 0, s, E, num_classes, (float *)(base + o_t),
                           (const double *)(base + o_m), (const double *)(base + o_s));
    if (counts_out) HIPCHK(c, hipMemcpyAsync(counts_out, base + o_c, (size_t)num_classes * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(means_out, base + o_m, (size_t)num_classes * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(stds_out, base + o_s, (size_t)num_classes * 32, hipMemcpyDeviceToHost, s));
    if (E && normalise_in_place) HIPCHK(c, hipMemcpyAsync(targets, base + o_t, (size_t)E * 20, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    return AZ_OK;
}

}  // extern "C"
