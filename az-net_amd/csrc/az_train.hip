// az_train.hip -- the training data layer's per-image work (lib/az_data_layer/roidb.py:110-341, lib/utils/bbox.pyx:20-60):
//   k_zoom_labels        _compute_zoom_labels of a list of regions (unit entry point)
//   k_train_ex_rois      _compute_ex_rois: the simulated zoom search with label noise, TRAIN_REP repetitions from the
//                        TRAIN.ADDREGIONS roots, then every object's super-regions; clip; MIN_SIDE filter
//   k_adj_count / k_adj_scan / k_adj_write     _compute_targets: greedy sub-region / object matching per example region
//   k_stats_partial / k_stats_final / k_normalise     per-sub-region means and stds over all targets, normalisation
// The example regions of an image depend on the noise stream position the previous image left, and a level on the one
// before it: that chain is walked by ONE workgroup for all images of a call (no launch and no host wait inside it; every
// count is a workgroup-uniform register).  Everything after it is independent per example region.
// f64 in the reference's operation order; compiled with -ffp-contract=off.
#include "az_geom_dev.h"

namespace {

constexpr int NT = 1024;           // threads of the chain's workgroup
constexpr int LV_C = 4096;         // children per level before _sift_dup (measured: < 700 at 800 px and 40 objects)
// LDS of k_train_ex_rois, in 8-byte words
constexpr int W_SORT = 0, W_TMP = LV_C, W_BINS = 2 * LV_C, W_SCZI = W_BINS + (SORT_NB + 2) / 2 + 7,
              W_SZR = W_SCZI + LV_C / 2, W_WSUM = W_SZR + LV_C / 2, W_MM = W_WSUM + 9, W_END = W_MM + 1;

// zoom_label: az_zoom_label of az_dev.h (az_diag.hip shares it)
__device__ __forceinline__ bool zoom_label(const double *r, const double *gt, int N, double max_ratio, double min_obj)
{
    return az_zoom_label(r, gt, N, max_ratio, min_obj);
}

__global__ void __launch_bounds__(256) k_zoom_labels(const double *__restrict__ rois, int R, const double *__restrict__ gt,
                                                      int N, double max_ratio, double min_obj, unsigned char *__restrict__ out)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < R) out[r] = zoom_label(rois + 4 * (size_t)r, gt, N, max_ratio, min_obj) ? 1 : 0;
}

// _clip_boxes + the MIN_SIDE filter (roidb.py:291-299); the kept box is rounded to f32 once (roidb.py:65)
__device__ __forceinline__ bool clip_keep(const double *b, int h, int w, double min_side, float *o)
{
    const double x1 = b[0] > 0.0 ? b[0] : 0.0, y1 = b[1] > 0.0 ? b[1] : 0.0;
    const double xm = (double)(w - 1), ym = (double)(h - 1);
    const double x2 = b[2] < xm ? b[2] : xm, y2 = b[3] < ym ? b[3] : ym;
    const double hh = y2 - y1 + 1.0, ww = x2 - x1 + 1.0;
    o[0] = (float)x1; o[1] = (float)y1; o[2] = (float)x2; o[3] = (float)y2;
    return (hh < ww ? hh : ww) >= min_side;
}

struct ExArgs {
    az_train_params p;
    int n_images;
    const int *sizes;              // [n][3]: h, w, K
    const double *gt;
    const int *gt_off;
    const double *noise;
    long long n_noise;
    float *ex;
    unsigned char *zoom;
    int *ex_off;                   // [n + 1]
    long long *used;               // [n]
    int cap;
    double *B0, *B1;               // [LV_C][4] each
    long long *status;             // [0]: 1 noise ran out, 2 a level outgrew LV_C, 4 a coordinate left the hash's range;
                                   // [1]: doubles needed where the noise ran out
};

__global__ void __launch_bounds__(NT) k_train_ex_rois(ExArgs a)
{
    extern __shared__ unsigned long long sbuf[];
    unsigned long long *ssort = sbuf + W_SORT, *stmp = sbuf + W_TMP;
    unsigned *sbins = reinterpret_cast<unsigned *>(sbuf + W_BINS), *s_mm = reinterpret_cast<unsigned *>(sbuf + W_MM);
    int *sczi = reinterpret_cast<int *>(sbuf + W_SCZI), *szr = reinterpret_cast<int *>(sbuf + W_SZR);
    int *wsum = reinterpret_cast<int *>(sbuf + W_WSUM);
    const int tid = threadIdx.x;
    const az_train_params &p = a.p;
    long long noff = 0;            // the noise stream's position: carried from image to image
    int E = 0;                     // example regions so far (counted past `cap`, written below it)
    if (tid == 0) a.ex_off[0] = 0;
    for (int img = 0; img < a.n_images; ++img) {
        const int h = a.sizes[3 * img], w = a.sizes[3 * img + 1], K = a.sizes[3 * img + 2];
        const int g0 = a.gt_off[img], N = a.gt_off[img + 1] - g0;
        const double *gt = a.gt + 4 * (size_t)g0;
        const double len[4] = {w - 1.0, h - 1.0, w - 1.0, h - 1.0};
        const long long noff0 = noff;
        for (int rep = 0; rep < p.train_rep; ++rep) {
            double *B = a.B0, *Bn = a.B1;
            int P = p.n_addregions;
            __syncthreads();
            if (tid < P)
                for (int q = 0; q < 4; ++q) B[4 * tid + q] = len[q] * p.addregions[tid][q];      // roidb.py:243
            __syncthreads();
            for (int lvl = 0; lvl < K; ++lvl) {
                if (noff + P > a.n_noise) {
                    if (tid == 0) { a.status[0] |= 1; a.status[1] = noff + P; }
                    return;
                }
                // ---- labels, append, noise, zoom selection (roidb.py:252-264) ----------------------------
                int PZ = 0;
                for (int base = 0; base < P; base += NT) {
                    const int r = base + tid;
                    int keep = 0, zf = 0, z = 0;
                    float o[4];
                    if (r < P) {
                        const double *b = B + 4 * (size_t)r;
                        z = zoom_label(b, gt, N, p.emb_reg_thresh, p.emb_obj_thresh);
                        const int err = a.noise[noff + r] <= p.zoom_err_prob;
                        zf = z != err;
                        keep = clip_keep(b, h, w, p.min_side, o);
                    }
                    int tot;
                    const int ex = block_excl_scan(keep | (zf << 16), &tot, wsum);
                    if (keep && E + (ex & 0xFFFF) < a.cap) {
                        const size_t at = (size_t)(E + (ex & 0xFFFF));
                        for (int q = 0; q < 4; ++q) a.ex[4 * at + q] = o[q];
                        a.zoom[at] = (unsigned char)z;
                    }
                    if (zf) szr[PZ + (ex >> 16)] = r;
                    E += tot & 0xFFFF;
                    PZ += tot >> 16;
                }
                noff += P;
                if (PZ == 0) break;
                __syncthreads();
                // ---- divide_region (div.pyx:15-76) -----------------------------------------------------
                int CH = 0;
                for (int base = 0; base < PZ; base += NT) {
                    const int zi = base + tid;
                    const int n = zi < PZ ? div_nchildren(div_plan(B + 4 * (size_t)szr[zi])) : 0;
                    int tot;
                    const int ex = block_excl_scan(n, &tot, wsum);
                    if (zi < PZ && CH + ex + n <= LV_C)
                        for (int bi = 0; bi < n; ++bi) sczi[CH + ex + bi] = (zi << 16) | bi;
                    CH += tot;
                }
                if (CH > LV_C) { if (tid == 0) a.status[0] |= 2; return; }
                __syncthreads();
                int bad = 0;
                for (int ci = tid; ci < CH; ci += NT) {
                    const double *r = B + 4 * (size_t)szr[sczi[ci] >> 16];
                    double c[4];
                    const long long key = div_child(r, div_plan(r), sczi[ci] & 0xFFFF, p.min_side, c);
                    bad |= (key < 0 || key >= (1ll << 40));
                    ssort[ci] = ((unsigned long long)key << 20) | (unsigned)ci;
                }
                if (__syncthreads_or(bad)) { if (tid == 0) a.status[0] |= 4; return; }
                // ---- _sift_dup (div.pyx:78-89): ascending hash, the first child of each ---------------------
                block_bucket_sort(ssort, CH, stmp, sbins, 40, wsum, s_mm);
                int Pn = 0;
                for (int base = 0; base < CH; base += NT) {
                    const int i = base + tid;
                    int head = 0;
                    unsigned long long wd = 0;
                    if (i < CH) {
                        wd = ssort[i];
                        head = (i == 0) || ((ssort[i - 1] >> 20) != (wd >> 20));
                    }
                    int tot;
                    const int ex = block_excl_scan(head, &tot, wsum);
                    if (head) {
                        const int ci = sczi[(int)(wd & 0xFFFFFu)];
                        const double *r = B + 4 * (size_t)szr[ci >> 16];
                        double c[4];
                        div_child_box(r, div_plan(r), ci & 0xFFFF, c);
                        for (int q = 0; q < 4; ++q) Bn[4 * (size_t)(Pn + ex) + q] = c[q];
                    }
                    Pn += tot;
                }
                P = Pn;
                double *t = B; B = Bn; Bn = t;
                __syncthreads();
            }
        }
        // ---- every object's super-regions (roidb.py:270-289) ----------------------------------------------
        const int S = p.n_subregion, NS = N * S;
        for (int base = 0; base < NS; base += NT) {
            const int i = base + tid;
            int keep = 0, z = 0;
            float o[4];
            if (i < NS) {
                const double *ri = gt + 4 * (size_t)(i / S), *rt = p.subregion[i % S];
                const double ls0 = (ri[2] - ri[0] + 1.0) / (rt[2] - rt[0]), ls1 = (ri[3] - ri[1] + 1.0) / (rt[3] - rt[1]);
                const double ts0 = ri[0] - ls0 * rt[0], ts1 = ri[1] - ls1 * rt[1];
                const double rs[4] = {ts0, ts1, ts0 + ls0 - 1.0, ts1 + ls1 - 1.0};
                z = zoom_label(rs, gt, N, p.emb_reg_thresh, p.emb_obj_thresh);
                keep = clip_keep(rs, h, w, p.min_side, o);
            }
            int tot;
            const int ex = block_excl_scan(keep, &tot, wsum);
            if (keep && E + ex < a.cap) {
                const size_t at = (size_t)(E + ex);
                for (int q = 0; q < 4; ++q) a.ex[4 * at + q] = o[q];
                a.zoom[at] = (unsigned char)z;
            }
            E += tot;
        }
        if (tid == 0) { a.ex_off[img + 1] = E; a.used[img] = noff - noff0; }
    }
}

// ---- adjacency targets (roidb.py:146-227) -----------------------------------------------------------------------
struct AdjArgs {
    az_train_params p;
    int n_images, E;
    const float *ex;
    const int *ex_off;
    const float *gt;
    const int *gt_off;
    int *cnt;                      // [E + 1]: matches per example region, then (k_adj_scan) their first row
    int *tgt_off;                  // [n + 1]
    double *targets;
    int cap;
};

__device__ __forceinline__ void widen(const float *s, double *d) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3]; }

// s_re = L * SUBREGION + delta, L = (x2 - x1, y2 - y1) without + 1 (roidb.py:174-178)
__device__ __forceinline__ void sub_region(const double *re, const double *t, double *o)
{
    const double L0 = re[2] - re[0], L1 = re[3] - re[1];
    o[0] = L0 * t[0] + re[0]; o[1] = L1 * t[1] + re[1]; o[2] = L0 * t[2] + re[0]; o[3] = L1 * t[3] + re[1];
}

__global__ void __launch_bounds__(256) k_adj_count(AdjArgs a)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.E) return;
    const int img = seg_of(a.ex_off, a.n_images, k);
    const int g0 = a.gt_off[img], N = a.gt_off[img + 1] - g0;
    double re[4], s0[4];
    widen(a.ex + 4 * (size_t)k, re);
    sub_region(re, a.p.subregion[0], s0);
    double mx = 0.0;
    int adj = 0;
    for (int n = 0; n < N; ++n) {
        double q[4];
        widen(a.gt + 4 * (size_t)(g0 + n), q);
        const double o = az_iou_f64(re, q);
        mx = o > mx ? o : mx;
        adj += az_iou_f64(s0, q) >= a.p.adj_thresh;
    }
    const int S = a.p.n_subregion;
    a.cnt[k] = (N == 0 || mx < a.p.adj_thresh) ? 0 : (adj < S ? adj : S);
}

// exclusive scan of cnt[0 .. E) in place, cnt[E] = total; tgt_off[i] = the first row of image i
__global__ void __launch_bounds__(1024) k_adj_scan(AdjArgs a)
{
    __shared__ int wsum[17];
    int run = 0;
    for (int base = 0; base < a.E; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < a.E ? a.cnt[i] : 0;
        int tot;
        const int ex = block_excl_scan(v, &tot, wsum);
        if (i < a.E) a.cnt[i] = run + ex;
        run += tot;
    }
    if (threadIdx.x == 0) a.cnt[a.E] = run;
    __syncthreads();
    for (int i = threadIdx.x; i <= a.n_images; i += 1024) a.tgt_off[i] = a.cnt[i < a.n_images ? a.ex_off[i] : a.E];
}

// _compute_bbox_deltas (roidb.py:206-227)
__device__ __forceinline__ void bbox_deltas(const double *ex, const double *gt, double eps, double *t)
{
    double ew = (ex[2] - ex[0] > 1.0 ? ex[2] - ex[0] : 1.0) + eps, eh = (ex[3] - ex[1] > 1.0 ? ex[3] - ex[1] : 1.0) + eps;
    const double ecx = ex[0] + 0.5 * ew, ecy = ex[1] + 0.5 * eh;
    double gw = (gt[2] - gt[0] > 1.0 ? gt[2] - gt[0] : 1.0) + eps, gh = (gt[3] - gt[1] > 1.0 ? gt[3] - gt[1] : 1.0) + eps;
    const double gcx = gt[0] + 0.5 * gw, gcy = gt[1] + 0.5 * gh;
    ew = ew > 1.0 ? ew : 1.0; eh = eh > 1.0 ? eh : 1.0; gw = gw > 1.0 ? gw : 1.0; gh = gh > 1.0 ? gh : 1.0;
    t[0] = (gcx - ecx) / ew;
    t[1] = (gcy - ecy) / eh;
    t[2] = log(gw / ew);
    t[3] = log(gh / eh);
}

// One wave per example region: the S x N IoU matrix in LDS, then `count` rounds of first-maximum / retire row and column.
__global__ void __launch_bounds__(64) k_adj_write(AdjArgs a)
{
    extern __shared__ double ov[];
    const int k = blockIdx.x, lane = threadIdx.x;
    const int row0 = a.cnt[k], count = a.cnt[k + 1] - row0;
    if (count == 0 || row0 + count > a.cap) return;
    const int img = seg_of(a.ex_off, a.n_images, k);
    const int g0 = a.gt_off[img], N = a.gt_off[img + 1] - g0, S = a.p.n_subregion;
    const int kloc = k - a.ex_off[img];
    double re[4];
    widen(a.ex + 4 * (size_t)k, re);
    for (int i = lane; i < S * N; i += 64) {
        double sr[4], q[4];
        sub_region(re, a.p.subregion[i / N], sr);
        widen(a.gt + 4 * (size_t)(g0 + i % N), q);
        ov[i] = az_iou_f64(sr, q);
    }
    __syncthreads();
    for (int n = lane; n < N; n += 64)
        if (ov[n] < a.p.adj_thresh)
            for (int s = 0; s < S; ++s) ov[s * N + n] = -1.0;
    __syncthreads();
    for (int round = 0; round < count; ++round) {
        double best = -2.0;
        int bi = 0x7FFFFFFF;
        for (int i = lane; i < S * N; i += 64)
            if (ov[i] > best) { best = ov[i]; bi = i; }
        for (int d = 32; d >= 1; d >>= 1) {         // np.argmax: the first maximum in row-major order
            const double ob = __shfl_xor(best, d, 64);
            const int oi = __shfl_xor(bi, d, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        const int s = bi / N, n = bi - s * N;
        if (lane == 0) {
            double q[4], t[4];
            widen(a.gt + 4 * (size_t)(g0 + n), q);
            bbox_deltas(re, q, a.p.eps, t);
            double *o = a.targets + 7 * (size_t)(row0 + round);
            o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
            o[4] = (double)kloc; o[5] = (double)s; o[6] = az_iou_f64(re, q);
        }
        __syncthreads();
        for (int j = lane; j < N; j += 64) ov[s * N + j] = -1.0;
        for (int j = lane; j < S; j += 64) ov[j * N + n] = -1.0;
        __syncthreads();
    }
}

// ---- means, stds, normalisation (roidb.py:110-134) ----------------------------------------------------------------
// Two levels, both in a fixed order: a workgroup per (chunk of ST_CHUNK rows, sub-region) with an LDS tree, then one
// thread per (sub-region, statistic) over the chunks in ascending order.  No atomics: the same bits on every run.
constexpr int ST_CHUNK = 4096, ST_T = 256;

__global__ void __launch_bounds__(ST_T) k_stats_partial(const double *__restrict__ t, long long T, int n_sub, double *part)
{
    __shared__ double sh[ST_T][9];
    const int cls = blockIdx.y, tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * ST_CHUNK;
    double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = tid; j < ST_CHUNK; j += ST_T) {
        const long long r = r0 + j;
        if (r < T && t[7 * r + 5] == (double)cls) {
            v[0] += 1.0;
            for (int q = 0; q < 4; ++q) { const double x = t[7 * r + q]; v[1 + q] += x; v[5 + q] += x * x; }
        }
    }
    for (int q = 0; q < 9; ++q) sh[tid][q] = v[q];
    __syncthreads();
    for (int d = ST_T / 2; d >= 1; d >>= 1) {
        if (tid < d)
            for (int q = 0; q < 9; ++q) sh[tid][q] += sh[tid + d][q];
        __syncthreads();
    }
    if (tid < 9) part[((size_t)blockIdx.x * n_sub + cls) * 9 + tid] = sh[0][tid];
}

__global__ void __launch_bounds__(256) k_stats_final(const double *__restrict__ part, int n_chunks, int n_sub, double eps,
                                                      double *means, double *stds)
{
    __shared__ double tot[16 * 9];
    const int tid = threadIdx.x;
    if (tid < n_sub * 9) {
        double s = 0.0;
        for (int c = 0; c < n_chunks; ++c) s += part[(size_t)c * n_sub * 9 + tid];
        tot[tid] = s;
    }
    __syncthreads();
    if (tid < n_sub * 4) {
        const int cls = tid / 4, q = tid % 4;
        const double cnt = tot[cls * 9] + eps;
        const double m = tot[cls * 9 + 1 + q] / cnt;
        means[tid] = m;
        stds[tid] = sqrt(tot[cls * 9 + 5 + q] / cnt - m * m);
    }
}

__global__ void __launch_bounds__(256) k_normalise(double *t, long long T, int n_sub, const double *__restrict__ means,
                                                    const double *__restrict__ stds)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= T) return;
    // the rows k_stats_partial counted: t[:, -2] == cls (roidb.py:132); a class like 2.5 or -0.5 belongs to none
    const double c = t[7 * r + 5];
    if (!(c >= 0.0 && c < (double)n_sub)) return;
    const int cls = (int)c;
    if ((double)cls != c) return;
    for (int q = 0; q < 4; ++q) t[7 * r + q] = (t[7 * r + q] - means[4 * cls + q]) / stds[4 * cls + q];
}

}  // namespace

void azk_zoom_labels(hipStream_t s, const double *rois, int R, const double *gt, int N, double max_ratio, double min_obj,
                     unsigned char *out)
{
    if (R > 0) hipLaunchKernelGGL(k_zoom_labels, dim3((R + 255) / 256), dim3(256), 0, s, rois, R, gt, N, max_ratio, min_obj, out);
}

int azk_train_level_cap() { return LV_C; }

// status: 2 long longs (zeroed here); B: 2 * LV_C * 4 doubles
int azk_train_ex_rois(hipStream_t s, const az_train_params *p, int n_images, const int *sizes3, const double *gt,
                      const int *gt_off, const double *noise, long long n_noise, float *ex, unsigned char *zoom,
                      int *ex_off, long long *used, int cap, double *B, long long *status)
{
    static bool attr = false;
    const size_t lds = (size_t)W_END * 8;
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_train_ex_rois), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds) != hipSuccess)
            return 1;
        attr = true;
    }
    if (hipMemsetAsync(status, 0, 2 * sizeof(long long), s) != hipSuccess) return 1;
    ExArgs a;
    a.p = *p; a.n_images = n_images; a.sizes = sizes3; a.gt = gt; a.gt_off = gt_off; a.noise = noise; a.n_noise = n_noise;
    a.ex = ex; a.zoom = zoom; a.ex_off = ex_off; a.used = used; a.cap = cap; a.B0 = B; a.B1 = B + 4 * (size_t)LV_C;
    a.status = status;
    hipLaunchKernelGGL(k_train_ex_rois, dim3(1), dim3(NT), lds, s, a);
    return hipGetLastError() != hipSuccess;
}

size_t azk_adj_lds_max() { return 128 * 1024; }

// stage 1: the counts and their scan (cnt [E + 1], tgt_off [n + 1]); stage 2 (after the caller knows T <= cap): the rows
int azk_train_adj_count(hipStream_t s, const az_train_params *p, int n_images, int E, const float *ex, const int *ex_off,
                        const float *gt, const int *gt_off, int *cnt, int *tgt_off)
{
    AdjArgs a;
    a.p = *p; a.n_images = n_images; a.E = E; a.ex = ex; a.ex_off = ex_off; a.gt = gt; a.gt_off = gt_off; a.cnt = cnt;
    a.tgt_off = tgt_off; a.targets = nullptr; a.cap = 0;
    if (E > 0) hipLaunchKernelGGL(k_adj_count, dim3((E + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_adj_scan, dim3(1), dim3(1024), 0, s, a);
    return hipGetLastError() != hipSuccess;
}

int azk_train_adj_write(hipStream_t s, const az_train_params *p, int n_images, int E, int max_gt, const float *ex,
                        const int *ex_off, const float *gt, const int *gt_off, int *cnt, double *targets, int cap)
{
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_adj_write), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)azk_adj_lds_max()) != hipSuccess)
            return 1;
        attr = true;
    }
    AdjArgs a;
    a.p = *p; a.n_images = n_images; a.E = E; a.ex = ex; a.ex_off = ex_off; a.gt = gt; a.gt_off = gt_off; a.cnt = cnt;
    a.tgt_off = nullptr; a.targets = targets; a.cap = cap;
    const size_t lds = (size_t)p->n_subregion * (size_t)(max_gt > 0 ? max_gt : 1) * sizeof(double);
    if (E > 0) hipLaunchKernelGGL(k_adj_write, dim3(E), dim3(64), lds, s, a);
    return hipGetLastError() != hipSuccess;
}

size_t azk_stats_part_doubles(long long T, int n_sub) { return (size_t)((T + ST_CHUNK - 1) / ST_CHUNK) * n_sub * 9 + 1; }

int azk_train_target_stats(hipStream_t s, int n_sub, double eps, double *targets, long long T, double *part, double *means,
                           double *stds, int normalise)
{
    const int n_chunks = (int)((T + ST_CHUNK - 1) / ST_CHUNK);
    if (n_chunks > 0) hipLaunchKernelGGL(k_stats_partial, dim3(n_chunks, n_sub), dim3(ST_T), 0, s, targets, T, n_sub, part);
    hipLaunchKernelGGL(k_stats_final, dim3(1), dim3(256), 0, s, part, n_chunks, n_sub, eps, means, stds);
    if (normalise && T > 0)
        hipLaunchKernelGGL(k_normalise, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, targets, T, n_sub, means, stds);
    return hipGetLastError() != hipSuccess;
}
