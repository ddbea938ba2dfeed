// az_eval_dev.h -- the device arithmetic that az_voc.hip (az_voc_eval) and az_ddiag.hip (az_det_diag_eval) share, and that
// az_coco.hip (az_coco_eval) and az_cdiag.hip (az_coco_diag_eval) share, so a diagnosis cannot drift from the evaluation it
// explains: VOCevaldet's overlap, the workgroup scan, xVOCap's curve and AP; maskApi's bbIou, COCOeval's thresholds and
// accumulate's curve; and the host-built per-image index of the ground truth that both diagnoses walk.
// Included after az_ctx.h.  -ffp-contract=off (Makefile): every product and sum rounds once, as MATLAB's and NumPy's doubles do.
#pragma once

#include <vector>

constexpr int EVAL_VT = 256;          // threads of every workgroup that scans with block_scan (4 waves)

// VOCevaldet's overlap of detection b with box g (1-based corners), in its operation order; false: no intersection
__device__ __forceinline__ bool voc_overlap(double b0, double b1, double b2, double b3, double g0x, double g0y, double g1x,
                                            double g1y, double *ov)
{
    const double iw = (b2 < g1x ? b2 : g1x) - (b0 > g0x ? b0 : g0x) + 1.0;
    const double ih = (b3 < g1y ? b3 : g1y) - (b1 > g0y ? b1 : g0y) + 1.0;
    if (!(iw > 0.0 && ih > 0.0)) return false;
    const double ua = (b2 - b0 + 1.0) * (b3 - b1 + 1.0) + (g1x - g0x + 1.0) * (g1y - g0y + 1.0) - iw * ih;
    *ov = iw * ih / ua;
    return true;
}

// inclusive scan over the workgroup in thread order; `carry` is combined in front and updated to the total
template <typename T, typename Op>
__device__ __forceinline__ T block_scan(T v, T &carry, T *s_w, Op op)
{
    const int lane = threadIdx.x & (AZ_WAVE - 1), w = threadIdx.x / AZ_WAVE;
    for (int d = 1; d < AZ_WAVE; d <<= 1) {
        const T u = __shfl_up(v, d, AZ_WAVE);
        if (lane >= d) v = op(u, v);
    }
    if (lane == AZ_WAVE - 1) s_w[w] = v;
    __syncthreads();
    T pre = carry;
    for (int k = 0; k < w; ++k) pre = op(pre, s_w[k]);
    v = op(pre, v);
    T tot = carry;
    for (int k = 0; k < EVAL_VT / AZ_WAVE; ++k) tot = op(tot, s_w[k]);
    __syncthreads();
    carry = tot;
    return v;
}

__device__ __forceinline__ double ap_threshold(int k)
{
    // MATLAB's 0:0.1:1: the first half a + k*d, the second half b - (n-k)*d, the middle (a+b)/2
    if (k == 5) return 0.5;
    return k < 5 ? (double)k * 0.1 : 1.0 - (double)(10 - k) * 0.1;
}

// One class's curve and AP, by the whole workgroup (EVAL_VT threads): its detections are positions [lo, hi) of the
// class-ranked order, tpfp(p) gives position p's count as TP << 32 | FP (each 0 or 1), npos divides the recall.
// rec / prec / smax: [>= hi] scratch, written at [lo, hi); s_u / s_d: EVAL_VT / AZ_WAVE LDS words each.
// *ap (the 11-point AP with metric_07, else the area) and *auc (xVOCap's area) are set in thread 0 only.
template <typename F>
__device__ __forceinline__ void voc_curve_ap(int lo, int hi, long long npos, int metric_07, F tpfp, double *__restrict__ rec,
                                             double *__restrict__ prec, double *__restrict__ smax, unsigned long long *s_u,
                                             double *s_d, double *ap, double *auc)
{
    const int t = threadIdx.x;
    const double dn = (double)npos;
    // forward: tp | fp packed (each < 2^31), cumsum, rec and prec
    unsigned long long carry = 0;
    for (int p0 = lo; p0 < hi; p0 += EVAL_VT) {
        const int p = p0 + t;
        unsigned long long v = p < hi ? tpfp(p) : 0ull;
        v = block_scan(v, carry, s_u, [](unsigned long long a, unsigned long long b) { return a + b; });
        if (p < hi) {
            const double tp = (double)(v >> 32), fp = (double)(v & 0xffffffffull);
            rec[p] = tp / dn;
            prec[p] = tp / (fp + tp);
        }
    }
    __syncthreads();
    // backward: suffix max of prec, NaN ignored unless every value is NaN (MATLAB's max)
    double dcarry = NAN;
    for (int p1 = hi; p1 > lo; p1 -= EVAL_VT) {
        const int p = p1 - 1 - t;
        double v = p >= lo ? prec[p] : NAN;
        v = block_scan(v, dcarry, s_d, [](double a, double b) { return fmax(a, b); });
        if (p >= lo) smax[p] = v;
    }
    __syncthreads();
    // xVOCap: mrec = [0; rec; 1], mpre = running max of [0; prec; 0] from the end; sum where mrec changes
    double part = 0.0;
    for (int p = lo + t; p < hi; p += EVAL_VT) {
        const double prev = p > lo ? rec[p - 1] : 0.0;
        if (rec[p] != prev) part += (rec[p] - prev) * fmax(smax[p], 0.0);
    }
    {
        double zero = 0.0;
        block_scan(part, zero, s_d, [](double a, double b) { return a + b; });
        part = zero;
    }
    if (t == 0) {
        const double last = hi > lo ? rec[hi - 1] : 0.0;
        if (last != 1.0) part += (1.0 - last) * 0.0;
        double a11 = 0.0;
        if (metric_07) {
            for (int k = 0; k <= 10; ++k) {
                const double th = ap_threshold(k);
                double pk = 0.0;
                if (npos > 0) {                               // npos = 0: rec is NaN, no rec >= t
                    int a = lo, b = hi;                       // first p with rec[p] >= th (rec ascends)
                    while (a < b) {
                        const int mid = a + ((b - a) >> 1);
                        if (rec[mid] >= th) b = mid; else a = mid + 1;
                    }
                    if (a < hi) pk = smax[a];
                }
                a11 = a11 + pk / 11.0;
            }
        } else {
            a11 = part;
        }
        *ap = a11;
        *auc = part;
    }
}

// ---- COCOeval (az_coco.hip, az_cdiag.hip) ---------------------------------------------------------------------------------
constexpr int COCO_NT = 10, COCO_NR = 101;
constexpr int COCO_MAXDET = 100;      // maxDets[-1]: evaluateImg keeps a segment's first 100 detections

// np.linspace(.5, .95, 10) and np.linspace(0, 1, 101): i * step + start, the last one set to stop
__device__ __forceinline__ double iou_thr(int t) { return t == COCO_NT - 1 ? 0.95 : (double)t * ((0.95 - 0.5) / 9.0) + 0.5; }
__device__ __forceinline__ double rec_thr(int r) { return r == COCO_NR - 1 ? 1.0 : (double)r * 0.01; }

// maskApi.c bbIou of detection [dx, dy, dw, dh] (area da = dw * dh) with box [gx, gy, gw, gh]; a crowd box's union is the
// detection's area.  false (and *o untouched): w <= 0 or h <= 0, the pair does not count
__device__ __forceinline__ bool bb_iou(double dx, double dy, double dw, double dh, double da, double gx, double gy, double gw,
                                       double gh, bool crowd, double *o)
{
    const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
    if (!(w > 0.0)) return false;
    const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
    if (!(h > 0.0)) return false;
    const double i = w * h;
    const double u = crowd ? da : da + gw * gh - i;
    *o = i / u;
    return true;
}

// accumulate's curves of one (category, area range, maxDets) at NQ IoU thresholds that share one npig, by the whole workgroup
// (EVAL_VT threads): the category's detections are positions [dlo, dhi) of the class-ranked order; row(p, &tb, &fb) says
// whether position p is among its segment's first maxDets and gives its TP / FP bits (bit q: threshold q).  Cumulative
// counts are exact integers; the precision of every TP is filed under the last recall threshold it reaches (atomicMax on
// the bit pattern: pr >= 0, bits order as values), and a suffix max over the buckets is the envelope +
// searchsorted(rc, recThrs, 'left').  precision[(q * COCO_NR + r) * tstride + pcol], recall[q * tstride + rcol]; -1 where
// npig is 0.  s_w: EVAL_VT / AZ_WAVE words, bucket: NQ rows, c_r: COCO_NR ints, all LDS.
template <int NQ, typename F>
__device__ __forceinline__ void coco_curve(int dlo, int dhi, unsigned long long np, F row, double *__restrict__ precision,
                                           double *__restrict__ recall, size_t tstride, size_t pcol, size_t rcol,
                                           unsigned long long *s_w, unsigned long long (*bucket)[COCO_NR], int *c_r)
{
    const int t = threadIdx.x;
    const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
    if (np == 0) {                                   // accumulate leaves -1
        for (int e = t; e < NQ * COCO_NR; e += EVAL_VT) precision[(size_t)e * tstride + pcol] = -1.0;
        if (t < NQ) recall[(size_t)t * tstride + rcol] = -1.0;
        return;
    }
    const double dn = (double)np;
    if (t < COCO_NR) {
        const double th = rec_thr(t);
        long long x = 0, y = (long long)np;          // smallest c with c / npig >= th (c = npig gives 1.0)
        while (x < y) {
            const long long mid = (x + y) >> 1;
            if ((double)mid / dn >= th) y = mid; else x = mid + 1;
        }
        c_r[t] = (int)x;
    }
    for (int e = t; e < NQ * COCO_NR; e += EVAL_VT) bucket[e / COCO_NR][e % COCO_NR] = 0ull;
    __syncthreads();
    unsigned long long carry[NQ];
    for (int q = 0; q < NQ; ++q) carry[q] = 0;
    int nd = 0;
    for (int p0 = dlo; p0 < dhi; p0 += EVAL_VT) {
        const int p = p0 + t;
        unsigned tb = 0, fb = 0;
        bool keep = false;
        if (p < dhi) keep = row(p, &tb, &fb);
        nd += __syncthreads_count(keep);
        for (int q = 0; q < NQ; ++q) {
            const unsigned long long v = block_scan(((unsigned long long)((tb >> q) & 1u) << 32) | ((fb >> q) & 1u),
                                                    carry[q], s_w, add);
            if ((tb >> q) & 1u) {
                const long long j = (long long)(v >> 32);
                const double tp = (double)j, fp = (double)(v & 0xffffffffull);
                const double pr = tp / (fp + tp + 2.220446049250313e-16);   // np.spacing(1)
                int x = 0, y = COCO_NR - 1;                              // last r with c_r[r] <= j (c_r[0] = 0)
                while (x < y) {
                    const int mid = (x + y + 1) >> 1;
                    if (c_r[mid] <= j) x = mid; else y = mid - 1;
                }
                atomicMax(&bucket[q][x], (unsigned long long)__double_as_longlong(pr));
            }
        }
    }
    __syncthreads();
    for (int e = t; e < NQ * COCO_NR; e += EVAL_VT) {
        const int q = e / COCO_NR, r = e % COCO_NR;
        unsigned long long b = 0;
        for (int x = r; x < COCO_NR; ++x) b = bucket[q][x] > b ? bucket[q][x] : b;
        precision[(size_t)e * tstride + pcol] = __longlong_as_double((long long)b);
    }
    if (t < NQ) {
        double tot = 0.0;
        for (int q = 0; q < NQ; ++q)
            if (q == t) tot = (double)(carry[q] >> 32);
        recall[(size_t)t * tstride + rcol] = nd ? tot / dn : 0.0;
    }
}

// ---- the image-major index of the ground truth (az_ddiag.hip, az_cdiag.hip; host) ---------------------------------------
// image -> its boxes' rows in the class-major gt arrays and their classes, in (class, position) order, O(S + G): a wave
// meets the other classes' boxes without walking n_classes offset pairs per detection.  ioff [n_images + 1], ig / ic [G].
inline void image_index(int n_classes, int n_images, const int32_t *gt_off, int G, std::vector<int> &ioff, std::vector<int> &ig,
                        std::vector<int> &ic)
{
    ioff.assign((size_t)n_images + 1, 0);
    ig.resize((size_t)G);
    ic.resize((size_t)G);
    for (int k = 0; k < n_classes; ++k)
        for (int i = 0; i < n_images; ++i) {
            const long long s = (long long)k * n_images + i;
            ioff[(size_t)i + 1] += gt_off[s + 1] - gt_off[s];
        }
    for (int i = 0; i < n_images; ++i) ioff[(size_t)i + 1] += ioff[i];
    std::vector<int> fill(ioff.begin(), ioff.end() - 1);
    for (int k = 0; k < n_classes; ++k)
        for (int i = 0; i < n_images; ++i) {
            const long long s = (long long)k * n_images + i;
            for (int g = gt_off[s]; g < gt_off[s + 1]; ++g) {
                ig[(size_t)fill[i]] = g;
                ic[(size_t)fill[i]++] = k;
            }
        }
}
