// az_eval_dev.h -- the device arithmetic that az_voc.hip (az_voc_eval) and az_ddiag.hip (az_det_diag_eval) share, so the
// diagnosis cannot drift from the evaluation it explains: VOCevaldet's overlap, the workgroup scan, xVOCap's curve and AP.
// Included after az_ctx.h.  -ffp-contract=off (Makefile): every product and sum rounds once, as MATLAB's doubles do.
#pragma once

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
