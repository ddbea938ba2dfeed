// az_coco.hip -- imdb.evaluate_detections for COCO (lib/datasets/coco.py:_do_coco_eval, which runs pycocotools'
// COCOeval evaluate / accumulate / summarize), box IoU.  The semantics are restated in DESIGN §1c; every category of a
// result set is evaluated in one call:
//   rank_by_score   (az_voc.hip) stable LSD radix passes over the f64 scores: each (category, image) segment's
//                   detections and each category's detections in (-score, input order) -- both of COCOeval's mergesorts
//   k_coco_match    one wave per (category, image) segment, grid-striding: its first 100 detections in rank order, one at a
//                   time; the lanes compute the f64 IoU against 64 ground-truth boxes at a time, then lane a*10+t (40 lanes)
//                   runs evaluateImg's greedy step for area range a and IoU threshold t over those boxes (broadcast by
//                   shuffles), holding its claims in a register (the first 64 boxes) or in a byte per (box, lane) in HBM.
//                   Result: per detection a 40-bit TP mask and a 40-bit FP mask (bit a*10+t) and its rank in the segment
//   k_coco_acc      one workgroup per (category, area range, maxDets): npig, the category's detections in rank order with
//                   segment rank < maxDets, cumulative TP / FP counts per threshold (exact integers), precision at every
//                   TP, bucketed by the recall thresholds it reaches; a suffix max over the buckets is accumulate's
//                   envelope + searchsorted(rc, recThrs, 'left')
// summarize runs on the host over the copied precision / recall, with NumPy's pairwise mean.
// -ffp-contract=off (Makefile): every product and sum rounds once, as maskApi.c's and NumPy's double arithmetic do.
#include "az_ctx.h"
#include "az_eval_dev.h"

#include <vector>

namespace {

constexpr int CT = EVAL_VT;           // threads of every workgroup here (4 waves)
constexpr int NT = COCO_NT, NR = COCO_NR, NA = 4, NM = 3;
constexpr int MAXDET = COCO_MAXDET;
constexpr int NL = NA * NT;           // (area range, threshold) lanes of k_coco_match
// iou_thr, rec_thr, bb_iou and accumulate's curve (coco_curve) live in az_eval_dev.h: az_cdiag.hip (az_coco_diag_eval)
// calls the same.
__device__ __forceinline__ double area_lo(int a) { return a == 2 ? 1024.0 : (a == 3 ? 9216.0 : 0.0); }
__device__ __forceinline__ double area_hi(int a) { return a == 1 ? 1024.0 : (a == 2 ? 9216.0 : 1e10); }

__global__ void __launch_bounds__(CT) k_coco_match(int S, int D, const int *__restrict__ det_off, const unsigned *__restrict__ ps,
                                                    const double *__restrict__ det_box, const int *__restrict__ gt_off,
                                                    const double *__restrict__ gt_box, const double *__restrict__ gt_area,
                                                    const unsigned char *__restrict__ gt_crowd, unsigned char *__restrict__ claim,
                                                    int *__restrict__ segrank, unsigned long long *__restrict__ tpm,
                                                    unsigned long long *__restrict__ fpm, int *__restrict__ mout,
                                                    signed char *__restrict__ iout)
{
    const int lane = threadIdx.x & (AZ_WAVE - 1);
    const int nw = gridDim.x * (CT / AZ_WAVE);
    const bool act = lane < NL;
    const int a = act ? lane / NT : 0, t = act ? lane % NT : 0;
    const double thr = iou_thr(t), lo = area_lo(a), hi = area_hi(a);
    for (int s = blockIdx.x * (CT / AZ_WAVE) + threadIdx.x / AZ_WAVE; s < S; s += nw) {
        const int d0 = det_off[s], n = det_off[s + 1] - d0;
        if (n == 0) continue;
        const int g0 = gt_off[s], G = gt_off[s + 1] - g0;
        for (int p = lane; p < n; p += AZ_WAVE) {
            const unsigned d = ps[d0 + p];
            segrank[d] = p;
            if (p >= MAXDET && mout)
                for (int l = 0; l < NL; ++l) {
                    mout[(size_t)l * D + d] = -1;
                    iout[(size_t)l * D + d] = -1;
                }
        }
        const int nm = n < MAXDET ? n : MAXDET;
        unsigned long long claim0 = 0;                    // bit j: this lane's (a, t) has matched box j (j < 64)
        for (int r = 0; r < nm; ++r) {
            const unsigned d = ps[d0 + r];
            const double *db = det_box + (size_t)d * 4;
            const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
            const double da = dw * dh;
            int bn = -1, bj = -1;                         // best: not ignored (1) / ignored (0), IoU, box
            double bi = 0.0;
            for (int c0 = 0; c0 < G; c0 += AZ_WAVE) {
                const int cnt = G - c0 < AZ_WAVE ? G - c0 : AZ_WAVE;
                double o = 0.0;
                unsigned fl = 0;                          // bits 0-3: ignored in area range a; bit 4: crowd
                if (lane < cnt) {
                    const int j = g0 + c0 + lane;
                    const double *q = gt_box + (size_t)j * 4;
                    const double gx = q[0], gy = q[1], gw = q[2], gh = q[3];
                    const bool crowd = gt_crowd[j] != 0;
                    const double ar = gt_area[j];
                    for (int k = 0; k < NA; ++k)
                        if (crowd || ar < area_lo(k) || ar > area_hi(k)) fl |= 1u << k;
                    if (crowd) fl |= 16u;
                    bb_iou(dx, dy, dw, dh, da, gx, gy, gw, gh, crowd, &o);
                }
                for (int jj = 0; jj < cnt; ++jj) {
                    const double oj = __shfl(o, jj, AZ_WAVE);
                    const unsigned fj = __shfl(fl, jj, AZ_WAVE);
                    if (!act) continue;
                    const int j = c0 + jj;
                    const bool taken = j < AZ_WAVE ? ((claim0 >> j) & 1ull) != 0 : claim[(size_t)(g0 + j) * NL + lane] != 0;
                    if ((taken && !(fj & 16u)) || !(oj >= thr)) continue;
                    const int ni = (fj >> a) & 1u ? 0 : 1;
                    // evaluateImg walks non-ignored boxes first and takes every box with IoU >= the best so far:
                    // the last box of the highest IoU in the first group that has one
                    if (ni > bn || (ni == bn && oj >= bi)) { bn = ni; bi = oj; bj = j; }
                }
            }
            bool ign;
            if (bj >= 0) {
                if (bj < AZ_WAVE) claim0 |= 1ull << bj;
                else claim[(size_t)(g0 + bj) * NL + lane] = 1;
                ign = bn == 0;
            } else {
                ign = da < lo || da > hi;
            }
            const unsigned long long tb = __ballot(act && bj >= 0 && !ign), fb = __ballot(act && bj < 0 && !ign);
            if (lane == 0) { tpm[d] = tb; fpm[d] = fb; }
            if (mout && act) {
                mout[(size_t)lane * D + d] = bj;
                iout[(size_t)lane * D + d] = ign ? 1 : 0;
            }
        }
    }
}

__global__ void __launch_bounds__(CT) k_coco_acc(int K, int n_images, const int *__restrict__ det_off,
                                                  const int *__restrict__ gt_off, const double *__restrict__ gt_area,
                                                  const unsigned char *__restrict__ gt_crowd, const unsigned *__restrict__ pc,
                                                  const int *__restrict__ segrank, const unsigned long long *__restrict__ tpm,
                                                  const unsigned long long *__restrict__ fpm, double *__restrict__ precision,
                                                  double *__restrict__ recall)
{
    __shared__ unsigned long long s_w[CT / AZ_WAVE];
    __shared__ unsigned long long bucket[NT][NR];   // bit pattern of the highest precision reached in each recall bucket
    __shared__ int c_r[NR];                         // fewest TPs whose recall reaches recThrs[r]
    const int t = threadIdx.x;
    const int m = blockIdx.x % NM, a = (blockIdx.x / NM) % NA, k = blockIdx.x / (NM * NA);
    const int maxdet = m == 0 ? 1 : (m == 1 ? 10 : 100);
    const double lo = area_lo(a), hi = area_hi(a);
    const long long seg0 = (long long)k * n_images, seg1 = seg0 + n_images;
    const int dlo = det_off[seg0], dhi = det_off[seg1], glo = gt_off[seg0], ghi = gt_off[seg1];
    const size_t col = ((size_t)k * NA + a) * NM + m;            // (k, a, m) in [.., K, A, M]
    const size_t tstride = (size_t)K * NA * NM;
    unsigned long long np = 0;
    for (int j = glo + t; j < ghi; j += CT) np += (gt_crowd[j] || gt_area[j] < lo || gt_area[j] > hi) ? 0u : 1u;
    {
        unsigned long long zero = 0;
        block_scan(np, zero, s_w, [](unsigned long long x, unsigned long long y) { return x + y; });
        np = zero;
    }
    coco_curve<NT>(dlo, dhi, np, [&](int p, unsigned *tb, unsigned *fb) {
        const unsigned d = pc[p];
        if (segrank[d] >= maxdet) return false;
        *tb = (unsigned)(tpm[d] >> (NT * a)) & 1023u;
        *fb = (unsigned)(fpm[d] >> (NT * a)) & 1023u;
        return true;
    }, precision, recall, tstride, col, col, s_w, bucket, c_r);
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// NumPy's add.reduce of a contiguous f64 array: pairwise_sum over each 8192-element buffer, the buffers added in turn
double pairwise_sum(const double *a, size_t n)
{
    if (n < 8) {
        double r = 0.0;
        for (size_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        size_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum(a, n2) + pairwise_sum(a + n2, n - n2);
}

double np_mean_or_m1(const std::vector<double> &v)   // summarize: np.mean(s[s > -1]), or -1 if empty
{
    if (v.empty()) return -1.0;
    double s = 0.0;
    for (size_t c = 0; c < v.size(); c += 8192) s += pairwise_sum(v.data() + c, v.size() - c < 8192 ? v.size() - c : 8192);
    return s / (double)v.size();
}

}  // namespace

int az_coco_eval(az_ctx *c, int n_classes, int n_images, const double *det_box, const double *det_score,
                 const int32_t *det_off, const double *gt_box, const double *gt_area, const uint8_t *gt_crowd,
                 const int32_t *gt_off, double *precision_out, double *recall_out, double *stats_out,
                 int32_t *dt_match_out, int8_t *dt_ignore_out)
{
    if (!c || n_classes < 0 || n_images < 0 || !det_off || !gt_off || !stats_out || (!dt_match_out != !dt_ignore_out))
        return fail(c, AZ_ERR_INVALID, "az_coco_eval: bad arguments");
    const long long S = (long long)n_classes * n_images;
    if (S >= 0x7fffffffLL || (long long)n_classes * NA * NM * NT * NR >= 0x7fffffffLL)
        return fail(c, AZ_ERR_CAPACITY, "az_coco_eval: more segments than int32 offsets address");
    if (det_off[0] != 0 || gt_off[0] != 0) return fail(c, AZ_ERR_INVALID, "az_coco_eval: offsets must start at 0");
    for (long long s = 0; s < S; ++s)
        if (det_off[s + 1] < det_off[s] || gt_off[s + 1] < gt_off[s])
            return fail(c, AZ_ERR_INVALID, "az_coco_eval: offsets must ascend");
    const int D = det_off[S], G = gt_off[S];
    if ((D && (!det_box || !det_score)) || (G && (!gt_box || !gt_area || !gt_crowd)))
        return fail(c, AZ_ERR_INVALID, "az_coco_eval: NULL array");
    size_t hist_n = 0, sums_n = 0;
    rank_scratch_sizes(D, &hist_n, &sums_n);
    if (hist_n >= 0x7fffffffULL)
        return fail(c, AZ_ERR_CAPACITY, "az_coco_eval: too many detections");
    const size_t nprec = (size_t)NT * NR * n_classes * NA * NM, nrec = (size_t)NT * n_classes * NA * NM;
    std::vector<double> prec(nprec), rec(nrec);
    if (n_classes && n_images) {
        // one arena: inputs, ranking scratch, per-detection results, claims, precision / recall
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
        const size_t o_box = take((size_t)D * 32), o_score = take((size_t)D * 8), o_doff = take(((size_t)S + 1) * 4);
        const size_t o_gbox = take((size_t)G * 32), o_garea = take((size_t)G * 8), o_gcrowd = take((size_t)G);
        const size_t o_goff = take(((size_t)S + 1) * 4), o_key = take((size_t)D * 8), o_seg = take((size_t)D * 4);
        size_t o_perm[4];
        for (auto &o : o_perm) o = take((size_t)D * 4);
        const size_t o_hist = take(hist_n * 4), o_sums = take(sums_n * 4), o_rank = take((size_t)D * 4);
        const size_t o_tpm = take((size_t)D * 8), o_fpm = take((size_t)D * 8), o_claim = take((size_t)G * NL);
        const size_t o_mout = dt_match_out ? take((size_t)D * NL * 4) : 0, o_iout = dt_match_out ? take((size_t)D * NL) : 0;
        const size_t o_prec = take(nprec * 8), o_rec = take(nrec * 8);
        HIPCHK(c, hipSetDevice(c->device));
        int rc;
        if ((rc = scratch_grow(c, 9, off)) != AZ_OK) return rc;
        char *A = (char *)c->scratch[9].p;
        hipStream_t s = c->stream;
        auto *dbox = (double *)(A + o_box), *dscore = (double *)(A + o_score), *gbox = (double *)(A + o_gbox);
        auto *garea = (double *)(A + o_garea);
        auto *gcrowd = (unsigned char *)(A + o_gcrowd), *claim = (unsigned char *)(A + o_claim);
        auto *doff = (int *)(A + o_doff), *goff = (int *)(A + o_goff), *segrank = (int *)(A + o_rank);
        auto *tpm = (unsigned long long *)(A + o_tpm), *fpm = (unsigned long long *)(A + o_fpm);
        auto *mout = dt_match_out ? (int *)(A + o_mout) : nullptr;
        auto *iout = dt_match_out ? (signed char *)(A + o_iout) : nullptr;
        auto *dprec = (double *)(A + o_prec), *drec = (double *)(A + o_rec);
        if (D) {
            HIPCHK(c, hipMemcpyAsync(dbox, det_box, (size_t)D * 32, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(dscore, det_score, (size_t)D * 8, hipMemcpyHostToDevice, s));
        }
        if (G) {
            HIPCHK(c, hipMemcpyAsync(gbox, gt_box, (size_t)G * 32, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(garea, gt_area, (size_t)G * 8, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(gcrowd, gt_crowd, (size_t)G, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemsetAsync(claim, 0, (size_t)G * NL, s));
        }
        HIPCHK(c, hipMemcpyAsync(doff, det_off, ((size_t)S + 1) * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(goff, gt_off, ((size_t)S + 1) * 4, hipMemcpyHostToDevice, s));
        const unsigned *pseg = nullptr, *pcls = nullptr;
        if (D) {
            RankScratch rs{(unsigned long long *)(A + o_key), (unsigned *)(A + o_seg),
                           {(unsigned *)(A + o_perm[0]), (unsigned *)(A + o_perm[1]), (unsigned *)(A + o_perm[2]),
                            (unsigned *)(A + o_perm[3])},
                           (unsigned *)(A + o_hist), (unsigned *)(A + o_sums)};
            rank_by_score(s, D, S, n_images, n_classes, (const double *)dscore, (const int *)doff, rs, &pseg, &pcls);
            long long nb = (S + (CT / AZ_WAVE) - 1) / (CT / AZ_WAVE);
            if (nb > 8192) nb = 8192;
            hipLaunchKernelGGL(k_coco_match, dim3((unsigned)nb), dim3(CT), 0, s, (int)S, D, (const int *)doff, pseg,
                               (const double *)dbox, (const int *)goff, (const double *)gbox, (const double *)garea,
                               (const unsigned char *)gcrowd, claim, segrank, tpm, fpm, mout, iout);
        }
        hipLaunchKernelGGL(k_coco_acc, dim3((unsigned)(n_classes * NA * NM)), dim3(CT), 0, s, n_classes, n_images,
                           (const int *)doff, (const int *)goff, (const double *)garea, (const unsigned char *)gcrowd, pcls,
                           (const int *)segrank, (const unsigned long long *)tpm, (const unsigned long long *)fpm, dprec, drec);
        HIPCHK(c, hipGetLastError());
        if (D && dt_match_out) {
            HIPCHK(c, hipMemcpyAsync(dt_match_out, mout, (size_t)D * NL * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipMemcpyAsync(dt_ignore_out, iout, (size_t)D * NL, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(c, hipMemcpyAsync(prec.data(), dprec, nprec * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(rec.data(), drec, nrec * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    } else {
        // no segments: every entry stays -1, as accumulate leaves it
        for (auto &v : prec) v = -1.0;
        for (auto &v : rec) v = -1.0;
    }
    // summarize (_summarizeDets): {ap, iou index or -1, area, maxDets index}
    static const int spec[12][4] = {{1, -1, 0, 2}, {1, 0, 0, 2}, {1, 5, 0, 2}, {1, -1, 1, 2}, {1, -1, 2, 2}, {1, -1, 3, 2},
                                    {0, -1, 0, 0}, {0, -1, 0, 1}, {0, -1, 0, 2}, {0, -1, 1, 2}, {0, -1, 2, 2}, {0, -1, 3, 2}};
    const size_t K = (size_t)n_classes;
    for (int q = 0; q < 12; ++q) {
        const int ap = spec[q][0], ti = spec[q][1], ai = spec[q][2], mi = spec[q][3];
        std::vector<double> v;
        for (int t = 0; t < NT; ++t) {
            if (ti >= 0 && t != ti) continue;
            const int nr = ap ? NR : 1;
            for (int r = 0; r < nr; ++r)
                for (size_t k = 0; k < K; ++k) {
                    const double x = ap ? prec[(((size_t)t * NR + r) * K + k) * NA * NM + ai * NM + mi]
                                        : rec[((size_t)t * K + k) * NA * NM + ai * NM + mi];
                    if (x > -1.0) v.push_back(x);
                }
        }
        stats_out[q] = np_mean_or_m1(v);
    }
    if (precision_out) std::copy(prec.begin(), prec.end(), precision_out);
    if (recall_out) std::copy(rec.begin(), rec.end(), recall_out);
    return AZ_OK;
}
