// az_ddiag.hip -- why a detector's AP is what it is ("Detection diagnosis"): every detection of a VOC
// evaluation typed after Hoiem et al., "Diagnosing Error in Object Detectors" (ECCV 2012), and the AP recomputed with each
// type of error fixed, after TIDE (Bolya et al., ECCV 2020).  The layout, the ranking (rank_by_score, az_voc.hip) and the
// arithmetic (az_eval_dev.h) are az_voc_eval's; a whole image set is diagnosed in one call:
//   image index      on the host, O(S + G): per image the ground truth of every class as (box, class) in (class, position)
//                    order, so a wave meets the other classes' boxes without walking n_classes offset pairs per detection
//   k_ddiag_match    one wave per (class, image) segment, grid-striding: the segment's detections in rank order, the lanes
//                    over the image's boxes of ALL classes (64 at a time), two running maxima per lane (same class, other
//                    class) and two wave arg-max reductions, the first box in (class, position) order winning ties; the
//                    claim is the claiming detection's index in a per-box int32 -> IGN 0 / TP 1 / DUP 2 / LOC 3 / SIM 4 /
//                    OTH 5 / BG 6.  Then, in the same wave, the segment's LOC rows again in rank order: fixed where the
//                    box is not difficult, nothing claimed it in the whole first pass, and no earlier LOC row was fixed
//                    onto it (TIDE's rule)
//   k_ddiag_tables   one workgroup per class over the class-ranked order: npos and the missed objects (block_scan), the
//                    count of each type among the first floor(cut * npos) detections of every cut and in all (each row
//                    filed once under the first cut that holds it, in LDS; prefix sums over the cuts at the end)
//   k_ddiag_ap       one workgroup per class, one launch per variant over ONE set of rec / prec / smax scratch: k_voc_class's
//                    curve and AP (voc_curve_ap) with the variant's (tp, fp) of each type and its npos
// f64 throughout, -ffp-contract=off (Makefile).  The tables are integer counts: the LDS atomics' order does not show.
#include "az_ctx.h"
#include "az_eval_dev.h"

namespace {

constexpr int DT = EVAL_VT;           // threads of every workgroup here (4 waves)
constexpr int DD_MAX_CUTS = 16, DD_TYPES = 7, DD_VARIANTS = 8;
enum : int { T_IGN = 0, T_TP = 1, T_DUP = 2, T_LOC = 3, T_SIM = 4, T_OTH = 5, T_BG = 6 };

struct DdCuts { int n; double v[DD_MAX_CUTS]; };

__global__ void __launch_bounds__(DT) k_ddiag_match(int S, int n_images, const int *__restrict__ det_off,
                                                     const unsigned *__restrict__ ps, const double *__restrict__ det_box,
                                                     const int *__restrict__ gt_off, const double *__restrict__ gt_box,
                                                     const unsigned char *__restrict__ gt_diff, const int *__restrict__ img_off,
                                                     const int *__restrict__ img_g, const int *__restrict__ img_c,
                                                     const int *__restrict__ group, double min_ov, double bg_ov, int *gclaim,
                                                     unsigned char *gfix, signed char *type_out, double *__restrict__ ov_same,
                                                     int *arg_same, double *__restrict__ ov_other,
                                                     int *__restrict__ other_class, unsigned char *__restrict__ loc_fixed)
{
    const int lane = threadIdx.x & (AZ_WAVE - 1);
    const int nw = gridDim.x * (DT / AZ_WAVE);
    for (int s = blockIdx.x * (DT / AZ_WAVE) + threadIdx.x / AZ_WAVE; s < S; s += nw) {        // wave-uniform
        const int d0 = det_off[s], n = det_off[s + 1] - d0;
        if (n == 0) continue;
        const int c = s / n_images, img = s - c * n_images;
        const int g0 = gt_off[s];
        const int i0 = img_off[img], M = img_off[img + 1] - i0;
        const int gc = group ? group[c] : c;
        double q0 = 0, q1 = 0, q2 = 0, q3 = 0;            // this lane's first box (j = lane) and its class
        int qc = -1;
        if (lane < M) {
            const double *q = gt_box + (size_t)img_g[i0 + lane] * 4;
            q0 = q[0]; q1 = q[1]; q2 = q[2]; q3 = q[3];
            qc = img_c[i0 + lane];
        }
        bool any_loc = false;
        for (int c0 = 0; c0 < n; c0 += AZ_WAVE) {
            const int cnt = n - c0 < AZ_WAVE ? n - c0 : AZ_WAVE;
            unsigned my = 0;
            double m0 = 0, m1 = 0, m2 = 0, m3 = 0;
            if (lane < cnt) {
                my = ps[d0 + c0 + lane];
                const double *b = det_box + (size_t)my * 4;
                m0 = b[0]; m1 = b[1]; m2 = b[2]; m3 = b[3];
            }
            int r_ty = T_BG, r_as = -1, r_oc = -1;        // lane t keeps detection t's results
            double r_ovs = 0.0, r_ovo = 0.0;
            for (int t = 0; t < cnt; ++t) {
                const double b0 = __shfl(m0, t, AZ_WAVE), b1 = __shfl(m1, t, AZ_WAVE);
                const double b2 = __shfl(m2, t, AZ_WAVE), b3 = __shfl(m3, t, AZ_WAVE);
                const int cur = (int)__shfl(my, t, AZ_WAVE);
                double bs = -INFINITY, bo = -INFINITY;
                int js = 0x7fffffff, jo = 0x7fffffff;
                for (int j = lane; j < M; j += AZ_WAVE) {
                    double g0x = q0, g0y = q1, g1x = q2, g1y = q3;
                    int jc = qc;
                    if (j >= AZ_WAVE) {
                        const double *q = gt_box + (size_t)img_g[i0 + j] * 4;
                        g0x = q[0]; g0y = q[1]; g1x = q[2]; g1y = q[3];
                        jc = img_c[i0 + j];
                    }
                    double ov;
                    if (voc_overlap(b0, b1, b2, b3, g0x, g0y, g1x, g1y, &ov)) {
                        // j ascends per lane, and with it (class, position): the first box keeps a tie
                        if (jc == c) {
                            if (ov > bs) { bs = ov; js = j; }
                        } else if (ov > bo) { bo = ov; jo = j; }
                    }
                }
                for (int o = AZ_WAVE / 2; o > 0; o >>= 1) {
                    const double os = __shfl_xor(bs, o, AZ_WAVE), oo = __shfl_xor(bo, o, AZ_WAVE);
                    const int ojs = __shfl_xor(js, o, AZ_WAVE), ojo = __shfl_xor(jo, o, AZ_WAVE);
                    if (os > bs || (os == bs && ojs < js)) { bs = os; js = ojs; }
                    if (oo > bo || (oo == bo && ojo < jo)) { bo = oo; jo = ojo; }
                }
                // wave-uniform from here
                const bool has_s = js < M, has_o = jo < M;
                const int gs = has_s ? img_g[i0 + js] : -1;   // the box's row in gt_box
                const int oc = has_o ? img_c[i0 + jo] : -1;
                int ty;
                if (has_s && bs >= min_ov) {
                    int r = 0;
                    if (lane == 0) {                           // one lane owns every claim of the segment
                        if (gt_diff[gs]) r = T_IGN;
                        else if (gclaim[gs] < 0) { gclaim[gs] = cur; r = T_TP; }
                        else r = T_DUP;
                    }
                    ty = __shfl(r, 0, AZ_WAVE);
                } else if (has_s && bs >= bg_ov) {
                    ty = T_LOC;
                    any_loc = true;
                } else if (has_o && bo >= bg_ov) {
                    ty = gc == (group ? group[oc] : oc) ? T_SIM : T_OTH;
                } else {
                    ty = T_BG;
                }
                if (lane == t) {
                    r_ty = ty;
                    r_as = has_s ? gs - g0 : -1; r_ovs = has_s ? bs : 0.0;
                    r_oc = oc; r_ovo = has_o ? bo : 0.0;
                }
            }
            if (lane < cnt) {
                type_out[my] = (signed char)r_ty;
                ov_same[my] = r_ovs; arg_same[my] = r_as;
                ov_other[my] = r_ovo; other_class[my] = r_oc;
            }
        }
        if (!any_loc) continue;
        // the segment's LOC rows again, now that every claim of the segment is made (a later TP's too)
        for (int c0 = 0; c0 < n; c0 += AZ_WAVE) {
            const int cnt = n - c0 < AZ_WAVE ? n - c0 : AZ_WAVE;
            unsigned my = 0;
            int gs = 0;
            bool isloc = false;
            if (lane < cnt) {
                my = ps[d0 + c0 + lane];
                isloc = type_out[my] == T_LOC;                 // this lane's own store of the first pass
                if (isloc) gs = g0 + arg_same[my];
            }
            unsigned long long mask = __ballot(isloc);
            while (mask) {
                const int t = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int gt = __shfl(gs, t, AZ_WAVE);
                int r = 0;
                if (lane == 0 && !gt_diff[gt] && gclaim[gt] < 0 && !gfix[gt]) { gfix[gt] = 1; r = 1; }
                r = __shfl(r, 0, AZ_WAVE);
                if (lane == t && r) loc_fixed[my] = 1;
            }
        }
    }
}

__global__ void __launch_bounds__(DT) k_ddiag_tables(int n_images, const int *__restrict__ det_off, const int *__restrict__ gt_off,
                                                      const unsigned char *__restrict__ gt_diff, const int *__restrict__ gclaim,
                                                      const unsigned *__restrict__ pc, const signed char *__restrict__ type,
                                                      const unsigned char *__restrict__ loc_fixed, DdCuts cuts,
                                                      long long *__restrict__ table, long long *__restrict__ miss,
                                                      long long *__restrict__ fp_at, long long *__restrict__ npos8)
{
    __shared__ unsigned long long s_u[DT / AZ_WAVE];
    __shared__ unsigned s_h[(DD_MAX_CUTS + 1) * DD_TYPES];    // [cut that first holds the row | none][type]
    __shared__ unsigned s_fix;
    __shared__ int s_n[DD_MAX_CUTS];
    __shared__ unsigned long long s_np;
    const int c = blockIdx.x, t = threadIdx.x;
    const long long seg0 = (long long)c * n_images, seg1 = seg0 + n_images;
    const int lo = det_off[seg0], hi = det_off[seg1];
    const int glo = gt_off[seg0], ghi = gt_off[seg1];
    if (t < (DD_MAX_CUTS + 1) * DD_TYPES) s_h[t] = 0;
    if (t == 0) s_fix = 0;
    // npos << 32 | missed: non-difficult boxes of the class, and those of them no detection claimed
    unsigned long long np = 0;
    for (int j = glo + t; j < ghi; j += DT)
        if (!gt_diff[j]) np += (1ull << 32) | (gclaim[j] < 0 ? 1ull : 0ull);
    {
        unsigned long long zero = 0;
        block_scan(np, zero, s_u, [](unsigned long long a, unsigned long long b) { return a + b; });
        if (t == 0) s_np = zero;
    }
    __syncthreads();
    const long long npos = (long long)(s_np >> 32);
    if (t < cuts.n) {
        const double x = floor(cuts.v[t] * (double)npos);
        s_n[t] = x >= (double)(hi - lo) ? hi - lo : (int)x;
    }
    __syncthreads();
    for (int p = lo + t; p < hi; p += DT) {
        const unsigned idx = pc[p];
        const int r = p - lo;
        int b = 0;
        while (b < cuts.n && r >= s_n[b]) ++b;                // the cuts ascend: so do their counts
        atomicAdd(&s_h[b * DD_TYPES + type[idx]], 1u);
        if (loc_fixed[idx]) atomicAdd(&s_fix, 1u);
    }
    __syncthreads();
    if (t < DD_TYPES) {
        long long run = 0;
        for (int k = 0; k < cuts.n; ++k) {
            run += s_h[k * DD_TYPES + t];
            fp_at[((size_t)c * cuts.n + k) * DD_TYPES + t] = run;
        }
        run += s_h[cuts.n * DD_TYPES + t];
        table[(size_t)c * DD_TYPES + t] = run;
        if (t == T_TP) {                                      // the variants' npos: 6 the objects found, 7 + the LOC rows fixed
            for (int v = 0; v < DD_VARIANTS; ++v)
                npos8[(size_t)c * DD_VARIANTS + v] = v == 6 ? run : (v == 7 ? run + (long long)s_fix : npos);
            miss[c] = (long long)(s_np & 0xffffffffull);
        }
    }
}

__global__ void __launch_bounds__(DT) k_ddiag_ap(int n_images, const int *__restrict__ det_off, const unsigned *__restrict__ pc,
                                                  const signed char *__restrict__ type, const unsigned char *__restrict__ loc_fixed,
                                                  const long long *__restrict__ npos8, int v, int metric_07,
                                                  double *__restrict__ rec, double *__restrict__ prec, double *__restrict__ smax,
                                                  double *__restrict__ ap_fix)
{
    __shared__ unsigned long long s_u[DT / AZ_WAVE];
    __shared__ double s_d[DT / AZ_WAVE];
    const int c = blockIdx.x;
    const long long seg0 = (long long)c * n_images;
    const int lo = det_off[seg0], hi = det_off[seg0 + n_images];
    const int gone = v >= 1 && v <= 5 ? v + 1 : -1;           // the type variant v takes out: 1 DUP .. 5 BG
    const bool fix = v == 2 || v == 7;
    double ap = 0.0, auc = 0.0;
    voc_curve_ap(lo, hi, npos8[(size_t)c * DD_VARIANTS + v], metric_07, [&](int p) -> unsigned long long {
        const unsigned idx = pc[p];
        const int ty = type[idx];
        if (ty == T_TP || (fix && ty == T_LOC && loc_fixed[idx])) return 1ull << 32;
        return ty >= T_DUP && v != 7 && ty != gone ? 1ull : 0ull;
    }, rec, prec, smax, s_u, s_d, &ap, &auc);
    if (threadIdx.x == 0) ap_fix[(size_t)c * DD_VARIANTS + v] = ap;
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

int az_det_diag_eval(az_ctx *c, int n_classes, int n_images, const double *det_box, const double *det_conf,
                     const int32_t *det_off, const double *gt_box, const uint8_t *gt_difficult, const int32_t *gt_off,
                     double min_overlap, double bg_overlap, int metric_07, const int32_t *class_group, const double *cuts,
                     int n_cuts, int8_t *type_out, double *ov_same_out, int32_t *arg_same_out, double *ov_other_out,
                     int32_t *other_class_out, uint8_t *loc_fixed_out, int32_t *gt_claim_out, int64_t *type_table_out,
                     int64_t *miss_out, int64_t *fp_at_out, int64_t *npos_out, double *ap_fix_out, float *kernel_ms_out)
{
    if (!c || n_classes < 0 || n_images < 0 || !det_off || !gt_off || n_cuts < 0 || (n_cuts && !cuts))
        return fail(c, AZ_ERR_INVALID, "az_det_diag_eval: bad arguments");
    if (min_overlap != min_overlap || bg_overlap != bg_overlap || bg_overlap < 0.0 || bg_overlap > min_overlap)
        return fail(c, AZ_ERR_INVALID, "az_det_diag_eval: the thresholds need 0 <= bg_overlap <= min_overlap");
    if (n_cuts > DD_MAX_CUTS) return fail(c, AZ_ERR_INVALID, "az_det_diag_eval: at most 16 cuts");
    for (int k = 0; k < n_cuts; ++k)
        if (!std::isfinite(cuts[k]) || cuts[k] < 0.0 || (k && cuts[k] < cuts[k - 1]))      // (inf * (npos = 0) would be NaN rows)
            return fail(c, AZ_ERR_INVALID, "az_det_diag_eval: the cuts must be finite, non-negative and ascend");
    const long long S = (long long)n_classes * n_images;
    if (S >= 0x7fffffffLL)
        return fail(c, AZ_ERR_CAPACITY, "az_det_diag_eval: more segments than int32 offsets address");
    if (det_off[0] != 0 || gt_off[0] != 0) return fail(c, AZ_ERR_INVALID, "az_det_diag_eval: offsets must start at 0");
    for (long long s = 0; s < S; ++s)
        if (det_off[s + 1] < det_off[s] || gt_off[s + 1] < gt_off[s])
            return fail(c, AZ_ERR_INVALID, "az_det_diag_eval: offsets must ascend");
    const int D = det_off[S], G = gt_off[S];
    if ((D && (!det_box || !det_conf)) || (G && (!gt_box || !gt_difficult)))
        return fail(c, AZ_ERR_INVALID, "az_det_diag_eval: NULL array");
    if (n_classes == 0) {
        if (kernel_ms_out) *kernel_ms_out = 0.f;
        return AZ_OK;
    }
    size_t hist_n = 0, sums_n = 0;
    rank_scratch_sizes(D, &hist_n, &sums_n);
    if (hist_n >= 0x7fffffffULL) return fail(c, AZ_ERR_CAPACITY, "az_det_diag_eval: too many detections");
    // the image-major index of the ground truth (az_eval_dev.h)
    std::vector<int> ioff, ig, ic;
    image_index(n_classes, n_images, gt_off, G, ioff, ig, ic);
    // one arena: inputs, the index, the ranking's scratch, per-detection and per-box results, one set of curves, the tables
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    const size_t o_box = take((size_t)D * 32), o_conf = take((size_t)D * 8), o_doff = take(((size_t)S + 1) * 4);
    const size_t o_gbox = take((size_t)G * 32), o_gdif = take((size_t)G), o_goff = take(((size_t)S + 1) * 4);
    const size_t o_ioff = take(((size_t)n_images + 1) * 4), o_ig = take((size_t)G * 4), o_ic = take((size_t)G * 4);
    const size_t o_grp = take((size_t)n_classes * 4);
    const size_t o_key = take((size_t)D * 8), o_seg = take((size_t)D * 4);
    size_t o_perm[4];
    for (auto &o : o_perm) o = take((size_t)D * 4);
    const size_t o_hist = take(hist_n * 4), o_sums = take(sums_n * 4);
    const size_t o_type = take((size_t)D), o_ovs = take((size_t)D * 8), o_as = take((size_t)D * 4), o_ovo = take((size_t)D * 8);
    const size_t o_oc = take((size_t)D * 4), o_fixed = take((size_t)D), o_claim = take((size_t)G * 4), o_gfix = take((size_t)G);
    const size_t o_rec = take((size_t)D * 8), o_prec = take((size_t)D * 8), o_smax = take((size_t)D * 8);
    const size_t n_tab = (size_t)n_classes * DD_TYPES, n_fp = (size_t)n_classes * n_cuts * DD_TYPES;
    const size_t n_ap = (size_t)n_classes * DD_VARIANTS;
    const size_t o_tab = take(n_tab * 8), o_miss = take((size_t)n_classes * 8), o_fp = take(n_fp * 8);
    const size_t o_np8 = take(n_ap * 8), o_ap = take(n_ap * 8);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = scratch_grow(c, 8, off)) != AZ_OK) return rc;
    char *A = (char *)c->scratch[8].p;
    hipStream_t s = c->stream;
    auto *dbox = (double *)(A + o_box), *dconf = (double *)(A + o_conf), *gbox = (double *)(A + o_gbox);
    auto *doff = (int *)(A + o_doff), *goff = (int *)(A + o_goff), *d_ioff = (int *)(A + o_ioff);
    auto *d_ig = (int *)(A + o_ig), *d_ic = (int *)(A + o_ic), *d_grp = (int *)(A + o_grp);
    auto *gdif = (unsigned char *)(A + o_gdif), *d_fixed = (unsigned char *)(A + o_fixed), *d_gfix = (unsigned char *)(A + o_gfix);
    auto *d_type = (signed char *)(A + o_type);
    auto *d_ovs = (double *)(A + o_ovs), *d_ovo = (double *)(A + o_ovo);
    auto *d_as = (int *)(A + o_as), *d_oc = (int *)(A + o_oc), *d_claim = (int *)(A + o_claim);
    auto *rec = (double *)(A + o_rec), *prec = (double *)(A + o_prec), *smax = (double *)(A + o_smax);
    auto *d_tab = (long long *)(A + o_tab), *d_miss = (long long *)(A + o_miss), *d_fp = (long long *)(A + o_fp);
    auto *d_np8 = (long long *)(A + o_np8);
    auto *d_ap = (double *)(A + o_ap);
    if (D) {
        HIPCHK(c, hipMemcpyAsync(dbox, det_box, (size_t)D * 32, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dconf, det_conf, (size_t)D * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(d_fixed, 0, (size_t)D, s));
    }
    if (G) {
        HIPCHK(c, hipMemcpyAsync(gbox, gt_box, (size_t)G * 32, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(gdif, gt_difficult, (size_t)G, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_ig, ig.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_ic, ic.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(d_claim, 0xff, (size_t)G * 4, s));           // -1: unclaimed
        HIPCHK(c, hipMemsetAsync(d_gfix, 0, (size_t)G, s));
    }
    HIPCHK(c, hipMemcpyAsync(doff, det_off, ((size_t)S + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(goff, gt_off, ((size_t)S + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_ioff, ioff.data(), ((size_t)n_images + 1) * 4, hipMemcpyHostToDevice, s));
    if (class_group) HIPCHK(c, hipMemcpyAsync(d_grp, class_group, (size_t)n_classes * 4, hipMemcpyHostToDevice, s));
    DdCuts dc;
    dc.n = n_cuts;
    for (int k = 0; k < DD_MAX_CUTS; ++k) dc.v[k] = k < n_cuts ? cuts[k] : 0.0;
    Event e0, e1;
    if (kernel_ms_out) {
        HIPCHK(c, e0.create(hipEventDefault));
        if (e1.create(hipEventDefault) != hipSuccess) return fail(c, AZ_ERR_HIP, "az_det_diag_eval: hipEventCreate");
        hipEventRecord(e0, s);
    }
    const unsigned *pseg = nullptr, *pcls = nullptr;
    if (D) {
        RankScratch rs{(unsigned long long *)(A + o_key), (unsigned *)(A + o_seg),
                       {(unsigned *)(A + o_perm[0]), (unsigned *)(A + o_perm[1]), (unsigned *)(A + o_perm[2]),
                        (unsigned *)(A + o_perm[3])},
                       (unsigned *)(A + o_hist), (unsigned *)(A + o_sums)};
        rank_by_score(s, D, S, n_images, n_classes, (const double *)dconf, (const int *)doff, rs, &pseg, &pcls);
        long long nb = (S + (DT / AZ_WAVE) - 1) / (DT / AZ_WAVE);
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(k_ddiag_match, dim3((unsigned)nb), dim3(DT), 0, s, (int)S, n_images, (const int *)doff, pseg,
                           (const double *)dbox, (const int *)goff, (const double *)gbox, (const unsigned char *)gdif,
                           (const int *)d_ioff, (const int *)d_ig, (const int *)d_ic,
                           class_group ? (const int *)d_grp : (const int *)nullptr, min_overlap, bg_overlap, d_claim, d_gfix,
                           d_type, d_ovs, d_as, d_ovo, d_oc, d_fixed);
    }
    hipLaunchKernelGGL(k_ddiag_tables, dim3(n_classes), dim3(DT), 0, s, n_images, (const int *)doff, (const int *)goff,
                       (const unsigned char *)gdif, (const int *)d_claim, pcls, (const signed char *)d_type,
                       (const unsigned char *)d_fixed, dc, d_tab, d_miss, d_fp, d_np8);
    for (int v = 0; v < DD_VARIANTS; ++v)
        hipLaunchKernelGGL(k_ddiag_ap, dim3(n_classes), dim3(DT), 0, s, n_images, (const int *)doff, pcls,
                           (const signed char *)d_type, (const unsigned char *)d_fixed, (const long long *)d_np8, v,
                           metric_07 ? 1 : 0, rec, prec, smax, d_ap);
    if (kernel_ms_out) hipEventRecord(e1, s);
    HIPCHK(c, hipGetLastError());
    // the per-class tables are staged and reach the caller only once the whole call has succeeded; the per-row outputs
    // (D- and G-sized) are copied straight into the caller's arrays: after AZ_ERR_HIP their contents are undefined
    std::vector<int64_t> h_tab(n_tab), h_miss((size_t)n_classes), h_fp(n_fp), h_np8(n_ap);
    std::vector<double> h_ap(n_ap);
    auto back = [&](void *dst, const void *src, size_t bytes) {
        return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    HIPCHK(c, back(type_out, d_type, (size_t)D));
    HIPCHK(c, back(ov_same_out, d_ovs, (size_t)D * 8));
    HIPCHK(c, back(arg_same_out, d_as, (size_t)D * 4));
    HIPCHK(c, back(ov_other_out, d_ovo, (size_t)D * 8));
    HIPCHK(c, back(other_class_out, d_oc, (size_t)D * 4));
    HIPCHK(c, back(loc_fixed_out, d_fixed, (size_t)D));
    HIPCHK(c, back(gt_claim_out, d_claim, (size_t)G * 4));
    HIPCHK(c, back(h_tab.data(), d_tab, n_tab * 8));
    HIPCHK(c, back(h_miss.data(), d_miss, (size_t)n_classes * 8));
    HIPCHK(c, back(h_fp.data(), d_fp, n_fp * 8));
    HIPCHK(c, back(h_np8.data(), d_np8, n_ap * 8));
    HIPCHK(c, back(h_ap.data(), d_ap, n_ap * 8));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.f;
    if (kernel_ms_out) HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    if (type_table_out) memcpy(type_table_out, h_tab.data(), n_tab * 8);
    if (miss_out) memcpy(miss_out, h_miss.data(), (size_t)n_classes * 8);
    if (fp_at_out && n_fp) memcpy(fp_at_out, h_fp.data(), n_fp * 8);
    if (npos_out)
        for (int k = 0; k < n_classes; ++k) npos_out[k] = h_np8[(size_t)k * DD_VARIANTS];
    if (ap_fix_out) memcpy(ap_fix_out, h_ap.data(), n_ap * 8);
    if (kernel_ms_out) *kernel_ms_out = ms;
    return AZ_OK;
}
