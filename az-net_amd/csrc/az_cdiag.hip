// az_cdiag.hip -- why a COCO evaluation's AP@[.5:.95] is what it is ("Detection diagnosis, COCO protocol"): the
// detection diagnosis of az_ddiag.hip (Hoiem et al., ECCV 2012; TIDE, Bolya et al., ECCV 2020) under COCOeval's rules --
// area range all, maxDets 100, each of the ten IoU thresholds.  The layout, the ranking (rank_by_score, az_voc.hip) and the
// arithmetic (az_eval_dev.h: iou_thr, bb_iou, coco_curve) are az_coco_eval's; a whole result set is diagnosed in one call:
//   image index      on the host (image_index, az_eval_dev.h): per image the ground truth of every category as (box, class)
//                    in (class, position) order, crowd boxes included -- the match needs them, the maxima skip them
//   k_cdiag_match    one wave per (category, image) segment, grid-striding: its first 100 detections in rank order, one at a
//                    time.  The lanes take the image's boxes of ALL categories 64 at a time: each lane keeps two running
//                    maxima over the boxes that count (own category, other categories), and the chunk's own boxes are
//                    broadcast in position order to lanes 0-9 (one per threshold), which run evaluateImg's greedy step as
//                    k_coco_match's lanes a = 0 do.  Two wave arg-max reductions, the first box in (category, position)
//                    order winning ties.  A claim is the claiming detection's input index in a per-(threshold, box) int32.
//                    Then, in the same wave, each threshold lane walks its LOC rows again in rank order (a bit mask in
//                    registers, arg_same in LDS): fixed where nothing claimed the box at t and no earlier LOC row was
//                    fixed onto it (TIDE's rule)
//   k_cdiag_tables   one workgroup per category: the boxes that count, per threshold the count of each type, the fixed rows
//                    and the missed boxes (integer LDS atomics), and each variant's npig
//   k_cdiag_acc      one workgroup per (category, variant, threshold): coco_curve with the variant's TP / FP bit and npig
// A box "counts" when it is not a crowd box and its area field lies in [0, 1e10]: COCOeval's gtIgnore = 0 in area range all.
// f64 throughout, -ffp-contract=off (Makefile).  The tables are integer counts: the LDS atomics' order does not show.
#include "az_ctx.h"
#include "az_eval_dev.h"

namespace {

constexpr int DT = EVAL_VT;           // threads of every workgroup here (4 waves)
constexpr int NT = COCO_NT, NR = COCO_NR;
constexpr int CD_TYPES = 7, CD_VARIANTS = 8;
constexpr double AREA_HI = 1e10;      // area range all: [0, 1e5 ** 2]
enum : int { T_IGN = 0, T_TP = 1, T_DUP = 2, T_LOC = 3, T_SIM = 4, T_OTH = 5, T_BG = 6 };

__global__ void __launch_bounds__(DT) k_cdiag_match(int S, int n_images, int D, int G, const int *__restrict__ det_off,
                                                     const unsigned *__restrict__ ps, const double *__restrict__ det_box,
                                                     const int *__restrict__ gt_off, const double *__restrict__ gt_box,
                                                     const double *__restrict__ gt_area, const unsigned char *__restrict__ gt_crowd,
                                                     const int *__restrict__ img_off, const int *__restrict__ img_g,
                                                     const int *__restrict__ img_c, const int *__restrict__ group, double bg_ov,
                                                     int *gclaim, unsigned char *gfix, signed char *__restrict__ type_out,
                                                     double *__restrict__ ov_same, int *__restrict__ arg_same,
                                                     double *__restrict__ ov_other, int *__restrict__ other_class,
                                                     unsigned char *__restrict__ loc_fixed)
{
    __shared__ int s_as[DT / AZ_WAVE][COCO_MAXDET];       // per wave: the box row of each ranked detection's arg_same
    const int lane = threadIdx.x & (AZ_WAVE - 1), wv = threadIdx.x / AZ_WAVE;
    const int nw = gridDim.x * (DT / AZ_WAVE);
    const bool act = lane < NT;                           // lane t < 10: threshold t
    const double thr = iou_thr(act ? lane : 0);
    for (int s = blockIdx.x * (DT / AZ_WAVE) + wv; s < S; s += nw) {                           // wave-uniform
        const int d0 = det_off[s], n = det_off[s + 1] - d0;
        if (n == 0) continue;
        const int k = s / n_images, img = s - k * n_images;
        const int g0 = gt_off[s], Gs = gt_off[s + 1] - g0;
        const int i0 = img_off[img], M = img_off[img + 1] - i0;
        const int gk = group ? group[k] : k;
        for (int p = COCO_MAXDET + lane; p < n; p += AZ_WAVE) {    // past the cap: not evaluated
            const unsigned d = ps[d0 + p];
            for (int t = 0; t < NT; ++t) type_out[(size_t)t * D + d] = -1;
            ov_same[d] = 0.0; arg_same[d] = -1;
            ov_other[d] = 0.0; other_class[d] = -1;
        }
        const int nm = n < COCO_MAXDET ? n : COCO_MAXDET;
        unsigned long long loc0 = 0, loc1 = 0;            // this lane's LOC rows: bit r (r < 64), bit r - 64
        for (int r = 0; r < nm; ++r) {
            const unsigned d = ps[d0 + r];
            const double *db = det_box + (size_t)d * 4;
            const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
            const double da = dw * dh;
            double bs = -INFINITY, bo = -INFINITY;        // the running maxima of this lane
            int js = 0x7fffffff, jo = 0x7fffffff;
            int bn = -1, bj = -1;                         // the match: not ignored (1) / ignored (0), IoU, box row
            double bi = 0.0;
            for (int c0 = 0; c0 < M; c0 += AZ_WAVE) {
                const int cnt = M - c0 < AZ_WAVE ? M - c0 : AZ_WAVE;
                double o = 0.0;
                unsigned fl = 0;                          // bit 0: ignored; bit 1: crowd
                int row = -1;
                bool own = false;
                if (lane < cnt) {
                    const int j = c0 + lane;
                    row = img_g[i0 + j];
                    const int jc = img_c[i0 + j];
                    own = jc == k;
                    const double *q = gt_box + (size_t)row * 4;
                    const bool crowd = gt_crowd[row] != 0;
                    const double ar = gt_area[row];
                    if (crowd || ar < 0.0 || ar > AREA_HI) fl |= 1u;
                    if (crowd) fl |= 2u;
                    const bool hit = bb_iou(dx, dy, dw, dh, da, q[0], q[1], q[2], q[3], crowd, &o);
                    // j ascends per lane, and with it (category, position): the first box keeps a tie
                    if (hit && !fl) {
                        if (own) {
                            if (o > bs) { bs = o; js = j; }
                        } else if (o > bo) { bo = o; jo = j; }
                    }
                }
                unsigned long long mask = __ballot(own);  // the segment's own boxes of this chunk, in position order
                while (mask) {
                    const int jj = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const double oj = __shfl(o, jj, AZ_WAVE);
                    const unsigned fj = __shfl(fl, jj, AZ_WAVE);
                    const int rj = __shfl(row, jj, AZ_WAVE);
                    if (!act) continue;
                    const bool taken = gclaim[(size_t)lane * G + rj] >= 0;
                    if ((taken && !(fj & 2u)) || !(oj >= thr)) continue;
                    const int ni = (fj & 1u) ? 0 : 1;
                    // evaluateImg walks non-ignored boxes first and takes every box with IoU >= the best so far:
                    // the last box of the highest IoU in the first group that has one
                    if (ni > bn || (ni == bn && oj >= bi)) { bn = ni; bi = oj; bj = rj; }
                }
            }
            for (int x = AZ_WAVE / 2; x > 0; x >>= 1) {
                const double os = __shfl_xor(bs, x, AZ_WAVE), oo = __shfl_xor(bo, x, AZ_WAVE);
                const int ojs = __shfl_xor(js, x, AZ_WAVE), ojo = __shfl_xor(jo, x, AZ_WAVE);
                if (os > bs || (os == bs && ojs < js)) { bs = os; js = ojs; }
                if (oo > bo || (oo == bo && ojo < jo)) { bo = oo; jo = ojo; }
            }
            // bs, js, bo, jo are wave-uniform from here
            const bool has_s = js < M, has_o = jo < M;
            const int gs = has_s ? img_g[i0 + js] : -1;   // the box's row in gt_box
            const int oc = has_o ? img_c[i0 + jo] : -1;
            if (act) {
                int ty;
                if (bj >= 0) {
                    // a box that is not a crowd box is taken from now on (an ignored one too: evaluateImg's gtm)
                    if (!gt_crowd[bj]) gclaim[(size_t)lane * G + bj] = (int)d;
                    ty = bn == 0 ? T_IGN : T_TP;
                } else if (da < 0.0 || da > AREA_HI) {
                    ty = T_IGN;
                } else if (has_s && bs >= thr) {
                    ty = T_DUP;
                } else if (has_s && bs >= bg_ov) {
                    ty = T_LOC;
                    if (r < 64) loc0 |= 1ull << r; else loc1 |= 1ull << (r - 64);
                } else if (has_o && bo >= bg_ov) {
                    ty = gk == (group ? group[oc] : oc) ? T_SIM : T_OTH;
                } else {
                    ty = T_BG;
                }
                type_out[(size_t)lane * D + d] = (signed char)ty;
            }
            if (lane == 0) {
                s_as[wv][r] = gs;
                ov_same[d] = has_s ? bs : 0.0; arg_same[d] = has_s ? gs - g0 : -1;
                ov_other[d] = has_o ? bo : 0.0; other_class[d] = oc;
            }
        }
        // each threshold's LOC rows again, now that every claim of the segment is made (a later TP's too); the lane reads
        // its own claims, and arg_same from LDS (written by lane 0 of this wave, which runs in lockstep)
        while (loc0 | loc1) {
            int r;
            if (loc0) { r = __ffsll((long long)loc0) - 1; loc0 &= loc0 - 1; }
            else { r = 64 + __ffsll((long long)loc1) - 1; loc1 &= loc1 - 1; }
            const int gt = s_as[wv][r];
            const size_t at = (size_t)lane * G + gt;
            if (gclaim[at] < 0 && !gfix[at]) {
                gfix[at] = 1;
                loc_fixed[(size_t)lane * D + ps[d0 + r]] = 1;
            }
        }
        // gt_claim speaks of the boxes that count: an ignored box that was taken is reported unclaimed
        for (int j = lane; j < Gs; j += AZ_WAVE) {
            const double ar = gt_area[g0 + j];
            if (!gt_crowd[g0 + j] && (ar < 0.0 || ar > AREA_HI))
                for (int t = 0; t < NT; ++t) gclaim[(size_t)t * G + g0 + j] = -1;
        }
    }
}

__global__ void __launch_bounds__(DT) k_cdiag_tables(int n_images, int D, int G, const int *__restrict__ det_off,
                                                      const int *__restrict__ gt_off, const double *__restrict__ gt_area,
                                                      const unsigned char *__restrict__ gt_crowd, const int *__restrict__ gclaim,
                                                      const signed char *__restrict__ type, const unsigned char *__restrict__ loc_fixed,
                                                      long long *__restrict__ table, long long *__restrict__ miss,
                                                      long long *__restrict__ npos, long long *__restrict__ npig)
{
    __shared__ unsigned s_h[NT][CD_TYPES], s_fix[NT], s_miss[NT], s_np;
    const int k = blockIdx.x, t = threadIdx.x;
    const long long seg0 = (long long)k * n_images, seg1 = seg0 + n_images;
    const int lo = det_off[seg0], hi = det_off[seg1];
    const int glo = gt_off[seg0], ghi = gt_off[seg1];
    if (t < NT * CD_TYPES) s_h[t / CD_TYPES][t % CD_TYPES] = 0;
    if (t < NT) { s_fix[t] = 0; s_miss[t] = 0; }
    if (t == 0) s_np = 0;
    __syncthreads();
    for (int j = glo + t; j < ghi; j += DT) {
        if (gt_crowd[j] || gt_area[j] < 0.0 || gt_area[j] > AREA_HI) continue;
        atomicAdd(&s_np, 1u);
        for (int q = 0; q < NT; ++q)
            if (gclaim[(size_t)q * G + j] < 0) atomicAdd(&s_miss[q], 1u);
    }
    // the class's detections are contiguous in input order: the tables need no ranking
    for (int d = lo + t; d < hi; d += DT)
        for (int q = 0; q < NT; ++q) {
            const int ty = type[(size_t)q * D + d];
            if (ty < 0) continue;
            atomicAdd(&s_h[q][ty], 1u);
            if (loc_fixed[(size_t)q * D + d]) atomicAdd(&s_fix[q], 1u);
        }
    __syncthreads();
    if (t < NT * CD_TYPES) table[(size_t)k * NT * CD_TYPES + t] = s_h[t / CD_TYPES][t % CD_TYPES];
    if (t < NT) miss[(size_t)k * NT + t] = s_miss[t];
    if (t == 0) npos[k] = s_np;
    if (t < NT * CD_VARIANTS) {       // the variants' npig: 6 the objects found, 7 + the LOC rows fixed
        const int q = t / CD_VARIANTS, v = t % CD_VARIANTS;
        npig[((size_t)k * NT + q) * CD_VARIANTS + v] =
            v == 6 ? (long long)s_h[q][T_TP] : (v == 7 ? (long long)s_h[q][T_TP] + (long long)s_fix[q] : (long long)s_np);
    }
}

__global__ void __launch_bounds__(DT) k_cdiag_acc(int K, int n_images, int D, const int *__restrict__ det_off,
                                                   const unsigned *__restrict__ pc, const signed char *__restrict__ type,
                                                   const unsigned char *__restrict__ loc_fixed, const long long *__restrict__ npig,
                                                   double *__restrict__ precision, double *__restrict__ recall)
{
    __shared__ unsigned long long s_w[DT / AZ_WAVE];
    __shared__ unsigned long long bucket[1][NR];
    __shared__ int c_r[NR];
    const int q = blockIdx.x % NT, v = (blockIdx.x / NT) % CD_VARIANTS, k = blockIdx.x / (NT * CD_VARIANTS);
    const long long seg0 = (long long)k * n_images;
    const int dlo = det_off[seg0], dhi = det_off[seg0 + n_images];
    const int gone = v >= 1 && v <= 5 ? v + 1 : -1;           // the type variant v takes out: 1 DUP .. 5 BG
    const bool fix = v == 2 || v == 7;
    const signed char *ty_q = type + (size_t)q * D;
    const unsigned char *fx_q = loc_fixed + (size_t)q * D;
    // prec_fix [8][10][101][K], recall_fix [8][10][K]
    coco_curve<1>(dlo, dhi, (unsigned long long)npig[((size_t)k * NT + q) * CD_VARIANTS + v],
                  [&](int p, unsigned *tb, unsigned *fb) {
                      const unsigned d = pc[p];
                      const int ty = ty_q[d];
                      if (ty < 0) return false;               // past its segment's first 100
                      const bool tp = ty == T_TP || (fix && ty == T_LOC && fx_q[d]);
                      *tb = tp ? 1u : 0u;
                      *fb = !tp && ty >= T_DUP && v != 7 && ty != gone ? 1u : 0u;
                      return true;
                  },
                  precision, recall, (size_t)K, ((size_t)v * NT + q) * NR * K + k, ((size_t)v * NT + q) * K + k, s_w, bucket, c_r);
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

int az_coco_diag_eval(az_ctx *c, int n_classes, int n_images, const double *det_box, const double *det_score,
                      const int32_t *det_off, const double *gt_box, const double *gt_area, const uint8_t *gt_crowd,
                      const int32_t *gt_off, double bg_overlap, const int32_t *class_group, double *ov_same_out,
                      int32_t *arg_same_out, double *ov_other_out, int32_t *other_class_out, int8_t *type_out,
                      uint8_t *loc_fixed_out, int32_t *gt_claim_out, int64_t *npos_out, int64_t *type_table_out,
                      int64_t *miss_out, double *prec_fix_out, double *recall_fix_out, float *kernel_ms_out)
{
    if (!c || n_classes < 0 || n_images < 0 || !det_off || !gt_off)
        return fail(c, AZ_ERR_INVALID, "az_coco_diag_eval: bad arguments");
    if (bg_overlap != bg_overlap || bg_overlap < 0.0 || bg_overlap > 0.5)
        return fail(c, AZ_ERR_INVALID, "az_coco_diag_eval: bg_overlap must lie in [0, 0.5]");
    const long long S = (long long)n_classes * n_images;
    if (S >= 0x7fffffffLL || (long long)n_classes * CD_VARIANTS * NT * NR >= 0x7fffffffLL)
        return fail(c, AZ_ERR_CAPACITY, "az_coco_diag_eval: more segments than int32 offsets address");
    if (det_off[0] != 0 || gt_off[0] != 0) return fail(c, AZ_ERR_INVALID, "az_coco_diag_eval: offsets must start at 0");
    for (long long s = 0; s < S; ++s)
        if (det_off[s + 1] < det_off[s] || gt_off[s + 1] < gt_off[s])
            return fail(c, AZ_ERR_INVALID, "az_coco_diag_eval: offsets must ascend");
    const int D = det_off[S], G = gt_off[S];
    if ((D && (!det_box || !det_score)) || (G && (!gt_box || !gt_area || !gt_crowd)))
        return fail(c, AZ_ERR_INVALID, "az_coco_diag_eval: NULL array");
    size_t hist_n = 0, sums_n = 0;
    rank_scratch_sizes(D, &hist_n, &sums_n);
    if (hist_n >= 0x7fffffffULL) return fail(c, AZ_ERR_CAPACITY, "az_coco_diag_eval: too many detections");
    if (n_classes == 0) {
        if (kernel_ms_out) *kernel_ms_out = 0.f;
        return AZ_OK;
    }
    const size_t K = (size_t)n_classes;
    const size_t n_tab = K * NT * CD_TYPES, n_miss = K * NT, n_npig = K * NT * CD_VARIANTS;
    const size_t n_prec = (size_t)CD_VARIANTS * NT * NR * K, n_rec = (size_t)CD_VARIANTS * NT * K;
    std::vector<int> ioff, ig, ic;
    image_index(n_classes, n_images, gt_off, G, ioff, ig, ic);
    // one arena: inputs, the index, the ranking's scratch, per-detection and per-box results, the tables, the curves
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    const size_t o_box = take((size_t)D * 32), o_score = take((size_t)D * 8), o_doff = take(((size_t)S + 1) * 4);
    const size_t o_gbox = take((size_t)G * 32), o_garea = take((size_t)G * 8), o_gcrowd = take((size_t)G);
    const size_t o_goff = take(((size_t)S + 1) * 4);
    const size_t o_ioff = take(((size_t)n_images + 1) * 4), o_ig = take((size_t)G * 4), o_ic = take((size_t)G * 4);
    const size_t o_grp = take(K * 4);
    const size_t o_key = take((size_t)D * 8), o_seg = take((size_t)D * 4);
    size_t o_perm[4];
    for (auto &o : o_perm) o = take((size_t)D * 4);
    const size_t o_hist = take(hist_n * 4), o_sums = take(sums_n * 4);
    const size_t o_type = take((size_t)D * NT), o_fixed = take((size_t)D * NT);
    const size_t o_ovs = take((size_t)D * 8), o_as = take((size_t)D * 4), o_ovo = take((size_t)D * 8), o_oc = take((size_t)D * 4);
    const size_t o_claim = take((size_t)G * NT * 4), o_gfix = take((size_t)G * NT);
    const size_t o_tab = take(n_tab * 8), o_miss = take(n_miss * 8), o_npos = take(K * 8), o_npig = take(n_npig * 8);
    const size_t o_prec = take(n_prec * 8), o_rec = take(n_rec * 8);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = scratch_grow(c, 9, off)) != AZ_OK) return rc;
    char *A = (char *)c->scratch[9].p;
    hipStream_t s = c->stream;
    auto *dbox = (double *)(A + o_box), *dscore = (double *)(A + o_score), *gbox = (double *)(A + o_gbox);
    auto *garea = (double *)(A + o_garea);
    auto *gcrowd = (unsigned char *)(A + o_gcrowd), *d_fixed = (unsigned char *)(A + o_fixed), *d_gfix = (unsigned char *)(A + o_gfix);
    auto *doff = (int *)(A + o_doff), *goff = (int *)(A + o_goff), *d_ioff = (int *)(A + o_ioff);
    auto *d_ig = (int *)(A + o_ig), *d_ic = (int *)(A + o_ic), *d_grp = (int *)(A + o_grp);
    auto *d_type = (signed char *)(A + o_type);
    auto *d_ovs = (double *)(A + o_ovs), *d_ovo = (double *)(A + o_ovo);
    auto *d_as = (int *)(A + o_as), *d_oc = (int *)(A + o_oc), *d_claim = (int *)(A + o_claim);
    auto *d_tab = (long long *)(A + o_tab), *d_miss = (long long *)(A + o_miss), *d_npos = (long long *)(A + o_npos);
    auto *d_npig = (long long *)(A + o_npig);
    auto *d_prec = (double *)(A + o_prec), *d_rec = (double *)(A + o_rec);
    if (D) {
        HIPCHK(c, hipMemcpyAsync(dbox, det_box, (size_t)D * 32, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dscore, det_score, (size_t)D * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(d_fixed, 0, (size_t)D * NT, s));
    }
    if (G) {
        HIPCHK(c, hipMemcpyAsync(gbox, gt_box, (size_t)G * 32, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(garea, gt_area, (size_t)G * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(gcrowd, gt_crowd, (size_t)G, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_ig, ig.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_ic, ic.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(d_claim, 0xff, (size_t)G * NT * 4, s));      // -1: unclaimed
        HIPCHK(c, hipMemsetAsync(d_gfix, 0, (size_t)G * NT, s));
    }
    HIPCHK(c, hipMemcpyAsync(doff, det_off, ((size_t)S + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(goff, gt_off, ((size_t)S + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_ioff, ioff.data(), ((size_t)n_images + 1) * 4, hipMemcpyHostToDevice, s));
    if (class_group) HIPCHK(c, hipMemcpyAsync(d_grp, class_group, K * 4, hipMemcpyHostToDevice, s));
    Event e0, e1;
    if (kernel_ms_out) {
        HIPCHK(c, e0.create(hipEventDefault));
        if (e1.create(hipEventDefault) != hipSuccess) return fail(c, AZ_ERR_HIP, "az_coco_diag_eval: hipEventCreate");
        hipEventRecord(e0, s);
    }
    const unsigned *pseg = nullptr, *pcls = nullptr;
    if (D) {
        RankScratch rs{(unsigned long long *)(A + o_key), (unsigned *)(A + o_seg),
                       {(unsigned *)(A + o_perm[0]), (unsigned *)(A + o_perm[1]), (unsigned *)(A + o_perm[2]),
                        (unsigned *)(A + o_perm[3])},
                       (unsigned *)(A + o_hist), (unsigned *)(A + o_sums)};
        rank_by_score(s, D, S, n_images, n_classes, (const double *)dscore, (const int *)doff, rs, &pseg, &pcls);
        long long nb = (S + (DT / AZ_WAVE) - 1) / (DT / AZ_WAVE);
        if (nb > 8192) nb = 8192;
        hipLaunchKernelGGL(k_cdiag_match, dim3((unsigned)nb), dim3(DT), 0, s, (int)S, n_images, D, G, (const int *)doff, pseg,
                           (const double *)dbox, (const int *)goff, (const double *)gbox, (const double *)garea,
                           (const unsigned char *)gcrowd, (const int *)d_ioff, (const int *)d_ig, (const int *)d_ic,
                           class_group ? (const int *)d_grp : (const int *)nullptr, bg_overlap, d_claim, d_gfix, d_type, d_ovs,
                           d_as, d_ovo, d_oc, d_fixed);
    }
    hipLaunchKernelGGL(k_cdiag_tables, dim3(n_classes), dim3(DT), 0, s, n_images, D, G, (const int *)doff, (const int *)goff,
                       (const double *)garea, (const unsigned char *)gcrowd, (const int *)d_claim, (const signed char *)d_type,
                       (const unsigned char *)d_fixed, d_tab, d_miss, d_npos, d_npig);
    hipLaunchKernelGGL(k_cdiag_acc, dim3((unsigned)(n_classes * CD_VARIANTS * NT)), dim3(DT), 0, s, n_classes, n_images, D,
                       (const int *)doff, pcls, (const signed char *)d_type, (const unsigned char *)d_fixed,
                       (const long long *)d_npig, d_prec, d_rec);
    if (kernel_ms_out) hipEventRecord(e1, s);
    HIPCHK(c, hipGetLastError());
    // the per-class tables and the curves are staged and reach the caller only once the whole call has succeeded; the
    // per-row outputs (D- and G-sized) are copied straight into the caller's arrays: after AZ_ERR_HIP their contents are
    // undefined
    std::vector<int64_t> h_tab(n_tab), h_miss(n_miss), h_npos(K);
    std::vector<double> h_prec(prec_fix_out ? n_prec : 0), h_rec(recall_fix_out ? n_rec : 0);
    auto back = [&](void *dst, const void *src, size_t bytes) {
        return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    HIPCHK(c, back(ov_same_out, d_ovs, (size_t)D * 8));
    HIPCHK(c, back(arg_same_out, d_as, (size_t)D * 4));
    HIPCHK(c, back(ov_other_out, d_ovo, (size_t)D * 8));
    HIPCHK(c, back(other_class_out, d_oc, (size_t)D * 4));
    HIPCHK(c, back(type_out, d_type, (size_t)D * NT));
    HIPCHK(c, back(loc_fixed_out, d_fixed, (size_t)D * NT));
    HIPCHK(c, back(gt_claim_out, d_claim, (size_t)G * NT * 4));
    HIPCHK(c, back(h_tab.data(), d_tab, n_tab * 8));
    HIPCHK(c, back(h_miss.data(), d_miss, n_miss * 8));
    HIPCHK(c, back(h_npos.data(), d_npos, K * 8));
    HIPCHK(c, back(prec_fix_out ? h_prec.data() : nullptr, d_prec, n_prec * 8));
    HIPCHK(c, back(recall_fix_out ? h_rec.data() : nullptr, d_rec, n_rec * 8));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.f;
    if (kernel_ms_out) HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    if (type_table_out) memcpy(type_table_out, h_tab.data(), n_tab * 8);
    if (miss_out) memcpy(miss_out, h_miss.data(), n_miss * 8);
    if (npos_out) memcpy(npos_out, h_npos.data(), K * 8);
    if (prec_fix_out) memcpy(prec_fix_out, h_prec.data(), n_prec * 8);
    if (recall_fix_out) memcpy(recall_fix_out, h_rec.data(), n_rec * 8);
    if (kernel_ms_out) *kernel_ms_out = ms;
    return AZ_OK;
}
