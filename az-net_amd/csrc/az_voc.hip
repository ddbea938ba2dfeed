// az_voc.hip -- imdb.evaluate_detections for PASCAL VOC (lib/datasets/pascal_voc.py:147-190, which hands the results
// files to the devkit's VOCevaldet.m and the wrapper's xVOCap.m under MATLAB).  The semantics are restated in DESIGN §1b;
// every class of an image set is evaluated in one call:
//   k_voc_prep      per detection: order-preserving u64 key of -confidence (ascending key = MATLAB's sort(-conf)),
//                   and its segment (class * n_images + image) by a binary search of det_off
//   k_voc_hist /    one stable LSD radix pass (8-bit digit) over a permutation: per-tile digit counts, one scan of the
//   k_voc_scan* /   [digit][tile] table (chunk sums, their scan, chunks from their base), and a scatter that ranks equal digits inside each wave with 8 ballots
//   k_voc_scatter   (wave, then wave-order offsets in LDS): ties keep their order, so
//                     8 key passes          -> every detection ranked by (-conf, file order)
//                     + segment-id passes   -> each (class, image) segment's detections in rank order
//                     + class-id passes     -> each class's detections in rank order (MATLAB's stable sort)
//                   (rank_by_score, which az_coco.hip shares)
//   k_voc_match     one wave per (class, image) segment, grid-striding: the segment's detections in rank order, the
//                   lanes over its ground-truth boxes (64 at a time), f64 overlap in VOCevaldet's operation order, a wave
//                   arg-max with the first box winning ties, then the claim (bit in a register for the first 2048 boxes,
//                   a byte in HBM past that) -> +1 TP / -1 FP / 0 difficult, in input order
//   k_voc_class     one workgroup per class: npos, cumsum of TP / FP in rank order -> rec, prec; suffix max of prec
//                   (MATLAB's max ignores NaN: fmax) -> the 11-point AP (metric_07) and xVOCap's area
// The overlap, the workgroup scan and the curve / AP body live in az_eval_dev.h: az_ddiag.hip (az_det_diag_eval) calls the same.
// -ffp-contract=off (Makefile): every product and sum rounds once, as MATLAB's double arithmetic does.
#include "az_ctx.h"
#include "az_eval_dev.h"

namespace {

constexpr int VT = EVAL_VT;           // threads of every workgroup here (4 waves)
constexpr int VITEMS = 8;             // rounds of VT elements per radix tile
constexpr int VTILE = VT * VITEMS;

__device__ __forceinline__ unsigned long long conf_key(double conf)
{
    double x = -conf;
    if (x != x) return ~0ull;         // NaN sorts last, as MATLAB's ascending sort puts it
    if (x == 0.0) x = 0.0;            // -0 and +0 compare equal: one key, so the stable order decides
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ void __launch_bounds__(VT) k_voc_prep(int D, int S, const double *__restrict__ conf, const int *__restrict__ det_off,
                                                  unsigned long long *__restrict__ key, unsigned *__restrict__ seg)
{
    const int d = blockIdx.x * VT + threadIdx.x;
    if (d >= D) return;
    key[d] = conf_key(conf[d]);
    int lo = 0, hi = S;               // last s with det_off[s] <= d (det_off[S] = D > d)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (det_off[mid] <= d) lo = mid; else hi = mid;
    }
    seg[d] = (unsigned)lo;
}

// digit of element `idx` in pass (mode, shift): mode 0 key byte, 1 segment byte, 2 class byte
__device__ __forceinline__ unsigned voc_digit(int mode, int shift, unsigned idx, const unsigned long long *__restrict__ key,
                                              const unsigned *__restrict__ seg, unsigned n_images)
{
    if (mode == 0) return (unsigned)(key[idx] >> shift) & 255u;
    const unsigned s = seg[idx];
    return ((mode == 1 ? s : s / n_images) >> shift) & 255u;
}

__global__ void __launch_bounds__(VT) k_voc_hist(int D, int mode, int shift, const unsigned *__restrict__ perm_in,
                                                  const unsigned long long *__restrict__ key, const unsigned *__restrict__ seg,
                                                  unsigned n_images, unsigned *__restrict__ hist)
{
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * VTILE;
    for (int r = 0; r < VITEMS; ++r) {
        const int p = base + r * VT + threadIdx.x;
        if (p < D) atomicAdd(&h[voc_digit(mode, shift, perm_in ? perm_in[p] : (unsigned)p, key, seg, n_images)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of n counts in place: per-chunk sums of SCH counts, one workgroup over the sums, then every chunk
// scanned from its base
constexpr int SCH = VT * 4;

__global__ void __launch_bounds__(VT) k_voc_scan_sum(const unsigned *__restrict__ a, int n, unsigned *__restrict__ sums)
{
    __shared__ unsigned s_w[VT / AZ_WAVE];
    const int base = blockIdx.x * SCH;
    unsigned v = 0;
    for (int k = 0; k < 4; ++k) {
        const int i = base + k * VT + threadIdx.x;
        if (i < n) v += a[i];
    }
    unsigned tot = 0;
    block_scan(v, tot, s_w, [](unsigned x, unsigned y) { return x + y; });
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// one workgroup, n small (the chunk sums): a contiguous run per thread
__global__ void __launch_bounds__(1024) k_voc_scan(unsigned *__restrict__ a, int n)
{
    __shared__ unsigned part[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024;
    const int lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    unsigned s = 0;
    for (int i = lo; i < hi; ++i) s += a[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned run = part[t] - s;
    for (int i = lo; i < hi; ++i) {
        const unsigned v = a[i];
        a[i] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(VT) k_voc_scan_add(unsigned *__restrict__ a, int n, const unsigned *__restrict__ sums)
{
    __shared__ unsigned s_w[VT / AZ_WAVE];
    const int i0 = blockIdx.x * SCH + 4 * threadIdx.x;
    unsigned v[4], loc = 0;
    for (int k = 0; k < 4; ++k) {
        v[k] = i0 + k < n ? a[i0 + k] : 0u;
        loc += v[k];
    }
    unsigned carry = sums[blockIdx.x];
    unsigned run = block_scan(loc, carry, s_w, [](unsigned x, unsigned y) { return x + y; }) - loc;
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < n) a[i0 + k] = run;
        run += v[k];
    }
}

__global__ void __launch_bounds__(VT) k_voc_scatter(int D, int mode, int shift, const unsigned *__restrict__ perm_in,
                                                     const unsigned long long *__restrict__ key, const unsigned *__restrict__ seg,
                                                     unsigned n_images, const unsigned *__restrict__ hist,
                                                     unsigned *__restrict__ perm_out)
{
    __shared__ unsigned run[256];                 // tile's base + elements of this tile placed so far, per digit
    __shared__ unsigned wcnt[VT / AZ_WAVE][256];  // this round: elements per (wave, digit), then the wave's offset
    const int t = threadIdx.x, lane = t & (AZ_WAVE - 1), w = t / AZ_WAVE;
    run[t] = hist[(size_t)t * gridDim.x + blockIdx.x];
    for (int k = 0; k < VT / AZ_WAVE; ++k) wcnt[k][t] = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int base = blockIdx.x * VTILE;
    __syncthreads();
    for (int r = 0; r < VITEMS; ++r) {
        const int p = base + r * VT + t;
        const bool ok = p < D;
        const unsigned idx = ok ? (perm_in ? perm_in[p] : (unsigned)p) : 0u;
        const unsigned dg = ok ? voc_digit(mode, shift, idx, key, seg, n_images) : 0u;
        unsigned long long eq = __ballot(ok);
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot(ok && ((dg >> b) & 1u));
            eq &= ((dg >> b) & 1u) ? m : ~m;
        }
        const unsigned rank = (unsigned)__popcll(eq & lt);
        if (ok && !(eq >> lane >> 1)) wcnt[w][dg] = rank + 1;      // the last lane of its digit in the wave
        __syncthreads();
        {
            unsigned acc = run[t];
            for (int k = 0; k < VT / AZ_WAVE; ++k) {
                const unsigned c = wcnt[k][t];
                wcnt[k][t] = acc;
                acc += c;
            }
            run[t] = acc;
        }
        __syncthreads();
        if (ok) perm_out[wcnt[w][dg] + rank] = idx;
        __syncthreads();
        for (int k = 0; k < VT / AZ_WAVE; ++k) wcnt[k][t] = 0;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(VT) k_voc_match(int S, const int *__restrict__ det_off, const unsigned *__restrict__ ps,
                                                   const double *__restrict__ det_box, const int *__restrict__ gt_off,
                                                   const double *__restrict__ gt_box, const unsigned char *__restrict__ gt_diff,
                                                   unsigned char *__restrict__ gclaim, double min_ov,
                                                   signed char *__restrict__ match)
{
    const int lane = threadIdx.x & (AZ_WAVE - 1);
    const int nw = gridDim.x * (VT / AZ_WAVE);
    for (int s = blockIdx.x * (VT / AZ_WAVE) + threadIdx.x / AZ_WAVE; s < S; s += nw) {
        const int d0 = det_off[s], n = det_off[s + 1] - d0;
        if (n == 0) continue;
        const int g0 = gt_off[s], G = gt_off[s + 1] - g0;
        double q0 = 0, q1 = 0, q2 = 0, q3 = 0;            // this lane's first box (j = lane)
        if (lane < G) {
            const double *q = gt_box + (size_t)(g0 + lane) * 4;
            q0 = q[0]; q1 = q[1]; q2 = q[2]; q3 = q[3];
        }
        unsigned dbits = 0, cbits = 0;                    // j = lane + 64 k, k < 32
        for (int k = 0; k < 32; ++k) {
            const int j = lane + AZ_WAVE * k;
            if (j >= G) break;
            if (gt_diff[g0 + j]) dbits |= 1u << k;
        }
        for (int c0 = 0; c0 < n; c0 += AZ_WAVE) {
            const int cnt = n - c0 < AZ_WAVE ? n - c0 : AZ_WAVE;
            unsigned my = 0;
            double m0 = 0, m1 = 0, m2 = 0, m3 = 0;
            if (lane < cnt) {
                my = ps[d0 + c0 + lane];
                const double *b = det_box + (size_t)my * 4;
                m0 = b[0]; m1 = b[1]; m2 = b[2]; m3 = b[3];
            }
            int myres = 0;
            for (int t = 0; t < cnt; ++t) {
                const double b0 = __shfl(m0, t, AZ_WAVE), b1 = __shfl(m1, t, AZ_WAVE);
                const double b2 = __shfl(m2, t, AZ_WAVE), b3 = __shfl(m3, t, AZ_WAVE);
                double best = -INFINITY;
                int bj = 0x7fffffff;
                for (int j = lane; j < G; j += AZ_WAVE) {
                    double g0x = q0, g0y = q1, g1x = q2, g1y = q3;
                    if (j >= AZ_WAVE) {
                        const double *q = gt_box + (size_t)(g0 + j) * 4;
                        g0x = q[0]; g0y = q[1]; g1x = q[2]; g1y = q[3];
                    }
                    double ov;                                    // j ascends per lane: the first box keeps a tie
                    if (voc_overlap(b0, b1, b2, b3, g0x, g0y, g1x, g1y, &ov) && ov > best) { best = ov; bj = j; }
                }
                for (int o = AZ_WAVE / 2; o > 0; o >>= 1) {
                    const double ob = __shfl_xor(best, o, AZ_WAVE);
                    const int oj = __shfl_xor(bj, o, AZ_WAVE);
                    if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
                }
                int res = -1;                                  // below the overlap: false positive
                if (best >= min_ov && bj < G) {                // wave-uniform (bj < G: some box overlapped)
                    const int owner = bj & (AZ_WAVE - 1), k = bj / AZ_WAVE;
                    int r = 0;
                    if (lane == owner) {
                        const bool diff = k < 32 ? ((dbits >> k) & 1u) : gt_diff[g0 + bj] != 0;
                        if (!diff) {
                            const bool taken = k < 32 ? ((cbits >> k) & 1u) : gclaim[g0 + bj] != 0;
                            r = taken ? -1 : 1;
                            if (!taken) {
                                if (k < 32) cbits |= 1u << k; else gclaim[g0 + bj] = 1;
                            }
                        }
                    }
                    res = __shfl(r, owner, AZ_WAVE);
                }
                if (lane == t) myres = res;
            }
            if (lane < cnt) match[my] = (signed char)myres;
        }
    }
}

__global__ void __launch_bounds__(VT) k_voc_class(int n_images, const int *__restrict__ det_off, const int *__restrict__ gt_off,
                                                   const unsigned char *__restrict__ gt_diff, const unsigned *__restrict__ pc,
                                                   const signed char *__restrict__ match, int metric_07,
                                                   double *__restrict__ rec, double *__restrict__ prec,
                                                   double *__restrict__ smax, long long *__restrict__ npos_out,
                                                   double *__restrict__ ap_out, double *__restrict__ auc_out)
{
    __shared__ unsigned long long s_u[VT / AZ_WAVE];
    __shared__ double s_d[VT / AZ_WAVE];
    __shared__ long long s_np;
    const int c = blockIdx.x, t = threadIdx.x;
    const long long seg0 = (long long)c * n_images, seg1 = seg0 + n_images;
    const int lo = det_off[seg0], hi = det_off[seg1];
    const int glo = gt_off[seg0], ghi = gt_off[seg1];
    // npos: non-difficult boxes of the class
    unsigned long long np = 0;
    for (int j = glo + t; j < ghi; j += VT) np += gt_diff[j] ? 0u : 1u;
    {
        unsigned long long zero = 0;
        block_scan(np, zero, s_u, [](unsigned long long a, unsigned long long b) { return a + b; });
        if (t == 0) s_np = (long long)zero;
    }
    __syncthreads();
    const long long npos = s_np;
    double ap = 0.0, part = 0.0;
    voc_curve_ap(lo, hi, npos, metric_07, [&](int p) -> unsigned long long {
        const int m = match[pc[p]];
        return m > 0 ? (1ull << 32) : (m < 0 ? 1ull : 0ull);
    }, rec, prec, smax, s_u, s_d, &ap, &part);
    if (t == 0) {
        npos_out[c] = npos;
        ap_out[c] = ap;
        auc_out[c] = part;
    }
}

int bytes_for(long long v)          // 8-bit digits needed for values 0..v
{
    int n = 0;
    while (v > 0) { ++n; v >>= 8; }
    return n;
}

}  // namespace

void rank_scratch_sizes(int D, size_t *hist_n, size_t *sums_n)
{
    const size_t nblk = ((size_t)D + VTILE - 1) / VTILE;
    *hist_n = nblk * 256;
    *sums_n = (nblk * 256 + SCH - 1) / SCH;
}

void rank_by_score(hipStream_t s, int D, long long S, int n_images, int n_classes, const double *score, const int *det_off,
                   const RankScratch &r, const unsigned **by_seg, const unsigned **by_class)
{
    const int nblk = (D + VTILE - 1) / VTILE, nsch = (nblk * 256 + SCH - 1) / SCH;
    hipLaunchKernelGGL(k_voc_prep, dim3((D + VT - 1) / VT), dim3(VT), 0, s, D, (int)S, score, det_off, r.key, r.seg);
    // a chain of stable passes from `in` (nullptr: identity) through the two buffers `a`, `b` in turn
    auto passes = [&](int mode, int nbytes, const unsigned *in, unsigned *a, unsigned *b) {
        const unsigned *cur = in;
        for (int k = 0; k < nbytes; ++k) {
            unsigned *out = (k & 1) ? b : a;
            hipLaunchKernelGGL(k_voc_hist, dim3(nblk), dim3(VT), 0, s, D, mode, 8 * k, cur,
                               (const unsigned long long *)r.key, (const unsigned *)r.seg, (unsigned)n_images, r.hist);
            hipLaunchKernelGGL(k_voc_scan_sum, dim3(nsch), dim3(VT), 0, s, (const unsigned *)r.hist, nblk * 256, r.sums);
            hipLaunchKernelGGL(k_voc_scan, dim3(1), dim3(1024), 0, s, r.sums, nsch);
            hipLaunchKernelGGL(k_voc_scan_add, dim3(nsch), dim3(VT), 0, s, r.hist, nblk * 256, (const unsigned *)r.sums);
            hipLaunchKernelGGL(k_voc_scatter, dim3(nblk), dim3(VT), 0, s, D, mode, 8 * k, cur,
                               (const unsigned long long *)r.key, (const unsigned *)r.seg, (unsigned)n_images,
                               (const unsigned *)r.hist, out);
            cur = out;
        }
        return cur;
    };
    const unsigned *pk = passes(0, 8, nullptr, r.perm[0], r.perm[1]);      // ends in perm[1]
    const unsigned *pseg = passes(1, bytes_for(S - 1), pk, r.perm[2], r.perm[3]);   // perm[1] (no pass), [2] or [3]
    unsigned *fa = pseg == r.perm[2] ? r.perm[3] : r.perm[2], *fb = r.perm[0];
    *by_class = passes(2, bytes_for(n_classes - 1), pk, fa, fb);
    *by_seg = pseg;
}

namespace {

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

int az_voc_eval(az_ctx *c, int n_classes, int n_images, const double *det_box, const double *det_conf,
                const int32_t *det_off, const double *gt_box, const uint8_t *gt_difficult, const int32_t *gt_off,
                double min_overlap, int metric_07, int8_t *match_out, double *rec_out, double *prec_out,
                int64_t *npos_out, double *ap_out, double *ap_auc_out)
{
    if (!c || n_classes < 0 || n_images < 0 || !det_off || !gt_off || (n_classes && (!npos_out || !ap_out || !ap_auc_out)))
        return fail(c, AZ_ERR_INVALID, "az_voc_eval: bad arguments");
    const long long S = (long long)n_classes * n_images;
    if (S >= 0x7fffffffLL)
        return fail(c, AZ_ERR_CAPACITY, "az_voc_eval: more segments than int32 offsets address");
    if (det_off[0] != 0 || gt_off[0] != 0) return fail(c, AZ_ERR_INVALID, "az_voc_eval: offsets must start at 0");
    for (long long s = 0; s < S; ++s)
        if (det_off[s + 1] < det_off[s] || gt_off[s + 1] < gt_off[s])
            return fail(c, AZ_ERR_INVALID, "az_voc_eval: offsets must ascend");
    const int D = det_off[S], G = gt_off[S];
    if ((D && (!det_box || !det_conf)) || (G && (!gt_box || !gt_difficult)))
        return fail(c, AZ_ERR_INVALID, "az_voc_eval: NULL array");
    if (n_classes == 0) return AZ_OK;
    const int nblk = (D + VTILE - 1) / VTILE;
    if ((long long)nblk * 256 >= 0x7fffffffLL) return fail(c, AZ_ERR_CAPACITY, "az_voc_eval: too many detections");
    // one arena: inputs, keys, segments, four permutations, radix table, match, claims, curves, per-class results
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    const size_t o_box = take((size_t)D * 4 * sizeof(double)), o_conf = take((size_t)D * sizeof(double));
    const size_t o_doff = take(((size_t)S + 1) * sizeof(int)), o_gbox = take((size_t)G * 4 * sizeof(double));
    const size_t o_gdif = take((size_t)G), o_goff = take(((size_t)S + 1) * sizeof(int));
    const size_t o_key = take((size_t)D * 8), o_seg = take((size_t)D * 4);
    size_t o_perm[4];
    for (auto &o : o_perm) o = take((size_t)D * 4);
    const int nsch = (nblk * 256 + SCH - 1) / SCH;
    const size_t o_hist = take((size_t)nblk * 256 * 4), o_sums = take((size_t)nsch * 4), o_match = take((size_t)D), o_claim = take((size_t)G);
    const size_t o_rec = take((size_t)D * 8), o_prec = take((size_t)D * 8), o_smax = take((size_t)D * 8);
    const size_t o_np = take((size_t)n_classes * 8), o_ap = take((size_t)n_classes * 8), o_auc = take((size_t)n_classes * 8);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = scratch_grow(c, 8, off)) != AZ_OK) return rc;
    char *A = (char *)c->scratch[8].p;
    hipStream_t s = c->stream;
    auto *dbox = (double *)(A + o_box), *dconf = (double *)(A + o_conf), *gbox = (double *)(A + o_gbox);
    auto *doff = (int *)(A + o_doff), *goff = (int *)(A + o_goff);
    auto *gdif = (unsigned char *)(A + o_gdif), *claim = (unsigned char *)(A + o_claim);
    auto *key = (unsigned long long *)(A + o_key);
    auto *seg = (unsigned *)(A + o_seg), *hist = (unsigned *)(A + o_hist), *sums = (unsigned *)(A + o_sums);
    unsigned *perm[4];
    for (int i = 0; i < 4; ++i) perm[i] = (unsigned *)(A + o_perm[i]);
    auto *match = (signed char *)(A + o_match);
    auto *rec = (double *)(A + o_rec), *prec = (double *)(A + o_prec), *smax = (double *)(A + o_smax);
    auto *np = (long long *)(A + o_np);
    auto *ap = (double *)(A + o_ap), *auc = (double *)(A + o_auc);
    if (D) {
        HIPCHK(c, hipMemcpyAsync(dbox, det_box, (size_t)D * 4 * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dconf, det_conf, (size_t)D * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (G) {
        HIPCHK(c, hipMemcpyAsync(gbox, gt_box, (size_t)G * 4 * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(gdif, gt_difficult, (size_t)G, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(claim, 0, (size_t)G, s));
    }
    HIPCHK(c, hipMemcpyAsync(doff, det_off, ((size_t)S + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(goff, gt_off, ((size_t)S + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    const unsigned *pseg = nullptr, *pcls = nullptr;
    if (D) {
        RankScratch rs{key, seg, {perm[0], perm[1], perm[2], perm[3]}, hist, sums};
        rank_by_score(s, D, S, n_images, n_classes, (const double *)dconf, (const int *)doff, rs, &pseg, &pcls);
        long long nb = (S + (VT / AZ_WAVE) - 1) / (VT / AZ_WAVE);
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(k_voc_match, dim3((unsigned)nb), dim3(VT), 0, s, (int)S, (const int *)doff, pseg,
                           (const double *)dbox, (const int *)goff, (const double *)gbox, (const unsigned char *)gdif,
                           claim, min_overlap, match);
    }
    hipLaunchKernelGGL(k_voc_class, dim3(n_classes), dim3(VT), 0, s, n_images, (const int *)doff, (const int *)goff,
                       (const unsigned char *)gdif, pcls, (const signed char *)match, metric_07 ? 1 : 0, rec, prec, smax,
                       np, ap, auc);
    HIPCHK(c, hipGetLastError());
    if (D && match_out) HIPCHK(c, hipMemcpyAsync(match_out, match, (size_t)D, hipMemcpyDeviceToHost, s));
    if (D && rec_out) HIPCHK(c, hipMemcpyAsync(rec_out, rec, (size_t)D * 8, hipMemcpyDeviceToHost, s));
    if (D && prec_out) HIPCHK(c, hipMemcpyAsync(prec_out, prec, (size_t)D * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(npos_out, np, (size_t)n_classes * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(ap_out, ap, (size_t)n_classes * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(ap_auc_out, auc, (size_t)n_classes * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return AZ_OK;
}

// rank_by_score alone on host arrays, for tests: both permutations of the D detections
int az_rank_unit(az_ctx *c, int n_classes, int n_images, const double *score, const int32_t *det_off,
                 uint32_t *by_seg_out, uint32_t *by_class_out)
{
    if (!c || n_classes < 0 || n_images < 0 || !det_off) return fail(c, AZ_ERR_INVALID, "az_rank_unit: bad arguments");
    const long long S = (long long)n_classes * n_images;
    if (S >= 0x7fffffffLL)
        return fail(c, AZ_ERR_CAPACITY, "az_rank_unit: more segments than int32 offsets address");
    if (det_off[0] != 0) return fail(c, AZ_ERR_INVALID, "az_rank_unit: offsets must start at 0");
    for (long long s = 0; s < S; ++s)
        if (det_off[s + 1] < det_off[s]) return fail(c, AZ_ERR_INVALID, "az_rank_unit: offsets must ascend");
    const int D = det_off[S];
    if (D == 0) return AZ_OK;
    if (!score || !by_seg_out || !by_class_out) return fail(c, AZ_ERR_INVALID, "az_rank_unit: NULL array");
    size_t hist_n = 0, sums_n = 0;
    rank_scratch_sizes(D, &hist_n, &sums_n);
    if (hist_n >= 0x7fffffffULL) return fail(c, AZ_ERR_CAPACITY, "az_rank_unit: too many detections");
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    const size_t o_score = take((size_t)D * sizeof(double)), o_doff = take(((size_t)S + 1) * sizeof(int));
    const size_t o_key = take((size_t)D * 8), o_seg = take((size_t)D * 4);
    size_t o_perm[4];
    for (auto &o : o_perm) o = take((size_t)D * 4);
    const size_t o_hist = take(hist_n * 4), o_sums = take(sums_n * 4);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = scratch_grow(c, 8, off)) != AZ_OK) return rc;
    char *A = (char *)c->scratch[8].p;
    hipStream_t s = c->stream;
    auto *dscore = (double *)(A + o_score);
    auto *doff = (int *)(A + o_doff);
    HIPCHK(c, hipMemcpyAsync(dscore, score, (size_t)D * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(doff, det_off, ((size_t)S + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    RankScratch rs{(unsigned long long *)(A + o_key), (unsigned *)(A + o_seg),
                   {(unsigned *)(A + o_perm[0]), (unsigned *)(A + o_perm[1]), (unsigned *)(A + o_perm[2]),
                    (unsigned *)(A + o_perm[3])},
                   (unsigned *)(A + o_hist), (unsigned *)(A + o_sums)};
    const unsigned *pseg = nullptr, *pcls = nullptr;
    rank_by_score(s, D, S, n_images, n_classes, (const double *)dscore, (const int *)doff, rs, &pseg, &pcls);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(by_seg_out, pseg, (size_t)D * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(by_class_out, pcls, (size_t)D * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return AZ_OK;
}
