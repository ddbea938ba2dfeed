// az_postproc.hip -- Soft-NMS (Bodla et al., ICCV 2017) and box voting (Gidaris & Komodakis, ICCV 2015) behind apply_nms's
// call site: many small independent groups of [x1, y1, x2, y2, score] float32 rows per call (one per class per image), the
// shape az_nms_batched serves.  The definitions are include/aznet_hip.h's (az_soft_nms_batched, az_box_vote_batched); every
// operation rounds once (no contraction), so a NumPy restatement gives the same bits (tests/postproc_ref.py).
//   k_soft_nms_small   groups of 1 .. 256 boxes: a workgroup of 256 per group, a box per thread in registers, the group's
//                      boxes in LDS for the winner's broadcast.  A round = wave arg-max over (score, index) by butterfly,
//                      the waves' winners through LDS (one barrier; the slots alternate between rounds), the decay.
//   k_soft_nms_large   groups of 257 .. 4096 boxes: a workgroup of 1024 per group, four boxes per thread; the winner's
//                      owner hands its box over through LDS (a second barrier per round).
//   k_box_vote         a workgroup of 256 per group, a thread per kept box: the group's rows pass through LDS 256 at a
//                      time and every thread walks them in index order, summing in float64.
// IoU is k_nms_mask's arithmetic (az_select.hip) operation for operation; the tie rule is k_nms_rank_count's.  No atomics.
#include "az_ctx.h"

namespace {

constexpr int PP_SMALL = 256;                    // boxes per group of k_soft_nms_small = its threads
constexpr int PP_LARGE_NT = 1024, PP_LARGE_K = 4;
static_assert(PP_LARGE_NT * PP_LARGE_K == AZ_SOFT_NMS_MAX, "k_soft_nms_large holds AZ_SOFT_NMS_MAX boxes");
constexpr int PP_VOTE_NT = 256;

// does (as, ai) come before (bs, bi)?  index -1: no box.  Higher score first, of equal scores the higher index.
__device__ __forceinline__ bool pp_before(float as, int ai, float bs, int bi)
{
    return ai >= 0 && (bi < 0 || as > bs || (as == bs && ai > bi));
}

__device__ __forceinline__ float pp_area(float x1, float y1, float x2, float y2)
{
    float w = x2 - x1; w = w + 1.0f;
    float h = y2 - y1; h = h + 1.0f;
    return w * h;
}

__device__ __forceinline__ float pp_iou(float ix1, float iy1, float ix2, float iy2, float iarea,
                                        float jx1, float jy1, float jx2, float jy2, float jarea)
{
    const float xx1 = ix1 >= jx1 ? ix1 : jx1;
    const float yy1 = iy1 >= jy1 ? iy1 : jy1;
    const float xx2 = ix2 <= jx2 ? ix2 : jx2;
    const float yy2 = iy2 <= jy2 ? iy2 : jy2;
    float tw = xx2 - xx1; tw = tw + 1.0f;
    float th = yy2 - yy1; th = th + 1.0f;
    const float w = 0.0f >= tw ? 0.0f : tw;
    const float h = 0.0f >= th ? 0.0f : th;
    const float inter = w * h;
    float den = iarea + jarea; den = den - inter;
    return inter / den;
}

// One group of n <= NT * K boxes at g by the whole workgroup (NT threads): thread t holds the boxes t, t + NT, ...
// sb: LDS for the group's boxes when K == 1 ([NT]), else one slot for the winner's box; slot_s / slot_i: [2][NT / 64].
// The loop runs at most n rounds whatever the scores are (every round with a winner retires one box), and a winner is an
// alive box's own index, so nothing outside [0, n) is emitted.
template <int NT, int K>
__device__ __forceinline__ void soft_nms_group(const float *__restrict__ g, int n, int method, double thresh, float sigma,
                                               double min_score, long long *__restrict__ keep, float *__restrict__ scores_out,
                                               int *__restrict__ nkeep, float4 *sb, float *slot_s, int *slot_i)
{
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float x1[K], y1[K], x2[K], y2[K], ar[K], sc[K];
    bool alive[K];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const int j = tid + q * NT;
        alive[q] = j < n;
        x1[q] = y1[q] = x2[q] = y2[q] = ar[q] = sc[q] = 0.0f;
        if (alive[q]) {
            const float *d = g + 5 * (size_t)j;
            x1[q] = d[0]; y1[q] = d[1]; x2[q] = d[2]; y2[q] = d[3]; sc[q] = d[4];
            ar[q] = pp_area(x1[q], y1[q], x2[q], y2[q]);
            if (K == 1) sb[j] = make_float4(x1[q], y1[q], x2[q], y2[q]);
        }
    }
    int cnt = 0;
    for (int round = 0; round < n; ++round) {
        float bs = 0.0f;
        int bi = -1;
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (alive[q] && pp_before(sc[q], tid + q * NT, bs, bi)) { bs = sc[q]; bi = tid + q * NT; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (pp_before(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        // lane 0's word is the wave's (with scores outside the stated domain the lanes may disagree; one lane speaks)
        const int p = (round & 1) * NW;
        if (lane == 0) { slot_s[p + wave] = bs; slot_i[p + wave] = bi; }
        __syncthreads();                                       // (also publishes sb[] before its first use)
        float ws = slot_s[p];
        int wi = slot_i[p];
#pragma unroll
        for (int w = 1; w < NW; ++w)
            if (pp_before(slot_s[p + w], slot_i[p + w], ws, wi)) { ws = slot_s[p + w]; wi = slot_i[p + w]; }
        if (wi < 0) break;                                     // nothing alive (every thread read the same words)
        if (tid == 0) { keep[cnt] = wi; scores_out[cnt] = ws; }
        ++cnt;
        float4 wb;
        if (K == 1) {
            wb = sb[wi];
        } else {
            if (tid == (wi & (NT - 1))) {
                const int wq = wi / NT;
#pragma unroll
                for (int q = 0; q < K; ++q)
                    if (q == wq) sb[0] = make_float4(x1[q], y1[q], x2[q], y2[q]);
            }
            __syncthreads();
            wb = sb[0];
            // (the next write of sb[0] comes after the next round's barrier above, which every thread reaches after this read)
        }
        const float warea = pp_area(wb.x, wb.y, wb.z, wb.w);
#pragma unroll
        for (int q = 0; q < K; ++q) {
            if (!alive[q]) continue;
            if (tid + q * NT == wi) { alive[q] = false; continue; }
            const float ovr = pp_iou(wb.x, wb.y, wb.z, wb.w, warea, x1[q], y1[q], x2[q], y2[q], ar[q]);
            float w;
            if (method == AZ_NMS_GAUSSIAN) {
                float e = ovr * ovr; e = -e; e = e / sigma;
                w = expf(e);
            } else {
                const bool over = (double)ovr >= thresh;
                w = !over ? 1.0f : method == AZ_NMS_LINEAR ? 1.0f - ovr : 0.0f;
            }
            sc[q] = sc[q] * w;
            if ((double)sc[q] < min_score) alive[q] = false;
        }
    }
    if (tid == 0) *nkeep = cnt;
}

__global__ void __launch_bounds__(PP_SMALL)
k_soft_nms_small(const float *__restrict__ dets, const int *__restrict__ goff, const int *__restrict__ gsel, int method,
                 double thresh, float sigma, double min_score, long long *__restrict__ keep, float *__restrict__ scores_out,
                 int *__restrict__ nkeep)
{
    __shared__ float4 sb[PP_SMALL];
    __shared__ float slot_s[2 * PP_SMALL / 64];
    __shared__ int slot_i[2 * PP_SMALL / 64];
    const int g = gsel[blockIdx.x];
    const int base = goff[g];
    const int n = min(goff[g + 1] - base, PP_SMALL);
    soft_nms_group<PP_SMALL, 1>(dets + 5 * (size_t)base, n, method, thresh, sigma, min_score, keep + base, scores_out + base,
                                nkeep + g, sb, slot_s, slot_i);
}

__global__ void __launch_bounds__(PP_LARGE_NT)
k_soft_nms_large(const float *__restrict__ dets, const int *__restrict__ goff, const int *__restrict__ gsel, int method,
                 double thresh, float sigma, double min_score, long long *__restrict__ keep, float *__restrict__ scores_out,
                 int *__restrict__ nkeep)
{
    __shared__ float4 sb[1];
    __shared__ float slot_s[2 * PP_LARGE_NT / 64];
    __shared__ int slot_i[2 * PP_LARGE_NT / 64];
    const int g = gsel[blockIdx.x];
    const int base = goff[g];
    const int n = min(goff[g + 1] - base, PP_LARGE_NT * PP_LARGE_K);
    soft_nms_group<PP_LARGE_NT, PP_LARGE_K>(dets + 5 * (size_t)base, n, method, thresh, sigma, min_score, keep + base,
                                            scores_out + base, nkeep + g, sb, slot_s, slot_i);
}

// Group g = gsel[blockIdx.x]; thread t votes for the kept boxes t, t + 256, ...: out[(base + k)][0..3].
__global__ void __launch_bounds__(PP_VOTE_NT)
k_box_vote(const float *__restrict__ dets, const int *__restrict__ goff, const int *__restrict__ gsel,
           const long long *__restrict__ keep, const int *__restrict__ nkeep, double vote_thresh, float *__restrict__ out)
{
    __shared__ float tile[PP_VOTE_NT][6];                     // x1, y1, x2, y2, score, area
    const int tid = threadIdx.x;
    const int g = gsel[blockIdx.x];
    const int base = goff[g];
    const int n = goff[g + 1] - base;
    const int nk = min(nkeep[g], n);
    const float *gd = dets + 5 * (size_t)base;
    for (int k0 = 0; k0 < nk; k0 += PP_VOTE_NT) {             // (uniform: the barriers below are reached by every thread)
        const int k = k0 + tid;
        const bool act = k < nk;
        int ki = act ? (int)keep[base + k] : 0;
        ki = ki < 0 ? 0 : ki >= n ? n - 1 : ki;               // (checked on the host; never an address outside the group)
        const float kx1 = gd[5 * (size_t)ki], ky1 = gd[5 * (size_t)ki + 1], kx2 = gd[5 * (size_t)ki + 2], ky2 = gd[5 * (size_t)ki + 3];
        const float karea = pp_area(kx1, ky1, kx2, ky2);
        double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int jb = 0; jb < n; jb += PP_VOTE_NT) {
            __syncthreads();
            const int j = jb + tid;
            if (j < n) {
                const float *d = gd + 5 * (size_t)j;
                tile[tid][0] = d[0]; tile[tid][1] = d[1]; tile[tid][2] = d[2]; tile[tid][3] = d[3]; tile[tid][4] = d[4];
                tile[tid][5] = pp_area(d[0], d[1], d[2], d[3]);
            }
            __syncthreads();
            const int lim = min(PP_VOTE_NT, n - jb);
            if (act)
                for (int jj = 0; jj < lim; ++jj) {
                    const float ovr = pp_iou(kx1, ky1, kx2, ky2, karea, tile[jj][0], tile[jj][1], tile[jj][2], tile[jj][3], tile[jj][5]);
                    if ((double)ovr >= vote_thresh) {
                        const double s = (double)tile[jj][4];
                        sw = sw + s;
                        s0 = s0 + s * (double)tile[jj][0];
                        s1 = s1 + s * (double)tile[jj][1];
                        s2 = s2 + s * (double)tile[jj][2];
                        s3 = s3 + s * (double)tile[jj][3];
                    }
                }
        }
        if (act) {
            float *o = out + 4 * (size_t)(base + k);
            const bool none = sw == 0.0;
            o[0] = none ? kx1 : (float)(s0 / sw);
            o[1] = none ? ky1 : (float)(s1 / sw);
            o[2] = none ? kx2 : (float)(s2 / sw);
            o[3] = none ? ky2 : (float)(s3 / sw);
        }
    }
}

// The scratch of both entries grown to `total` boxes and n_groups groups, as nms_reserve grows the NMS scratch: the members of
// a group are freed and allocated together, the capacity doubles.
int pp_reserve(az_ctx *c, int total, int n_groups)
{
    if (total > c->pp_box_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->pp_box_cap = 0;
        size_t cap = 4096;
        while (cap < (size_t)total) cap *= 2;
        Buf *b = c->pp_box_own;
        HIPCHK(c, reserve_group({{&b[0], cap * 5 * 4}, {&b[1], cap * 8}, {&b[2], cap * 4}, {&b[3], cap * 4 * 4}}));
        c->pp_box_cap = (int)std::min(cap, (size_t)0x7fffffff);
    }
    if (n_groups > c->pp_grp_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->pp_grp_cap = 0;
        size_t cap = 1024;
        while (cap < (size_t)n_groups) cap *= 2;
        Buf *b = c->pp_grp_own;
        HIPCHK(c, reserve_group({{&b[0], (cap + 1) * 4}, {&b[1], cap * 4}, {&b[2], cap * 4}}));
        c->pp_grp_cap = (int)std::min(cap, (size_t)0x7fffffff);
    }
    return AZ_OK;
}

// What both entries ask of the groups before anything is enqueued; small / large: the non-empty groups by kernel.
int pp_check_groups(az_ctx *c, const std::string &who, const int32_t *offsets, int n_groups, std::vector<int> &small,
                    std::vector<int> &large)
{
    if (offsets[0] != 0) return fail(c, AZ_ERR_INVALID, who + ": offsets must start at 0");
    for (int g = 0; g < n_groups; ++g)
        if (offsets[g + 1] < offsets[g]) return fail(c, AZ_ERR_INVALID, who + ": offsets must ascend");
    for (int g = 0; g < n_groups; ++g) {
        const int n = offsets[g + 1] - offsets[g];
        if (n > AZ_SOFT_NMS_MAX)
            return fail(c, AZ_ERR_CAPACITY, who + ": group " + std::to_string(g) + " has " + std::to_string(n) + " boxes (at most " +
                                                std::to_string(AZ_SOFT_NMS_MAX) + ")");
        if (n > 0) (n <= PP_SMALL ? small : large).push_back(g);
    }
    return AZ_OK;
}

// dets and offsets to the device, the counts cleared
int pp_upload(az_ctx *c, const float *dets, const int32_t *offsets, int n_groups, int total)
{
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->pp_box_own[0].p, dets, (size_t)total * 5 * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->pp_grp_own[0].p, offsets, ((size_t)n_groups + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    return AZ_OK;
}

}  // namespace

extern "C" {

int az_soft_nms_batched(az_ctx *c, const float *dets, const int32_t *offsets, int n_groups, int method, double thresh,
                        double sigma, double min_score, int64_t *keep, float *scores_out, int32_t *n_keep)
{
    const std::string who = "az_soft_nms_batched";
    if (!c || n_groups < 0 || (n_groups && (!offsets || !n_keep))) return fail(c, AZ_ERR_INVALID, who + ": bad arguments");
    if (method != AZ_NMS_HARD && method != AZ_NMS_LINEAR && method != AZ_NMS_GAUSSIAN)
        return fail(c, AZ_ERR_INVALID, who + ": method must be AZ_NMS_HARD, AZ_NMS_LINEAR or AZ_NMS_GAUSSIAN");
    const float fsigma = (float)sigma;
    if (method == AZ_NMS_GAUSSIAN && (!(fsigma > 0.0f) || !std::isfinite(fsigma)))
        return fail(c, AZ_ERR_INVALID, who + ": sigma must be positive and finite (as a float32)");
    if (method != AZ_NMS_GAUSSIAN && std::isnan(thresh)) return fail(c, AZ_ERR_INVALID, who + ": thresh is NaN");
    if (!(min_score >= 0.0)) return fail(c, AZ_ERR_INVALID, who + ": min_score must not be negative");
    if (n_groups == 0) return AZ_OK;
    std::vector<int> small, large;
    int rc = pp_check_groups(c, who, offsets, n_groups, small, large);
    if (rc != AZ_OK) return rc;
    const int total = offsets[n_groups];
    if (total > 0 && (!dets || !keep || !scores_out)) return fail(c, AZ_ERR_INVALID, who + ": NULL array");
    for (int g = 0; g < n_groups; ++g) n_keep[g] = 0;
    if (total == 0) return AZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = pp_reserve(c, total, n_groups)) != AZ_OK) return rc;
    if ((rc = pp_upload(c, dets, offsets, n_groups, total)) != AZ_OK) return rc;
    hipStream_t s = c->stream;
    const float *d_dets = c->pp_box_own[0].as<float>();
    long long *d_keep = c->pp_box_own[1].as<long long>();
    float *d_sc = c->pp_box_own[2].as<float>();
    const int *d_off = c->pp_grp_own[0].as<int>();
    int *d_sel = c->pp_grp_own[1].as<int>(), *d_nk = c->pp_grp_own[2].as<int>();
    HIPCHK(c, hipMemsetAsync(d_nk, 0, (size_t)n_groups * sizeof(int), s));
    if (!small.empty()) HIPCHK(c, hipMemcpyAsync(d_sel, small.data(), small.size() * sizeof(int), hipMemcpyHostToDevice, s));
    if (!large.empty())
        HIPCHK(c, hipMemcpyAsync(d_sel + small.size(), large.data(), large.size() * sizeof(int), hipMemcpyHostToDevice, s));
    if (!(c->profiling & 4)) clear_events(c);
    if (!small.empty()) {
        Timed t(c, "soft_nms", (int)small.size());
        hipLaunchKernelGGL(k_soft_nms_small, dim3((unsigned)small.size()), dim3(PP_SMALL), 0, s, d_dets, d_off, d_sel, method, thresh,
                           fsigma, min_score, d_keep, d_sc, d_nk);
    }
    if (!large.empty()) {
        Timed t(c, "soft_nms_large", (int)large.size());
        hipLaunchKernelGGL(k_soft_nms_large, dim3((unsigned)large.size()), dim3(PP_LARGE_NT), 0, s, d_dets, d_off,
                           d_sel + small.size(), method, thresh, fsigma, min_score, d_keep, d_sc, d_nk);
    }
    std::vector<long long> hk((size_t)total);
    std::vector<float> hs((size_t)total);
    std::vector<int> hn((size_t)n_groups);
    HIPCHK(c, hipMemcpyAsync(hk.data(), d_keep, (size_t)total * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(hs.data(), d_sc, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(hn.data(), d_nk, (size_t)n_groups * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));               // `small`, `large` and the three vectors live on this frame
    HIPCHK(c, hipGetLastError());
    for (int g = 0; g < n_groups; ++g)
        if (hn[g] < 0 || hn[g] > offsets[g + 1] - offsets[g]) return fail(c, AZ_ERR_HIP, who + ": bad count");
    for (int g = 0; g < n_groups; ++g) {
        n_keep[g] = hn[g];
        for (int k = 0; k < hn[g]; ++k) {
            keep[offsets[g] + k] = hk[(size_t)offsets[g] + k];
            scores_out[offsets[g] + k] = hs[(size_t)offsets[g] + k];
        }
    }
    return AZ_OK;
}

int az_box_vote_batched(az_ctx *c, const float *dets, const int32_t *offsets, int n_groups, const int64_t *keep,
                        const int32_t *n_keep, double vote_thresh, float *boxes_out)
{
    const std::string who = "az_box_vote_batched";
    if (!c || n_groups < 0 || (n_groups && (!offsets || !n_keep))) return fail(c, AZ_ERR_INVALID, who + ": bad arguments");
    if (std::isnan(vote_thresh)) return fail(c, AZ_ERR_INVALID, who + ": vote_thresh is NaN");
    if (n_groups == 0) return AZ_OK;
    std::vector<int> small, large;
    int rc = pp_check_groups(c, who, offsets, n_groups, small, large);
    if (rc != AZ_OK) return rc;
    const int total = offsets[n_groups];
    if (total > 0 && (!dets || !keep || !boxes_out)) return fail(c, AZ_ERR_INVALID, who + ": NULL array");
    std::vector<int> voting;                          // the groups with a kept box, one workgroup each
    for (int g = 0; g < n_groups; ++g) {
        const int n = offsets[g + 1] - offsets[g];
        if (n_keep[g] < 0 || n_keep[g] > n) return fail(c, AZ_ERR_INVALID, who + ": n_keep[" + std::to_string(g) + "] outside its group");
        for (int k = 0; k < n_keep[g]; ++k) {
            const int64_t i = keep[offsets[g] + k];
            if (i < 0 || i >= n) return fail(c, AZ_ERR_INVALID, who + ": a keep index of group " + std::to_string(g) + " is outside it");
        }
        if (n_keep[g] > 0) voting.push_back(g);
    }
    if (voting.empty()) return AZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = pp_reserve(c, total, n_groups)) != AZ_OK) return rc;
    if ((rc = pp_upload(c, dets, offsets, n_groups, total)) != AZ_OK) return rc;
    hipStream_t s = c->stream;
    long long *d_keep = c->pp_box_own[1].as<long long>();
    float *d_out = c->pp_box_own[3].as<float>();
    int *d_sel = c->pp_grp_own[1].as<int>(), *d_nk = c->pp_grp_own[2].as<int>();
    HIPCHK(c, hipMemcpyAsync(d_keep, keep, (size_t)total * sizeof(long long), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_nk, n_keep, (size_t)n_groups * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_sel, voting.data(), voting.size() * sizeof(int), hipMemcpyHostToDevice, s));
    if (!(c->profiling & 4)) clear_events(c);
    {
        Timed t(c, "box_vote", (int)voting.size());
        hipLaunchKernelGGL(k_box_vote, dim3((unsigned)voting.size()), dim3(PP_VOTE_NT), 0, s, c->pp_box_own[0].as<float>(),
                           c->pp_grp_own[0].as<int>(), d_sel, d_keep, d_nk, vote_thresh, d_out);
    }
    std::vector<float> hb((size_t)total * 4);
    HIPCHK(c, hipMemcpyAsync(hb.data(), d_out, (size_t)total * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));               // `voting` and `hb` live on this frame
    HIPCHK(c, hipGetLastError());
    for (int g : voting)
        std::memcpy(boxes_out + 4 * (size_t)offsets[g], hb.data() + 4 * (size_t)offsets[g], (size_t)n_keep[g] * 4 * sizeof(float));
    return AZ_OK;
}

}  // extern "C"
