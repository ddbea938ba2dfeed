// az_iterloc.hip -- iterative box localisation (Gidaris & Komodakis, ICCV 2015, the half that goes with box voting): the
// class boxes of one head pass that score well become the proposals of the next.  Two kernels per extra round:
//   k_iter_select  the sources of the next round: threshold (f32, >=), ordered compaction in ascending flat index f, the
//                  top-max_rows cut (az_topk's rule: the higher score, ties to the lower f) -- the kept pairs STAY in ascending
//                  f, which is why this is not azk_topk (score order) plus a sort;
//   k_iter_take    column class[e] of the round's head outputs into the extras lists, read through inv (the un-dedup gather
//                  of azk_det_gather and the column pick in one step: the same copies, bit for bit).
// Integer / comparison work and plain copies: no arithmetic on a score or a box.
#include "az_dev.h"

namespace {

constexpr int SEL_NT = 1024;

// exclusive prefix of a 0/1 flag over the workgroup, in thread order, and the workgroup's total
__device__ __forceinline__ int block_rank(bool flag, int *wsum, int *total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    __syncthreads();                                  // (wsum of the previous call has been read by everyone)
    if (lane == 0) wsum[wid] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SEL_NT / 64; ++w) { const int t = wsum[w]; all += t; if (w < wid) before += t; }
    *total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// One workgroup.  Element f of the N candidates:
//   first (prev_n == nullptr): N = P * (ncls - 1), f = (j - 1) * P + i (class-major) -> score prob[i][j], box pred[i][j];
//   later rounds:              N = min(*prev_n, max_rows), the previous round's extras: score pscore[f], box pbox[f], class
//                              pcls[f].
// Writes the kept boxes into B, their class / source row into cls_out / src_out, the count into *count_out and *Pptr,
// and clears *Uptr (k_dedup_rois adds into it).
__global__ void __launch_bounds__(SEL_NT)
k_iter_select(const float *__restrict__ prob, const double *__restrict__ pred, int P, int ncls,
              const int *prev_n, const float *__restrict__ pscore, const double *__restrict__ pbox,
              const int *__restrict__ pcls, float min_score, int max_rows, double *B, int *cls_out, int *src_out,
              int *count_out, int *Pptr, int *Uptr)
{
    __shared__ int hist[256];
    __shared__ int wsum[SEL_NT / 64];
    __shared__ unsigned s_prefix;
    __shared__ int s_need;
    const int tid = threadIdx.x;
    const bool first = prev_n == nullptr;
    int N;
    if (first) N = P * (ncls - 1);
    else { N = *prev_n; if (N > max_rows) N = max_rows; }
    auto score_of = [&](int f) -> float {
        if (!first) return pscore[f];
        const int j = f / P, i = f - j * P;
        return prob[(size_t)i * ncls + j + 1];
    };
    auto passes = [&](float sc) -> bool { return sc >= min_score; };      // (f32; false for a NaN on either side)

    // how many pass the threshold
    int mine = 0;
    for (int f = tid; f < N; f += SEL_NT) mine += passes(score_of(f)) ? 1 : 0;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    if (mine) atomicAdd(&hist[0], mine);
    __syncthreads();
    const int n_pass = hist[0];
    __syncthreads();

    // more than max_rows: the max_rows-th largest key T among them (radix select, 8 bits a pass) and how many of the
    // elements equal to T are still wanted
    const bool capped = n_pass > max_rows;
    unsigned T = 0;
    int need_eq = 0;
    if (capped) {
        if (tid == 0) { s_prefix = 0; s_need = max_rows; }
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned prefix = s_prefix;
            for (int f = tid; f < N; f += SEL_NT) {
                const float sc = score_of(f);
                if (!passes(sc)) continue;
                const unsigned key = score_key(sc);
                if (shift == 24 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int need = s_need, d = 255;
                for (; d > 0; --d) { if (hist[d] >= need) break; need -= hist[d]; }
                s_need = need;
                s_prefix = (prefix << 8) | (unsigned)d;
            }
            __syncthreads();
        }
        T = s_prefix;
        need_eq = s_need;
    }

    // ordered compaction, SEL_NT candidates at a time
    int n_out = 0, n_eq = 0;
    for (int base = 0; base < N; base += SEL_NT) {
        const int f = base + tid;
        bool keep = false, eq = false;
        int j = 0, i = 0;
        if (f < N) {
            const float sc = score_of(f);
            keep = passes(sc);
            if (keep && capped) {
                const unsigned key = score_key(sc);
                eq = key == T;
                keep = key >= T;
            }
        }
        if (capped) {                                 // ties across the cut: the first need_eq of them in f
            int tot_eq;
            const int r = block_rank(eq, wsum, &tot_eq);
            if (eq && n_eq + r >= need_eq) keep = false;
            n_eq += tot_eq;
        }
        int tot;
        const int slot = n_out + block_rank(keep, wsum, &tot);
        if (keep) {
            const double *src;
            if (first) { j = f / P; i = f - j * P; ++j; src = pred + ((size_t)i * ncls + j) * 4; }
            else { j = pcls[f]; i = f; src = pbox + (size_t)f * 4; }
#pragma unroll
            for (int q = 0; q < 4; ++q) B[(size_t)slot * 4 + q] = src[q];
            cls_out[slot] = j;
            src_out[slot] = i;
        }
        n_out += tot;
    }
    if (tid == 0) { *count_out = n_out; *Pptr = n_out; *Uptr = 0; }
}

__global__ void __launch_bounds__(256)
k_iter_take(const int *Nptr, int cap, const int *__restrict__ inv, const int *__restrict__ cls, int ncls,
            const float *__restrict__ prob_u, const double *__restrict__ pred_u, float *score_out, double *box_out)
{
    int N = *Nptr;
    if (N > cap) N = cap;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < N; e += gridDim.x * blockDim.x) {
        const size_t src = (size_t)inv[e] * ncls + cls[e];
        score_out[e] = prob_u[src];
#pragma unroll
        for (int q = 0; q < 4; ++q) box_out[(size_t)e * 4 + q] = pred_u[src * 4 + q];
    }
}

}  // namespace

void azk_iter_select(hipStream_t s, const float *prob, const double *pred, int P, int ncls, const int *prev_n,
                     const float *pscore, const double *pbox, const int *pcls, float min_score, int max_rows, double *B,
                     int *cls_out, int *src_out, int *count_out, int *Pptr, int *Uptr)
{
    hipLaunchKernelGGL(k_iter_select, dim3(1), dim3(SEL_NT), 0, s, prob, pred, P, ncls, prev_n, pscore, pbox, pcls,
                       min_score, max_rows, B, cls_out, src_out, count_out, Pptr, Uptr);
}

void azk_iter_take(hipStream_t s, const int *Nptr, int cap, const int *inv, const int *cls, int ncls, const float *prob_u,
                   const double *pred_u, float *score_out, double *box_out)
{
    int g = (cap + 255) / 256;
    g = g < 1 ? 1 : g;
    hipLaunchKernelGGL(k_iter_take, dim3(g), dim3(256), 0, s, Nptr, cap, inv, cls, ncls, prob_u, pred_u, score_out, box_out);
}
