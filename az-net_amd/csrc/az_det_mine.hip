// az_det_mine.hip -- online hard-example mining for the detection trainer (Shrivastava et al., CVPR 2016): one call runs the
// trainer's TEST-phase forward over a whole pool of rows, computes one loss per row, runs greedy NMS per image with the loss
// as score and hands back the first `per_image` survivors of every image.
//   forward          exactly what az_det_solver_forward_test / _forward_test_skip enqueue (RoIPool or the skip front, then
//                    det_head_forward(train = false)) in the trainer's current precision; no softmax launch of its own
//   k_det_row_loss   one wave per row: the row's softmax cross-entropy (k_solver_softmax_loss's arithmetic) plus the SmoothL1
//                    of its own class's four deltas (k_solver_smooth_l1's with weight 1), the row's NMS record
//                    [x1, y1, x2, y2, loss] and a flag when a loss, or the sum of a row's exponentials, is not finite
//   NMS              nms_groups_dev (az_nms.hip): the kernels of az_nms_batched / az_nms on the records where they lie
//   k_mine_select    per image: keep list -> global row indices, the first per_image of them -> sel
// Nothing but the selection (and, on request, the row losses) comes back to the host.  No floating-point atomics: the same
// call from the same state gives the same bits.  Parameter gradients, history and the accumulate flag are not touched.
#include "az_det_solver.h"

namespace {

__device__ __forceinline__ float mine_wave_max(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float mine_wave_sum(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);       // (k_solver_softmax_loss's butterfly)
    return v;
}

// Row r = 4 * blockIdx.x + wave.  ncls <= 256: up to four columns per lane (lane, lane + 64, ...), the sum lane-strided and
// then over the butterfly, p = e / sum -- as k_solver_softmax_loss computes them.  cls = -log(max(p[label], FLT_MIN));
// bbox = ((f0 + f1) + f2) + f3 over the label's four columns (label > 0 and targets given, else 0); loss = cls + bbox.
constexpr int MINE_PER_LANE = 4;
__global__ void __launch_bounds__(256) k_det_row_loss(const float *__restrict__ x, const float *__restrict__ bb,
                                                      const float *__restrict__ labels, const float *__restrict__ t4,
                                                      const float *__restrict__ rois, int R, int ncls, float *__restrict__ loss,
                                                      float *__restrict__ lcls, float *__restrict__ lbb, float *__restrict__ rec,
                                                      int *__restrict__ flag)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    if (r >= R) return;                          // (the whole wave)
    const float *xr = x + (size_t)r * ncls;
    float v[MINE_PER_LANE];
    float m = -FLT_MAX;
#pragma unroll
    for (int q = 0; q < MINE_PER_LANE; ++q) {
        const int j = lane + 64 * q;
        v[q] = j < ncls ? xr[j] : -FLT_MAX;
        m = fmaxf(m, v[q]);
    }
    m = mine_wave_max(m);
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < MINE_PER_LANE; ++q) {
        const int j = lane + 64 * q;
        v[q] = j < ncls ? expf(v[q] - m) : 0.0f;
        s = s + v[q];
    }
    s = mine_wave_sum(s);
    const int lab = (int)labels[r];              // (checked on the host: a class)
    float pl = 0.0f;
#pragma unroll
    for (int q = 0; q < MINE_PER_LANE; ++q)
        if (lane + 64 * q == lab) pl = v[q] / s;
    pl = __shfl(pl, lab & 63, 64);
    const float cls = -logf(fmaxf(pl, FLT_MIN));
    float box = 0.0f;
    if (lab > 0 && t4) {                         // (wave-uniform)
        const int q = lane & 3;
        const float d = bb[(size_t)r * 4 * ncls + 4 * lab + q] - t4[4 * (size_t)r + q];
        const float ad = fabsf(d);
        const float f = ad < 1.0f ? 0.5f * d * d : ad - 0.5f;
        const float f0 = __shfl(f, 0, 64), f1 = __shfl(f, 1, 64), f2 = __shfl(f, 2, 64), f3 = __shfl(f, 3, 64);
        box = ((f0 + f1) + f2) + f3;
    }
    const float tot = cls + box;
    if (lane == 0) {
        loss[r] = tot; lcls[r] = cls; lbb[r] = box;
        if (!isfinite(tot) || !isfinite(s)) atomicOr(flag, 1);      // (max(NaN, FLT_MIN) is FLT_MIN: the clamp would hide a NaN score)
    }
    if (lane < 5) rec[5 * (size_t)r + lane] = lane < 4 ? rois[5 * (size_t)r + 1 + lane] : tot;
}

// Image i = blockIdx.x owns the rows [off[i], off[i + 1]); keep holds its keep list as indices inside the image, descending
// loss.  keep_rows[off[i] + k] = the k-th kept row (global), -1 behind the list; sel[i * per_image + k] for k < min(per_image,
// kept), n_sel[i] their number.
__global__ void __launch_bounds__(256) k_mine_select(const int *__restrict__ off, const long long *__restrict__ keep,
                                                     const int *__restrict__ nkeep, int per_image, int *__restrict__ keep_rows,
                                                     int *__restrict__ sel, int *__restrict__ n_sel)
{
    const int i = blockIdx.x, o = off[i], n = off[i + 1] - o;
    const int nk = min(nkeep[i], n);
    for (int k = threadIdx.x; k < n; k += 256) keep_rows[o + k] = k < nk ? o + (int)(keep[o + k] & 0xFFFFFFFFll) : -1;
    const int ns = min(nk, per_image);
    for (int k = threadIdx.x; k < ns; k += 256) sel[(size_t)i * per_image + k] = o + (int)(keep[o + k] & 0xFFFFFFFFll);
    if (threadIdx.x == 0) n_sel[i] = ns;
}

// What both entries refuse before anything is enqueued, beyond their front's own checks; fills s->mn.off (the images' row ranges).
int det_mine_check(az_det_solver *s, int N, const float *rois, int R, const float *labels, double nms_thresh, int per_image,
                   const int32_t *sel_out, const int32_t *n_sel_out, const std::string &who)
{
    az_ctx *c = s->c;
    if (!labels || !sel_out || !n_sel_out) return fail(c, AZ_ERR_INVALID, who + ": null labels, sel_out or n_sel_out");
    if (per_image < 1) return fail(c, AZ_ERR_INVALID, who + ": per_image must be at least 1");
    if (!std::isfinite(nms_thresh) || nms_thresh < 0.0) return fail(c, AZ_ERR_INVALID, who + ": nms_thresh must be finite and not negative");
    if ((long long)N * per_image > 0x3fffffffLL) return fail(c, AZ_ERR_INVALID, who + ": N * per_image too large");
    const int nc = s->ncls;
    for (int r = 0; r < R; ++r)
        if (!(labels[r] >= 0.0f && labels[r] < (float)nc) || labels[r] != std::floor(labels[r]))
            return fail(c, AZ_ERR_INVALID, who + ": label " + std::to_string(labels[r]) + " of row " + std::to_string(r) + " is no class in [0, " + std::to_string(nc) + ")");
    for (int r = 1; r < R; ++r)
        if (rois[5 * (size_t)r] < rois[5 * (size_t)(r - 1)])
            return fail(c, AZ_ERR_INVALID, who + ": the image index of row " + std::to_string(r) + " is below the row's before it (column 0 must not decrease)");
    std::vector<int> &off = s->mn.off;
    off.assign((size_t)N + 1, R);
    int r = 0;
    for (int i = 0; i < N; ++i) {                // (tr_check_rois: every index is a whole number in [0, N))
        off[i] = r;
        while (r < R && (int)rois[5 * (size_t)r] == i) ++r;
    }
    return AZ_OK;
}

// The mining buffers, allocated with the trainer's memory at the first call (rows: maxR) and whenever a call brings more images
int det_mine_reserve(az_det_solver *s, int N)
{
    az_det_solver::Mine &m = s->mn;
    int rc = AZ_OK;
    const size_t R = (size_t)s->maxR;
#define SA(p, n) if (rc == AZ_OK) rc = tr_alloc(s, &m.p, (n))
    if (!m.flag) { SA(rec, R * 5); SA(loss, R); SA(lcls, R); SA(lbb, R); SA(tgt4, R * 4); SA(keep, R); SA(keep_rows, R); SA(flag, 1); }
    if (rc == AZ_OK && N > m.capN) {             // (the smaller arrays stay in allocs until destroy, as attach_skip's slabs do)
        const size_t n = (size_t)N + (size_t)N / 2 + 16;
        m.capN = 0;
        SA(goff, n + 1); SA(gsel, n); SA(nkeep, n); SA(nsel, n);
        if (rc == AZ_OK) m.capN = (int)n;
    }
#undef SA
    return rc;
}

// The part behind the forward pass: row losses, records, NMS, selection; waits for the stream and hands the result over
int det_mine_finish(az_det_solver *s, int N, int R, const float *labels, const float *targets, double nms_thresh, int per_image,
                    int32_t *sel_out, int32_t *n_sel_out, float *row_loss_out, const std::string &who)
{
    az_ctx *c = s->c;
    az_det_solver::Mine &m = s->mn;
    hipStream_t st = c->stream;
    s->trained = 0; s->sk.trained = 0;
    m.R = 0; m.N = 0;
    // the selection [N][per_image]: on the context's scratch (its size is the caller's, not the trainer's)
    int rc = scratch_grow(c, 0, (size_t)N * per_image * sizeof(int));
    if (rc != AZ_OK) return rc;
    int *sel = (int *)c->scratch[0].p;
    HIPCHK(c, hipMemcpyAsync(s->labels, labels, (size_t)R * sizeof(float), hipMemcpyHostToDevice, st));
    if (targets) HIPCHK(c, hipMemcpyAsync(m.tgt4, targets, (size_t)R * 4 * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(m.goff, m.off.data(), ((size_t)N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(m.flag, 0, sizeof(int), st));
    { Timed t(c, "row_loss", 0);
      hipLaunchKernelGGL(k_det_row_loss, dim3((R + 3) / 4), dim3(256), 0, st, s->s_cls, s->s_bb, s->labels,
                         targets ? m.tgt4 : (const float *)nullptr, s->rois, R, s->ncls, m.loss, m.lcls, m.lbb, m.rec, m.flag); }
    if ((rc = nms_groups_dev(c, m.rec, m.off.data(), m.goff, m.gsel, m.small, N, nms_thresh, m.keep, m.nkeep, who.c_str())) != AZ_OK) return rc;
    { Timed t(c, "mine_select", 0);
      hipLaunchKernelGGL(k_mine_select, dim3(N), dim3(256), 0, st, m.goff, m.keep, m.nkeep, per_image, m.keep_rows, sel, m.nsel); }
    int h_flag = 0;
    m.h_sel.resize((size_t)N * per_image);
    m.h_nsel.resize((size_t)N);
    HIPCHK(c, hipMemcpyAsync(&h_flag, m.flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(m.h_nsel.data(), m.nsel, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(m.h_sel.data(), sel, (size_t)N * per_image * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    m.R = R; m.N = N;                            // (the losses can be fetched, also behind the error below)
    if (h_flag) return fail(c, AZ_ERR_INVALID, who + ": a row's scores or its loss are not finite");
    for (int i = 0; i < N; ++i) {
        const int ns = m.h_nsel[i];
        if (ns < 0 || ns > per_image || ns > m.off[i + 1] - m.off[i]) return fail(c, AZ_ERR_HIP, who + ": the kernels left no result");
    }
    for (int i = 0; i < N; ++i) {
        n_sel_out[i] = m.h_nsel[i];
        std::memcpy(sel_out + (size_t)i * per_image, m.h_sel.data() + (size_t)i * per_image, (size_t)m.h_nsel[i] * sizeof(int));
    }
    if (row_loss_out) HIPCHK(c, hipMemcpy(row_loss_out, m.loss, (size_t)R * sizeof(float), hipMemcpyDeviceToHost));
    return AZ_OK;
}

}  // namespace

bool det_mine_fetch(az_det_solver *s, const std::string &nm, const void **src, size_t *bytes)
{
    const az_det_solver::Mine &m = s->mn;
    if (!m.rec || !m.R) return false;
    const size_t R = (size_t)m.R;
    struct Ent { const char *n; const void *p; size_t b; };
    const Ent tab[] = {{"mine_loss", m.loss, R * 4}, {"mine_loss_cls", m.lcls, R * 4}, {"mine_loss_bbox", m.lbb, R * 4},
                       {"mine_keep", m.keep_rows, R * 4}, {"mine_nkeep", m.nkeep, (size_t)m.N * 4}};
    for (const Ent &e : tab) if (nm == e.n) { *src = e.p; *bytes = e.b; return true; }
    return false;
}

extern "C" {

int az_det_solver_mine(az_det_solver *s, const float *conv_dev, int N, int H, int W, int channels_last, const float *rois, int R,
                       const float *labels, const float *targets, double nms_thresh, int per_image, int32_t *sel_out,
                       int32_t *n_sel_out, float *row_loss_out)
{
    const std::string who = "az_det_solver_mine";
    int rc = tr_check_step(s, conv_dev, N, H, W, rois, R, who);
    if (rc != AZ_OK) return rc;
    az_ctx *c = s->c;
    if (s->sk.attached) return fail(c, AZ_ERR_STATE, who + ": the trainer carries a skip front (az_det_solver_mine_skip)");
    if ((rc = det_mine_check(s, N, rois, R, labels, nms_thresh, per_image, sel_out, n_sel_out, who)) != AZ_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = det_mine_reserve(s, N)) != AZ_OK) return rc;
    if (!(c->profiling & 4)) clear_events(c);
    if ((rc = tr_roi_pool_forward(s, conv_dev, N, H, W, channels_last, rois, R)) != AZ_OK) return rc;
    det_head_forward(s, R, false, 0, 0);
    return det_mine_finish(s, N, R, labels, targets, nms_thresh, per_image, sel_out, n_sel_out, row_loss_out, who);
}

int az_det_solver_mine_skip(az_det_solver *s, int n_src, const int *Cs, const void *const *maps_dev, const int *Hs, const int *Ws,
                            int N, int channels_last, const float *rois, int R, const float *labels, const float *targets,
                            double nms_thresh, int per_image, int32_t *sel_out, int32_t *n_sel_out, float *row_loss_out)
{
    const std::string who = "az_det_solver_mine_skip";
    int rc = skip_pass_check(s, who, n_src, Cs, maps_dev, Hs, Ws, N, rois, R);
    if (rc != AZ_OK) return rc;
    az_ctx *c = s->c;
    if ((rc = det_mine_check(s, N, rois, R, labels, nms_thresh, per_image, sel_out, n_sel_out, who)) != AZ_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = det_mine_reserve(s, N)) != AZ_OK) return rc;
    if (!(c->profiling & 4)) clear_events(c);
    if ((rc = skip_test_forward(s, maps_dev, Hs, Ws, N, channels_last, rois, R)) != AZ_OK) return rc;
    return det_mine_finish(s, N, R, labels, targets, nms_thresh, per_image, sel_out, n_sel_out, row_loss_out, who);
}

}  // extern "C"
