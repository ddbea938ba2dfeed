// az_batch.hip -- SEVERAL images walk their zoom trees in lockstep: the two small kernels that make the rois every image
// forwards at a level go through the head in ONE pass, and (below them) the host side, batch_launch_impl.
//
// The reference forwards one image at a time (lib/detect/test.py:508-513, one `_az_forward` per level of one image,
// test.py:373-391); its roi blob nevertheless carries Caffe's batch index in column 0 (test.py:93-97, always 0 there).
// At a tuned threshold a level of one image is a few dozen rois -- far too few for a pass over the 411 MB of int6 weights
// to be anything but a weight stream -- and what one image does at a level does not depend on any other image.  So B
// images (of one shape or of several, as long as their searches have the same number of levels) are searched together: every image keeps its own tree (an az_ctx of its own: regions, counters,
// candidates, geometry kernels as workgroups (., b) of one launch, az_fused.hip / az_level.hip / az_static.hip), and per
// level
//   k_batch_gather    concatenates the images' unique rois -- column 0 = the image's index in the batch, which RoIPool
//                     reads as Caffe's roi_batch_ind (az_head.hip) -- and their anchor boxes, and leaves the row offsets
//                     and the pass's row count on the device (no host synchronisation anywhere); also every image's
//                     map size (RoIPool clamps a window to ITS map) and every row's image size (the heads clip a decoded
//                     box to ITS image): the images of a batch may differ in shape;
//   the head          RoIPool, int6, slab sum, int7, heads: the unchanged kernels on the concatenated rows (a row's bits do
//                     not depend on which rows share its launch: tests/test_gpu_parity.py);
//   k_batch_scatter   hands every image its rows of the head's outputs, where its geometry kernel expects them.
// Same results as the level loop on each image alone, bit for bit (tests/test_gpu_batch.py).
#include "az_search.h"

namespace {

// offsets of the images' rows in the pass; an image whose search has failed (error word set) forwards nothing more
__device__ __forceinline__ int batch_offsets(const AzGatherArgs &a, int *off /* [n + 1], LDS or registers */)
{
    int run = 0;
    for (int b = 0; b < a.n; ++b) {
        off[b] = run;
        int r = *a.rows[b];
        if ((a.err[b] && *a.err[b] != 0) || r < 0) r = 0;
        run += r;
    }
    off[a.n] = run;
    return run;
}

__global__ void __launch_bounds__(256) k_batch_gather(AzGatherArgs a)
{
    __shared__ int off[AZ_BATCH_MAX + 1];
    if (threadIdx.x == 0) batch_offsets(a, off);
    __syncthreads();
    const int total = off[a.n];
    if (total > a.capR) {
        // the pass does not fit the head's buffers: every image's search is marked and run again on its own (host)
        if (blockIdx.x == 0 && threadIdx.x < a.n && a.err[threadIdx.x]) atomicOr(a.err[threadIdx.x], 2048);
        if (blockIdx.x == 0 && threadIdx.x == 0) { for (int b = 0; b <= a.n; ++b) a.off_out[b] = 0; a.off_out[AZ_BATCH_MAX + 1] = 0; }
        return;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x <= a.n) a.off_out[threadIdx.x] = off[threadIdx.x];
        if (threadIdx.x == 0) a.off_out[AZ_BATCH_MAX + 1] = total;          // the pass's row count (the head kernels' Mptr)
        if (threadIdx.x < a.n) {
            a.feats_out[threadIdx.x] = a.feat[threadIdx.x];
            a.feat_hw_out[2 * threadIdx.x] = a.fh[threadIdx.x];
            a.feat_hw_out[2 * threadIdx.x + 1] = a.fw[threadIdx.x];
        }
    }
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < total; r += gridDim.x * blockDim.x) {
        int b = 0;
        while (b + 1 < a.n && r >= off[b + 1]) ++b;
        const int i = r - off[b];
        const float *src = a.rois[b] + 5 * (size_t)i;
        float *dst = a.rois_cat + 5 * (size_t)r;
        dst[0] = (float)b;                                                   // Caffe's roi_batch_ind
        dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3]; dst[4] = src[4];
        a.row_hw_out[2 * (size_t)r] = a.im_h[b];
        a.row_hw_out[2 * (size_t)r + 1] = a.im_w[b];
        if (a.ubox[b]) {
            const double *ub = a.ubox[b] + 4 * (size_t)i;
            double *ud = a.ubox_cat + 4 * (size_t)r;
            ud[0] = ub[0]; ud[1] = ub[1]; ud[2] = ub[2]; ud[3] = ub[3];
        }
    }
}

// one wave per row of the pass
__global__ void __launch_bounds__(256) k_batch_scatter(AzScatterArgs a)
{
    __shared__ int off[AZ_BATCH_MAX + 1];
    if (threadIdx.x <= a.n) off[threadIdx.x] = a.off[threadIdx.x];
    __syncthreads();
    const int total = off[a.n];
    const int lane = threadIdx.x & 63;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < total; r += nwaves) {
        int b = 0;
        while (b + 1 < a.n && r >= off[b + 1]) ++b;
        const size_t i = (size_t)(r - off[b]);
        if (lane == 0) a.zoom_d[b][i] = a.zoom[r];
        if (lane < AZ_NSUB) {
            a.score_d[b][i * AZ_NSUB + lane] = a.score[(size_t)r * AZ_NSUB + lane];
            a.keep_d[b][i * AZ_NSUB + lane] = a.keep[(size_t)r * AZ_NSUB + lane];
            if (a.key) a.key_d[b][i * AZ_NSUB + lane] = a.key[(size_t)r * AZ_NSUB + lane];
        }
        if (lane < 4 * AZ_NSUB) a.pred_d[b][i * 4 * AZ_NSUB + lane] = a.pred[(size_t)r * 4 * AZ_NSUB + lane];
    }
}

static_assert(sizeof(AzGatherArgs) <= 4000 && sizeof(AzScatterArgs) <= 4000, "kernel arguments are limited to 4 KB");

}  // namespace

void azk_batch_gather(hipStream_t s, const AzGatherArgs &a)
{
    hipLaunchKernelGGL(k_batch_gather, dim3(16), dim3(256), 0, s, a);
}

void azk_batch_scatter(hipStream_t s, const AzScatterArgs &a)
{
    hipLaunchKernelGGL(k_batch_scatter, dim3(64), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------------------------------------------
// A batch of images of one shape searched in lockstep (include/aznet_hip.h: az_batch_launch; az_batch.hip).
// Image b's tree lives in slots[b] (an az_ctx of its own); the head passes run in lane L's buffers on L's stream:
//   pass 0   the root and its children of every image (rows that depend on the image shape only: the first 1 + |B1| rows of
//            the cached speculative pre-pass), outputs straight into L's zoom_s / score_s / delta_s -- image b's at row
//            b * (1 + |B1|), a host-known offset; k_spec_levels (two fused levels) of every image in one launch
//   level l  (l = 2 .. nlev-1) gather of the images' unique rois -> ONE head pass -> scatter -> k_level_geom of every image
//            in one launch (the last level: k_final_select, which also makes the top-k into the image's result block)
// then every image's result block on its way to the host, as for a search launched alone.
namespace {

template <typename T> T *args_at(unsigned char *base, size_t &off, int n)
{
    off = (off + 15) & ~(size_t)15;
    T *p = reinterpret_cast<T *>(base + off);
    off += sizeof(T) * (size_t)n;
    return p;
}

void head_pass_batch(az_ctx *L, az_ctx::Batch &B, const AzHeadDims &d, const int *Mptr, int im_h, int im_w, double eps, float *zoom, float *score,
                     float *delta, double min_side, bool keep_flags, bool keys, bool many_rows)
{
    hipStream_t s = L->stream;
    // (gemm mode 3 -- int6 on the 16-bit matrix cores, every fp32 operand as three bf16 terms: the planes carry no per-map
    //  scale, so the images of a batch share a pass there as well; mode 2's fp16 terms are scaled per map: not taken)
    azk_roi_pool(s, nullptr, d, L->spatial_scale, B.rois_cat, Mptr, L->maxR, L->pool5, L->pool5p,
                 azk_act_plane_elems(L->maxR, d.K6), L->gemm_parts, 0, 0, nullptr, B.feats, B.feat_hw);
    // (only the device knows the row count; both kernels are correct and bit-identical for any: the last batch's rows decide)
    fc_layer_forward(L, s, L->fc6, {L->pool5, L->pool5p, azk_act_plane_elems(L->maxR, d.K6), L->part, L->t6, L->h6, L->gscale}, Mptr,
                     many_rows, {"fc6_gemm", "fc6_reduce", "fc6_L", "fc6_L_reduce", "fc6_U"}, -1, nullptr, false);
    float *p7 = L->part7 ? L->part7 : L->part;
    azk_fc_gemm(s, L->h6, d.n6, L->W7, d.n6, Mptr, L->maxR, d.n7, d.n6, L->S7, p7, 1 << 30, nullptr);
    azk_tail(s, p7, L->S7, L->b7, d.n7, L->Wt, L->bt, B.ubox_cat, Mptr, L->maxR, im_h, im_w, eps, zoom, score, delta,
             L->pred_u, keep_flags ? L->keep_u : nullptr, min_side, (keep_flags && keys) ? L->key_u : nullptr, B.row_hw);
}

}  // namespace

int batch_launch_impl(az_ctx *L, az_ctx::Batch &B, int n_all, az_ctx **slots_all, const az_params *pa_all, const float *const *maps_all,
                      const int *Hs_all, const int *Ws_all, int *not_taken)
{
    *not_taken = 0;
    int rc = check_ready(L, false, true);          // (join: the passes work in the lane's per-search head buffers)
    if (rc) return rc;
    if (!pa_all || n_all < 1 || n_all > AZ_BATCH_MAX || !slots_all || !maps_all || !Hs_all || !Ws_all)
        return fail(L, AZ_ERR_INVALID, "az_batch_launch: bad arguments");
    const az_params *p = &pa_all[0];                // (what the images of a batch must share is checked against the first)
    for (int b = 0; b < n_all; ++b) {
        const az_params &q = pa_all[b];
        if (Hs_all[b] <= 0 || Ws_all[b] <= 0 || q.im_h <= 0 || q.im_w <= 0 || !(q.scale > 0) || q.batch_size <= 0 || !(q.min_side > 0))
            return fail(L, AZ_ERR_INVALID, "az_batch_launch: bad arguments");
        if (!q.fixed_num || (q.reserved & 4)) return fail(L, AZ_ERR_INVALID, "az_batch_launch: fixed proposal count, not the tuner's variant");
        if (q.num_proposals != p->num_proposals || q.reserved != p->reserved || q.eps != p->eps || q.min_side != p->min_side)
            return fail(L, AZ_ERR_INVALID, "az_batch_launch: the images of a batch share num_proposals, eps, min_side and the flags");
    }
    const int k = p->num_proposals;
    if (k <= 0) return fail(L, AZ_ERR_INVALID, "az_batch_launch: num_proposals must be positive");
    if (k > AZ_TOPK_MAX) return fail(L, AZ_ERR_CAPACITY, "az_batch_launch: num_proposals > 4096");
    int nlev = 0;                                   // the batch's deepest tree; image b walks nl_all[b] levels
    int nl_all[AZ_BATCH_MAX];
    for (int b = 0; b < n_all; ++b) {
        nl_all[b] = num_levels(pa_all[b].im_h, pa_all[b].im_w, pa_all[b].min_side) - 1;
        nlev = nl_all[b] > nlev ? nl_all[b] : nlev;
    }
    for (int b = 0; b < n_all; ++b) {
        if (!slots_all[b] || !maps_all[b]) return fail(L, AZ_ERR_INVALID, "az_batch_launch: null slot / map");
        if (!slots_all[b]->pend.empty()) return fail(L, AZ_ERR_STATE, "az_batch_launch: an image slot still holds an unfetched search");
    }
    HIPCHK(L, hipSetDevice(L->device));
    hipStream_t s = L->stream;
    // (before anything can decide that the images are searched one by one: those searches use the slices, too)
    const size_t res_slot = RES_HDR + (size_t)AZ_TOPK_MAX * 36;
    if (!B.res_dev) {
        HIPCHK(L, reserve_group({{&B.res_own[0], res_slot * AZ_BATCH_MAX}, {&B.res_own[1], res_slot * AZ_BATCH_MAX}}));
        B.res_dev = B.res_own[0].as<unsigned char>(); B.res_host = B.res_own[1].as<unsigned char>();
        HIPCHK(L, hipMemsetAsync(B.res_dev, 0, res_slot * AZ_BATCH_MAX, s));
    }
    // this batch's blocks: k proposals each, side by side
    const size_t res_stride = (RES_HDR + (size_t)k * 36 + 255) & ~(size_t)255;
    for (int b = 0; b < n_all; ++b) {
        az_ctx *t = slots_all[b];
        t->cnt = reinterpret_cast<AzCounts *>(B.res_dev + (size_t)b * res_stride);
        t->h_res[0] = B.res_host + (size_t)b * res_stride;
    }
    auto skip_at = [&](int line) {
        if (L->env.full_debug) fprintf(stderr, "az: batch not taken in lockstep (%s:%d)\n", __FILE__, line);
        *not_taken = 1;
        return AZ_ERR_STATE;
    };
#define skip() skip_at(__LINE__)
    if (nlev > AZ_MAX_LEVELS || (p->reserved & (1 | 2 | 8 | 16)) || L->gemm_parts == 2) return skip();
    for (int b = 0; b < n_all; ++b) if (nl_all[b] < 3) return skip();        // (an image too small for two fused levels + one more)
    // the images may differ in shape (each has its own pre-pass, its own map size, its own clipping box) and in the number of
    // levels (an image's last level gets its final selection where the others get their mid-tree geometry kernel; it has no
    // rows in the passes after that); a shape one of the contexts has learnt not to take on the fused kernels keeps the batch
    // off them
    struct Pre { const float *urois; const double *B1; const int *choff, *Udev; int P1, CH; };
    std::vector<Pre> pre_all(n_all);
    long rows0_all = 0;
    for (int b = 0; b < n_all; ++b) {
        const az_params &q = pa_all[b];
        az_ctx *t = slots_all[b];
        for (const az_ctx *x : {(const az_ctx *)L, (const az_ctx *)t}) {
            if ((q.im_h == x->nofuse_h && q.im_w == x->nofuse_w) || (q.im_h == x->nofuse_lv_h && q.im_w == x->nofuse_lv_w)) return skip();
            for (const auto &e : x->lv_limits) if (e.h == q.im_h && e.w == q.im_w) return skip();
        }
        // the shape's pre-pass (B1, the rois of root + B1, counters): cached per shape on the lane
        SearchPlan sp{};
        sp.fused = true; sp.defer_root = false;
        if ((rc = ensure_spec_cache(L, &q, sp)) != AZ_OK) return rc;
        if (L->spc[0].h != q.im_h || L->spc[0].w != q.im_w) return skip();     // (the pre-pass outgrew the context: nofuse_*)
        pre_all[b] = {L->spec_urois[0], L->specB1[0], L->spec_choff[0], L->spec_U[0], L->spc[0].P1, L->spc[0].CH};
        rows0_all += 1 + L->spc[0].P1;
    }
    if ((size_t)rows0_all > (size_t)L->maxR) return skip();
    if (!B.off) {
        Buf *o = B.own;
        HIPCHK(L, reserve_group({{&o[0], (AZ_BATCH_MAX + 2) * sizeof(int)}, {&o[1], (size_t)L->maxR * 5 * sizeof(float)},
                                 {&o[2], (size_t)L->maxR * 4 * sizeof(double)}, {&o[3], AZ_BATCH_MAX * sizeof(float *)},
                                 {&o[4], AZ_BATCH_MAX * 2 * sizeof(int)}, {&o[5], (size_t)L->maxR * 2 * sizeof(int)}}));
        B.off = o[0].as<int>(); B.rois_cat = o[1].as<float>(); B.ubox_cat = o[2].as<double>(); B.feats = o[3].as<const float *>();
        B.feat_hw = o[4].as<int>(); B.row_hw = o[5].as<int>();
        HIPCHK(L, hipMemsetAsync(B.ubox_cat, 0, (size_t)L->maxR * 4 * sizeof(double), s));
    }
    const size_t need = 64 + ((sizeof(AzFusedArgs) + 16) + (sizeof(AzLevelArgs) + sizeof(AzFinalArgs) + 32) * (size_t)nlev) * AZ_BATCH_MAX;
    if (B.args_cap < need) {
        if (B.args_dev) HIPCHK(L, hipStreamSynchronize(s));
        B.args_dev = nullptr; B.args_host = nullptr; B.args_cap = 0;
        HIPCHK(L, reserve_group({{&B.args_own[0], need}, {&B.args_own[1], need}}));
        B.args_dev = B.args_own[0].as<unsigned char>(); B.args_host = B.args_own[1].as<unsigned char>(); B.args_cap = need;
    }
    // A batch whose levels would not fit the head's buffers (max_regions rows per pass) -- going by the rows per image of the
    // last batch fetched on this lane -- is enqueued as several lockstep programs, one after the other, of as many images each
    // as fit (a pass that overflows all the same marks its images: they are searched again alone by az_batch_fetch).
    int per = n_all;
    if (B.hint_n > 0) {
        long mx = 0;
        for (int l = 0; l < AZ_MAX_LEVELS; ++l) mx = B.rows_hint[l] > mx ? B.rows_hint[l] : mx;
        const double per_img = (double)mx / B.hint_n;
        if (per_img * n_all > 0.9 * L->maxR) per = (int)(0.9 * L->maxR / per_img);
        if (per < 1) per = 1;
    }
    size_t off = 0;
    for (int i0 = 0; i0 < n_all; i0 += per) {
        const int n = n_all - i0 < per ? n_all - i0 : per;
        az_ctx **slots = slots_all + i0;
        const float *const *maps = maps_all + i0;
        const az_params *pa = pa_all + i0;
        const int *Hs = Hs_all + i0, *Ws = Ws_all + i0;
        const Pre *pre = pre_all.data() + i0;
        const int *nl = nl_all + i0;
        int off0[AZ_BATCH_MAX + 1];                   // first row of every image in pass 0 (root + its children: host-known)
        off0[0] = 0;
        for (int b = 0; b < n; ++b) off0[b + 1] = off0[b] + 1 + pre[b].P1;
        AzHeadDims d = L->d;
        d.H = Hs[0]; d.W = Ws[0];                     // (RoIPool takes every image's own size from the batch's table)
        // ---- the geometry kernels' arguments, all levels, all images of the part: one block, one copy
        const size_t off_begin = off;
        AzFusedArgs *fa = args_at<AzFusedArgs>(B.args_host, off, n);
        const size_t off_fa = (size_t)((unsigned char *)fa - B.args_host);
        // (per level: the images that go on -- k_level_geom -- and the images whose last level it is -- k_final_select)
        std::vector<size_t> off_lv(nlev, 0), off_fin(nlev, 0);
        std::vector<AzLevelArgs *> la(nlev, nullptr);
        std::vector<AzFinalArgs *> fin(nlev, nullptr);
        std::vector<int> n_mid(nlev, 0), n_fin(nlev, 0);
        for (int l = 2; l < nlev; ++l) {
            la[l] = args_at<AzLevelArgs>(B.args_host, off, n); off_lv[l] = (size_t)((unsigned char *)la[l] - B.args_host);
            fin[l] = args_at<AzFinalArgs>(B.args_host, off, n); off_fin[l] = (size_t)((unsigned char *)fin[l] - B.args_host);
        }
        for (int b = 0; b < n; ++b) {
            az_ctx *t = slots[b];
            const az_params *p = &pa[b];
            const int P1 = pre[b].P1, rows0 = 1 + P1;
            auto INV = [&](int l) { return (l & 1) ? t->inv_odd : t->inv; };
            {
                AzFusedArgs a;
                std::memset(&a, 0, sizeof(a));
                a.cnt = t->cnt;
                a.B[0] = t->B[0]; a.B[1] = t->B[1]; a.srcB[0] = t->srcB[0]; a.srcB[1] = t->srcB[1];
                a.index = t->index; a.inv = INV(2); a.zr = t->zr; a.choff = t->choff; a.csrc = t->csrc;
                a.choff_all = pre[b].choff; a.specB1 = pre[b].B1;
                a.reset = 1; a.specP1 = P1; a.specCH = pre[b].CH; a.specU = rows0;
                a.ubox = t->ubox; a.pred_u = t->pred_u; a.Yall = t->Yall; a.Z = t->Z; a.child = t->child;
                a.zoom_u = t->zoom_u; a.score_u = t->score_u; a.delta_u = t->delta_u; a.Sall = t->Sall;
                a.zoom_s = L->zoom_s + (size_t)off0[b]; a.score_s = L->score_s + (size_t)off0[b] * AZ_NSUB;
                a.delta_s = L->delta_s + (size_t)off0[b] * 4 * AZ_NSUB;
                a.scale = p->scale; a.Tz = p->Tz; a.min_side = p->min_side; a.eps = p->eps; a.dedup = (float)p->dedup;
                a.batch = p->batch_size; a.im_h = p->im_h; a.im_w = p->im_w; a.nlev = nl[b]; a.n_fused = 2;
                a.capR = t->maxR; a.capCh = t->maxCh; a.capCand = t->maxCand;
                a.rois = t->rois; a.urois = t->urois; a.next_dedup = 1; a.defer_root = 0; a.cut_next = 0; a.cut_short = 0;
                a.spec_next = 0; a.choff_next = t->choff_pair; a.crow = t->crow; a.spatial_scale = L->spatial_scale;
                a.row_map = nullptr; a.root_row = 0; a.stab = nullptr; a.stabT = 0;
                a.pred_v = t->pred_v; a.score_v = t->score_v; a.zoom_v = t->zoom_v; a.keep_v = t->keep_v; a.key_v = t->key_v;
                fa[b] = a;
            }
            for (int l = 2; l + 1 < nl[b]; ++l) {
                AzLevelArgs a;
                std::memset(&a, 0, sizeof(a));
                const int cur = l & 1;
                a.cnt = t->cnt; a.level = l; a.nlev = nl[b]; a.cut_next = 0;
                a.B = t->B[cur]; a.Bnext = t->B[cur ^ 1];
                a.pred_u = t->pred_u; a.score_u = t->score_u; a.zoom_u = t->zoom_u; a.keep_u = t->keep_u; a.Uptr = &t->cnt->U[l];
                a.urois = t->urois; a.index = t->index; a.inv = INV(l); a.inv_next = INV(l + 1); a.ubox = t->ubox;
                a.Yall = t->Yall; a.Sall = t->Sall;
                a.scale = p->scale; a.Tz = p->Tz; a.min_side = p->min_side; a.dedup = (float)p->dedup;
                a.batch = p->batch_size; a.capR = t->maxR; a.capCh = t->maxCh; a.capCand = t->maxCand;
                a.force_root = 1; a.root_row = 0; a.lookup_next = 0; a.spec_next = 0;
                a.delta_u = t->delta_u; a.choff_all = t->choff_pair; a.choff_next = t->choff_pair; a.crow = t->crow;
                a.stab = nullptr; a.stabT = 0; a.root_row_full = 0; a.score_all = t->score_s; a.zoom_all = t->zoom_s;
                a.pred_v = t->pred_v; a.score_v = t->score_v; a.zoom_v = t->zoom_v; a.keep_v = t->keep_v; a.key_v = t->key_v;
                a.im_h = p->im_h; a.im_w = p->im_w; a.eps = p->eps; a.spatial_scale = L->spatial_scale;
                la[l][n_mid[l]++] = a;
            }
            {
                AzFinalArgs a;
                std::memset(&a, 0, sizeof(a));
                const int l = nl[b] - 1;
                a.cnt = t->cnt; a.level = l; a.inv = INV(l); a.key_u = t->key_u; a.pred_u = t->pred_u;
                a.score_u = t->score_u; a.zoom_u = t->zoom_u; a.Yall = t->Yall; a.Sall = t->Sall; a.Tz = p->Tz;
                a.force_root = 0; a.capCand = t->maxCand; a.k = k;
                a.Yout = (double *)((unsigned char *)t->cnt + RES_HDR);
                a.Sout = (float *)((unsigned char *)t->cnt + RES_HDR + (size_t)k * 32);
                fin[l][n_fin[l]++] = a;
            }
        }
        HIPCHK(L, hipMemcpyAsync(B.args_dev + off_begin, B.args_host + off_begin, off - off_begin, hipMemcpyHostToDevice, s));

        // ---- pass 0: root + B1 of every image
        AzGatherArgs g;
        std::memset(&g, 0, sizeof(g));
        g.n = n; g.capR = L->maxR; g.off_out = B.off; g.rois_cat = B.rois_cat; g.ubox_cat = B.ubox_cat; g.feats_out = B.feats;
        g.feat_hw_out = B.feat_hw; g.row_hw_out = B.row_hw;
        for (int b = 0; b < n; ++b) {
            g.rows[b] = pre[b].Udev + 1;                  // (ensure_spec_cache: the pass without the third level's rows)
            g.err[b] = nullptr;                           // (the image's counters are cleared by k_spec_levels, behind this pass)
            g.rois[b] = pre[b].urois; g.ubox[b] = nullptr; g.feat[b] = maps[b];
            g.fh[b] = Hs[b]; g.fw[b] = Ws[b]; g.im_h[b] = pa[b].im_h; g.im_w[b] = pa[b].im_w;
        }
        azk_batch_gather(s, g);
        const int *Mptr = B.off + AZ_BATCH_MAX + 1;
        head_pass_batch(L, B, d, Mptr, p->im_h, p->im_w, p->eps, L->zoom_s, L->score_s, L->delta_s, 0.0, false, false,
                        off0[n] >= L->gemm12_dual_rows);
        azk_spec_levels_batch(s, reinterpret_cast<const AzFusedArgs *>(B.args_dev + off_fa), n);
        // ---- the levels
        for (int l = 2; l < nlev; ++l) {
            const bool last = n_fin[l] > 0;               // (some image's last level: the heads also emit the selection keys)
            for (int b = 0; b < n; ++b) {
                az_ctx *t = slots[b];
                g.rows[b] = &t->cnt->PR[l]; g.err[b] = &t->cnt->err; g.rois[b] = t->urois; g.ubox[b] = t->ubox; g.feat[b] = maps[b];
            }
            azk_batch_gather(s, g);
            head_pass_batch(L, B, d, Mptr, p->im_h, p->im_w, p->eps, L->zoom_u, L->score_u, L->delta_u, p->min_side, true, last,
                            (B.hint_n > 0 ? (long)B.rows_hint[l] * n / B.hint_n : 0) >= L->gemm12_dual_rows);
            AzScatterArgs sc;
            std::memset(&sc, 0, sizeof(sc));
            sc.n = n; sc.off = B.off; sc.zoom = L->zoom_u; sc.score = L->score_u; sc.pred = L->pred_u; sc.keep = L->keep_u;
            sc.key = last ? L->key_u : nullptr;
            for (int b = 0; b < n; ++b) {
                az_ctx *t = slots[b];
                sc.zoom_d[b] = t->zoom_u; sc.score_d[b] = t->score_u; sc.pred_d[b] = t->pred_u; sc.keep_d[b] = t->keep_u; sc.key_d[b] = t->key_u;
            }
            azk_batch_scatter(s, sc);
            if (n_mid[l]) azk_level_geom_batch(s, reinterpret_cast<const AzLevelArgs *>(B.args_dev + off_lv[l]), n_mid[l]);
            if (n_fin[l]) azk_final_select_batch(s, reinterpret_cast<const AzFinalArgs *>(B.args_dev + off_fin[l]), n_fin[l]);
        }
        HIPCHK(L, hipGetLastError());
        // ---- every image's record on its way to the host; the searches enter the slots' queues
        for (int b = 0; b < n; ++b) {
            az_ctx *t = slots[b];
            az_ctx::PendingSearch q;
            q.p = pa[b]; q.nlev = nl[b]; q.batch = 1;
            q.npass = 0;
            q.pass_lv[q.npass] = -1; q.pass_src[q.npass++] = -(1 + pre[b].P1) - 1;
            for (int l = 2; l < nl[b]; ++l) {
                q.pass_lv[q.npass] = l;
                q.pass_src[q.npass++] = (int)(&t->cnt->PR[l] - reinterpret_cast<int *>(t->cnt));
            }
            t->feat = maps[b]; t->d.H = Hs[b]; t->d.W = Ws[b];
            q.feat = maps[b]; q.fH = Hs[b]; q.fW = Ws[b]; q.feat_gen = t->feat_gen; q.feat_is_copy = false;
            q.slot = 0;                                   // (the slot's queue is empty: its first result slot, a slice of the arena)
            if (b == 0) HIPCHK(L, hipMemcpyAsync(B.res_host + (size_t)i0 * res_stride, B.res_dev + (size_t)i0 * res_stride, res_stride * n, hipMemcpyDeviceToHost, s));
            HIPCHK(L, hipEventRecord(t->ev_res[q.slot], s));
            q.copied = true;
            q.last_s = s;
            t->last_s = s;
            t->cand_n = -1;
            t->slot_busy[q.slot] = true;
            t->pend.push_back(q);
        }

    }
    L->last_s = s;
    return AZ_OK;
#undef skip
}
