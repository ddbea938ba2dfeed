// az_ctx.hip -- the host helpers every translation unit behind the C ABI shares (declared in az_ctx.h): the geometry buffers,
// the pinned staging, one head pass with its stream and event staging, an fc layer's loader and forward path (FcLayer), the choice between the two fp32 fc GEMMs, the joins
// and checks an entry point starts with.
#include "az_ctx.h"

// Buffers that depend only on the ctx limits (region / candidate capacity).
int ensure_geom(az_ctx *c)
{
    if (c->geom_ready) return AZ_OK;
    hipError_t e0 = hipSetDevice(c->device);
    if (e0 != hipSuccess) return fail(c, AZ_ERR_HIP, "hipSetDevice failed");
    const size_t R = (size_t)c->maxR, CAND = (size_t)c->maxCand, CH = (size_t)c->maxCh;
    int rc;
    DevList &list = c->allocs_geom;
    {   // result block: the counters, then (fixed proposal count) the selected boxes and scores, so that
        // az_propose_fetch is ONE device-to-host copy
        unsigned char *blk = nullptr;
        if ((rc = dalloc(c, list, &blk, RES_HDR + (size_t)AZ_TOPK_MAX * 36)) != AZ_OK) return rc;
        c->cnt = (AzCounts *)blk;
    }
    AZ_A(B[0], R * 4); AZ_A(B[1], R * 4); AZ_A(rois, R * 5); AZ_A(urois, R * 5); AZ_A(key, R); AZ_A(ckey, CH);
    AZ_A(grp, R); AZ_A(index, R); AZ_A(inv, R); AZ_A(inv_odd, R); AZ_A(choff, R); AZ_A(bc_c, (R * AZ_NSUB + 255) / 256 + 1);
    AZ_A(bc_z, (R * AZ_NSUB + 255) / 256 + 1);
    AZ_A(first, CH > R ? CH : R); AZ_A(cflag, R * AZ_NSUB); AZ_A(zflag, R); AZ_A(keep_u, R * AZ_NSUB);
    AZ_A(ubox, R * 4); AZ_A(pred_u, R * AZ_NSUB * 4); AZ_A(Yall, CAND * 4); AZ_A(Z, R * 4); AZ_A(child, CH * 4);
    AZ_A(Yout, CAND * 4); AZ_A(Sout, CAND); AZ_A(sel_idx, CAND); AZ_A(rank_part, (size_t)azk_topk_scratch_ints((int)CAND));
    AZ_A(zoom_u, R); AZ_A(score_u, R * AZ_NSUB); AZ_A(delta_u, R * 4 * AZ_NSUB); AZ_A(Sall, CAND);
    AZ_A(zr, R); AZ_A(csrc, CH); AZ_A(choff_all, R); AZ_A(srcB[0], R); AZ_A(srcB[1], R);
    AZ_A(zoom_s, R); AZ_A(score_s, R * AZ_NSUB); AZ_A(delta_s, R * 4 * AZ_NSUB);
    AZ_A(zoom_s2, R); AZ_A(score_s2, R * AZ_NSUB); AZ_A(delta_s2, R * 4 * AZ_NSUB);
    for (int i = 0; i < 2; ++i) { AZ_A(spec_scr_urois[i], R * 5); AZ_A(spec_scr_B1[i], R * 4); AZ_A(spec_scr_choff[i], R); }
    AZ_A(key_u, R * AZ_NSUB);
    AZ_A(choff_pair, R); AZ_A(crow, CH > 8192 ? CH : 8192);
    AZ_A(pred_v, R * AZ_NSUB * 4); AZ_A(score_v, R * AZ_NSUB); AZ_A(zoom_v, R); AZ_A(keep_v, R * AZ_NSUB); AZ_A(key_v, R * AZ_NSUB);
    AZ_A(pred_w, R * AZ_NSUB * 4); AZ_A(score_w, R * AZ_NSUB); AZ_A(zoom_w, R); AZ_A(keep_w, R * AZ_NSUB); AZ_A(key_w, R * AZ_NSUB);
    if (hipMemset(c->ubox, 0, R * 4 * sizeof(double)) != hipSuccess) return fail(c, AZ_ERR_HIP, "hipMemset failed");
    // (a search whose fused level kernel overflows is rerun by the host, but the kernels already enqueued behind it still
    //  run, on whatever the level's inv_index buffer holds: it must always hold valid rows)
    if (hipMemset(c->inv, 0, R * sizeof(int)) != hipSuccess || hipMemset(c->inv_odd, 0, R * sizeof(int)) != hipSuccess ||
        hipMemset(c->index, 0, R * sizeof(int)) != hipSuccess)
        return fail(c, AZ_ERR_HIP, "hipMemset failed");
    c->geom_ready = true;
    return AZ_OK;
}

void clear_events(az_ctx *c)
{
    for (auto &e : c->events) {
        if (e.slot >= 0) continue;
        for (hipEvent_t ev : {e.a, e.b}) c->event_pool.put(ev);
    }
    c->events.clear();
}

// K of lib/detect/test.py:365-368 (Python-2 integer division when MIN_SIDE is integral).
int num_levels(int h, int w, double min_side)
{
    const int side = h < w ? h : w;
    double q;
    if (min_side == std::floor(min_side) && min_side >= 1.0) q = (double)(side / (int)min_side);
    else q = (double)side / min_side;
    if (!(q >= 1.0)) return 0;
    return (int)(std::log2(q) + 1.0);
}

int ensure_host(az_ctx *c, int cap)
{
    if (cap <= c->h_cap) return AZ_OK;
    c->h_cap = 0; c->h_Y = nullptr; c->h_S = nullptr;
    HIPCHK(c, reserve_group({{&c->h_own[0], (size_t)cap * 4 * sizeof(double)}, {&c->h_own[1], (size_t)cap * sizeof(float)}}));
    c->h_Y = c->h_own[0].as<double>(); c->h_S = c->h_own[1].as<float>();
    c->h_cap = cap;
    return AZ_OK;
}

int set_count(az_ctx *c, int *dptr, int v)
{
    // (a 32-bit fill carries the value in the command: nothing on this frame to keep alive, no synchronisation)
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)dptr, v, 1, c->stream));
    return AZ_OK;
}

// Two-term (fp16) mode: the scale of this map's pool5 terms, once per enqueued search / head forward (one small launch).
void prep_scale(az_ctx *c)
{
    if (c->gemm_parts == 2 && c->feat)
        azk_feat_scale(c->stream, c->feat, (long long)c->d.C * c->d.H * c->d.W, c->gscale, c->fc6.w_scale);
}

// One fp32 fc layer's split-K GEMM: the many-row kernel when the layer fits it, the caller expects many rows and the context
// has not disabled the kernel (gemm12_min_rows == 0x7fffffff: AZ_GEMM12_MIN=0, or azk_fc_gemm12_prepare failed), k_fc_splitk
// otherwise.  Both are correct (and bit-identical) for any row count: a wrong `many_rows` costs efficiency, never a result.
void fc_gemm_fp32(const az_ctx *c, hipStream_t s, const float *x, int ldx, const float *W, const int *Mptr, int N, int K, int S,
                  float *part, bool many_rows, unsigned long long *ts)
{
    if (many_rows && c->gemm12_min_rows != 0x7fffffff && azk_fc_gemm12_fits(N, K, S))
        azk_fc_gemm12(s, x, ldx, W, K, Mptr, c->maxR, N, K, S, azk_fc_chunk(K, S), part, 0, ts);
    else
        azk_fc_gemm(s, x, ldx, W, K, Mptr, c->maxR, N, K, S, part, 1 << 30, ts);
}

float fc_weight_scale(const float *w, size_t n)
{
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) { const float a = fabsf(w[i]); if (a > mx) mx = a; }
    if (!(mx > 0.f && mx < INFINITY)) return 1.f;
    int e;
    (void)frexpf(mx, &e);
    return ldexpf(1.f, 15 - e);
}

int fc_layer_alloc(az_ctx *c, DevList &list, FcLayer &f, int parts)
{
    int rc = f.r ? dalloc(c, list, &f.L, azk_tiled_elems(f.r, f.K)) : dalloc(c, list, &f.W, azk_tiled_elems(f.N, f.K));
    if (!rc && f.r) rc = dalloc(c, list, &f.U, (size_t)f.N * f.r);
    if (!rc) rc = dalloc(c, list, &f.b, (size_t)f.N);
    if (!rc && parts) rc = dalloc(c, list, &f.Wp, (size_t)parts * azk_weight_plane_elems(f.N, f.K));
    return rc;
}

// Weights: Caffe [out, in] row-major is already the K-contiguous "B^T" layout the GEMM reads.  A layer that reads pool5,
// which this library keeps bin-major ([p][c], see az_head.hip), gets its columns permuted to match (c*49 + p -> p*C + c).
// The GEMM streams weights tile-major (azk_tile_weights): permute in a row-major temporary, then tile.
int fc_layer_load(az_ctx *c, FcLayer &f, const float *L, const float *W, const float *b, int permC, float *stage, float *tmp)
{
    const size_t lead = (size_t)f.lead();
    const int parts = f.Wp ? c->gemm_parts : 0;
    HIPCHK(c, hipMemcpy(permC ? stage : tmp, f.r ? L : W, lead * f.K * 4, hipMemcpyHostToDevice));
    if (permC) azk_permute_k(c->stream, stage, tmp, (long long)lead, permC, 1);
    if (parts) {          // 16-bit terms of the (permuted, row-major) weights; two fp16 terms: of the scaled weights
        f.w_scale = parts == 2 ? fc_weight_scale(W, (size_t)f.N * f.K) : 0.f;
        azk_split_weight_planes(c->stream, tmp, f.Wp, f.N, f.K, parts, f.w_scale);
    }
    azk_tile_weights(c->stream, tmp, f.r ? f.L : f.W, (int)lead, f.K);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // (the U factor stays row-major [N, r]: the U stage reads Caffe's layout as it is)
    if (f.r) HIPCHK(c, hipMemcpy(f.U, W, (size_t)f.N * f.r * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(f.b, b, (size_t)f.N * 4, hipMemcpyHostToDevice));
    return AZ_OK;
}

// A truncated-SVD layer: t = x . L^T on the split-K GEMM (SL chunks, a fixed function of (K, r); `zero` is the zero bias
// that makes azk_fc_reduce a plain slab sum), then y = relu(t . U^T + b) in one launch (k_lowrank_gemm at every row count:
// a 128 x 128-tile variant for many rows was measured slower).  The L stage's two kernels give a row the
// same bits whatever `many_rows` says.
void fc_layer_forward(az_ctx *c, hipStream_t s, const FcLayer &f, const FcWork &w, const int *Mptr, bool many_rows,
                      const FcNames &names, int level, unsigned long long *ts, bool timed)
{
    const int prof_keep = c->profiling;
    if (!timed) c->profiling &= ~(1 | 2);
    const int prof_pass = c->profiling;
    if (f.r) {
        { Timed t(c, names.L, level, 1);
          fc_gemm_fp32(c, s, w.x, f.K, f.L, Mptr, f.r, f.K, f.SL, w.part, many_rows); }
        { Timed t(c, names.L_reduce, level);
          azk_fc_reduce(s, w.part, f.zero, Mptr, c->maxR, f.r, f.SL, w.t, f.r, 0); }
        { Timed t(c, names.U, level, 1);
          azk_lowrank_gemm(s, w.t, f.r, f.U, f.b, Mptr, c->maxR, f.N, f.r, 1, w.y, f.N); }
    } else {
        if (ts) c->profiling &= ~(1 | 2);                      // (no event pair around a launch that times itself)
        { Timed t(c, names.gemm, level, 1);
          if (c->gemm_parts && f.Wp)
              azk_fc_gemm_terms(s, w.xp, f.K, w.xp_stride, f.Wp, f.K, azk_weight_plane_elems(f.N, f.K), Mptr, c->maxR, f.N, f.K,
                                f.S, azk_fc_chunk(f.K, f.S), w.part, c->gemm_parts, w.gscale);
          else
              fc_gemm_fp32(c, s, w.x, f.K, f.W, Mptr, f.N, f.K, f.S, w.part, many_rows, ts); }
        c->profiling = prof_pass;
        { Timed t(c, names.reduce, level);
          azk_fc_reduce(s, w.part, f.b, Mptr, c->maxR, f.N, f.S, w.y, f.N, 1); }
    }
    c->profiling = prof_keep;
}

// One forward of the head on the `U` rois in ctx->urois (anchors in ctx->ubox); scores and
// deltas go to the given arrays, decoded boxes to ctx->pred_u.
void launch_head(az_ctx *c, const int *Uptr, int level, int im_h, int im_w, double eps, float *zoom, float *score,
                 float *delta, double min_side, bool keep_flags, int coop_tail, const float *urois, const double *ubox,
                 int rows_hint, bool keys)
{
    const AzHeadDims &d = c->d;
    if (c->npass < AZ_MAX_LEVELS + 2) {
        const int *c0 = reinterpret_cast<const int *>(c->cnt);
        const bool in_cnt = Uptr >= c0 && Uptr < c0 + sizeof(AzCounts) / sizeof(int);
        c->pass_lv[c->npass] = level;
        c->pass_src[c->npass++] = in_cnt ? (int)(Uptr - c0) : -(rows_hint > 0 ? rows_hint : 0) - 1;
    }
    const bool split = c->split_now && c->stream2 && c->ev_h6 && c->ev_i7;
    hipStream_t s2 = split ? c->stream2 : c->stream;
    // Stage 1 of a staged search waits for the int7 of the previous one (ev_i7) -- RoIPool included: beside int7 the
    // HBM-bound RoIPool of the next image costs that int7 40 us (70 -> 110) to hide 27 of its own, and the int6 behind it
    // starts later for it.  Measured on one lane, three searches queued: 1.181 -> 1.128 ms per image (two queued: 1.135 ->
    // 1.141: there the host's launch latency did the same by accident).  The same order across the two lanes of a context
    // (a lane's many-row RoIPool behind the OTHER lane's int7, an event both ways) was measured too: 1.114 -> 1.138 ms, not kept.
    // int6 has to wait for that int7 in any case: h6, which this pass's slab sum writes, is that int7's operand -- and an
    // int6 that starts while int7's workgroups still hold CUs runs with stragglers to its end (one persistent workgroup per
    // CU, work dealt statically: measured 1.13 -> 1.24 ms per image when the two overlapped)
    if (c->i7_live) { if (hipStreamWaitEvent(c->stream, c->ev_i7, 0) != hipSuccess) c->async_err = 1; c->i7_live = false; }
    { Timed t(c, "roi_pool", level);
      azk_roi_pool(c->stream, c->feat, d, c->spatial_scale, urois ? urois : c->urois, Uptr, c->maxR, c->pool5, c->pool5p,
                   azk_act_plane_elems(c->maxR, d.K6), c->gemm_parts, 0, coop_tail, c->gemm_parts == 2 ? c->gscale : nullptr,
                   c->pyr_now ? c->pyr_feats : nullptr, c->pyr_now ? c->pyr_hw : nullptr); }
    // (profiling bit 3: the fp32 GEMM launches record their own span instead of an event pair)
    auto span_slot = [&](const char *name) -> unsigned long long * {
        if (!(c->profiling & 8) || !c->span_ring || c->span_next >= az_ctx::SPAN_SLOTS) return nullptr;
        const int sl = c->span_next++;
        c->events.push_back({name, level, nullptr, nullptr, sl});
        return c->span_ring + 2 * (size_t)sl;
    };
    const int prof_keep = c->profiling;
    // many rows: the caller knows the row count on the host (a one-pass plan) -- one weight tile per 12 strips --, or only the
    // device knows it (rows_hint == -1) and the last search had many rows at this level.  The self-timing span is the fp32
    // full-rank layer's alone
    const bool many6 = rows_hint >= c->gemm12_min_rows || rows_hint == -1;
    fc_layer_forward(c, c->stream, c->fc6, {c->pool5, c->pool5p, azk_act_plane_elems(c->maxR, d.K6), c->part, c->t6, c->h6, c->gscale},
                     Uptr, many6, {"fc6_gemm", "fc6_reduce", "fc6_L", "fc6_L_reduce", "fc6_U"}, level,
                     (c->fc6.r || c->gemm_parts) ? nullptr : span_slot("fc6_gemm"));
    // int7 stays in stage 1 -- RoIPool, int6, slab sum, int7 back to back on `stream`: the chip-wide kernels of consecutive
    // images follow each other without an event hop (each ~13 us on the critical path: slab sum -> int7 on the second
    // stream, int7 -> the next image's RoIPool back on the first); stage 2 = the heads (+ geometry, or stage 3).  int7 writes
    // its slabs where the previous search's heads read theirs: it waits for that search's stage 2, which ended ~1000 us
    // before.  One lane, three queued: 1.130-1.135 -> 1.116 ms per image.  (A head without slabs of int7's own: int7 in stage 2.)
    const bool i7_first = split && c->part7;
    if (split && !i7_first) {
        // stage 2 from here on: int7 behind the slab sum, everything the caller enqueues behind this pass behind int7
        if (hipEventRecord(c->ev_h6, c->stream) != hipSuccess || hipStreamWaitEvent(s2, c->ev_h6, 0) != hipSuccess) c->async_err = 1;
        c->gs = s2; c->ts = s2;
    }
    float *p7 = c->part7 ? c->part7 : c->part;
    bool ring = false;
    if (i7_first) {
        if (!c->part7_no_room && !c->part7_ring[1]) {
            c->part7_ring[0] = c->part7;
            for (int q = 1; q < 3 && !c->part7_no_room; ++q)
                if (c->allocs.alloc(&c->part7_ring[q], (size_t)c->S7 * c->maxR * d.n7) != hipSuccess) { c->err.clear(); (void)hipGetLastError(); c->part7_no_room = true; }
            if (c->part7_no_room) c->part7_ring[1] = c->part7_ring[2] = nullptr;     // (no room: one buffer + the wait)
        }
        if (!c->part7_no_room && c->part7_ring[2] && c->part7_ring[0] == c->part7) {
            p7 = c->part7_ring[c->part7_turn];
            c->part7_turn = (c->part7_turn + 1) % 3;
            ring = !c->part7_wait;           // (a failed launch's buffer is not among the three unfetched searches': wait once)
            c->part7_wait = false;
        }
    }
    unsigned long long *ts7 = span_slot("fc7_gemm");
    if (ts7) c->profiling &= ~(1 | 2);
    if (i7_first && !ring && c->s2_live && hipStreamWaitEvent(c->stream, c->ev_s2, 0) != hipSuccess) c->async_err = 1;
    if (i7_first && c->s3_live && !c->three_now && hipStreamWaitEvent(c->stream, c->ev_s3, 0) != hipSuccess) c->async_err = 1;
    { Timed t(c, "fc7_gemm", level, 1);
      azk_fc_gemm(i7_first ? c->stream : s2, c->h6, d.n6, c->W7, d.n6, Uptr, c->maxR, d.n7, d.n6, c->S7, p7, 1 << 30, ts7); }
    c->profiling = prof_keep;
    if (i7_first) {
        // stage 2 from here on: the heads behind int7
        if (hipEventRecord(c->ev_h6, c->stream) != hipSuccess || hipStreamWaitEvent(s2, c->ev_h6, 0) != hipSuccess) c->async_err = 1;
        c->gs = s2; c->ts = s2;
    } else if (split) { if (hipEventRecord(c->ev_i7, s2) != hipSuccess) c->async_err = 1; c->i7_live = true; }
    const bool three = split && c->three_now && c->stream3 && c->ev_tail;
    // (three stages: the heads write the output set the geometry of the search before the previous one read)
    if (three && c->g_live[c->out_par]) {
        if (hipStreamWaitEvent(s2, c->ev_geo[c->out_par], 0) != hipSuccess) c->async_err = 1;
        c->g_live[c->out_par] = false;
    }
    { Timed t(c, "tail", level);       // (finishes int7 as well: slab sum + bias + ReLU while staging its rows)
      azk_tail(s2, p7, c->S7, c->b7, d.n7, c->Wt, c->bt, ubox ? ubox : c->ubox, Uptr, c->maxR, im_h, im_w,
               eps, zoom, score, delta, c->pred_u, keep_flags ? c->keep_u : nullptr, min_side,
               (keep_flags && keys) ? c->key_u : nullptr); }
    if (three) {
        // stage 3 from here on: whatever the caller enqueues behind this pass goes to the third stream, behind the heads
        if (hipEventRecord(c->ev_tail, s2) != hipSuccess || hipStreamWaitEvent(c->stream3, c->ev_tail, 0) != hipSuccess) c->async_err = 1;
        c->gs = c->stream3; c->ts = c->stream3;
    }
}

// Scratch slot `i` of the evaluation entry points, grown to at least `bytes` (half as much again + 256 when it grows).
int scratch_grow(az_ctx *c, int i, size_t bytes)
{
    const hipError_t e = c->scratch[i].reserve(bytes, bytes + bytes / 2 + 256);
    if (e != hipSuccess) return fail(c, AZ_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    return AZ_OK;
}

// `stream` waits for everything the context has enqueued on its second stream (stage 2 of two-stage searches): called by
// whatever touches the per-search buffers and is not stage 1 of another two-stage search.
void join_s2(az_ctx *c)
{
    if (c && c->s2_live && c->stream2 && c->ev_s2) {
        if (hipStreamWaitEvent(c->stream, c->ev_s2, 0) != hipSuccess) c->async_err = 1;
        c->i7_live = false;                       // (ev_i7 lies before ev_s2 on that stream)
    }
    if (c && c->s3_live && c->stream3 && c->ev_s3 && hipStreamWaitEvent(c->stream, c->ev_s3, 0) != hipSuccess) c->async_err = 1;
}

int check_geom(az_ctx *c)
{
    if (!c) return AZ_ERR_INVALID;
    join_s2(c);
    return ensure_geom(c);
}

int check_ready(az_ctx *c, bool need_feat, bool join)
{
    if (!c) return AZ_ERR_INVALID;
    if (!c->head_loaded) return fail(c, AZ_ERR_STATE, "az_load_head has not been called");
    if (need_feat && !c->feat) return fail(c, AZ_ERR_STATE, "no feature map set");
    if (join) join_s2(c);
    return AZ_OK;
}
