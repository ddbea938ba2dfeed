// az_capi.hip -- the C ABI of libaznet_hip.so (include/aznet_hip.h): context lifecycle, head and feature maps, the two
// lanes and the public launch / fetch entry points, measurement switches, the native exchange.  The forms of a search live
// in az_plan.hip / az_shape.hip / az_search.hip / az_batch.hip, the unit entry points in az_units.hip.  There is no CPU fallback anywhere in this library: without a
// gfx950 device az_create fails with AZ_ERR_NO_DEVICE.
#include "az_ctx.h"

extern "C" {

const char *az_version(void) { return AZ_VERSION_STR; }
int az_abi_sizes(void) { return (int)(sizeof(az_params) & 0xffff) | (int)((sizeof(az_stats) & 0xffff) << 16); }

int az_create(int device, az_ctx **out)
{
    if (!out) return AZ_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return AZ_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return AZ_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return AZ_ERR_NO_DEVICE;   // gfx950 code objects only
    if (hipSetDevice(device) != hipSuccess) return AZ_ERR_NO_DEVICE;
    az_ctx *c = new az_ctx();
    c->device = device;
    c->env = az_read_env();
    c->use_graphs = c->env.graph ? 1 : 0; c->plan_cache_max = c->env.plan_cache; c->gemm12_min_rows = c->env.gemm12_min;
    bool ok = c->stream.create(hipStreamNonBlocking) == hipSuccess && c->h_cnt_own.reserve(RES_HDR + (size_t)AZ_TOPK_MAX * 36) == hipSuccess;
    for (int i = 0; i < 3 && ok; ++i) {
        ok = c->h_res_own[i].reserve(RES_HDR + (size_t)AZ_TOPK_MAX * 36) == hipSuccess && c->ev_res[i].create(hipEventDisableTiming) == hipSuccess;
        c->h_res[i] = c->h_res_own[i].as<unsigned char>();
    }
    if (!ok) { delete c; return AZ_ERR_HIP; }
    c->h_cnt = c->h_cnt_own.as<AzCounts>();
    *out = c;
    return AZ_OK;
}

static void destroy_twin(az_ctx *c);
static void destroy_batch(az_ctx *c);

// One head buffer set for the dims / limits / GEMM mode of `t`, allocated in o->allocs (o's error is set on failure):
// pool5, the split-K slabs (`part`: both layers' slabs, at least part_min elements), h6, h7, int7's slabs, the L stage's
// rows t6 of a truncated-SVD int6 and, in the 16-bit-term modes, the operand planes and the scale block, cleared on stream s and waited for.
static int alloc_head_set(az_ctx *o, const az_ctx *t, size_t part_min, hipStream_t s, const char *clear_msg, az_ctx::HeadSet *h)
{
    const size_t R = (size_t)t->maxR;
    const AzHeadDims &d = t->d;
    // (int6's slabs: the full layer's, or the L stage's of a truncated-SVD int6)
    const size_t p6 = t->fc6.slab_elems(R), p7 = (size_t)t->S7 * R * d.n7, planes = (size_t)t->gemm_parts * azk_act_plane_elems((int)R, d.K6);
    auto A = [&](auto **p, size_t n) { return dalloc(o, o->allocs, p, n); };
    *h = az_ctx::HeadSet();                   // (a set made again for a head with fewer optional buffers keeps none of the old)
    int rc = A(&h->pool5, R * d.K6);
    if (!rc) rc = A(&h->part, std::max(std::max(p6, p7), part_min));
    if (!rc) rc = A(&h->h6, R * d.n6);
    if (!rc) rc = A(&h->h7, R * d.n7);
    if (!rc) rc = A(&h->part7, p7);
    if (!rc && t->fc6.r) rc = A(&h->t6, R * t->fc6.r);
    if (!rc && t->gemm_parts) rc = A(&h->pool5p, planes);
    if (!rc && t->gemm_parts) rc = A(&h->gscale, 4);
    if (rc) return rc;
    if (t->gemm_parts) {
        if (hipMemsetAsync(h->pool5p, 0, planes * 2, s) != hipSuccess || hipMemsetAsync(h->gscale, 0, 4 * sizeof(float), s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return fail(o, AZ_ERR_HIP, clear_msg);
    }
    return AZ_OK;
}

static void use_head_set(az_ctx *t, const az_ctx::HeadSet &h)
{
    t->pool5 = h.pool5; t->part = h.part; t->h6 = h.h6; t->h7 = h.h7; t->part7 = h.part7; t->pool5p = h.pool5p; t->gscale = h.gscale;
    t->t6 = h.t6;
}

int az_destroy(az_ctx *c)
{
    if (!c) return AZ_ERR_INVALID;
    az_solver_free_all(c);
    az_det_solver_free_all(c);
    destroy_twin(c);
    destroy_batch(c);
    if (c->comm) { if (c->comm_stream) hipStreamSynchronize(c->comm_stream); azk_rccl_destroy(c->comm); c->comm = nullptr; }
    hipSetDevice(c->device);
    for (hipStream_t s : {(hipStream_t)c->stream, (hipStream_t)c->stream2, (hipStream_t)c->stream3}) if (s) hipStreamSynchronize(s);
    clear_events(c);
    for (auto &g : c->graphs) hipGraphExecDestroy(g.second.exec);
    for (auto *q : c->plans) delete q;
    delete c;                                 // (the members' destructors release everything else: az_res.h)
    return AZ_OK;
}

const char *az_last_error(const az_ctx *c) { return c ? c->err.c_str() : "null context"; }

void *az_stream(az_ctx *c) { return c ? (void *)c->stream : nullptr; }

int az_set_limits(az_ctx *c, int max_regions, int max_candidates)
{
    if (!c || max_regions < 64 || max_candidates < max_regions) return fail(c, AZ_ERR_INVALID, "bad limits");
    if (c->head_loaded || c->geom_ready) return fail(c, AZ_ERR_STATE, "az_set_limits must precede the first use of the context");
    c->maxR = max_regions;
    c->maxCand = max_candidates;
    c->maxCh = 4 * max_regions;
    return AZ_OK;
}

int az_set_gemm_mode(az_ctx *c, int parts)
{
    if (!c || !(parts == 0 || parts == 2 || parts == 3)) return fail(c, AZ_ERR_INVALID, "az_set_gemm_mode: 0, 2 or 3");
    if (c->head_loaded) return fail(c, AZ_ERR_STATE, "az_set_gemm_mode must precede az_load_head");
    if (parts && c->det_loaded && (c->det_fc6.r || c->det_fc7.r))
        return fail(c, AZ_ERR_STATE, "az_set_gemm_mode: a low-rank detection head is loaded (az_load_det_head_lowrank is fp32 only)");
    c->gemm_parts = parts;
    return AZ_OK;
}

}  // extern "C"

// az_load_head / az_load_head_lowrank (`who`) past the checks that are one entry's alone.  r6 == 0: int6 at full rank, W6 its
// [n6, C*49] weight, L6 unused; otherwise W6 is int6's U factor [n6, r6] and L6 its L factor [r6, C*49].  Whatever is refused
// is refused before the loaded head is touched.
static int load_head(az_ctx *c, const char *who, int C, int n6, int n71, int n72, int r6, const float *L6, const float *W6,
                     const float *b6, const float *W71, const float *b71, const float *W72, const float *b72, const float *Was,
                     const float *bas, const float *Wab, const float *bab, const float *Wz, const float *bz)
{
    if (!c) return AZ_ERR_INVALID;
    const std::string me(who);
    if (!W6 || !b6 || !W71 || !b71 || !W72 || !b72 || !Was || !bas || !Wab || !bab || !Wz || !bz || ((r6 != 0) != (L6 != nullptr)))
        return fail(c, AZ_ERR_INVALID, me + ": null weight pointer");
    if (C <= 0 || (C & 3) || n6 <= 0 || (n6 & 3) || n71 <= 0 || (n71 & 3) || n72 <= 0 || (n72 & 3))
        return fail(c, AZ_ERR_INVALID, me + ": C, n6, n71, n72 must be positive multiples of 4");
    if (azk_tail_lds_bytes(n71 + n72) > 64 * 1024)
        return fail(c, AZ_ERR_INVALID, me + ": n71 + n72 too large for the tail kernel's LDS tile");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
    if (c->stream3) HIPCHK(c, hipStreamSynchronize(c->stream3));
    c->s2_live = false; c->i7_live = false; c->part7 = nullptr;
    for (float *&q : c->part7_ring) q = nullptr;          // (freed with the head's other buffers below)
    c->part7_turn = 0;
    c->s3_live = false; c->g_live[0] = c->g_live[1] = false;
    destroy_twin(c);                          // (the second lane reads this head's buffers: rebuilt at the next launch)
    destroy_batch(c);
    c->allocs.release();
    c->spare.ready = false; c->spare.ev_live = false;      // (its buffers were in `allocs`, released above; the slots are gone)
    c->head_loaded = false;
    c->fc6.W = c->fc6.L = c->fc6.U = c->fc6.zero = c->t6 = nullptr;
    // (captured launch sequences hold the old head's launches and buffers)
    for (auto &g : c->graphs) hipGraphExecDestroy(g.second.exec);
    c->graphs.clear();
    {
        int rg = ensure_geom(c);
        if (rg) return rg;
    }
    AzHeadDims &d = c->d;
    d.C = C; d.pooled = 7; d.K6 = C * 49; d.n6 = n6; d.n71 = n71; d.n72 = n72; d.n7 = n71 + n72;
    d.H = d.W = 0;
    c->S7 = azk_fc_split(d.n6);
    if (c->fc6.r != r6 && !c->cal.pinned) c->cal = az_ctx::PassCal();      // (measured head-pass costs are measured again on the other int6; a table the caller set stays)
    c->fc6 = FcLayer{n6, d.K6, azk_fc_split(d.K6), r6, r6 ? azk_az_lowrank_split(d.K6, r6) : 0};
    int rc;
    DevList &list = c->allocs;
    if ((rc = fc_layer_alloc(c, list, c->fc6, c->gemm_parts)) != AZ_OK) return rc;
    if (r6) {
        AZ_A(fc6.zero, r6);
        HIPCHK(c, hipMemsetAsync(c->fc6.zero, 0, (size_t)r6 * sizeof(float), c->stream));
    }
    AZ_A(W7, azk_tiled_elems(d.n7, n6)); AZ_A(b7, d.n7);
    AZ_A(Wt, 64 * azk_tail_weight_rows(d.n7)); AZ_A(bt, 64);
    const size_t in6 = (size_t)c->fc6.lead() * d.K6;      // the [., C*49] matrix that is permuted and tiled
    {   // (`part` also stages it for the column permutation, and az_roi_pool's rows in Caffe's order: more than the slabs when S6 n6 < K6)
        az_ctx::HeadSet hs;
        if ((rc = alloc_head_set(c, c, std::max(in6, (size_t)c->maxR * d.K6), c->stream, "az_load_head: clearing the operand planes", &hs)) != AZ_OK) return rc;
        use_head_set(c, hs);
    }
    // (`tmp`, the loader's row-major temporary, serves both layers: the larger of the two blocks)
    Buf tg;
    HIPCHK(c, tg.reserve(std::max(in6, (size_t)d.n7 * n6) * 4));
    float *tmp = tg.as<float>();
    if ((rc = fc_layer_load(c, c->fc6, L6, W6, b6, C, c->part, tmp)) != AZ_OK) return rc;
    // int7_1 and int7_2 both read int6: one GEMM with the two weight blocks stacked along N.
    HIPCHK(c, hipMemcpy(tmp, W71, (size_t)n71 * n6 * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(tmp + (size_t)n71 * n6, W72, (size_t)n72 * n6 * 4, hipMemcpyHostToDevice));
    azk_tile_weights(c->stream, tmp, c->W7, d.n7, n6);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->b7, b71, (size_t)n71 * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->b7 + n71, b72, (size_t)n72 * 4, hipMemcpyHostToDevice));
    // tail weights, k-major [n7][64]: outputs 0..10 adj_score, 11..54 adj_bbox (k < n71), output 55
    // zoom_score (k >= n71); everything else zero
    {
        std::vector<float> wt(64 * azk_tail_weight_rows(d.n7), 0.f);
        for (int o = 0; o < 11; ++o)
            for (int k = 0; k < n71; ++k) wt[(size_t)k * 64 + o] = Was[(size_t)o * n71 + k];
        for (int o = 0; o < 44; ++o)
            for (int k = 0; k < n71; ++k) wt[(size_t)k * 64 + 11 + o] = Wab[(size_t)o * n71 + k];
        for (int k = 0; k < n72; ++k) wt[(size_t)(n71 + k) * 64 + 55] = Wz[k];
        HIPCHK(c, hipMemcpy(c->Wt, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipMemset(c->bt, 0, 64 * 4));
    HIPCHK(c, hipMemcpy(c->bt, bas, 11 * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->bt + 11, bab, 44 * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->bt + 55, bz, 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipDeviceSynchronize());
    // the many-row GEMM's LDS opt-in is per device; without it every launch stays on k_fc_splitk
    if (azk_fc_gemm12_prepare() != 0) { (void)hipGetLastError(); c->gemm12_min_rows = 0x7fffffff; }
    if (c->gemm_parts && azk_fc_terms_prepare(c->gemm_parts) != 0) {
        (void)hipGetLastError();
        return fail(c, AZ_ERR_HIP, "az_load_head: the 16-bit-term GEMM's LDS opt-in failed on this device (az_set_gemm_mode)");
    }
    c->head_loaded = true;
    return AZ_OK;
}

extern "C" {

int az_load_head(az_ctx *c, int C, int n6, int n71, int n72, const float *W6, const float *b6,
                 const float *W71, const float *b71, const float *W72, const float *b72, const float *Was,
                 const float *bas, const float *Wab, const float *bab, const float *Wz, const float *bz)
{
    return load_head(c, "az_load_head", C, n6, n71, n72, 0, nullptr, W6, b6, W71, b71, W72, b72, Was, bas, Wab, bab, Wz, bz);
}

// Truncated-SVD int6 (Fast R-CNN section 4.4): L6 [r6, C*49] (no bias) then U6 [n6, r6] (+ b6, ReLU); the rest as az_load_head.
int az_load_head_lowrank(az_ctx *c, int C, int n6, int n71, int n72, int r6, const float *L6, const float *U6, const float *b6,
                         const float *W71, const float *b71, const float *W72, const float *b72, const float *Was,
                         const float *bas, const float *Wab, const float *bab, const float *Wz, const float *bz)
{
    if (!c) return AZ_ERR_INVALID;
    if (!L6) return fail(c, AZ_ERR_INVALID, "az_load_head_lowrank: null weight pointer");
    if (r6 < 4 || (r6 & 3) || r6 > AZ_LOWRANK_MAX || r6 > n6 || (C > 0 && r6 > (long long)C * 49))
        return fail(c, AZ_ERR_INVALID, "az_load_head_lowrank: r6 is a multiple of 4 in [4, min(n6, C * 49, AZ_LOWRANK_MAX)]");
    if (c->gemm_parts)
        return fail(c, AZ_ERR_STATE, "az_load_head_lowrank: fp32 only (the 16-bit-term GEMM modes of az_set_gemm_mode do not run a low-rank int6)");
    return load_head(c, "az_load_head_lowrank", C, n6, n71, n72, r6, L6, U6, b6, W71, b71, W72, b72, Was, bas, Wab, bab, Wz, bz);
}

int az_az_lowrank_split(int K, int r) { return (K > 0 && r > 0) ? azk_az_lowrank_split(K, r) : AZ_ERR_INVALID; }

}  // extern "C"

// The context's two channel-last copies (and the NCHW staging buffer) hold at least n elements.
static int ensure_feat_copies(az_ctx *c, size_t n)
{
    if (n <= c->feat_owned_elems) return AZ_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->twin) HIPCHK(c, hipStreamSynchronize(c->twin->stream));      // (a lane may be copying out of the old buffers)
    for (float *&f : c->feat_owned) f = nullptr;
    c->feat_stage = nullptr; c->feat_owned_elems = 0;
    ++c->feat_gen;
    Buf *b = c->feat_own;
    HIPCHK(c, reserve_group({{&b[0], n * 4}, {&b[1], n * 4}, {&b[2], n * 4}, {&b[3], n * 4}}));
    for (int i = 0; i < az_ctx::NFEAT; ++i) c->feat_owned[i] = b[i].as<float>();
    c->feat_stage = b[az_ctx::NFEAT].as<float>(); c->feat_owned_elems = n;
    return AZ_OK;
}

int set_feature_map_common(az_ctx *c, const float *src, bool src_is_host, int C, int H, int W, bool wait)
{
    int rc = check_ready(c, false, false);
    if (rc) return rc;
    if (!src || C != c->d.C || H <= 0 || W <= 0)
        return fail(c, AZ_ERR_INVALID, "feature map: channel count must match the loaded head");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)C * H * W;
    if ((rc = ensure_feat_copies(c, n)) != AZ_OK) return rc;
    // a second lane may still have to take its private copy of the map this context held two hand-overs ago (the copy
    // waits behind that lane's earlier search): the buffer is not written before it has
    if (c->twin && c->twin->ev_copy_live) HIPCHK(c, hipStreamWaitEvent(c->stream, c->twin->ev_copy, 0));
    const float *nchw = src;
    if (src_is_host) {
        HIPCHK(c, hipMemcpyAsync(c->feat_stage, src, n * 4, hipMemcpyHostToDevice, c->stream));
        nchw = c->feat_stage;
    }
    // RoIPool reads the map channel-last: one transpose per image, outside the level loop.
    c->feat_turn = (c->feat_turn + 1) % az_ctx::NFEAT;
    azk_nchw_to_nhwc(c->stream, nchw, c->feat_owned[c->feat_turn], C, H * W);
    if (wait) HIPCHK(c, hipStreamSynchronize(c->stream));      // the caller may now reuse / free `src`
    c->feat = c->feat_owned[c->feat_turn];
    c->d.H = H; c->d.W = W;
    return AZ_OK;
}

// The head buffers of a lane: pool5, split-K slabs, h6, h7 (a second lane has them from the start; a batch slot gets them
// when one of its searches has to be run again on its own).
int ensure_lane_head(az_ctx *t)
{
    if (!t || t->head_bufs) return AZ_OK;
    int rc;
    HIPCHK(t, hipSetDevice(t->device));
    if (t->batch_set && t->owner) {
        // a batch slot: the owner's spare set (az_ctx.h: SpareHead), created at its first use
        az_ctx *o = t->owner;
        auto &sp = o->spare;
        if (!sp.ready) {
            if ((rc = alloc_head_set(o, t, 0, o->stream, "batch slot: clearing the spare operand planes", &sp)) != AZ_OK) { t->err = o->err; return rc; }
            if (sp.ev.create(hipEventDisableTiming) != hipSuccess) return fail(t, AZ_ERR_HIP, "batch slot: the spare head set's event");
            sp.ready = true; sp.ev_live = false;
        }
        use_head_set(t, sp);
        t->head_shared = true;
        t->head_bufs = true;
        return AZ_OK;
    }
    az_ctx::HeadSet hs;
    if ((rc = alloc_head_set(t, t, 0, t->stream, "lane: clearing the operand planes", &hs)) != AZ_OK) return rc;
    use_head_set(t, hs);
    t->head_bufs = true;
    return AZ_OK;
}

extern "C" {

int az_set_feature_map_dev(az_ctx *c, const float *dev_ptr, int C, int H, int W)
{
    return set_feature_map_common(c, dev_ptr, false, C, H, W);
}

int az_set_feature_map_host(az_ctx *c, const float *host_ptr, int C, int H, int W)
{
    return set_feature_map_common(c, host_ptr, true, C, H, W);
}

int az_set_feature_map_dev_async(az_ctx *c, const float *dev_ptr, int C, int H, int W)
{
    return set_feature_map_common(c, dev_ptr, false, C, H, W, false);
}

int az_set_feature_map_dev_nhwc(az_ctx *c, const float *dev_ptr, int C, int H, int W)
{
    int rc = check_ready(c, false, false);
    if (rc) return rc;
    if (!dev_ptr || C != c->d.C || H <= 0 || W <= 0)
        return fail(c, AZ_ERR_INVALID, "feature map: channel count must match the loaded head");
    c->feat = dev_ptr;                 // already in the layout RoIPool reads: borrowed, no copy
    c->d.H = H; c->d.W = W;
    return AZ_OK;
}

// ---- lanes ----------------------------------------------------------------------------------------------------------
static void destroy_twin(az_ctx *c)
{
    if (!c || !c->twin) return;
    az_ctx *t = c->twin;
    c->twin = nullptr;
    // (the twin's allocation lists hold only its own buffers: the head's weights belong to the owner)
    az_destroy(t);
    c->lane_order.clear();
    c->lane_next = 0;
}

// The image slots and pass buffers of the batches this lane has run (az_batch_launch).
static void destroy_batch(az_ctx *c)
{
    if (!c) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto &B : c->bsets) {
        for (az_ctx *t : B.slots) {
            if (t->stream) hipStreamSynchronize(t->stream);
            az_destroy(t);
        }
        B.slots.clear();
        B = az_ctx::Batch();                  // (its owners release the pass buffers and the arenas)
    }
    c->bset_turn = 0;
    c->batch_order.clear();
    c->batch_next = 0;
}

// A lane of context c: an az_ctx with its own stream, staging and per-search buffers that READS c's weights.
static int make_lane(az_ctx *c, az_ctx **out, bool with_head, const char *what)
{
    *out = nullptr;
    if (!c->head_loaded) return fail(c, AZ_ERR_STATE, std::string(what) + " needs a loaded head");
    az_ctx *t = nullptr;
    int rc = az_create(c->device, &t);
    if (rc) return fail(c, rc, std::string(what) + ": could not create the lane");
    t->owner = c;
    t->maxR = c->maxR; t->maxCand = c->maxCand; t->maxCh = c->maxCh;
    auto bail = [&](int code, const char *msg) { c->err = t->err.empty() ? std::string(what) + ": " + msg : t->err; az_destroy(t); return code; };
    if ((rc = ensure_geom(t)) != AZ_OK) return bail(rc, "geometry buffers");
    t->d = c->d; t->d.H = t->d.W = 0;
    // (the weights: int6 as its record, whatever it holds; int7 and the tail)
    t->fc6 = c->fc6; t->S7 = c->S7; t->W7 = c->W7; t->b7 = c->b7; t->Wt = c->Wt; t->bt = c->bt;
    t->gemm_parts = c->gemm_parts; t->spatial_scale = c->spatial_scale;
    t->head_bufs = false;
    if (with_head && (rc = ensure_lane_head(t)) != AZ_OK) return bail(rc, "head buffers");
    t->env = c->env; t->plan_cache_max = c->plan_cache_max; t->gemm12_min_rows = c->gemm12_min_rows; t->gemm12_dual_rows = c->gemm12_dual_rows;
    t->head_loaded = true;
    t->profiling = c->profiling; t->use_graphs = c->use_graphs; t->cal = c->cal;
    *out = t;
    return AZ_OK;
}

// The second lane.
static int ensure_twin(az_ctx *c)
{
    if (c->twin) return AZ_OK;
    az_ctx *t = nullptr;
    const int rc = make_lane(c, &t, true, "az_set_lanes");
    if (rc) return rc;
    c->twin = t;
    return AZ_OK;
}

int az_set_lanes(az_ctx *c, int lanes)
{
    if (!c || c->owner || (lanes != 1 && lanes != 2)) return fail(c, AZ_ERR_INVALID, "az_set_lanes: 1 or 2");
    if (!c->lane_order.empty() || !c->pend.empty() || !c->batch_order.empty()) return fail(c, AZ_ERR_STATE, "az_set_lanes: searches are still queued");
    c->batch_next = 0;
    c->lanes = lanes;
    c->lane_next = 0;
    return AZ_OK;
}

// The context (lane) the next search launched through the public entry points runs on.
static az_ctx *next_lane(az_ctx *c, const az_params *p, int *lane_out, int *rc_out)
{
    *lane_out = 0; *rc_out = AZ_OK;
    // (only searches that can be queued take turns: fixed proposal count, not the tuner's variant)
    if (!c || c->owner || c->lanes != 2 || !c->head_loaded || (p && (!p->fixed_num || (p->reserved & 4)))) return c;
    if (c->lane_next == 0) return c;
    if ((*rc_out = ensure_twin(c)) != AZ_OK) return nullptr;
    *lane_out = 1;
    return c->twin;
}

void *az_last_stream(az_ctx *c)
{
    if (!c) return nullptr;
    az_ctx *t = (!c->owner && !c->lane_order.empty() && c->lane_order.back() == 1 && c->twin) ? c->twin : c;
    return (void *)(t->last_s ? t->last_s : t->stream);       // (a two-stage search ends on the lane's second stream)
}

void *az_next_stream(az_ctx *c)
{
    if (!c) return nullptr;
    int lane, rc;
    az_ctx *t = next_lane(c, nullptr, &lane, &rc);
    return (void *)(t ? t->stream : c->stream);
}

static int launch_routed(az_ctx *c, const az_params *p, const float *dev_map, int C, int H, int W, int channels_last)
{
    if (!c) return AZ_ERR_INVALID;
    int lane, rc;
    az_ctx *t = next_lane(c, p, &lane, &rc);
    if (!t) return rc;
    if (dev_map) {
        // the map is handed to the lane that runs the search: an NCHW map is transposed on THAT lane's stream into that
        // lane's copies, a channel-last one is borrowed
        rc = channels_last ? az_set_feature_map_dev_nhwc(t, dev_map, C, H, W) : set_feature_map_common(t, dev_map, false, C, H, W, false);
        if (rc) { if (t != c) c->err = t->err; return rc; }
    } else if (t != c) {
        // the map was set on the context itself: the lane takes it behind whatever the context's stream still has to do to it
        // (an un-awaited transpose).  A map the caller holds in the channel-last layout is read where it lies (the caller
        // keeps it untouched until the fetch); one of the CONTEXT's own channel-last copies is copied into the lane's own
        // buffers -- the context writes its two copies in turn, and this lane's search may be fetched (or even start) only
        // after the context has been handed the map after next.
        if (!c->feat) return fail(c, AZ_ERR_STATE, "no feature map set");
        t->d.H = c->d.H; t->d.W = c->d.W;
        HIPCHK(c, t->ev_hand.create(hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(t->ev_hand, c->stream));
        HIPCHK(c, hipStreamWaitEvent(t->stream, t->ev_hand, 0));
        if (c->feat == c->feat_owned[0] || c->feat == c->feat_owned[1] || c->feat == c->feat_owned[2]) {
            const size_t n = (size_t)c->d.C * c->d.H * c->d.W;
            if ((rc = ensure_feat_copies(t, n)) != AZ_OK) { c->err = t->err; return rc; }
            t->feat_turn = (t->feat_turn + 1) % az_ctx::NFEAT;
            HIPCHK(c, hipMemcpyAsync(t->feat_owned[t->feat_turn], c->feat, n * 4, hipMemcpyDeviceToDevice, t->stream));
            HIPCHK(c, t->ev_copy.create(hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(t->ev_copy, t->stream));
            t->ev_copy_live = true;
            t->feat = t->feat_owned[t->feat_turn];
        } else
            t->feat = c->feat;
    }
    if (t != c) {
        if (t->cal.state == 0 && c->cal.state != 0) t->cal = c->cal;
        t->profiling = c->profiling; t->use_graphs = c->use_graphs;
    }
    rc = launch_impl(t, p);
    if (rc) { if (t != c) c->err = t->err; return rc; }
    if (t == c && c->cal.state == 1 && c->twin && c->twin->cal.state == 0) c->twin->cal = c->cal;
    c->lane_order.push_back(lane);
    if (c->lanes == 2 && p->fixed_num && !(p->reserved & 4)) c->lane_next ^= 1;
    return AZ_OK;
}

int az_propose_launch(az_ctx *c, const az_params *p)
{
    if (c && c->owner) return launch_impl(c, p);
    return launch_routed(c, p, nullptr, 0, 0, 0, 0);
}

int az_propose_launch_on(az_ctx *c, const az_params *p, const float *dev_map, int C, int H, int W, int channels_last)
{
    if (!dev_map) return fail(c, AZ_ERR_INVALID, "az_propose_launch_on: null map");
    return launch_routed(c, p, dev_map, C, H, W, channels_last);
}

int az_propose_fetch(az_ctx *c, double *boxes_out, float *scores_out, int cap, int *n_out, az_stats *st)
{
    if (!c || c->lane_order.empty()) return fail(c, AZ_ERR_STATE, "az_propose_fetch without az_propose_launch");
    if (!boxes_out || !n_out || cap < 0) return fail(c, AZ_ERR_INVALID, "az_propose_fetch: bad arguments");
    const int lane = c->lane_order.front();
    c->lane_order.pop_front();
    az_ctx *t = lane ? c->twin : c;
    if (!t || t->pend.empty()) return fail(c, AZ_ERR_STATE, "az_propose_fetch: the lane's queue is empty");
    c->last_fetch_lane = lane;
    const int rc = fetch_entry(t, 0, boxes_out, scores_out, cap, n_out, st);
    if (rc && t != c) c->err = t->err;
    return rc;
}

// ---- a batch of images in lockstep (az_batch.hip: batch_launch_impl) --------------------------------------------------
static az_ctx *batch_lane(az_ctx *c, int *lane_out, int *rc_out)
{
    *lane_out = 0; *rc_out = AZ_OK;
    if (c->lanes != 2 || c->batch_next == 0) return c;
    if ((*rc_out = ensure_twin(c)) != AZ_OK) return nullptr;
    *lane_out = 1;
    return c->twin;
}

void *az_batch_next_stream(az_ctx *c)
{
    if (!c || c->owner) return c ? (void *)c->stream : nullptr;
    int lane, rc;
    az_ctx *L = batch_lane(c, &lane, &rc);
    return (void *)(L ? L->stream : c->stream);
}

int az_batch_launch(az_ctx *c, int n, const az_params *p, const float *const *maps, int C, int H, int W)
{
    if (!p || n < 1 || n > AZ_BATCH_MAX) return fail(c, AZ_ERR_INVALID, "az_batch_launch: 1 .. AZ_BATCH_MAX maps of the loaded head's channel count");
    az_params pa[AZ_BATCH_MAX];
    int Hs[AZ_BATCH_MAX], Ws[AZ_BATCH_MAX];
    for (int b = 0; b < n; ++b) { pa[b] = *p; Hs[b] = H; Ws[b] = W; }
    return az_batch_launch_shapes(c, n, pa, maps, C, Hs, Ws);
}

int az_batch_launch_shapes(az_ctx *c, int n, const az_params *pa, const float *const *maps, int C, const int *Hs, const int *Ws)
{
    if (!c || c->owner) return fail(c, AZ_ERR_INVALID, "az_batch_launch: the context itself, not a lane");
    if (!c->head_loaded) return fail(c, AZ_ERR_STATE, "az_load_head has not been called");
    if (!pa || !maps || !Hs || !Ws || n < 1 || n > AZ_BATCH_MAX || C != c->d.C)
        return fail(c, AZ_ERR_INVALID, "az_batch_launch: 1 .. AZ_BATCH_MAX maps of the loaded head's channel count");
    for (int b = 0; b < n; ++b)
        if (Hs[b] <= 0 || Ws[b] <= 0) return fail(c, AZ_ERR_INVALID, "az_batch_launch: 1 .. AZ_BATCH_MAX maps of the loaded head's channel count");
    int lane, rc;
    az_ctx *L = batch_lane(c, &lane, &rc);
    if (!L) return rc;
    // (the batch's pre-pass and passes write the lane's counters and per-roi outputs: a search of the lane whose result block
    //  is not on its way yet -- variable proposal count, the tuner's variant -- would lose them; launch_impl's rule for queueing)
    if (!L->pend.empty() && !L->pend.back().copied)
        return fail(c, AZ_ERR_STATE, "az_batch_launch: a search without a fixed proposal count is still unfetched on this lane");
    const int set = L->bset_turn;
    auto &B = L->bsets[set];
    if (B.n_live) return fail(c, AZ_ERR_STATE, "az_batch_launch: two batches per lane are already in flight, fetch one first");
    HIPCHK(c, hipSetDevice(c->device));
    while ((int)B.slots.size() < n) {
        az_ctx *t = nullptr;
        if ((rc = make_lane(c, &t, false, "az_batch_launch")) != AZ_OK) return rc;
        t->batch_set = &B;
        B.slots.push_back(t);
    }
    for (int b = 0; b < n; ++b) {
        az_ctx *t = B.slots[b];
        if (t->cal.state == 0 && c->cal.state != 0) t->cal = c->cal;
        t->profiling = 0; t->use_graphs = 0;
    }
    if (L != c) { if (L->cal.state == 0 && c->cal.state != 0) L->cal = c->cal; }
    int not_taken = 0;
    rc = batch_launch_impl(L, B, n, B.slots.data(), pa, maps, Hs, Ws, &not_taken);
    if (rc && !not_taken) {
        // (a HIP call failed somewhere in the launch sequence: whatever was enqueued is waited for and dropped, so that the
        //  slots do not sit on half a batch)
        const std::string msg = L->err;
        (void)hipStreamSynchronize(L->stream);
        (void)hipGetLastError();
        for (int b = 0; b < n; ++b) { B.slots[b]->pend.clear(); for (bool &sb : B.slots[b]->slot_busy) sb = false; }
        c->err = msg;
        return rc;
    }
    B.lockstep = !not_taken;
    if (not_taken) {
        // this shape / these settings: one search per image, each on its slot's own stream, behind whatever the caller made
        // the batch's stream wait for
        HIPCHK(c, L->ev_hand.create(hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(L->ev_hand, L->stream));
        for (int b = 0; b < n; ++b) {
            az_ctx *t = B.slots[b];
            if (!maps[b]) return fail(c, AZ_ERR_INVALID, "az_batch_launch: null map");
            HIPCHK(c, hipStreamWaitEvent(t->stream, L->ev_hand, 0));
            t->feat = maps[b]; t->d.H = Hs[b]; t->d.W = Ws[b];
            if ((rc = launch_impl(t, &pa[b])) != AZ_OK) {
                c->err = t->err;
                // (the images launched so far are dropped: nothing of this batch can be fetched)
                for (int q = 0; q < b; ++q) {
                    az_ctx *u = B.slots[q];
                    (void)hipStreamSynchronize(u->stream);
                    u->pend.clear();
                    for (bool &sb : u->slot_busy) sb = false;
                }
                return rc;
            }
        }
    }
    B.n_live = n; B.next_fetch = 0;
    for (int &r : B.rows_acc) r = 0;
    c->batch_order.push_back(lane | (set << 1));
    L->bset_turn ^= 1;
    if (c->lanes == 2) c->batch_next ^= 1;
    return AZ_OK;
}

int az_batch_fetch(az_ctx *c, int i, double *boxes_out, float *scores_out, int cap, int *n_out, az_stats *st)
{
    if (!c || c->owner || c->batch_order.empty()) return fail(c, AZ_ERR_STATE, "az_batch_fetch without az_batch_launch");
    if (!boxes_out || !n_out || cap < 0) return fail(c, AZ_ERR_INVALID, "az_batch_fetch: bad arguments");
    const int lane = c->batch_order.front() & 1, set = c->batch_order.front() >> 1;
    az_ctx *L = lane ? c->twin : c;
    if (!L) return fail(c, AZ_ERR_STATE, "az_batch_fetch: the lane is gone");
    auto &B = L->bsets[set];
    if (i != B.next_fetch || i >= B.n_live) return fail(c, AZ_ERR_INVALID, "az_batch_fetch: the images of a batch are fetched in order, each once");
    az_ctx *t = B.slots[i];
    int rc = t->pend.empty() ? fail(t, AZ_ERR_STATE, "az_batch_fetch: the image's search is not queued") :
                               fetch_entry(t, 0, boxes_out, scores_out, cap, n_out, st);
    if (rc) c->err = t->err;
    if (++B.next_fetch == B.n_live) {
        if (B.lockstep)       // (what the lane's next batches go by: both sets)
            for (auto &S : L->bsets) { for (int l = 0; l < AZ_MAX_LEVELS; ++l) S.rows_hint[l] = B.rows_acc[l]; S.hint_n = B.n_live; }
        B.n_live = 0; B.next_fetch = 0;
        c->batch_order.pop_front();
    }
    return rc;
}

// Every image of the oldest unfetched batch in one call: image i's boxes at boxes_out + i * cap * 4, its scores at
// scores_out + i * cap (may be NULL), its count in n_out[i], its statistics in st[i] (may be NULL).  Returns the first error
// (the remaining images are still collected, their n_out = -1 on error).
int az_batch_fetch_all(az_ctx *c, double *boxes_out, float *scores_out, int cap, int *n_out, az_stats *st)
{
    if (!c || c->owner || c->batch_order.empty()) return fail(c, AZ_ERR_STATE, "az_batch_fetch_all without az_batch_launch");
    if (!boxes_out || !n_out || cap < 0) return fail(c, AZ_ERR_INVALID, "az_batch_fetch_all: bad arguments");
    const int lane = c->batch_order.front() & 1, set = c->batch_order.front() >> 1;
    az_ctx *L = lane ? c->twin : c;
    if (!L) return fail(c, AZ_ERR_STATE, "az_batch_fetch_all: the lane is gone");
    const int n = L->bsets[set].n_live, i0 = L->bsets[set].next_fetch;
    int first = AZ_OK;
    std::string msg;
    for (int i = 0; i < i0; ++i) n_out[i] = 0;          // (already fetched one by one)
    for (int i = i0; i < n; ++i) {
        const int rc = az_batch_fetch(c, i, boxes_out + (size_t)i * cap * 4, scores_out ? scores_out + (size_t)i * cap : nullptr, cap,
                                      &n_out[i], st ? &st[i] : nullptr);
        if (rc) { n_out[i] = -1; if (!first) { first = rc; msg = c->err; } }
    }
    if (first) c->err = msg;
    return first;
}

int az_propose(az_ctx *c, const az_params *p, double *boxes_out, float *scores_out, int cap, int *n_out,
               az_stats *st)
{
    // (launch + fetch of the SAME search, on the context's own lane: with another search still queued the fetch would
    //  return that one's result)
    if (c && (!c->lane_order.empty() || !c->pend.empty()))
        return fail(c, AZ_ERR_STATE, "az_propose: a search launched with az_propose_launch is still queued, fetch it first");
    if (!boxes_out || !n_out || cap < 0) return fail(c, AZ_ERR_INVALID, "az_propose: bad arguments");
    int rc = launch_impl(c, p);
    if (rc) return rc;
    if (c) c->last_fetch_lane = 0;
    return fetch_entry(c, 0, boxes_out, scores_out, cap, n_out, st);
}

int az_measure_box(az_ctx *c, double *mfma_f32_tflops, double *copy_tb_per_s)
{
    if (!c) return AZ_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int rc = azk_measure_box(c->stream, mfma_f32_tflops, copy_tb_per_s, (size_t)1 << 30);
    if (rc) { (void)hipGetLastError(); return fail(c, AZ_ERR_HIP, std::string("az_measure_box: ") + hipGetErrorString((hipError_t)rc)); }
    return AZ_OK;
}

int az_set_pass_costs(az_ctx *c, int n, const int32_t *rows, const double *us)
{
    if (!c || n < 0 || n == 1 || n > 6 || (n && (!rows || !us))) return fail(c, AZ_ERR_INVALID, "az_set_pass_costs: 0 or 2..6 points");
    for (int i = 0; i < n; ++i)
        if (rows[i] <= 0 || !(us[i] > 0) || (i && (rows[i] <= rows[i - 1] || us[i] < us[i - 1])))
            return fail(c, AZ_ERR_INVALID, "az_set_pass_costs: rows and costs must ascend");
    c->cal = az_ctx::PassCal();
    for (int i = 0; i < n; ++i) { c->cal.rows[i] = rows[i]; c->cal.us[i] = us[i]; }
    c->cal.n = n;
    c->cal.state = n ? 1 : 0;
    c->cal.pinned = n > 0;                    // (the caller's table: a head reload does not measure over it)
    if (c->twin) c->twin->cal = c->cal;
    return AZ_OK;
}

int az_get_pass_costs(az_ctx *c, int32_t *rows_out, double *us_out, int cap, int *n_out)
{
    if (!c || !n_out || cap < 0) return fail(c, AZ_ERR_INVALID, "az_get_pass_costs: bad arguments");
    const int n = c->cal.state == 1 ? c->cal.n : 0;
    *n_out = n;
    if (n > cap) return fail(c, AZ_ERR_CAPACITY, "az_get_pass_costs: cap too small");
    for (int i = 0; i < n; ++i) { if (rows_out) rows_out[i] = c->cal.rows[i]; if (us_out) us_out[i] = c->cal.us[i]; }
    return AZ_OK;
}

// ---- the exchange step of an image-sharded run, natively (az_rccl.hip) ------------------------------------------------
int az_rccl_unique_id(void *id_out, size_t cap)
{
    if (!id_out || cap < 128) return AZ_ERR_INVALID;
    std::string why;
    return azk_rccl_unique_id(id_out, &why) ? AZ_ERR_HIP : AZ_OK;
}

int az_rccl_init(az_ctx *c, const void *id, size_t id_bytes, int nranks, int rank)
{
    if (!c || c->owner || !id || id_bytes < 128 || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(c, AZ_ERR_INVALID, "az_rccl_init: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->comm_stream.create(hipStreamNonBlocking));
    for (auto &e : c->comm_ev) HIPCHK(c, e.create(hipEventDisableTiming));
    if (c->comm) { HIPCHK(c, hipStreamSynchronize(c->comm_stream)); azk_rccl_destroy(c->comm); c->comm = nullptr; }
    std::string why;
    if (azk_rccl_init(id, nranks, rank, &c->comm, &why)) return fail(c, AZ_ERR_HIP, "az_rccl_init: " + why);
    c->comm_ranks = nranks; c->comm_rank = rank;
    return AZ_OK;
}

int az_gather_records(az_ctx *c, const void *send_dev, void *recv_dev, size_t bytes_per_rank)
{
    if (!c || c->owner || !send_dev || !recv_dev || !bytes_per_rank) return fail(c, AZ_ERR_INVALID, "az_gather_records: bad arguments");
    if (!c->comm) return fail(c, AZ_ERR_STATE, "az_gather_records: no communicator (az_rccl_init)");
    HIPCHK(c, hipSetDevice(c->device));
    // the records were staged on the lanes' streams: the collective's stream waits, on the device, for what both have
    // queued so far
    HIPCHK(c, hipEventRecord(c->comm_ev[0], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->comm_ev[0], 0));
    if (c->twin) {
        HIPCHK(c, hipEventRecord(c->comm_ev[1], c->twin->stream));
        HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->comm_ev[1], 0));
    }
    // (two-stage searches stage their records on the lanes' second streams)
    for (az_ctx *l : {c, c->twin})
        if (l && l->s2_live && l->ev_s2) HIPCHK(c, hipStreamWaitEvent(c->comm_stream, l->ev_s2, 0));
    for (az_ctx *l : {c, c->twin})
        if (l && l->s3_live && l->ev_s3) HIPCHK(c, hipStreamWaitEvent(c->comm_stream, l->ev_s3, 0));
    std::string why;
    if (azk_rccl_all_gather(c->comm, c->comm_stream, send_dev, recv_dev, bytes_per_rank, &why))
        return fail(c, AZ_ERR_HIP, "az_gather_records: " + why);
    return AZ_OK;
}

int az_rccl_destroy(az_ctx *c)
{
    if (!c) return AZ_ERR_INVALID;
    if (c->comm) { hipSetDevice(c->device); hipStreamSynchronize(c->comm_stream); azk_rccl_destroy(c->comm); c->comm = nullptr; }
    return AZ_OK;
}

void *az_comm_stream(az_ctx *c) { return c ? (void *)c->comm_stream : nullptr; }

int az_result_record_layout(int k, size_t *bytes, size_t *n_off, size_t *boxes_off, size_t *scores_off)
{
    if (k <= 0 || k > AZ_TOPK_MAX) return AZ_ERR_INVALID;
    if (bytes) *bytes = RES_HDR + (size_t)k * 36;
    if (n_off) *n_off = offsetof(AzCounts, nsel);
    if (boxes_off) *boxes_off = RES_HDR;
    if (scores_off) *scores_off = RES_HDR + (size_t)k * 32;
    return AZ_OK;
}

int az_propose_stage_result_dev(az_ctx *c, void *dst_dev, size_t cap_bytes)
{
    // (applies to the search launched last: call it right behind az_propose_launch)
    if (!c) return AZ_ERR_INVALID;
    az_ctx *t = (!c->owner && !c->lane_order.empty() && c->lane_order.back() == 1) ? c->twin : c;
    if (!t) return fail(c, AZ_ERR_STATE, "az_propose_stage_result_dev without az_propose_launch");
    const int rc = stage_impl(t, dst_dev, cap_bytes);
    if (rc && t != c) c->err = t->err;
    return rc;
}


// The records of the batch launched last, image i to dst_dev + i * pitch: ONE strided device-to-device copy behind the batch
// (its result blocks lie side by side); an image that az_batch_fetch has to search again alone is staged again there.
int az_batch_stage_results_dev(az_ctx *c, void *dst_dev, size_t pitch_bytes, size_t cap_bytes)
{
    if (!c || c->owner || c->batch_order.empty()) return fail(c, AZ_ERR_STATE, "az_batch_stage_results_dev without az_batch_launch");
    az_ctx *L = (c->batch_order.back() & 1) ? c->twin : c;
    if (!L || !L->bsets[c->batch_order.back() >> 1].n_live) return fail(c, AZ_ERR_STATE, "az_batch_stage_results_dev: no batch in flight");
    auto &B = L->bsets[c->batch_order.back() >> 1];
    const int n = B.n_live;
    if (B.next_fetch) return fail(c, AZ_ERR_STATE, "az_batch_stage_results_dev: call it right behind az_batch_launch");
    az_ctx *t0 = B.slots[0];
    if (t0->pend.empty()) return fail(c, AZ_ERR_STATE, "az_batch_stage_results_dev: nothing queued");
    const size_t bytes = RES_HDR + (size_t)t0->pend.back().p.num_proposals * 36;
    if (!dst_dev || pitch_bytes < bytes || cap_bytes < pitch_bytes * (size_t)(n - 1) + bytes)
        return fail(c, AZ_ERR_INVALID, "az_batch_stage_results_dev: destination too small");
    HIPCHK(c, hipSetDevice(c->device));
    if (!B.lockstep) {
        // (the images were launched one by one on their slots: one copy each, on the slot's stream)
        for (int i = 0; i < n; ++i) {
            const int rc = stage_impl(B.slots[i], (unsigned char *)dst_dev + (size_t)i * pitch_bytes, bytes);
            if (rc) { c->err = B.slots[i]->err; return rc; }
        }
        return AZ_OK;
    }
    const size_t src_pitch = (size_t)((unsigned char *)B.slots[n > 1 ? 1 : 0]->cnt - (unsigned char *)B.slots[0]->cnt);
    hipStream_t s = L->stream;
    if (n > 1) HIPCHK(c, hipMemcpy2DAsync(dst_dev, pitch_bytes, B.res_dev, src_pitch, bytes, (size_t)n, hipMemcpyDeviceToDevice, s));
    else HIPCHK(c, hipMemcpyAsync(dst_dev, B.res_dev, bytes, hipMemcpyDeviceToDevice, s));
    for (int i = 0; i < n; ++i) {
        az_ctx *t = B.slots[i];
        auto &q = t->pend.back();
        q.stage_dst = (unsigned char *)dst_dev + (size_t)i * pitch_bytes; q.stage_cap = bytes;
        // ("the record is staged when the fetch returns": the slot's event again, behind the staging copy)
        if (q.copied) HIPCHK(c, hipEventRecord(t->ev_res[q.slot], s));
    }
    return AZ_OK;
}

int az_last_candidates(az_ctx *c, double *boxes_out, float *scores_out, int cap, int *n_out)
{
    if (c && !c->owner && c->last_fetch_lane == 1 && c->twin) {
        // (the search fetched last ran on the second lane: its candidates are in that lane's buffers)
        const int r2 = az_last_candidates(c->twin, boxes_out, scores_out, cap, n_out);
        if (r2) c->err = c->twin->err;
        return r2;
    }
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!n_out) return AZ_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
    if (c->stream3) HIPCHK(c, hipStreamSynchronize(c->stream3));
    if (c->cand_n < 0)
        return fail(c, AZ_ERR_STATE, "az_last_candidates: no fetched search, or a later call reused the candidate buffers");
    const int n = c->cand_n;
    *n_out = n;
    if (n > cap) return fail(c, AZ_ERR_CAPACITY, "az_last_candidates: cap too small");
    if (boxes_out) HIPCHK(c, hipMemcpy(boxes_out, c->Yall, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (scores_out) HIPCHK(c, hipMemcpy(scores_out, c->Sall, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_set_graphs(az_ctx *c, int on)
{
    if (!c) return AZ_ERR_INVALID;
    c->use_graphs = on ? 1 : 0;
    return AZ_OK;
}

int az_set_profiling(az_ctx *c, int on)
{
    if (!c) return AZ_ERR_INVALID;
    const int asked = on;
    if ((on & 8) && (on & 16) && c->span_ring) {
        // bit 4 with bit 3: forget the spans recorded so far WITHOUT touching the GPU -- the ring keeps handing out slots it
        // has not used yet (each is used once), so nothing has to be cleared: no stream synchronisation, no copy, no idle
        // gap in front of the region the caller is about to time
        std::vector<AzEventRec> keep;
        for (auto &e : c->events) if (e.slot < 0) keep.push_back(e);
        c->events.swap(keep);
        on &= ~16;
    } else if (on & 8) {
        on &= ~16;
        // every slot starts as (first-in = ~0, last-out = 0); a slot is used once between two calls of this function
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
        if (c->stream3) HIPCHK(c, hipStreamSynchronize(c->stream3));
        HIPCHK(c, c->span_own.reserve((size_t)az_ctx::SPAN_SLOTS * 16));
        c->span_ring = c->span_own.as<unsigned long long>();
        std::vector<unsigned long long> init((size_t)az_ctx::SPAN_SLOTS * 2);
        for (size_t i = 0; i < init.size(); i += 2) { init[i] = ~0ull; init[i + 1] = 0ull; }
        HIPCHK(c, hipMemcpy(c->span_ring, init.data(), init.size() * 8, hipMemcpyHostToDevice));
        // (spans recorded so far are gone with the slots)
        std::vector<AzEventRec> keep;
        for (auto &e : c->events) if (e.slot < 0) keep.push_back(e);
        c->events.swap(keep);
        c->span_next = 0;
    }
    c->profiling = on;
    if (!on) clear_events(c);
    if (c->twin) az_set_profiling(c->twin, asked);
    return AZ_OK;
}

int az_last_kernel_times(az_ctx *c, char *names_out, float *ms_out, int32_t *level_out, int cap, int *n_out)
{
    if (!c || !n_out) return AZ_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
    if (c->stream3) HIPCHK(c, hipStreamSynchronize(c->stream3));
    const int n = (int)c->events.size();
    *n_out = n;
    if (c->event_errors) {
        const int ne = c->event_errors;
        c->event_errors = 0;
        return fail(c, AZ_ERR_HIP, "az_last_kernel_times: " + std::to_string(ne) + " hipEvent call(s) failed while profiling");
    }
    std::vector<unsigned long long> spans;
    if (c->span_ring && c->span_next > 0) {
        spans.resize((size_t)c->span_next * 2);
        HIPCHK(c, hipMemcpy(spans.data(), c->span_ring, spans.size() * 8, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < n && i < cap; ++i) {
        float ms = 0.f;
        const int sl = c->events[i].slot;
        if (sl >= 0) {
            // 100 MHz ticks; a launch that left at once (another kernel owned it) or has not run reads as 0
            const unsigned long long t0 = (size_t)sl * 2 + 1 < spans.size() ? spans[(size_t)sl * 2] : ~0ull;
            const unsigned long long t1 = (size_t)sl * 2 + 1 < spans.size() ? spans[(size_t)sl * 2 + 1] : 0ull;
            ms = (t0 != ~0ull && t1 > t0) ? (float)((double)(t1 - t0) * 1e-5) : 0.f;
        } else
        if (hipEventElapsedTime(&ms, c->events[i].a, c->events[i].b) != hipSuccess)
            return fail(c, AZ_ERR_HIP, "az_last_kernel_times: hipEventElapsedTime failed");
        if (ms_out) ms_out[i] = ms;
        if (level_out) level_out[i] = c->events[i].level;
        if (names_out) {
            std::memset(names_out + 32 * i, 0, 32);
            std::strncpy(names_out + 32 * i, c->events[i].name.c_str(), 31);
        }
    }
    if (c->twin) {
        // the second lane's launches behind this lane's
        const int n0 = n < cap ? n : cap;
        int n2 = 0;
        const int rc = az_last_kernel_times(c->twin, names_out ? names_out + 32 * (size_t)n0 : nullptr, ms_out ? ms_out + n0 : nullptr,
                                            level_out ? level_out + n0 : nullptr, cap - n0, &n2);
        if (rc) { c->err = c->twin->err; return rc; }
        *n_out = n + n2;
    }
    return AZ_OK;
}

// --------------------------------------------------------------------------------------
// Training data layer (lib/az_data_layer/roidb.py; kernels in az_train.hip).
static_assert(sizeof(az_train_params) == 6 * 8 + 4 * 4 + 2 * AZ_TRAIN_MAX_REGIONS * 4 * 8, "az_train_params layout (ffi.AzTrainParams restates it)");

static int train_params_ok(const az_train_params *p)
{
    return p && p->n_addregions >= 1 && p->n_addregions <= AZ_TRAIN_MAX_REGIONS && p->n_subregion >= 1 &&
           p->n_subregion <= AZ_TRAIN_MAX_REGIONS && p->min_side > 0.0 && p->train_rep >= 0;
}

// a device arena in scratch slot `slot`: add() hands out 256-byte-aligned pieces, take() allocates
struct TrainArena {
    size_t total = 0;
    size_t add(size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; }
};

int az_zoom_labels(az_ctx *c, const double *rois, int R, const double *gt, int N, double max_area_ratio, double min_obj,
                   uint8_t *labels_out)
{
    if (!c || R < 0 || N < 0 || (R && (!rois || !labels_out)) || (N && !gt))
        return fail(c, AZ_ERR_INVALID, "az_zoom_labels: bad arguments");
    if (R == 0) return AZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    TrainArena ar;
    const size_t o_r = ar.add((size_t)R * 32), o_g = ar.add((size_t)N * 32 + 32), o_l = ar.add((size_t)R);
    int rc;
    if ((rc = scratch_grow(c, 0, ar.total)) != AZ_OK) return rc;
    char *base = (char *)c->scratch[0].p;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(base + o_r, rois, (size_t)R * 32, hipMemcpyHostToDevice, s));
    if (N) HIPCHK(c, hipMemcpyAsync(base + o_g, gt, (size_t)N * 32, hipMemcpyHostToDevice, s));
    azk_zoom_labels(s, (const double *)(base + o_r), R, (const double *)(base + o_g), N, max_area_ratio, min_obj,
                    (unsigned char *)(base + o_l));
    HIPCHK(c, hipMemcpyAsync(labels_out, base + o_l, (size_t)R, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return AZ_OK;
}

int az_train_ex_rois(az_ctx *c, const az_train_params *p, int n_images, const int32_t *sizes, const double *gt,
                     const int32_t *gt_off, const double *noise, long long n_noise, float *ex_boxes_out,
                     uint8_t *zoom_out, int32_t *ex_off_out, int cap, long long *noise_used_out, long long *needed_out)
{
    if (!c || !train_params_ok(p) || n_images < 0 || n_noise < 0 || cap < 0 || !ex_off_out || !needed_out ||
        (n_images && (!sizes || !gt_off || !noise_used_out)) || (n_noise && !noise) || (cap && (!ex_boxes_out || !zoom_out)))
        return fail(c, AZ_ERR_INVALID, "az_train_ex_rois: bad arguments");
    needed_out[0] = needed_out[1] = 0;
    ex_off_out[0] = 0;
    if (n_images == 0) return AZ_OK;
    std::vector<int> sizes3((size_t)n_images * 3);
    for (int i = 0; i < n_images; ++i) {
        const int h = sizes[2 * i], w = sizes[2 * i + 1];
        if (h <= 0 || w <= 0 || gt_off[i + 1] < gt_off[i] || gt_off[0] != 0)
            return fail(c, AZ_ERR_INVALID, "az_train_ex_rois: image sizes must be positive and gt_off ascend from 0");
        // K = int(np.log2(side / MIN_SIDE) + 1.0), roidb.py:247-250
        const double k = std::log2((double)(h < w ? h : w) / p->min_side) + 1.0;
        sizes3[3 * i] = h; sizes3[3 * i + 1] = w; sizes3[3 * i + 2] = k > 0.0 ? (int)k : 0;
        if (sizes3[3 * i + 2] > AZ_MAX_LEVELS) return fail(c, AZ_ERR_INVALID, "az_train_ex_rois: too many levels");
    }
    const int NG = gt_off[n_images];
    if (NG && !gt) return fail(c, AZ_ERR_INVALID, "az_train_ex_rois: NULL gt");
    HIPCHK(c, hipSetDevice(c->device));
    TrainArena ar;
    const size_t o_sz = ar.add(sizes3.size() * 4), o_gt = ar.add((size_t)NG * 32 + 32), o_go = ar.add(((size_t)n_images + 1) * 4),
                 o_no = ar.add((size_t)n_noise * 8 + 8), o_ex = ar.add((size_t)cap * 16 + 16), o_zo = ar.add((size_t)cap + 16),
                 o_eo = ar.add(((size_t)n_images + 1) * 4), o_us = ar.add((size_t)n_images * 8),
                 o_B = ar.add((size_t)azk_train_level_cap() * 8 * 8), o_st = ar.add(16);
    int rc;
    if ((rc = scratch_grow(c, 0, ar.total)) != AZ_OK) return rc;
    char *base = (char *)c->scratch[0].p;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(base + o_sz, sizes3.data(), sizes3.size() * 4, hipMemcpyHostToDevice, s));
    if (NG) HIPCHK(c, hipMemcpyAsync(base + o_gt, gt, (size_t)NG * 32, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(base + o_go, gt_off, ((size_t)n_images + 1) * 4, hipMemcpyHostToDevice, s));
    if (n_noise) HIPCHK(c, hipMemcpyAsync(base + o_no, noise, (size_t)n_noise * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(base + o_eo, 0, ((size_t)n_images + 1) * 4, s));
    if (azk_train_ex_rois(s, p, n_images, (const int *)(base + o_sz), (const double *)(base + o_gt), (const int *)(base + o_go),
                          (const double *)(base + o_no), n_noise, (float *)(base + o_ex), (unsigned char *)(base + o_zo),
                          (int *)(base + o_eo), (long long *)(base + o_us), cap, (double *)(base + o_B),
                          (long long *)(base + o_st)))
        return fail(c, AZ_ERR_HIP, "az_train_ex_rois: launch failed");
    long long status[2] = {0, 0};
    std::vector<int32_t> eoff((size_t)n_images + 1);
    HIPCHK(c, hipMemcpyAsync(status, base + o_st, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(eoff.data(), base + o_eo, eoff.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));     // status / eoff live on this frame
    if (status[0] & 1) {
        needed_out[0] = status[1];
        return fail(c, AZ_ERR_CAPACITY, "az_train_ex_rois: the noise ran out; at least " + std::to_string(status[1]) + " doubles are needed");
    }
    if (status[0] & 2)
        return fail(c, AZ_ERR_CAPACITY, "az_train_ex_rois: a level holds more than " + std::to_string(azk_train_level_cap()) +
                                            " children before the dedup");
    if (status[0] & 4)
        return fail(c, AZ_ERR_INVALID, "az_train_ex_rois: a region's coordinate leaves the dedup hash's range (negative, or >= 1000 * min_side)");
    const int E = eoff[n_images];
    if (E > cap) {
        needed_out[1] = E;
        return fail(c, AZ_ERR_CAPACITY, "az_train_ex_rois: cap too small; " + std::to_string(E) + " example regions");
    }
    std::memcpy(ex_off_out, eoff.data(), eoff.size() * 4);
    HIPCHK(c, hipMemcpyAsync(noise_used_out, base + o_us, (size_t)n_images * 8, hipMemcpyDeviceToHost, s));
    if (E) {
        HIPCHK(c, hipMemcpyAsync(ex_boxes_out, base + o_ex, (size_t)E * 16, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(zoom_out, base + o_zo, (size_t)E, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    return AZ_OK;
}

int az_train_adj_targets(az_ctx *c, const az_train_params *p, int n_images, const float *ex_boxes, const int32_t *ex_off,
                         const float *gt, const int32_t *gt_off, double *targets_out, int32_t *tgt_off_out, int cap)
{
    if (!c || !train_params_ok(p) || n_images < 0 || cap < 0 || !tgt_off_out || (n_images && (!ex_off || !gt_off)) ||
        (cap && !targets_out))
        return fail(c, AZ_ERR_INVALID, "az_train_adj_targets: bad arguments");
    tgt_off_out[0] = 0;
    if (n_images == 0) return AZ_OK;
    int max_gt = 0;
    for (int i = 0; i < n_images; ++i) {
        if (ex_off[i + 1] < ex_off[i] || gt_off[i + 1] < gt_off[i] || ex_off[0] != 0 || gt_off[0] != 0)
            return fail(c, AZ_ERR_INVALID, "az_train_adj_targets: offsets must ascend from 0");
        max_gt = std::max(max_gt, gt_off[i + 1] - gt_off[i]);
    }
    const int E = ex_off[n_images], NG = gt_off[n_images];
    if ((E && !ex_boxes) || (NG && !gt)) return fail(c, AZ_ERR_INVALID, "az_train_adj_targets: NULL array");
    if ((size_t)max_gt * p->n_subregion * sizeof(double) > azk_adj_lds_max())
        return fail(c, AZ_ERR_CAPACITY, "az_train_adj_targets: an image has more objects than the match matrix's LDS holds");
    HIPCHK(c, hipSetDevice(c->device));
    TrainArena ar;
    const size_t o_ex = ar.add((size_t)E * 16 + 16), o_eo = ar.add(((size_t)n_images + 1) * 4), o_gt = ar.add((size_t)NG * 16 + 16),
                 o_go = ar.add(((size_t)n_images + 1) * 4), o_cn = ar.add(((size_t)E + 1) * 4), o_to = ar.add(((size_t)n_images + 1) * 4);
    int rc;
    if ((rc = scratch_grow(c, 0, ar.total)) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 1, (size_t)cap * 56 + 56)) != AZ_OK) return rc;
    char *base = (char *)c->scratch[0].p;
    hipStream_t s = c->stream;
    if (E) HIPCHK(c, hipMemcpyAsync(base + o_ex, ex_boxes, (size_t)E * 16, hipMemcpyHostToDevice, s));
    if (NG) HIPCHK(c, hipMemcpyAsync(base + o_gt, gt, (size_t)NG * 16, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(base + o_eo, ex_off, ((size_t)n_images + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(base + o_go, gt_off, ((size_t)n_images + 1) * 4, hipMemcpyHostToDevice, s));
    if (azk_train_adj_count(s, p, n_images, E, (const float *)(base + o_ex), (const int *)(base + o_eo), (const float *)(base + o_gt),
                            (const int *)(base + o_go), (int *)(base + o_cn), (int *)(base + o_to)))
        return fail(c, AZ_ERR_HIP, "az_train_adj_targets: launch failed");
    // (the rows are written behind the counts without a host wait; a `cap` that turns out too small makes the kernel
    //  write nothing for the rows past it, and the call fails below)
    if (azk_train_adj_write(s, p, n_images, E, max_gt, (const float *)(base + o_ex), (const int *)(base + o_eo),
                            (const float *)(base + o_gt), (const int *)(base + o_go), (int *)(base + o_cn), (double *)c->scratch[1].p, cap))
        return fail(c, AZ_ERR_HIP, "az_train_adj_targets: launch failed");
    HIPCHK(c, hipMemcpyAsync(tgt_off_out, base + o_to, ((size_t)n_images + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const int T = tgt_off_out[n_images];
    if (T > cap) return fail(c, AZ_ERR_CAPACITY, "az_train_adj_targets: cap too small; " + std::to_string(T) + " targets");
    if (T) HIPCHK(c, hipMemcpy(targets_out, c->scratch[1].p, (size_t)T * 56, hipMemcpyDeviceToHost));
    return AZ_OK;
}

int az_train_target_stats(az_ctx *c, int n_sub, double eps, double *targets, long long T, double *means_out,
                          double *stds_out, int normalise_in_place)
{
    if (!c || n_sub < 1 || n_sub > AZ_TRAIN_MAX_REGIONS || T < 0 || (T && !targets) || !means_out || !stds_out)
        return fail(c, AZ_ERR_INVALID, "az_train_target_stats: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    TrainArena ar;
    const size_t o_pt = ar.add(azk_stats_part_doubles(T, n_sub) * 8), o_m = ar.add((size_t)n_sub * 32), o_s = ar.add((size_t)n_sub * 32);
    int rc;
    if ((rc = scratch_grow(c, 0, ar.total)) != AZ_OK) return rc;
    if ((rc = scratch_grow(c, 1, (size_t)T * 56 + 56)) != AZ_OK) return rc;
    char *base = (char *)c->scratch[0].p;
    hipStream_t s = c->stream;
    if (T) HIPCHK(c, hipMemcpyAsync(c->scratch[1].p, targets, (size_t)T * 56, hipMemcpyHostToDevice, s));
    if (azk_train_target_stats(s, n_sub, eps, (double *)c->scratch[1].p, T, (double *)(base + o_pt), (double *)(base + o_m),
                               (double *)(base + o_s), normalise_in_place))
        return fail(c, AZ_ERR_HIP, "az_train_target_stats: launch failed");
    HIPCHK(c, hipMemcpyAsync(means_out, base + o_m, (size_t)n_sub * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(stds_out, base + o_s, (size_t)n_sub * 32, hipMemcpyDeviceToHost, s));
    if (T && normalise_in_place) HIPCHK(c, hipMemcpyAsync(targets, c->scratch[1].p, (size_t)T * 56, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return AZ_OK;
}

}  // extern "C"
