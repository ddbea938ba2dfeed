// az_nms.hip -- greedy NMS behind the C ABI (kernels: az_select.hip): az_nms, az_nms_batched, the context's NMS scratch, NMS
// of records that are on the device already.  Small and unprofiled calls get their result through host-mapped memory that
// the host polls: a stream synchronisation costs an interrupt round trip (~10-15 us) on top of a kernel of about that length.
// Words written by the GPU may become visible out of order (posted PCIe writes), so each carries the call's sequence number
// and is taken only once it shows it; the stream's own completion is picked up by whatever uses it next (same stream).
#include "az_ctx.h"

unsigned nms_next_tag(az_ctx *c)
{
    do { ++c->nms_tag; } while (c->nms_tag == 0u || (c->nms_tag & 0x3FFFFFu) == 0u);
    return c->nms_tag;
}

namespace {

// The two packings of a tagged word; each is re-read, `spins` more times at the most, until it shows `tag` and a value in
// [0, max].  A group's count from the small-group kernels, one int: (tag & 0x3FFFFF) << 9 | count (a group: <= 256 boxes).
bool count_tagged(const volatile int *w, unsigned tag, int max, long spins, int *n)
{
    for (long k = 0;; ) {
        const unsigned x = (unsigned)*w;
        if ((x >> 9) == (tag & 0x3FFFFFu) && (*n = (int)(x & 0x1FFu)) <= max) return true;
        if (++k > spins) return false;
    }
}

// Every keep entry, and the general kernels' count, one long long: (long long)tag << 32 | value.
bool value_tagged(const volatile long long *w, unsigned tag, int max, long spins, int *v)
{
    for (long k = 0;; ) {
        const long long x = *w;
        if ((unsigned)((unsigned long long)x >> 32) == tag && (*v = (int)(x & 0xFFFFFFFFll)) >= 0 && *v <= max) return true;
        if (++k > spins) return false;
    }
}

// true when every one of the n keep words shows `tag`
bool nms_keep_tagged(const long long *hk, int n, unsigned tag, long spins)
{
    for (int i = 0; i < n; ++i) {
        const volatile long long *w = hk + i;
        for (long k = 0; (unsigned)((unsigned long long)*w >> 32) != tag;) if (++k > spins) return false;
    }
    return true;
}

// A host-mapped result block of at least `need` bytes (`want` when it grows) in *b; it grows behind everything on the
// stream: a kernel of an earlier call may still write the block it replaces.
int mapped_grow(az_ctx *c, Buf &own, size_t need, size_t want, unsigned char **b)
{
    if (!(own.p && need <= own.cap)) HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, own.reserve(need, want));
    *b = own.as<unsigned char>();
    return AZ_OK;
}

// The wait for a result in host-mapped memory.  ready(spins): the whole result is there under the call's tag, each word
// looked at `spins` more times at the most (a multiple of that for the word that lands last).  Profiling (`poll` off), or no
// answer within about a millisecond: the plain wait, after which everything is visible.
template <typename Ready>
int nms_wait(az_ctx *c, bool poll, Ready ready, const char *none)
{
    if (!(poll && ready(200000))) HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return ready(0) ? AZ_OK : fail(c, AZ_ERR_HIP, none);
}

}  // namespace

extern "C" {

int az_nms(az_ctx *c, const float *dets, int n, double thresh, int64_t *keep, int *n_keep)
{
    if (!c) return AZ_ERR_INVALID;
    if (n < 0 || (n && (!dets || !keep)) || !n_keep) return fail(c, AZ_ERR_INVALID, "az_nms: bad arguments");
    *n_keep = 0;
    if (n == 0) return AZ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    unsigned char *b;
    long long *hk;
    int nk = 0, rc;
    if (n <= azk_nms_small_max()) {
        // the reference's own call-site size (apply_nms, test.py:467-484: <= 100 boxes per class): ONE launch, no copy
        // commands -- the workgroup reads the boxes from and writes the keep list to host-mapped memory
        if ((rc = mapped_grow(c, c->h_nms_own, 8192, 8192, &b)) != AZ_OK) return rc;
        float *hd = (float *)b;                                         // [256][5] f32 = 5120 B
        hk = (long long *)(b + 5120);                                   // [256] i64 = 2048 B, then the count
        int *hn = (int *)(b + 5120 + 2048);
        std::memcpy(hd, dets, (size_t)n * 5 * sizeof(float));
        const unsigned tag = nms_next_tag(c);
        *hn = 0;
        if (!(c->profiling & 4)) clear_events(c);
        { Timed t(c, "nms", n);
          azk_nms_one_small(s, hd, n, thresh, hk, hn, tag); }
        rc = nms_wait(c, !c->profiling, [&](long spins) { return count_tagged(hn, tag, n, spins, &nk) && nms_keep_tagged(hk, nk, tag, spins); },
                      "az_nms: the kernel left no result");
    } else {
        if ((rc = nms_reserve(c, n, "az_nms")) != AZ_OK) return rc;
        int *nk_dev = c->nms_order + c->nms_cap;      // spare int after the order array
        unsigned long long *band = c->nms_mask + (size_t)c->nms_cap * ((c->nms_cap + 63) / 64);
        HIPCHK(c, hipMemcpyAsync(c->nms_dets, dets, (size_t)n * 5 * 4, hipMemcpyHostToDevice, s));
        if (!(c->profiling & 4)) clear_events(c);
        if (c->profiling) {
            { Timed t(c, "nms", n);
              azk_nms(s, c->nms_dets, n, thresh, c->nms_order, c->nms_sdets, c->nms_mask, band, (unsigned long long *)c->nms_rank, c->nms_keep, nk_dev); }
            HIPCHK(c, hipMemcpyAsync(&nk, nk_dev, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            HIPCHK(c, hipGetLastError());
            *n_keep = nk;
            if (nk) HIPCHK(c, hipMemcpy(keep, c->nms_keep, (size_t)nk * 8, hipMemcpyDeviceToHost));
            return AZ_OK;
        }
        // keep list and count straight into host-mapped memory, the count last (k_nms_scan): no copy-back commands, no
        // stream synchronisation -- the host polls the count
        const size_t need = (size_t)n * 8 + 64;
        if ((rc = mapped_grow(c, c->h_nmsg_own, need, need * 2, &b)) != AZ_OK) return rc;
        long long *hn = (long long *)b;                       // the count, then (+ 64 B) the keep list
        hk = hn + 8;
        const unsigned tag = nms_next_tag(c);
        *hn = 0;
        azk_nms(s, c->nms_dets, n, thresh, c->nms_order, c->nms_sdets, c->nms_mask, band, (unsigned long long *)c->nms_rank, hk, (int *)hn, tag);
        rc = nms_wait(c, true, [&](long spins) { return value_tagged(hn, tag, n, spins * 20, &nk) && nms_keep_tagged(hk, nk, tag, spins); },
                      "az_nms: the kernels left no result");
    }
    if (rc != AZ_OK) return rc;
    *n_keep = nk;
    for (int i = 0; i < nk; ++i) keep[i] = hk[i] & 0xFFFFFFFFll;
    return AZ_OK;
}

// apply_nms (lib/detect/test.py:467-484) calls nms once per class per image: n_groups independent
// problems, here in one call.  Groups of up to 256 boxes (all of them, at that call site) share ONE
// launch, a workgroup each; larger groups go through az_nms one by one.
int az_nms_batched(az_ctx *c, const float *dets, const int32_t *offsets, int n_groups, double thresh,
                   int64_t *keep, int32_t *n_keep)
{
    if (!c || n_groups < 0 || (n_groups && (!offsets || !n_keep)))
        return fail(c, AZ_ERR_INVALID, "az_nms_batched: bad arguments");
    if (n_groups == 0) return AZ_OK;
    const int total = offsets[n_groups];
    std::vector<int> small, large;
    for (int g = 0; g < n_groups; ++g) {
        const int n = offsets[g + 1] - offsets[g];
        if (n < 0) return fail(c, AZ_ERR_INVALID, "az_nms_batched: offsets must ascend");
        n_keep[g] = 0;
        if (n == 0) continue;
        (n <= azk_nms_small_max() ? small : large).push_back(g);
    }
    if (total > 0 && (!dets || !keep)) return fail(c, AZ_ERR_INVALID, "az_nms_batched: NULL array");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (!small.empty() && !c->profiling && total <= 16384) {
        // The reference's call site (apply_nms: 20 classes x <= 100 boxes per image): everything -- boxes, offsets, group
        // list, keep lists, counts -- lives in ONE host-mapped block; one launch, no copy commands, and the host polls a
        // flag that the last workgroup to finish raises (a stream synchronisation plus five copies cost 70 of 96 us).
        const size_t o_off = ((size_t)total * 5 * sizeof(float) + 15) & ~(size_t)15;
        const size_t o_sel = o_off + (((size_t)n_groups + 1) * sizeof(int) + 15 & ~(size_t)15);
        const size_t o_keep = o_sel + ((small.size() * sizeof(int) + 15) & ~(size_t)15);
        const size_t o_nk = o_keep + (size_t)total * sizeof(long long);
        const size_t o_flag = o_nk + (((size_t)n_groups * sizeof(int) + 15) & ~(size_t)15);
        const size_t need = o_flag + 64;
        unsigned char *b;
        int rc, nk;
        if ((rc = mapped_grow(c, c->h_nmsb_own, need, need + need / 2, &b)) != AZ_OK) return rc;
        if (!c->nms_done) {
            HIPCHK(c, c->nms_done_own.reserve(16));
            c->nms_done = c->nms_done_own.as<int>();
            HIPCHK(c, hipMemsetAsync(c->nms_done, 0, 16, s));
        }
        std::memcpy(b, dets, (size_t)total * 5 * sizeof(float));
        std::memcpy(b + o_off, offsets, ((size_t)n_groups + 1) * sizeof(int));
        std::memcpy(b + o_sel, small.data(), small.size() * sizeof(int));
        std::memset(b + o_nk, 0, (size_t)n_groups * sizeof(int));
        volatile int *flag = (volatile int *)(b + o_flag);
        const int seq = ++c->nms_seq;
        const unsigned tag = nms_next_tag(c);
        *flag = 0;
        azk_nms_small(s, (const float *)b, (const int *)(b + o_off), (const int *)(b + o_sel), (int)small.size(), thresh,
                      (long long *)(b + o_keep), (int *)(b + o_nk), c->nms_done, (int *)(b + o_flag), seq, tag);
        // the flag says "all workgroups are done"; each count and keep word is still taken by its own tag (see above)
        const long long *hk = (const long long *)(b + o_keep);
        const int *hn = (const int *)(b + o_nk);
        auto ready = [&](long spins) {
            for (long k = 0; spins && *flag != seq;) if (++k > spins * 2) return false;
            for (int g : small)
                if (!count_tagged(hn + g, tag, 0x1FF, spins, &nk) || !nms_keep_tagged(hk + offsets[g], nk, tag, spins)) return false;
            return true;
        };
        if ((rc = nms_wait(c, true, ready, "az_nms_batched: the kernel left no result")) != AZ_OK) return rc;
        for (int g : small) {
            if (!count_tagged(hn + g, tag, offsets[g + 1] - offsets[g], 0, &nk)) return fail(c, AZ_ERR_HIP, "az_nms_batched: bad count");
            n_keep[g] = nk;
            for (int k = 0; k < nk; ++k) keep[offsets[g] + k] = hk[(size_t)offsets[g] + k] & 0xFFFFFFFFll;
        }
    } else
    if (!small.empty()) {
        int rc;
        if ((rc = scratch_grow(c, 0, (size_t)total * 5 * sizeof(float))) != AZ_OK) return rc;
        if ((rc = scratch_grow(c, 1, ((size_t)n_groups + 1) * sizeof(int))) != AZ_OK) return rc;
        if ((rc = scratch_grow(c, 2, small.size() * sizeof(int))) != AZ_OK) return rc;
        if ((rc = scratch_grow(c, 3, (size_t)total * sizeof(long long))) != AZ_OK) return rc;
        if ((rc = scratch_grow(c, 4, (size_t)n_groups * sizeof(int))) != AZ_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(c->scratch[0].p, dets, (size_t)total * 5 * sizeof(float), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->scratch[1].p, offsets, ((size_t)n_groups + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->scratch[2].p, small.data(), small.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(c->scratch[4].p, 0, (size_t)n_groups * sizeof(int), s));
        if (!(c->profiling & 4)) clear_events(c);
        { Timed t(c, "nms_batched", (int)small.size());
          azk_nms_small(s, (const float *)c->scratch[0].p, (const int *)c->scratch[1].p, (const int *)c->scratch[2].p, (int)small.size(), thresh,
                        (long long *)c->scratch[3].p, (int *)c->scratch[4].p); }
        std::vector<long long> hk((size_t)total);
        HIPCHK(c, hipMemcpyAsync(hk.data(), c->scratch[3].p, (size_t)total * sizeof(long long), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(n_keep, c->scratch[4].p, (size_t)n_groups * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));           // `small`, `hk` live on this frame
        HIPCHK(c, hipGetLastError());
        for (int g : small)
            for (int k = 0; k < n_keep[g]; ++k) keep[offsets[g] + k] = hk[(size_t)offsets[g] + k];
    }
    for (int g : large) {
        int nk = 0;
        int rc = az_nms(c, dets + 5 * (size_t)offsets[g], offsets[g + 1] - offsets[g], thresh, keep + offsets[g], &nk);
        if (rc) return rc;
        n_keep[g] = nk;
    }
    return AZ_OK;
}

}  // extern "C"

// az_nms's growth of the context's scratch (dets, sdets, order, mask + band, rank, keep) to at least n boxes
int nms_reserve(az_ctx *c, int n, const char *who)
{
    if (n <= c->nms_cap) return AZ_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    Buf *b = c->nms_own;
    for (int i = 0; i < 6; ++i) b[i].reset();
    c->nms_cap = 0;
    int cap = 1024;
    while (cap < n) cap *= 2;
    const size_t W = (size_t)(cap + 63) / 64;
    if (azk_nms_scan_lds_bytes(cap) > 150000) return fail(c, AZ_ERR_CAPACITY, std::string(who) + ": n too large");
    HIPCHK(c, reserve_group({{&b[0], (size_t)cap * 5 * 4}, {&b[1], (size_t)cap * 5 * 4}, {&b[2], (size_t)cap * 4 + 16},
                             {&b[3], ((size_t)cap * W + azk_nms_band_words(cap)) * 8},      // mask, then band
                             {&b[4], (size_t)cap * 4}, {&b[5], (size_t)cap * 8 + 16}}));
    c->nms_dets = b[0].as<float>(); c->nms_sdets = b[1].as<float>(); c->nms_order = b[2].as<int>();
    c->nms_mask = b[3].as<unsigned long long>(); c->nms_rank = b[4].as<int>(); c->nms_keep = b[5].as<long long>();
    HIPCHK(c, hipMemset(c->nms_rank, 0, (size_t)cap * 4));
    c->nms_cap = cap;
    return AZ_OK;
}

// az_nms_batched's work on device-resident records (az_ctx.h).  gsel_dev receives the list of the groups that share the one
// k_nms_small launch, `small`, which the caller keeps alive until it has waited for the stream; keep_dev[off[g] ..] receives
// group g's keep list (index inside the group, descending score), nkeep_dev[g] its length.
int nms_groups_dev(az_ctx *c, const float *dets_dev, const int32_t *off, const int *goff_dev, int *gsel_dev, std::vector<int> &small,
                   int n_groups, double thresh, long long *keep_dev, int *nkeep_dev, const char *who)
{
    hipStream_t s = c->stream;
    std::vector<int> large;
    small.clear();
    int biggest = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int n = off[g + 1] - off[g];
        if (n <= 0) continue;
        (n <= azk_nms_small_max() ? small : large).push_back(g);
        biggest = std::max(biggest, n);
    }
    if (!large.empty()) { const int rc = nms_reserve(c, biggest, who); if (rc != AZ_OK) return rc; }
    HIPCHK(c, hipMemsetAsync(nkeep_dev, 0, (size_t)n_groups * sizeof(int), s));
    if (!small.empty()) {
        HIPCHK(c, hipMemcpyAsync(gsel_dev, small.data(), small.size() * sizeof(int), hipMemcpyHostToDevice, s));
        Timed t(c, "nms_batched", (int)small.size());
        azk_nms_small(s, dets_dev, goff_dev, gsel_dev, (int)small.size(), thresh, keep_dev, nkeep_dev);
    }
    for (int g : large) {
        const int n = off[g + 1] - off[g];
        Timed t(c, "nms", n);
        azk_nms(s, dets_dev + 5 * (size_t)off[g], n, thresh, c->nms_order, c->nms_sdets, c->nms_mask,
                c->nms_mask + (size_t)c->nms_cap * ((c->nms_cap + 63) / 64), (unsigned long long *)c->nms_rank, keep_dev + off[g],
                nkeep_dev + g);
    }
    return AZ_OK;
}
