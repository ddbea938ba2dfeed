// az_res_main.cpp -- the owners of az-net_amd/csrc/az_res.h on a counting fake of the runtime calls they use (no GPU, no HIP
// headers): every handle released exactly once, moved-from owners release nothing, a failed group reserve leaves the whole
// group empty, a failed "try" leaves the owner usable.  Built with the address and undefined-behaviour sanitizers by
// tests/test_res_host.py; exit status 0 = every check held.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct FakeEvent *hipEvent_t;
typedef struct FakeStream *hipStream_t;
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1 };

// live handles by kind ('d' device, 'h' pinned, 'e' event, 's' stream); a release of anything else is counted as bad
static std::map<void *, char> live;
static int n_made = 0, n_freed = 0, n_bad = 0, fail_in = 0;      // fail_in = k: the k-th creation from now on fails
static unsigned last_host_flags = 0;

static hipError_t make(void **p, size_t bytes, char kind)
{
    if (fail_in > 0 && --fail_in == 0) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    live[*p] = kind;
    ++n_made;
    return hipSuccess;
}
static hipError_t drop(void *p, char kind)
{
    auto it = live.find(p);
    if (it == live.end() || it->second != kind) { ++n_bad; return hipSuccess; }
    live.erase(it);
    free(p);
    ++n_freed;
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t bytes) { return make(p, bytes, 'd'); }
hipError_t hipFree(void *p) { return drop(p, 'd'); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags) { last_host_flags = flags; return make(p, bytes, 'h'); }
hipError_t hipHostFree(void *p) { return drop(p, 'h'); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make((void **)e, 8, 'e'); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop(e, 'e'); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return make((void **)s, 8, 's'); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { return make((void **)s, 8, 's'); }
hipError_t hipStreamDestroy(hipStream_t s) { return drop(s, 's'); }

#define AZ_RES_FAKE_HIP
#include "../../az-net_amd/csrc/az_res.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { ++failures; fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); } } while (0)
// nothing alive, nothing released twice or through the wrong call, as many releases as creations
static void balanced(const char *what)
{
    if (!live.empty() || n_bad || n_made != n_freed) {
        ++failures;
        fprintf(stderr, "%s: %zu live, %d bad releases, %d made, %d freed\n", what, live.size(), n_bad, n_made, n_freed);
    }
}

static void test_list()
{
    float *a = nullptr; double *b = nullptr; int *c = nullptr;
    {
        DevList l;
        CHECK(l.alloc(&a, 10) == hipSuccess && l.alloc(&b, 3) == hipSuccess && a && b);
        const size_t mark = l.mark();
        CHECK(l.alloc(&c, 7) == hipSuccess && l.alloc(&c, 9) == hipSuccess && live.size() == 4);
        l.release(mark);                               // from the mark on: the first two stay
        CHECK(live.size() == 2 && live.count(a) && live.count(b) && l.mark() == mark);
        // a "try" that fails: the view untouched, the list unchanged and usable
        int *t = nullptr;
        fail_in = 1;
        CHECK(l.alloc(&t, 5) == hipErrorOutOfMemory && t == nullptr && l.mark() == mark && live.size() == 2);
        CHECK(l.alloc(&t, 5) == hipSuccess && t && live.size() == 3);
        DevList m(std::move(l));                       // the moved-from list releases nothing
        CHECK(l.mark() == 0 && m.mark() == 3);
        l.release();
        CHECK(live.size() == 3);
        DevList n;
        CHECK(n.alloc(&c, 1) == hipSuccess);
        n = std::move(m);                              // (what n held is released here)
        CHECK(live.size() == 3 && m.mark() == 0);
    }
    balanced("list");
}

static void test_buf()
{
    {
        Buf d, h(Buf::PINNED), m(Buf::MAPPED);
        CHECK(d.reserve(100, 150 + 256) == hipSuccess && d.cap == 406 && live[d.p] == 'd');
        void *p0 = d.p;
        CHECK(d.reserve(406) == hipSuccess && d.p == p0);                  // fits: kept
        CHECK(d.reserve(407) == hipSuccess && d.cap == 407 && live.size() == 1);      // grows: the old block released
        CHECK(h.reserve(64) == hipSuccess && live[h.p] == 'h' && last_host_flags == hipHostMallocDefault);
        CHECK(m.reserve(64, 128) == hipSuccess && m.cap == 128 && last_host_flags == hipHostMallocMapped);
        fail_in = 1;                                    // a failed regrow: empty, capacity 0, nothing dangling
        CHECK(d.reserve(1000) == hipErrorOutOfMemory && d.p == nullptr && d.cap == 0 && live.size() == 2);
        CHECK(d.reserve(1000) == hipSuccess && d.cap == 1000);
        Buf e(std::move(d));
        CHECK(d.p == nullptr && d.cap == 0 && e.cap == 1000);
        d.reset();
        h = std::move(e);                               // takes the kind along: released through the right call
        CHECK(h.kind == Buf::DEVICE && live.size() == 2);
        m.reset(); m.reset();
        CHECK(m.p == nullptr && m.cap == 0 && live.size() == 1);
    }
    balanced("buffer");
}

static void test_group()
{
    for (int k = 1; k <= 6; ++k) {
        Buf b[6] = {Buf::DEVICE, Buf::DEVICE, Buf::PINNED, Buf::DEVICE, Buf::MAPPED, Buf::DEVICE};
        auto grow = [&](size_t n) {
            return reserve_group({{&b[0], n}, {&b[1], 2 * n}, {&b[2], n + 16}, {&b[3], 8 * n}, {&b[4], n}, {&b[5], n + 16}});
        };
        CHECK(grow(64) == hipSuccess && live.size() == 6);
        fail_in = k;
        CHECK(grow(128) == hipErrorOutOfMemory);
        for (const Buf &x : b) CHECK(x.p == nullptr && x.cap == 0);
        CHECK(live.empty());
        CHECK(grow(128) == hipSuccess && live.size() == 6 && b[3].cap == 1024 && b[5].cap == 144);
    }
    balanced("group");
}

static void test_handles()
{
    {
        Event e, f;
        Stream s, t;
        CHECK(!e && !s);
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && s.create(hipStreamNonBlocking) == hipSuccess && t.create(hipStreamNonBlocking, 0) == hipSuccess);
        hipEvent_t raw = e;
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && (hipEvent_t)e == raw && live.size() == 3);     // live: a no-op
        fail_in = 1;
        CHECK(f.create(hipEventDefault) == hipErrorOutOfMemory && !f && f.create(hipEventDefault) == hipSuccess);
        Event g(std::move(e));
        Stream u(std::move(s));
        CHECK(!e && !s && (hipEvent_t)g == raw && live.size() == 4);
        t = std::move(u);
        CHECK(live.size() == 3);
        EventPool pool;
        hipEvent_t a = nullptr, b = nullptr;
        CHECK(pool.grab(&a) && pool.grab(&b) && live.size() == 5);
        pool.put(a);
        hipEvent_t c = nullptr;
        CHECK(pool.grab(&c) && c == a && live.size() == 5);               // recycled
        fail_in = 1;
        hipEvent_t d = nullptr;
        CHECK(!pool.grab(&d));
        pool.put(b); pool.put(c);
    }
    balanced("handles");
}

int main()
{
    test_list();
    test_buf();
    test_group();
    test_handles();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("az_res: ok (%d handles made and released)\n", n_made);
    return 0;
}
