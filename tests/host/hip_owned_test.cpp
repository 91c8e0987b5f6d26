// hip_owned_test.cpp -- the owners of oat_amd/csrc/hip_owned.h against a fake runtime, on the CPU: every object the fake
// hands out is counted, a release of something not live aborts, and the k-th creating call can be made to fail.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

typedef int hipError_t;
typedef struct FakeEvent *hipEvent_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipHostMallocMapped = 2, hipEventDisableTiming = 2 };

static std::set<void *> g_live;      // what the fake has handed out and not taken back
static int g_calls = 0, g_fail_at = 0;       // creating calls so far; the one that fails (0: none)

static hipError_t fake_make(void **p, size_t bytes)
{
    if (++g_calls == g_fail_at) return hipErrorOutOfMemory;      // (*p left as it was: the owners must not rely on it)
    *p = malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    return hipSuccess;
}
static hipError_t fake_drop(void *p)
{
    if (!g_live.erase(p)) { fprintf(stderr, "release of %p, which is not live\n", p); abort(); }
    free(p);
    return hipSuccess;
}
static hipError_t hipMalloc(void **p, size_t bytes) { return fake_make(p, bytes); }
static hipError_t hipFree(void *p) { return fake_drop(p); }
static hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return fake_make(p, bytes); }
static hipError_t hipHostFree(void *p) { return fake_drop(p); }
static hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned)
{
    if (++g_calls == g_fail_at) return hipErrorOutOfMemory;
    if (!g_live.count(h)) abort();
    *d = h;
    return hipSuccess;
}
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return fake_make((void **)e, 8); }
static hipError_t hipEventDestroy(hipEvent_t e) { return fake_drop(e); }

#include "../../oat_amd/csrc/hip_owned.h"
using namespace oatgpu;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

struct Pipe {       // the shape of the marker pipeline's resources
    DevMem<long> planes, masks;
    HostMem<int> rec;
    std::vector<Event> ev;
    Event bits_ev;
};
static const int kRing = 3, kCreating = 2 + 2 + kRing + 1;      // creating calls of a full build (the alias lookup is one)

// build aside, as the setters do: true and `out` filled, or false and nothing of this build left
static bool build(Pipe &out)
{
    Pipe p;
    bool ok = p.planes.alloc(64) == hipSuccess;
    ok = ok && p.masks.alloc(192) == hipSuccess;
    ok = ok && p.rec.alloc(32, hipHostMallocMapped) == hipSuccess;
    if (ok) {
        p.ev.resize(kRing);
        for (auto &e : p.ev) ok = ok && e.create(hipEventDisableTiming) == hipSuccess;
    }
    ok = ok && p.bits_ev.create(0) == hipSuccess;
    if (ok) out = std::move(p);
    return ok;
}
static bool full(const Pipe &p)
{
    for (auto &e : p.ev) if (!(hipEvent_t)e) return false;
    return p.planes && p.masks.get() && p.rec.host() && p.rec.dev() == p.rec.host() && p.ev.size() == (size_t)kRing && (hipEvent_t)p.bits_ev;
}

int main()
{
    const size_t per_build = 2 + 1 + kRing + 1;      // live objects of a full build
    {   // a full build, then scope exit
        Pipe a;
        CHECK(build(a) && full(a) && g_live.size() == per_build && g_calls == kCreating);
    }
    CHECK(g_live.empty());
    {   // move-assignment onto a full object releases the old contents, and the source ends empty
        Pipe a, b;
        CHECK(build(a) && build(b) && g_live.size() == 2 * per_build);
        const long *kept = b.planes;
        a = std::move(b);
        CHECK(g_live.size() == per_build && full(a) && a.planes == kept);
        CHECK(!b.planes && !b.masks && !b.rec.host() && !b.rec.dev() && b.ev.empty() && !(hipEvent_t)b.bits_ev);
        a.planes.reset(); a.planes.reset();         // reset() twice is harmless
        a.rec.reset(); a.rec.reset();
        a.bits_ev.reset(); a.bits_ev.reset();
        CHECK(g_live.size() == per_build - 3 && !a.planes && !a.rec.dev());
        CHECK(a.masks.alloc(8) == hipSuccess && g_live.size() == per_build - 3);       // alloc on a full object releases first
        a = {};                                     // dropping a feature is assignment
        CHECK(g_live.empty());
    }
    for (int k = 1; k <= kCreating; ++k) {          // a build that fails at call k leaves nothing of its own behind
        Pipe kept, a;
        CHECK(build(kept));
        g_calls = 0; g_fail_at = k;
        CHECK(!build(a) && g_calls == k);
        g_fail_at = 0;
        CHECK(g_live.size() == per_build && full(kept));
        CHECK(!a.planes && !a.rec.host() && a.ev.empty());
        CHECK(build(a) && g_live.size() == 2 * per_build);      // ... and the next attempt starts from nothing
    }
    CHECK(g_live.empty());
    puts("hip_owned: ok");
    return 0;
}
