// test_buf.cpp -- the owners of csrc/eslam_buf.h against counting, malloc-backed stand-ins for the
// HIP calls they make (no HIP library is linked; built with ASan + UBSan by tests/test_buf.py).
// Every check prints on failure; the program exits non-zero if one failed or if an allocation or
// an event is still live at the end.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <utility>

#include "../../slam-eslam_amd/csrc/eslam_buf.h"

namespace {

std::set<void*> g_dev, g_pinned, g_events;   // live device blocks, pinned blocks, events
std::string g_log;                           // 'A' / 'F' per device or pinned allocation / free, in call order
long g_allocs = 0, g_frees = 0, g_syncs = 0, g_records = 0, g_event_creates = 0, g_timed_creates = 0;
long g_fail_from = 0, g_fail_count = 0;      // allocations g_fail_from .. + g_fail_count - 1 from now fail
size_t g_last_bytes = 0;
int g_failed = 0;

// the n-th allocation from now (1: the next) and the count - 1 after it fail
void fail_allocs(long n, long count = 1)
{
    g_fail_from = g_allocs + n;
    g_fail_count = count;
}

hipError_t stub_alloc(std::set<void*>& pool, void** p, size_t bytes)
{
    ++g_allocs;
    if (g_allocs >= g_fail_from && g_allocs < g_fail_from + g_fail_count) return hipErrorOutOfMemory;
    g_log += 'A';
    g_last_bytes = bytes;
    *p = malloc(bytes ? bytes : 1);
    pool.insert(*p);
    return hipSuccess;
}

hipError_t stub_free(std::set<void*>& pool, void* p)
{
    if (!p) return hipSuccess;
    if (!pool.erase(p)) {
        printf("FAIL: free of a block that is not live (double free, or the wrong kind of memory)\n");
        ++g_failed;
        return hipErrorInvalidValue;
    }
    ++g_frees;
    g_log += 'F';
    free(p);
    return hipSuccess;
}

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

size_t live() { return g_dev.size() + g_pinned.size(); }

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(g_dev, p, bytes); }
hipError_t hipFree(void* p) { return stub_free(g_dev, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return stub_alloc(g_pinned, p, bytes); }
hipError_t hipHostFree(void* p) { return stub_free(g_pinned, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned)
{
    ++g_event_creates;
    *e = (hipEvent_t)malloc(1);
    g_events.insert(*e);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e)
{
    ++g_timed_creates;
    return hipEventCreateWithFlags(e, 0);
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    if (!g_events.erase(e)) {
        printf("FAIL: destroy of an event that is not live\n");
        ++g_failed;
        return hipErrorInvalidValue;
    }
    free(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    ++g_records;
    return g_events.count(e) ? hipSuccess : hipErrorInvalidValue;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b)
{
    *ms = g_events.count(a) && g_events.count(b) && a != b ? 0.5f : -1000.0f;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
    ++g_syncs;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
}

using namespace eslam_buf;

static void test_lifetime()
{
    {
        Dev<uint32_t> d;
        Pinned<double> p;
        CHECK(d.get() == nullptr && d.cap() == 0);
        CHECK(d.alloc(100) == hipSuccess && p.alloc(64) == hipSuccess);
        CHECK(d.get() != nullptr && d.cap() == 100 && p.cap() == 64);
        CHECK(g_dev.size() == 1 && g_pinned.size() == 1);
        uint32_t* raw = d;                       // typed access without a cast
        CHECK(raw == d.get() && d.as<char>() == (char*)raw);
    }
    CHECK(live() == 0);                          // the destructor frees, each kind with its own call
    Dev<void> d;
    CHECK(d.alloc(10) == hipSuccess);
    const long frees = g_frees;
    d.reset();
    CHECK(live() == 0 && g_frees == frees + 1 && d.get() == nullptr && d.cap() == 0);
    d.reset();                                   // harmless
    CHECK(g_frees == frees + 1);
    CHECK(d.alloc(10) == hipSuccess && d.alloc(20) == hipSuccess);   // alloc over a held block frees it
    CHECK(live() == 1 && d.cap() == 20);
    fail_allocs(1);
    CHECK(d.alloc(30) != hipSuccess && d.get() == nullptr && d.cap() == 0 && live() == 0);
}

static void test_move()
{
    Dev<int> a, b;
    CHECK(a.alloc(8) == hipSuccess && b.alloc(16) == hipSuccess);
    int* pa = a;
    Dev<int> c(std::move(a));                    // ownership moves, nothing is freed
    CHECK(c.get() == pa && c.cap() == 8 && a.get() == nullptr && a.cap() == 0 && live() == 2);
    const long frees = g_frees;
    b = std::move(c);                            // the overwritten target's block goes
    CHECK(b.get() == pa && b.cap() == 8 && c.get() == nullptr && g_frees == frees + 1 && live() == 1);
    Dev<int>& self = b;
    b = std::move(self);                         // self-assignment keeps the block
    CHECK(b.get() == pa && live() == 1);
    struct Group { Dev<int> x; Dev<float> y; };
    Group g;
    CHECK(g.x.alloc(4) == hipSuccess && g.y.alloc(4) == hipSuccess && live() == 3);
    g = Group{};                                 // how the context drops a group of buffers
    CHECK(live() == 1 && g.x.get() == nullptr && g.y.get() == nullptr);
    b.reset();
    CHECK(live() == 0);
}

static void test_grow()
{
    Pinned<void> p;
    long syncs = g_syncs, allocs = g_allocs;
    CHECK(p.grow(0, nullptr) == hipSuccess && g_allocs == allocs && g_syncs == syncs);   // 0 <= 0
    CHECK(p.grow(1000, nullptr) == hipSuccess);
    CHECK(p.cap() == 1000 + 250 + 4096 && g_last_bytes == p.cap() && g_pinned.size() == 1 && g_syncs == syncs + 1);
    syncs = g_syncs; allocs = g_allocs;
    const long frees = g_frees;
    void* was = p;
    CHECK(p.grow(5346, nullptr) == hipSuccess);  // fits: no call at all
    CHECK(p.get() == was && g_syncs == syncs && g_allocs == allocs && g_frees == frees);
    g_log.clear();
    CHECK(p.grow(5347, nullptr) == hipSuccess);
    CHECK(g_log == "FA" && g_syncs == syncs + 1);   // the old block goes before the new one exists
    CHECK(p.cap() == 5347 + 5347 / 4 + 4096 && g_pinned.size() == 1 && g_dev.empty());
    fail_allocs(1);
    CHECK(p.grow(100000, nullptr) == hipErrorOutOfMemory);
    CHECK(p.get() == nullptr && p.cap() == 0 && live() == 0);   // empty after a failed growth
    CHECK(p.grow(8, nullptr) == hipSuccess && p.cap() == 8 + 2 + 4096);
}

static void test_grow_keep()
{
    Dev<eslam_scan_patch> d;
    const uint64_t unit = sizeof(eslam_scan_patch);
    hipError_t he = hipSuccess;
    long syncs = g_syncs;
    CHECK(d.grow_keep(10 * unit + 1, unit, nullptr, &he) == ESLAM_OK);
    // bytes + bytes / 4, rounded up to whole units
    const uint64_t want = (10 * unit + 1 + (10 * unit + 1) / 4 + unit - 1) / unit;
    CHECK(d.cap() == want && g_last_bytes == want * unit && g_syncs == syncs + 1 && live() == 1);
    syncs = g_syncs;
    long allocs = g_allocs;
    CHECK(d.grow_keep(want * unit, unit, nullptr, &he) == ESLAM_OK && g_allocs == allocs && g_syncs == syncs);   // fits
    g_log.clear();
    CHECK(d.grow_keep(want * unit + 1, unit, nullptr, &he) == ESLAM_OK);
    CHECK(g_log == "AF" && live() == 1);         // the new block exists before the old one goes
    // the first allocation fails, the second succeeds: the exact unit count
    const uint64_t bytes = 100 * unit + 3;
    fail_allocs(1);
    CHECK(d.grow_keep(bytes, unit, nullptr, &he) == ESLAM_OK);
    CHECK(d.cap() == 101 && g_last_bytes == 101 * unit && live() == 1);
    // both fail: out of memory, and the old block and capacity stay live and unchanged
    eslam_scan_patch* was = d;
    const long frees = g_frees;
    allocs = g_allocs;
    fail_allocs(1, 2);
    CHECK(d.grow_keep(1000 * unit, unit, nullptr, &he) == ESLAM_ERR_OUT_OF_MEMORY);
    CHECK(g_allocs == allocs + 2 && g_frees == frees && d.get() == was && d.cap() == 101 && g_dev.count(was) == 1);
    Dev<void> m;                                 // byte units (the scan build's scratch)
    CHECK(m.grow_keep(1001, 1, nullptr, &he) == ESLAM_OK && m.cap() == 1001 + 250);
}

static int three(Dev<int>* keep)
{
    Dev<int> a, b, c;
    if (a.alloc(16) != hipSuccess || b.alloc(16) != hipSuccess || c.alloc(16) != hipSuccess) return ESLAM_ERR_OUT_OF_MEMORY;
    *keep = std::move(a);
    return ESLAM_OK;
}

static void test_group()
{
    Dev<int> keep;
    fail_allocs(3);
    CHECK(three(&keep) == ESLAM_ERR_OUT_OF_MEMORY);
    CHECK(live() == 0 && keep.get() == nullptr); // the first two went when the scope ended
    CHECK(three(&keep) == ESLAM_OK && live() == 1);
}

static void test_events()
{
    {
        Event e;
        CHECK((hipEvent_t)e == nullptr);
        CHECK(e.create(false) == hipSuccess && g_events.size() == 1 && g_timed_creates == 0);
        hipEvent_t was = e;
        CHECK(e.create(false) == hipSuccess && (hipEvent_t)e == was && g_event_creates == 1);   // created once
        Event f(std::move(e));
        CHECK((hipEvent_t)f == was && (hipEvent_t)e == nullptr && g_events.size() == 1);
        Event t;
        CHECK(t.create(true) == hipSuccess && g_timed_creates == 1);
        t = std::move(f);                        // the overwritten event is destroyed
        CHECK((hipEvent_t)t == was && g_events.size() == 1);
    }
    CHECK(g_events.empty());
    {
        EventRing ring(5, 4), pair(2, 1);
        const long creates = g_event_creates;
        for (uint32_t k = 0; k < 5; ++k) ring.record(false, k, nullptr);
        CHECK(g_event_creates == creates && g_records == 0 && ring.steps() == 0);   // timing off: nothing
        ring.record(true, 0, nullptr);
        CHECK(g_event_creates == creates + 5 * kRingSteps && g_records == 1 && ring.steps() == 0);   // on first use
        for (uint32_t k = 1; k < 4; ++k) ring.record(true, k, nullptr);
        CHECK(ring.steps() == 0 && g_records == 4);
        ring.record(true, 4, nullptr);           // the closing index ends the step
        CHECK(ring.steps() == 1 && g_records == 5 && g_event_creates == creates + 5 * kRingSteps);
        ring.record(true, 0, nullptr);           // an open step is not counted
        double acc[5] = {-1, -1, -1, -1, -1};
        CHECK(ring.sums(acc) == 1 && ring.steps() == 0);   // every interval between two distinct live events, once
        CHECK(acc[0] == 0.5 && acc[1] == 0.5 && acc[2] == 0.5 && acc[3] == 0.5 && acc[4] == 0.5);
        for (uint32_t k = 0; k < 5; ++k) ring.record(true, k, nullptr);
        CHECK(ring.steps() == 1 && g_records == 11);
        g_records = 5;
        for (uint32_t s = 1; s < kRingSteps; ++s)
            for (uint32_t k = 0; k < 5; ++k) ring.record(true, k, nullptr);
        CHECK(ring.steps() == kRingSteps && kRingSteps == 2048 && g_records == 5 * 2048);
        for (uint32_t k = 0; k < 5; ++k) ring.record(true, k, nullptr);
        CHECK(ring.steps() == 2048 && g_records == 5 * 2048);   // the ring is full: recording stops
        ring.clear();
        ring.record(true, 0, nullptr);
        CHECK(ring.steps() == 0 && g_records == 5 * 2048 + 1 && g_event_creates == creates + 5 * kRingSteps);
        pair.record(true, 0, nullptr);
        pair.record(true, 1, nullptr);
        CHECK(pair.steps() == 1 && g_events.size() == 7 * kRingSteps);
    }
    CHECK(g_events.empty());                     // every event destroyed with its ring
}

int main()
{
    test_lifetime();
    test_move();
    test_grow();
    test_grow_keep();
    test_group();
    test_events();
    if (live() || !g_events.empty()) {
        printf("FAIL: %zu allocations and %zu events still live at exit\n", live(), g_events.size());
        ++g_failed;
    }
    if (g_failed) printf("test_buf: %d checks failed\n", g_failed);
    else printf("test_buf ok\n");
    return g_failed ? 1 : 0;
}
