// test_buf.cpp -- the owners of csrc/eslam_buf.h against counting, malloc-backed stand-ins for the
// HIP calls they make (no HIP library is linked; built with ASan + UBSan by tests/test_buf.py);
// its Carver, and the scratch layouts of csrc/eslam_scratch.h that are written with it.
// Every check prints on failure; the program exits non-zero if one failed or if an allocation or
// an event is still live at the end.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <utility>

#include "../../slam-eslam_amd/csrc/eslam_buf.h"
#include "../../slam-eslam_amd/csrc/eslam_scratch.h"

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

static bool aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 256 == 0; }

static void test_carver()
{
    // a null base only measures
    Carver m(nullptr);
    CHECK(m.bytes() == 0);
    CHECK(m.take<uint32_t>(5) == nullptr && m.bytes() == 256);
    CHECK(m.take_bytes(257) == nullptr && m.bytes() == 768);
    CHECK(m.take<double>(0) == nullptr && m.bytes() == 768);     // a count of 0 takes nothing
    CHECK(m.take_bytes(0) == nullptr && m.bytes() == 768);
    CHECK(m.take_bytes(13) == nullptr && m.bytes() == 1024);
    CHECK(m.take<uint64_t>(3) == nullptr && m.bytes() == 1280);
    // the same takes over a block: the same size, every array aligned and clear of the next
    char* block = static_cast<char*>(aligned_alloc(256, m.bytes()));
    Carver p(block);
    uint32_t* a = p.take<uint32_t>(5);
    char* b = static_cast<char*>(p.take_bytes(257));
    double* z = p.take<double>(0);
    void* z2 = p.take_bytes(0);
    char* odd = static_cast<char*>(p.take_bytes(13));
    uint64_t* w = p.take<uint64_t>(3);                           // after an odd-sized region
    CHECK(p.bytes() == m.bytes());
    CHECK(aligned(a) && aligned(b) && aligned(z) && aligned(odd) && aligned(w));
    CHECK((char*)a == block && b == block + 256 && (char*)z == block + 768 && z2 == (void*)z && odd == block + 768 &&
          (char*)w == block + 1024);
    CHECK((char*)(a + 5) <= b && b + 257 <= odd && odd + 13 <= (char*)w && (char*)(w + 3) <= block + p.bytes());
    for (int k = 0; k < 5; ++k) a[k] = 1u;                       // the sanitizers see every store
    for (int k = 0; k < 257; ++k) b[k] = 2;
    for (int k = 0; k < 13; ++k) odd[k] = 3;
    for (int k = 0; k < 3; ++k) w[k] = 4u;
    CHECK(a[4] == 1u && b[0] == 2 && b[256] == 2 && odd[12] == 3 && w[0] == 4u && w[2] == 4u);
    free(block);
    // another alignment
    alignas(64) char small[192];
    Carver q(small, 64);
    CHECK(q.take_bytes(1) == small && q.take<uint64_t>(9) == (uint64_t*)(small + 64) && q.bytes() == 192);
}

// A layout's arrays over a block of its measured size, as offsets from the block's start.
struct Placed {
    char* block;
    uint64_t bytes;
    explicit Placed(uint64_t b) : block(static_cast<char*>(aligned_alloc(256, b ? b : 256))), bytes(b) {}
    ~Placed() { free(block); }
    uint64_t off(const void* p) const { return (uint64_t)(static_cast<const char*>(p) - block); }
};

// The five scratch layouts of csrc/eslam_scratch.h against the offsets the hand-written chains of
// `off_*` constants gave before the Carver (restated here as plain arithmetic): no array moved.
static void test_layouts()
{
    using namespace eslam_host;
    using namespace eslam_dev;
    auto up = [](uint64_t b) { return (b + 255) & ~(uint64_t)255; };
    const uint64_t counts[3] = {1, 63, 257};
    static_assert(sizeof(float2) == 8 && sizeof(ScanPatch) == 32 && kSmCounters == 8 && kScanCounters == 4, "unit sizes");
    for (uint64_t x : counts)
        for (uint64_t y : counts)
            for (uint64_t v : counts) {
                {   // sm_scratch: x records, y cells, v scan patches
                    const uint64_t rec = x, ncell = y, sort_bytes = 1000 + 7 * x;
                    const uint64_t off_keys = 0, off_vals = off_keys + up((rec + 1) * 4), off_ko = off_vals + up(rec * 4),
                                   off_ord = off_ko + up(rec * 4), off_app = off_ord + up(rec * 4), off_add = off_app + up(rec * 8),
                                   off_seg = off_add + up(ncell * 4), off_tch = off_seg + up(ncell * 4),
                                   off_cnt = off_tch + up(ncell * 4), off_sort = off_cnt + up(8 * 8),
                                   off_sp = off_sort + up(sort_bytes), total = off_sp + up(v * 32);
                    SmScratch s = {};
                    ScanPatch* sp = nullptr;
                    Carver size(nullptr);
                    carve_sm(size, rec, ncell, v, sort_bytes, &s, &sp);
                    CHECK(size.bytes() == total && s.keys == nullptr && sp == nullptr);
                    Placed b(total);
                    Carver place(b.block);
                    carve_sm(place, rec, ncell, v, sort_bytes, &s, &sp);
                    CHECK(place.bytes() == total);
                    CHECK(b.off(s.keys) == off_keys && b.off(s.vals) == off_vals && b.off(s.keys_out) == off_ko &&
                          b.off(s.order) == off_ord && b.off(s.app) == off_app && b.off(s.add) == off_add &&
                          b.off(s.segpos) == off_seg && b.off(s.touched) == off_tch && b.off(s.cnt) == off_cnt &&
                          b.off(s.sort_tmp) == off_sort && s.sort_tmp_bytes == sort_bytes && b.off(sp) == off_sp);
                }
                for (int multi = 0; multi < 2; ++multi) {   // resample_to: x particles, y samples
                    const uint64_t n = x, samples = y, tn = (n + 255) / 256 + v, ts = (samples + 255) / 256 + v;
                    const uint64_t o_coarse = up(n * 8), o_cnt = o_coarse + up(tn * 8), o_anc = o_cnt + 256,
                                   o_out = o_anc + up(samples * 4), o_kept = o_out + (multi ? up(samples * 4) : 0),
                                   bytes = o_kept + up((ts + 1) * 4);
                    ResampleScratch r = {};
                    Carver size(nullptr);
                    carve_resample(size, n, tn, samples, ts, multi != 0, &r);
                    CHECK(size.bytes() == bytes && r.C == nullptr && r.anc_kept == nullptr);
                    Placed b(bytes);
                    Carver place(b.block);
                    carve_resample(place, n, tn, samples, ts, multi != 0, &r);
                    CHECK(place.bytes() == bytes);
                    CHECK(b.off(r.C) == 0 && b.off(r.coarse) == o_coarse && b.off(r.counter) == o_cnt && b.off(r.anc) == o_anc &&
                          b.off(r.anc_kept) == (multi ? o_out : o_anc) && b.off(r.kept) == o_kept);
                }
                {   // snap_census: x tables, y particles (the capacity), v pages
                    const uint64_t ntables = x, cap = y, npages = v;
                    const uint64_t o_first = 0, o_trank = o_first + up(ntables * 4), o_tlist = o_trank + up(ntables * 4),
                                   o_fref = o_tlist + up(cap * 4), o_prank = o_fref + up(npages * 8),
                                   o_plist = o_prank + up(npages * 4), total = o_plist + up(npages * 4);
                    SnapCensus c = {};
                    Carver size(nullptr);
                    carve_census(size, ntables, cap, npages, &c);
                    CHECK(size.bytes() == total && c.first == nullptr);
                    Placed b(total);
                    Carver place(b.block);
                    carve_census(place, ntables, cap, npages, &c);
                    CHECK(place.bytes() == total && c.counts == nullptr);
                    CHECK(b.off(c.first) == o_first && b.off(c.trank) == o_trank && b.off(c.tlist) == o_tlist &&
                          b.off(c.firstref) == o_fref && b.off(c.prank) == o_prank && b.off(c.plist) == o_plist);
                }
                {   // the particle-grid work block: x x y tiles, v blocks
                    const uint64_t tx = x, ty = y, blocks = v;
                    const uint64_t off_dir = 0, off_bsum = off_dir + up(tx * ty * 4), off_own = off_bsum + up((blocks + 1) * 4),
                                   total = off_own + up(8);
                    PgScratch g = {};
                    Carver size(nullptr);
                    carve_pgrid(size, tx, ty, blocks, &g);
                    CHECK(size.bytes() == total && g.dir == nullptr);
                    Placed b(total);
                    Carver place(b.block);
                    carve_pgrid(place, tx, ty, blocks, &g);
                    CHECK(place.bytes() == total && g.tx == tx && g.ty == ty);
                    CHECK(b.off(g.dir) == off_dir && b.off(g.bsum) == off_bsum && b.off(g.own) == off_own);
                }
            }
    const uint64_t points[4] = {0, 1, 63, 257};
    for (uint64_t n : points) {   // the scan work block: n points (0: the doubles still have one element)
        const uint64_t sort_bytes = 777 + n;
        const uint64_t u = up((n + 1) * 4), d = up((n ? n : 1) * 8);
        uint64_t off = 0, at[12];
        for (int k = 0; k < 6; ++k) { at[k] = off; off += u; }       // a, b, c, d, e, raw
        for (int k = 6; k < 10; ++k) { at[k] = off; off += d; }      // pz, var, sz, sv
        at[10] = off; off += up(4 * 8);                              // cnt
        at[11] = off; off += up(sort_bytes);                         // sort_tmp
        ScanWork w = {};
        Carver size(nullptr);
        carve_scan(size, n, sort_bytes, &w);
        CHECK(size.bytes() == off && w.a == nullptr && w.sort_tmp == nullptr);
        Placed b(off);
        Carver place(b.block);
        carve_scan(place, n, sort_bytes, &w);
        CHECK(place.bytes() == off && w.sort_tmp_bytes == sort_bytes);
        CHECK(b.off(w.a) == at[0] && b.off(w.b) == at[1] && b.off(w.c) == at[2] && b.off(w.d) == at[3] && b.off(w.e) == at[4] &&
              b.off(w.raw) == at[5] && b.off(w.pz) == at[6] && b.off(w.var) == at[7] && b.off(w.sz) == at[8] &&
              b.off(w.sv) == at[9] && b.off(w.cnt) == at[10] && b.off(w.sort_tmp) == at[11]);
    }
}

int main()
{
    test_carver();
    test_layouts();
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
