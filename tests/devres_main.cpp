// devres_main.cpp -- the contracts of DevEvent, HostBuf and StageTimer (prt_amd/csrc/prt_devres.h) on the CPU: a stand-alone program
// with counting fakes of the event and pinned-memory calls, built with -fsanitize=address,undefined by tests/test_devres_cpu.py.
// It links nothing of HIP.  Exit status 0 = every check holds.
#include "../prt_amd/csrc/prt_devres.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

// A fake event is a heap object (a double destroy or a use after destroy is the sanitizer's to report) that remembers the position
// of its last record in the program's sequence of records.
struct FakeEvent {
    long order = -1;
    unsigned flags = 0;
};
static long g_liveEvents = 0, g_created = 0, g_records = 0;
static long g_livePinned = 0, g_pinnedCalls = 0;
static size_t g_minBytes = (size_t)-1;
static long g_failCreateIn = 0; // k > 0: the k-th creation from now on is refused
static bool g_failPinned = false;
static unsigned g_lastFlags = 0xffffffffu;
static int g_failed = 0;

extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags)
{
    if (g_failCreateIn > 0 && --g_failCreateIn == 0) return hipErrorOutOfMemory; // (*e is left as it was)
    FakeEvent* f = new FakeEvent;
    f->flags = flags;
    g_lastFlags = flags;
    g_liveEvents++;
    g_created++;
    *e = (hipEvent_t)f;
    return hipSuccess;
}
extern "C" hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDefault); }
extern "C" hipError_t hipEventDestroy(hipEvent_t e)
{
    delete (FakeEvent*)e;
    g_liveEvents--;
    return hipSuccess;
}
extern "C" hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    ((FakeEvent*)e)->order = g_records++;
    return hipSuccess;
}
// The time between two events is a function of WHEN each was recorded: 100 per record between them, plus the position of the first
// within the program's records.  A stage attributed to the wrong pair of events, or to another repetition, gets another value.
static float fake_ms(long from, long to) { return 100.0f * (float)(to - from) + (float)from; }
extern "C" hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b)
{
    const FakeEvent *fa = (const FakeEvent*)a, *fb = (const FakeEvent*)b;
    if (fa->order < 0 || fb->order < 0) return hipErrorInvalidHandle; // never recorded
    *ms = fake_ms(fa->order, fb->order);
    return hipSuccess;
}
extern "C" hipError_t hipHostMalloc(void** p, size_t bytes, unsigned)
{
    g_pinnedCalls++;
    if (bytes < g_minBytes) g_minBytes = bytes;
    if (g_failPinned) {
        g_failPinned = false;
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes);
    g_livePinned++;
    return hipSuccess;
}
extern "C" hipError_t hipHostFree(void* p)
{
    free(p);
    g_livePinned--;
    return hipSuccess;
}

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

static_assert(!std::is_copy_constructible<DevEvent>::value && !std::is_copy_assignable<DevEvent>::value, "DevEvent must not be copyable");
static_assert(std::is_nothrow_move_constructible<DevEvent>::value && std::is_nothrow_move_assignable<DevEvent>::value, "DevEvent must move without throwing");
static_assert(!std::is_copy_constructible<HostBuf<float>>::value && !std::is_copy_assignable<HostBuf<float>>::value, "HostBuf must not be copyable");
static_assert(std::is_nothrow_move_constructible<HostBuf<float>>::value && std::is_nothrow_move_assignable<HostBuf<float>>::value,
              "HostBuf must move without throwing (std::vector moves it when it grows)");

// what the context keeps (prt_hip_ctx, PrtRefit): a ring of events, and a struct of pinned buffers that is replaced by assignment
struct Ring {
    DevEvent t0[4], t1[4];
};
struct Refit {
    int id = 0;
    HostBuf<float> root, vbox;
};
static_assert(std::is_nothrow_move_constructible<Refit>::value && !std::is_copy_constructible<Refit>::value, "a struct of HostBufs moves and does not copy");
static_assert(std::is_nothrow_move_constructible<Ring>::value && !std::is_copy_constructible<Ring>::value, "a struct of DevEvent arrays moves and does not copy");

// One repetition of a profile call: `marks` marks, then the lap.  *first = the position of the repetition's first record.
static hipError_t repetition(StageTimer& tm, int marks, bool discard, long* first)
{
    *first = g_records;
    hipError_t worst = hipSuccess;
    for (int k = 0; k < marks; k++) {
        hipError_t e = tm.mark(nullptr);
        if (e != hipSuccess) worst = e;
    }
    hipError_t e = tm.lap(discard);
    return worst != hipSuccess ? worst : e;
}

// an entry point that returns between two marks, as HIP_TRY does
static int abandoned_after_one_mark()
{
    StageTimer tm(3);
    if (tm.mark(nullptr) != hipSuccess) return 2;
    if (g_liveEvents != 1) return 3;
    return 1; // "the launch failed"
}

int main()
{
    {
        // ---- DevEvent: null until made, made once, destroyed with the object
        DevEvent e;
        CHECK(!(hipEvent_t)e && g_created == 0);
        CHECK(e.make() == hipSuccess && (hipEvent_t)e && g_created == 1 && g_liveEvents == 1 && g_lastFlags == hipEventDefault);
        hipEvent_t first = e;
        CHECK(e.make() == hipSuccess && (hipEvent_t)e == first && g_created == 1); // twice creates once
        CHECK(e.make(hipEventDisableTiming) == hipSuccess && (hipEvent_t)e == first && g_created == 1 && g_lastFlags == hipEventDefault); // kept
        DevEvent quiet;
        CHECK(quiet.make(hipEventDisableTiming) == hipSuccess && g_lastFlags == hipEventDisableTiming && ((FakeEvent*)(hipEvent_t)quiet)->flags == hipEventDisableTiming);
        // ---- a failed create leaves it null, and the next make creates
        DevEvent f;
        g_failCreateIn = 1;
        CHECK(f.make() == hipErrorOutOfMemory && !(hipEvent_t)f && g_liveEvents == 2);
        CHECK(f.make() == hipSuccess && (hipEvent_t)f && g_liveEvents == 3);
        // ---- moves hand the event over
        DevEvent m(std::move(e));
        CHECK(!(hipEvent_t)e && (hipEvent_t)m == first && g_liveEvents == 3);
        f = std::move(m); // onto a live one: that one is destroyed, once
        CHECK((hipEvent_t)f == first && !(hipEvent_t)m && g_liveEvents == 2);
        DevEvent& same = f;
        f = std::move(same);
        CHECK((hipEvent_t)f == first && g_liveEvents == 2);
        f.release();
        f.release();
        CHECK(!(hipEvent_t)f && g_liveEvents == 1);
    }
    CHECK(g_liveEvents == 0);
    {
        // ---- arrays of events in a vector that grows: the lazily made ones move along, each is destroyed once
        std::vector<Ring> rings;
        size_t reallocations = 0;
        for (int k = 0; k < 20; k++) {
            Ring r;
            CHECK(r.t0[k % 4].make() == hipSuccess && r.t1[k % 4].make() == hipSuccess); // the others stay null
            hipEvent_t h = r.t0[k % 4];
            const size_t cap = rings.capacity();
            rings.push_back(std::move(r));
            if (rings.capacity() != cap) reallocations++;
            CHECK((hipEvent_t)rings.back().t0[k % 4] == h && g_liveEvents == 2 * (k + 1));
        }
        CHECK(reallocations >= 4);
        for (int k = 0; k < 20; k++)
            for (int j = 0; j < 4; j++) CHECK(((hipEvent_t)rings[k].t0[j] != nullptr) == (j == k % 4));
    }
    CHECK(g_liveEvents == 0);
    {
        // ---- HostBuf: DevBuf's vocabulary
        HostBuf<double> b;
        CHECK(!b && b.size() == 0);
        CHECK(b.fit(10) == hipSuccess && b && b.size() == 10 && g_pinnedCalls == 1 && g_livePinned == 1);
        memset(b, 0, 10 * sizeof(double)); // (the sanitizer checks the size)
        double* first = b;
        CHECK(b.fit(10) == hipSuccess && b == first && g_pinnedCalls == 1); // the same size: kept
        CHECK(b.fit(20) == hipSuccess && b.size() == 20 && g_pinnedCalls == 2 && g_livePinned == 1); // another size: remade
        memset(b, 0, 20 * sizeof(double));
        CHECK(b.fit(5) == hipSuccess && b.size() == 5 && g_pinnedCalls == 3 && g_livePinned == 1);
        // ---- a failed allocation leaves the buffer empty, and the next request allocates again
        g_failPinned = true;
        CHECK(b.fit(10) == hipErrorOutOfMemory && !b && b.size() == 0 && g_livePinned == 0);
        CHECK(b.fit(5) == hipSuccess && b && b.size() == 5 && g_livePinned == 1); // the earlier size: not taken for present
        memset(b, 0, 5 * sizeof(double));
        // ---- zero elements still yield a pointer; no request is smaller than 64 bytes
        g_minBytes = (size_t)-1;
        HostBuf<uint32_t> z, one;
        CHECK(z.fit(0) == hipSuccess && z && z.size() == 0 && one.fit(1) == hipSuccess && one.size() == 1 && g_minBytes == 64);
        *one = 7u;
        CHECK(one[0] == 7u);
        const long calls = g_pinnedCalls;
        CHECK(z.fit(0) == hipSuccess && g_pinnedCalls == calls);
        // ---- release, moves
        z.release();
        z.release();
        CHECK(!z && z.size() == 0 && g_livePinned == 2);
        uint32_t* po = one;
        HostBuf<uint32_t> m(std::move(one));
        CHECK(!one && one.size() == 0 && m == po && m.size() == 1 && g_livePinned == 2);
        CHECK(z.fit(3) == hipSuccess && g_livePinned == 3);
        z = std::move(m); // onto a full one: its memory is freed, once
        CHECK(z == po && z.size() == 1 && !m && g_livePinned == 2);
        HostBuf<uint32_t>& same = z;
        z = std::move(same);
        CHECK(z == po && z.size() == 1 && g_livePinned == 2);
    }
    CHECK(g_livePinned == 0);
    {
        // ---- a vector of structs that hold pinned buffers grows; "R = PrtRefit{}" drops what a struct held
        std::vector<Refit> v;
        std::vector<float*> roots;
        for (int k = 0; k < 20; k++) {
            Refit r;
            r.id = k;
            CHECK(r.root.fit(6 * (size_t)(k + 1)) == hipSuccess); // vbox stays empty
            roots.push_back(r.root);
            v.push_back(std::move(r));
            CHECK(g_livePinned == k + 1);
        }
        for (int k = 0; k < 20; k++) {
            CHECK(v[k].id == k && v[k].root == roots[k] && v[k].root.size() == 6 * (size_t)(k + 1) && !v[k].vbox);
            memset(v[k].root, 0, 6 * (size_t)(k + 1) * sizeof(float));
        }
        CHECK(v[3].vbox.fit(6) == hipSuccess && g_livePinned == 21);
        v[3] = Refit{}; // both go
        CHECK(!v[3].root && !v[3].vbox && g_livePinned == 19);
        CHECK(v[3].root.fit(6) == hipSuccess && g_livePinned == 20); // a build after a forget allocates
    }
    CHECK(g_livePinned == 0);
    {
        // ---- StageTimer(3): four repetitions, the first discarded; medians by sorted[size / 2] of an odd and of an even count
        StageTimer tm(3);
        CHECK(g_liveEvents == 0); // nothing is created before the first mark
        float ms = -1.0f;
        CHECK(tm.median(0, &ms) == hipErrorInvalidValue && ms == -1.0f); // no sample yet
        long at[4];
        const long created = g_created;
        CHECK(repetition(tm, 4, true, &at[0]) == hipSuccess);
        CHECK(g_created == created + 4 && g_liveEvents == 4);
        CHECK(tm.median(0, &ms) == hipErrorInvalidValue); // the warm-up left no sample
        for (int r = 1; r < 4; r++) CHECK(repetition(tm, 4, false, &at[r]) == hipSuccess);
        CHECK(g_created == created + 4); // the events are reused
        CHECK(at[1] == at[0] + 4 && at[2] == at[0] + 8 && at[3] == at[0] + 12);
        // stage k of the repetition whose first record is `a` lies between records a + k and a + k + 1; three samples: the middle one
        for (uint32_t k = 0; k < 3; k++) CHECK(tm.median(k, &ms) == hipSuccess && ms == fake_ms(at[2] + k, at[2] + k + 1));
        CHECK(tm.median(3, &ms) == hipErrorInvalidValue); // there is no stage 3
        long at4;
        CHECK(repetition(tm, 4, false, &at4) == hipSuccess); // four samples: sorted[2], the third smallest
        for (uint32_t k = 0; k < 3; k++) CHECK(tm.median(k, &ms) == hipSuccess && ms == fake_ms(at[3] + k, at[3] + k + 1));
        // ---- a repetition with a missing or a surplus mark is an error and leaves no sample; the next one is whole again
        long bad, good;
        CHECK(repetition(tm, 3, false, &bad) == hipErrorInvalidValue);
        CHECK(repetition(tm, 5, false, &bad) == hipErrorInvalidValue);
        CHECK(tm.mark(nullptr) == hipSuccess && tm.mark(nullptr) == hipSuccess && tm.mark(nullptr) == hipSuccess && tm.mark(nullptr) == hipSuccess);
        CHECK(tm.mark(nullptr) == hipErrorInvalidValue); // the fifth is refused by mark itself ...
        CHECK(tm.lap() == hipErrorInvalidValue);         // ... and the lap does not attribute the four
        for (uint32_t k = 0; k < 3; k++) CHECK(tm.median(k, &ms) == hipSuccess && ms == fake_ms(at[3] + k, at[3] + k + 1)); // still four samples
        CHECK(repetition(tm, 4, false, &good) == hipSuccess); // five samples: sorted[2] is still the repetition at at[3]
        for (uint32_t k = 0; k < 3; k++) CHECK(tm.median(k, &ms) == hipSuccess && ms == fake_ms(at[3] + k, at[3] + k + 1));
        CHECK(g_created == created + 4 && g_liveEvents == 4);
    }
    CHECK(g_liveEvents == 0);
    {
        // ---- one stage, one repetition (the yardstick, the BVH build)
        StageTimer tm(1);
        long a;
        float ms = 0.0f;
        CHECK(repetition(tm, 2, false, &a) == hipSuccess && tm.median(0, &ms) == hipSuccess && ms == fake_ms(a, a + 1));
    }
    CHECK(g_liveEvents == 0);
    // ---- the early return: a timer abandoned after one mark
    CHECK(abandoned_after_one_mark() == 1 && g_liveEvents == 0);
    {
        // ---- the k-th creation fails: the mark that needed it reports it, nothing was recorded on it, and the events made so far go
        // with the timer
        StageTimer tm(3);
        g_failCreateIn = 3;
        const long records = g_records;
        CHECK(tm.mark(nullptr) == hipSuccess && tm.mark(nullptr) == hipSuccess && g_liveEvents == 2);
        CHECK(tm.mark(nullptr) == hipErrorOutOfMemory && g_liveEvents == 2 && g_records == records + 2);
        CHECK(tm.lap() == hipErrorInvalidValue); // two marks are not a repetition
    }
    CHECK(g_liveEvents == 0 && g_livePinned == 0);
    if (g_failed) return 1;
    puts("devres ok");
    return 0;
}
