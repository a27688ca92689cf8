// devbuf_main.cpp -- the contract of DevBuf (prt_amd/csrc/prt_devbuf.h) on the CPU: a stand-alone program with a malloc-backed,
// counting hipMalloc / hipFree / hipStreamSynchronize of its own, built with -fsanitize=address,undefined by tests/test_devbuf_cpu.py.
// It links nothing of HIP.  Exit status 0 = every check holds.
#include "../prt_amd/csrc/prt_devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

static std::string g_log;      // 'S' synchronise, 'F' free of live memory, 'M' allocation (also a refused one)
static long g_live = 0;        // allocations not yet freed
static bool g_failNext = false;
static int g_failed = 0;

extern "C" hipError_t hipMalloc(void** p, size_t bytes)
{
    g_log += 'M';
    if (g_failNext) {
        g_failNext = false;
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes);
    g_live++;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p)
{
    g_log += 'F';
    free(p);
    g_live--;
    return hipSuccess;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t)
{
    g_log += 'S';
    return hipSuccess;
}

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

// the calls since the last look
static std::string took()
{
    std::string s = g_log;
    g_log.clear();
    return s;
}

static_assert(!std::is_copy_constructible<DevBuf<float>>::value, "DevBuf must not be copyable");
static_assert(!std::is_copy_assignable<DevBuf<float>>::value, "DevBuf must not be copyable");

int main()
{
    hipStream_t s = nullptr;
    {
        // ---- exact policy
        DevBuf<double> b;
        CHECK(!b && b.size() == 0);
        bool fresh = false;
        CHECK(b.fit(10, s, &fresh) == hipSuccess && fresh && b && b.size() == 10);
        CHECK(took() == "M"); // nothing was live: nothing to wait for
        memset(b, 0, 10 * sizeof(double)); // (the sanitizer checks the size)
        double* first = b;
        fresh = false;
        CHECK(b.fit(10, s, &fresh) == hipSuccess && !fresh && b == first && b.size() == 10);
        CHECK(took() == ""); // reused without a synchronisation
        CHECK(b.fit(20, s, &fresh) == hipSuccess && fresh && b.size() == 20);
        CHECK(took() == "SFM"); // one synchronisation, then the free, then the allocation
        memset(b, 0, 20 * sizeof(double));
        fresh = false;
        CHECK(b.fit(5, s, &fresh) == hipSuccess && fresh && b.size() == 5);
        CHECK(took() == "SFM");
        CHECK(b.fit(5, s) == hipSuccess && took() == ""); // the flag is optional

        // ---- a failed allocation leaves the buffer empty, and the next request allocates again
        fresh = false;
        g_failNext = true;
        CHECK(b.fit(10, s, &fresh) == hipErrorOutOfMemory);
        CHECK(!b && b.size() == 0 && fresh); // the old contents are gone
        CHECK(took() == "SFM");
        fresh = false;
        CHECK(b.fit(5, s, &fresh) == hipSuccess && fresh && b && b.size() == 5); // the earlier size: not taken for present
        CHECK(took() == "M");
        memset(b, 0, 5 * sizeof(double));
    }
    CHECK(took() == "F" && g_live == 0); // destruction frees
    {
        // ---- grow policy
        DevBuf<uint32_t> g;
        bool fresh = false;
        CHECK(g.grow(10, s, &fresh) == hipSuccess && fresh && g.size() == 10 && took() == "M");
        uint32_t* first = g;
        fresh = false;
        CHECK(g.grow(4, s, &fresh) == hipSuccess && !fresh && g == first && g.size() == 10 && took() == "");
        CHECK(g.grow(10, s, &fresh) == hipSuccess && !fresh && g == first && took() == "");
        CHECK(g.grow(11, s, &fresh) == hipSuccess && fresh && g.size() == 11 && took() == "SFM");
        memset(g, 0, 11 * sizeof(uint32_t));
        g_failNext = true;
        CHECK(g.grow(100, s) == hipErrorOutOfMemory && !g && g.size() == 0 && took() == "SFM");
        CHECK(g.grow(4, s) == hipSuccess && g && g.size() == 4 && took() == "M"); // fewer than before the failure: allocated all the same
        // ---- release
        g.release();
        CHECK(!g && g.size() == 0 && took() == "F");
        g.release();
        CHECK(took() == "");
    }
    CHECK(took() == "" && g_live == 0); // an empty buffer frees nothing
    {
        // ---- zero elements still yield a pointer
        DevBuf<char> z, y;
        bool fresh = false;
        CHECK(z.fit(0, s, &fresh) == hipSuccess && fresh && z && z.size() == 0 && took() == "M");
        fresh = false;
        CHECK(z.fit(0, s, &fresh) == hipSuccess && !fresh && took() == "");
        CHECK(y.grow(0, s) == hipSuccess && y && took() == "M");
        // ---- swap exchanges the memory and the counts
        CHECK(y.grow(7, s) == hipSuccess && took() == "SFM");
        char *pz = z, *py = y;
        z.swap(y);
        CHECK(z == py && z.size() == 7 && y == pz && y.size() == 0 && took() == "");
        struct Rec { int a, b; };
        DevBuf<Rec> r;
        CHECK(r.fit(1, s) == hipSuccess && &r->b == &((Rec*)r)->b);
    }
    CHECK(g_live == 0);
    if (g_failed) return 1;
    puts("devbuf ok");
    return 0;
}
