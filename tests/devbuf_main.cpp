// devbuf_main.cpp -- the contract of DevBuf (prt_amd/csrc/prt_devbuf.h) on the CPU: a stand-alone program with a malloc-backed,
// counting hipMalloc / hipFree / hipStreamSynchronize of its own, built with -fsanitize=address,undefined by tests/test_devbuf_cpu.py.
// It links nothing of HIP.  Exit status 0 = every check holds.
#include "../prt_amd/csrc/prt_devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

static std::string g_log;      // 'S' synchronise, 'F' free of live memory, 'M' allocation (also a refused one)
static long g_live = 0;        // allocations not yet freed
static size_t g_minBytes = (size_t)-1; // the smallest request since it was last reset
static bool g_failNext = false;
static int g_failed = 0;

extern "C" hipError_t hipMalloc(void** p, size_t bytes)
{
    g_log += 'M';
    if (bytes < g_minBytes) g_minBytes = bytes;
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
static_assert(std::is_nothrow_move_constructible<DevBuf<float>>::value, "DevBuf must move without throwing (std::vector moves it when it grows)");
static_assert(std::is_nothrow_move_assignable<DevBuf<float>>::value, "DevBuf must move without throwing");

// what the scene keeps per mesh (PrtRefitMesh): a struct of buffers, held in a vector
struct Mesh {
    int id = 0;
    DevBuf<float> pos, nrm;
    DevBuf<uint32_t> off;
};
static_assert(std::is_nothrow_move_constructible<Mesh>::value && !std::is_copy_constructible<Mesh>::value, "a struct of DevBufs moves and does not copy");
// the four arrays of the environment light: one set held by the scene, another built aside and handed over (prt_edit.hip)
struct Env {
    DevBuf<double> texels;
    DevBuf<float> vert, hor;
    DevBuf<int> firstX;
};

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
    took();
    {
        // ---- move construction hands the memory over: the source is empty, nothing is allocated, freed or waited for
        DevBuf<float> a;
        CHECK(a.fit(9, s) == hipSuccess && took() == "M");
        float* pa = a;
        DevBuf<float> b(std::move(a));
        CHECK(!a && a.size() == 0 && b == pa && b.size() == 9 && took() == "");
        memset(b, 0, 9 * sizeof(float));
        DevBuf<float> e(std::move(a)); // from an empty one
        CHECK(!e && e.size() == 0 && !a && took() == "");
        // ---- move assignment onto a buffer that holds memory frees that memory, once, without a synchronisation
        DevBuf<float> t;
        CHECK(t.fit(4, s) == hipSuccess && took() == "M");
        t = std::move(b);
        CHECK(took() == "F" && t == pa && t.size() == 9 && !b && b.size() == 0);
        // ---- onto an empty buffer: nothing
        a = std::move(t);
        CHECK(took() == "" && a == pa && a.size() == 9 && !t && t.size() == 0);
        // ---- an empty source empties the target
        a = std::move(t);
        CHECK(took() == "F" && !a && a.size() == 0 && !t);
        // ---- self-assignment is harmless
        CHECK(a.fit(3, s) == hipSuccess && took() == "M");
        pa = a;
        DevBuf<float>& same = a;
        a = std::move(same);
        CHECK(took() == "" && a == pa && a.size() == 3);
        memset(a, 0, 3 * sizeof(float));
    }
    CHECK(took() == "F" && g_live == 0); // one live allocation was left, and the moved-from buffers freed nothing
    {
        // ---- a vector of structs that hold buffers: growing it moves them, and frees and allocates no device memory
        std::vector<Mesh> meshes;
        std::vector<float*> pos;
        std::vector<uint32_t*> off;
        size_t reallocations = 0;
        for (int k = 0; k < 40; k++) {
            Mesh m;
            m.id = k;
            CHECK(m.pos.fit(3 * (size_t)k, s) == hipSuccess && m.off.fit((size_t)k + 1, s) == hipSuccess); // nrm stays empty
            pos.push_back(m.pos);
            off.push_back(m.off);
            CHECK(took() == "MM");
            const size_t cap = meshes.capacity();
            meshes.push_back(std::move(m));
            if (meshes.capacity() != cap) reallocations++;
            CHECK(took() == "" && g_live == 2 * (k + 1));
        }
        CHECK(reallocations >= 4); // (capacity 1, 2, 4, ... 64)
        for (int k = 0; k < 40; k++) {
            CHECK(meshes[k].id == k && meshes[k].pos == pos[k] && meshes[k].off == off[k] && !meshes[k].nrm);
            CHECK(meshes[k].pos.size() == 3 * (size_t)k && meshes[k].off.size() == (size_t)k + 1);
            memset(meshes[k].off, 0, ((size_t)k + 1) * sizeof(uint32_t));
        }
        meshes = std::vector<Mesh>{}; // "drop it all"
        CHECK(took() == std::string(80, 'F') && g_live == 0); // each allocation once (twice would be the sanitizer's to report)
    }
    CHECK(took() == "" && g_live == 0);
    {
        // ---- no request is smaller than 64 bytes, and size() still counts elements
        g_minBytes = (size_t)-1;
        DevBuf<char> c0, c1;
        DevBuf<uint32_t> u3;
        CHECK(c0.fit(0, s) == hipSuccess && c1.fit(1, s) == hipSuccess && u3.fit(3, s) == hipSuccess && took() == "MMM");
        CHECK(g_minBytes == 64);
        CHECK(c0 && c0.size() == 0 && c1.size() == 1 && u3.size() == 3);
        memset(c1, 0, 64);
        DevBuf<double> d9;
        CHECK(d9.fit(9, s) == hipSuccess && took() == "M" && g_minBytes == 64); // above the floor: its own size
        memset(d9, 0, 9 * sizeof(double));
    }
    CHECK(took() == "FFFF" && g_live == 0);
    {
        // ---- the hand-over of prt_edit.hip: four buffers built aside replace four held ones
        Env held;
        CHECK(held.texels.fit(8, s) == hipSuccess && held.vert.fit(2, s) == hipSuccess && held.hor.fit(8, s) == hipSuccess && held.firstX.fit(2, s) == hipSuccess);
        CHECK(took() == "MMMM");
        double* t1 = nullptr;
        {
            Env b;
            DevBuf<uint32_t> result; // not handed over: freed with the scope
            CHECK(b.texels.fit(32, s) == hipSuccess && b.vert.fit(4, s) == hipSuccess && b.hor.fit(32, s) == hipSuccess && b.firstX.fit(4, s) == hipSuccess &&
                  result.fit(16, s) == hipSuccess);
            CHECK(took() == "MMMMM" && g_live == 9);
            t1 = b.texels;
            held.texels = std::move(b.texels);
            held.vert = std::move(b.vert);
            held.hor = std::move(b.hor);
            held.firstX = std::move(b.firstX);
            CHECK(took() == "FFFF" && g_live == 5); // the four old arrays, each once
            CHECK(!b.texels && !b.vert && !b.hor && !b.firstX);
        }
        CHECK(took() == "F" && g_live == 4); // the result words alone: the locals were empty
        CHECK(held.texels == t1 && held.texels.size() == 32 && held.vert.size() == 4 && held.hor.size() == 32 && held.firstX.size() == 4);
        memset(held.texels, 0, 32 * sizeof(double));
        held = Env{}; // the environment light is removed
        CHECK(took() == "FFFF" && g_live == 0 && !held.texels);
    }
    CHECK(took() == "" && g_live == 0);
    if (g_failed) return 1;
    puts("devbuf ok");
    return 0;
}
