// stage_main.cpp -- the contract of PrtIoArray and PrtStage (prt_amd/csrc/prt_stage.h) on the CPU: a stand-alone program with
// malloc-backed fakes of hipMalloc / hipFree / hipMemcpyAsync / hipStreamSynchronize that perform the copy and log every call in order,
// built with -fsanitize=address,undefined by tests/test_stage_cpu.py.  It links nothing of HIP.  Exit status 0 = every check holds.
#include "../prt_amd/csrc/prt_stage.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

struct Call {
    char kind; // 'M' allocation (also a refused one), 'F' free, 'S' synchronise, 'H' copy host to device, 'D' copy device to host
    const void* dst;
    const void* src;
    size_t bytes;
};
static std::vector<Call> g_log;
static long g_live = 0;
static size_t g_lastBytes = 0;
static bool g_failNext = false;
static int g_failed = 0;

extern "C" hipError_t hipMalloc(void** p, size_t bytes)
{
    g_log.push_back({'M', nullptr, nullptr, bytes});
    g_lastBytes = bytes;
    if (g_failNext) {
        g_failNext = false;
        return hipErrorOutOfMemory;
    }
    *p = aligned_alloc(256, (bytes + 255) / 256 * 256); // device allocations are at least 256-byte aligned; a copy past `bytes` rounded
    g_live++;                                           // up to the slice size is the sanitizer's to report
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p)
{
    g_log.push_back({'F', p, nullptr, 0});
    free(p);
    g_live--;
    return hipSuccess;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t)
{
    g_log.push_back({'S', nullptr, nullptr, 0});
    return hipSuccess;
}
extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
    g_log.push_back({kind == hipMemcpyHostToDevice ? 'H' : 'D', dst, src, bytes});
    memcpy(dst, src, bytes);
    return hipSuccess;
}

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

static size_t count_of(char kind, size_t from = 0)
{
    size_t n = 0;
    for (size_t i = from; i < g_log.size(); i++) n += g_log[i].kind == kind;
    return n;
}
static std::string kinds(size_t from = 0)
{
    std::string s;
    for (size_t i = from; i < g_log.size(); i++) s += g_log[i].kind;
    return s;
}

// The host-array path of an entry point: place, the launch, fetch.  hook stands for the launch; an error skips what follows.
static hipError_t run(PrtStage& st, PrtIoArray* io, uint32_t count, const std::function<void()>& hook)
{
    hipError_t e = st.place(io, count, nullptr);
    if (e != hipSuccess) return e;
    hook();
    return st.fetch(io, count, nullptr);
}

// Slices in table order, each 256-byte aligned and clear of the next; a null entry has none.
static void check_slices(const PrtIoArray* io, uint32_t count)
{
    const char* end = nullptr;
    for (uint32_t i = 0; i < count; i++) {
        if (!io[i].p) {
            CHECK(io[i].dev == nullptr);
            continue;
        }
        const char* d = (const char*)io[i].dev;
        CHECK(d != nullptr && ((uintptr_t)d & 255) == 0);
        CHECK(end == nullptr || d >= end);
        end = d + io[i].bytes;
    }
}

int main()
{
    {
        // ---- slices; one allocation per call; IN before the launch, OUT after it, one synchronise at the end
        PrtStage st;
        std::vector<char> a(100, 'a'), b(300, 0), c(256, 'c'), d(1, 0);
        PrtIoArray io[5] = {prt_io_in(a.data(), a.size(), 16), prt_io_out(nullptr, 4096, 4), prt_io_out(b.data(), b.size(), 4),
                            prt_io_in(c.data(), c.size(), 4), prt_io_out(d.data(), d.size(), 1)};
        size_t atHook = 0;
        CHECK(run(st, io, 5, [&] {
                  atHook = g_log.size();
                  check_slices(io, 5);
                  CHECK(memcmp(io[0].dev, a.data(), a.size()) == 0 && memcmp(io[3].dev, c.data(), c.size()) == 0); // the IN arrays are there
                  memset(io[2].dev, 'B', b.size());
                  memset(io[4].dev, 'D', d.size());
              }) == hipSuccess);
        CHECK(g_lastBytes == 256 + 512 + 256 + 256 && st.size() == g_lastBytes); // the null entry takes no room
        CHECK(kinds() == "MHHDDS" && atHook == 3); // an empty arena: no synchronise before the one allocation
        CHECK(g_log[1].dst == io[0].dev && g_log[1].src == a.data() && g_log[1].bytes == 100);
        CHECK(g_log[2].dst == io[3].dev && g_log[2].src == c.data() && g_log[2].bytes == 256);
        CHECK(g_log[3].dst == b.data() && g_log[3].src == io[2].dev && g_log[3].bytes == 300);
        CHECK(g_log[4].dst == d.data() && g_log[4].src == io[4].dev && g_log[4].bytes == 1);
        CHECK(b[0] == 'B' && b[299] == 'B' && d[0] == 'D');
        // ---- the arena serves: nothing is allocated, the slices are where they were
        const void* first = io[0].dev;
        size_t from = g_log.size();
        CHECK(run(st, io, 5, [] {}) == hipSuccess && kinds(from) == "HHDDS" && io[0].dev == first);
        // ---- a smaller call is served too, from the start of the arena
        from = g_log.size();
        CHECK(run(st, io + 3, 2, [] {}) == hipSuccess && kinds(from) == "HDS" && io[3].dev == first);
        // ---- the arena must grow with memory in hand: one synchronise, then one allocation, before any copy
        std::vector<char> big(5000, 'g');
        PrtIoArray more[2] = {prt_io_in(big.data(), big.size(), 4), prt_io_out(b.data(), b.size(), 4)};
        from = g_log.size();
        CHECK(run(st, more, 2, [&] { memset(more[1].dev, 'x', b.size()); }) == hipSuccess && kinds(from) == "SFMHDS" && g_live == 1);
        CHECK(st.size() == 5120 + 512 && b[0] == 'x');

        // ---- an OUT array is fetched at the size the launch left: trimmed to 3 of 64 entries, and to none
        std::vector<uint32_t> texels(64, 0xabababab);
        std::vector<char> hits(64 * 24, 'h');
        PrtIoArray ras[2] = {prt_io_out(texels.data(), texels.size() * 4, 4), prt_io_out(hits.data(), hits.size(), 4)};
        from = g_log.size();
        CHECK(run(st, ras, 2, [&] {
                  memset(ras[0].dev, 0, 64 * 4);
                  memset(ras[1].dev, 0, 64 * 24);
                  ras[0].bytes = 3 * 4;
                  ras[1].bytes = 3 * 24;
              }) == hipSuccess);
        CHECK(kinds(from) == "DDS" && g_log[from].bytes == 12 && g_log[from + 1].bytes == 72);
        CHECK(texels[2] == 0 && texels[3] == 0xabababab && hits[71] == 0 && hits[72] == 'h'); // entries at and beyond n stay
        ras[0].bytes = 64 * 4;
        ras[1].bytes = 64 * 24;
        from = g_log.size();
        CHECK(run(st, ras, 2, [&] { ras[0].bytes = ras[1].bytes = 0; }) == hipSuccess && kinds(from) == "S"); // nothing is copied; fetch still waits
        CHECK(texels[0] == 0 && texels[3] == 0xabababab);
    }
    CHECK(g_live == 0);
    {
        // ---- sizes 1, 3, 255, 256 and 257 in one table, in and out: no copy reaches a neighbouring slice
        PrtStage st;
        const size_t sizes[5] = {1, 3, 255, 256, 257};
        std::vector<std::vector<unsigned char>> in(5), out(5);
        PrtIoArray io[10];
        for (int k = 0; k < 5; k++) {
            in[k].assign(sizes[k], (unsigned char)(0x10 + k));
            out[k].assign(sizes[k], 0); // exactly the size: a copy beyond it is the sanitizer's to report
            io[2 * k] = prt_io_in(in[k].data(), sizes[k], 1);
            io[2 * k + 1] = prt_io_out(out[k].data(), sizes[k], 1);
        }
        CHECK(run(st, io, 10, [&] {
                  check_slices(io, 10);
                  for (int k = 0; k < 5; k++) memset(io[2 * k + 1].dev, 0x80 + k, sizes[k]);
                  for (int k = 0; k < 5; k++) // written after every OUT slice: an IN slice is still whole
                      for (size_t j = 0; j < sizes[k]; j++) CHECK(io[2 * k].as<unsigned char>()[j] == 0x10 + k);
              }) == hipSuccess);
        CHECK(g_lastBytes == 2 * (256 + 256 + 256 + 256 + 512));
        for (const Call& c : g_log)
            if (c.kind == 'H' || c.kind == 'D') {
                const char* dev = (const char*)(c.kind == 'H' ? c.dst : c.src);
                for (int i = 0; i < 10; i++) // the copy lies within one slice's own bytes
                    if (io[i].dev == dev) CHECK(c.bytes == io[i].bytes);
            }
        for (int k = 0; k < 5; k++)
            for (size_t j = 0; j < sizes[k]; j++) CHECK(out[k][j] == 0x80 + k);
    }
    CHECK(g_live == 0);
    {
        // ---- a total of 0 bytes still places (DevBuf's floor of 64 bytes), and copies nothing
        PrtStage st;
        char x = 0;
        PrtIoArray none[2] = {prt_io_in(nullptr, 100, 4), prt_io_out(&x, 0, 1)};
        size_t from = g_log.size();
        CHECK(run(st, none, 2, [] {}) == hipSuccess && kinds(from) == "MS" && g_lastBytes == 64 && none[0].dev == nullptr && none[1].dev != nullptr);
        from = g_log.size();
        CHECK(run(st, none, 2, [] {}) == hipSuccess && kinds(from) == "S");

        // ---- a refused allocation: the error comes back, the arena is empty, nothing was copied, and the next place works
        std::vector<char> a(1000, 'a'), b(1000, 0);
        PrtIoArray io[2] = {prt_io_in(a.data(), a.size(), 4), prt_io_out(b.data(), b.size(), 4)};
        g_failNext = true;
        from = g_log.size();
        bool launched = false;
        CHECK(run(st, io, 2, [&] { launched = true; }) == hipErrorOutOfMemory && !launched);
        CHECK(kinds(from) == "SFM" && st.size() == 0 && g_live == 0 && count_of('H', from) + count_of('D', from) == 0);
        from = g_log.size();
        CHECK(run(st, io, 2, [&] { memcpy(io[1].dev, io[0].dev, 1000); }) == hipSuccess && kinds(from) == "MHDS" && b[999] == 'a' && g_live == 1);
    }
    CHECK(g_live == 0);
    {
        // ---- the alignment test, and device arrays: the launch gets the caller's pointers, or nothing is touched
        alignas(64) static char mem[128];
        CHECK(aligned(nullptr, 16) && aligned(nullptr, 4) && aligned(mem, 16) && aligned(mem + 4, 4) && aligned(mem + 1, 1));
        CHECK(!aligned(mem + 2, 4) && !aligned(mem + 8, 16) && aligned(mem + 8, 4));
        PrtIoArray io[3] = {prt_io_in(mem, 32, 16), prt_io_out(nullptr, 24, 4), prt_io_out(mem + 36, 24, 4)};
        const size_t from = g_log.size();
        CHECK(prt_io_on_device(io, 3) && io[0].dev == mem && io[1].dev == nullptr && io[2].dev == mem + 36);
        PrtIoArray off2[2] = {prt_io_in(mem, 32, 16), prt_io_out(mem + 38, 24, 4)}, off8[2] = {prt_io_in(mem + 8, 32, 16), prt_io_out(mem + 36, 24, 4)};
        CHECK(!prt_io_on_device(off2, 2) && off2[0].dev == nullptr && off2[1].dev == nullptr);
        CHECK(!prt_io_on_device(off8, 2) && off8[0].dev == nullptr && off8[1].dev == nullptr);
        CHECK(g_log.size() == from); // nothing is allocated, copied or waited for on this path
    }
    if (g_failed) return 1;
    puts("stage ok");
    return 0;
}
