// atlas_filter_main.cpp -- the lightmap filter (prt_amd/csrc/prt_atlas_filter.h) on the CPU: a stand-alone program that runs the whole
// filter -- index, prepare, iterations -- over the cases of a file, with the text the kernels compile.  Built by
// tests/test_atlas_filter_cpu.py with -ffp-contract=off (and -fsanitize=address,undefined), which holds the numpy restatement
// tests/prt_atlas_filter_ref.py to its output word for word.  It links nothing of HIP and nothing of it is loaded into Python.
// Usage: atlas_filter_main <cases> <results>.  The file of cases (tests/prt_atlas_filter_cases.py write_cases): a count, then per case
// six words W H n stride iterations normalPowerLog2, two floats sigmaLuminance sigmaPosition, n texels, n points and n*stride values.
// The results: n*stride words per case.
#include "../prt_amd/csrc/prt_atlas_filter.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// 16-byte aligned storage for n elements of T
template <typename T> struct Aligned {
    explicit Aligned(size_t n) : p((T*)aligned_alloc(16, (n * sizeof(T) + 15) / 16 * 16 + 16)) {}
    ~Aligned() { free(p); }
    Aligned(const Aligned&) = delete;
    Aligned& operator=(const Aligned&) = delete;
    T* p;
};

static bool get(FILE* f, void* to, size_t bytes) { return bytes == 0 || fread(to, bytes, 1, f) == 1; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    if (!in || !res) return 2;
    uint32_t cases = 0;
    if (!get(in, &cases, 4)) return 3;
    for (uint32_t c = 0; c < cases; c++) {
        uint32_t h[6];
        float sig[2];
        if (!get(in, h, sizeof(h)) || !get(in, sig, sizeof(sig))) return 3;
        const uint32_t W = h[0], H = h[1], n = h[2], stride = h[3], iterations = h[4];
        const size_t floats = (size_t)n * stride;
        std::vector<uint32_t> texels(n), map((size_t)W * H, PRT_AF_NONE);
        std::vector<float> values(floats), out(floats), plane[2];
        Aligned<prt_bake_point> points(n);
        Aligned<PrtAfQuad> rec(n);
        if (!get(in, texels.data(), 4 * (size_t)n) || !get(in, points.p, sizeof(prt_bake_point) * (size_t)n) || !get(in, values.data(), 4 * floats)) return 3;
        for (auto& p : plane) p.assign(floats + n, 0.0f);
        PrtAfArgs A{};
        A.W = W;
        A.H = H;
        A.n = n;
        A.stride = stride;
        A.texels = texels.data();
        A.points = points.p;
        A.values = values.data();
        A.map = map.data();
        A.rec = rec.p;
        A.npl2 = h[5];
        A.sigL = sig[0];
        A.sigP2 = sig[1] * sig[1];
        // af_index_kernel: the minimum the atomic takes
        for (uint32_t q = 0; q < n; q++)
            if (prt_af_eligible(A, q) && q < map[texels[q]]) map[texels[q]] = q;
        for (uint32_t q = 0; q < n; q++) prt_af_prepare(A, q);
        // launch_filter of prt_atlas_filter.hip
        const bool multi = stride > 3;
        A.cin = A.values;
        A.vin = &A.rec->z;
        A.vinStride = 4;
        for (uint32_t i = 0; i < iterations; i++) {
            const bool last = i + 1 == iterations;
            float* pl = plane[i & 1].data();
            A.step = 1u << i;
            A.cout = last ? out.data() : pl;
            A.vout = last ? nullptr : pl + floats;
            for (uint32_t q = 0; q < n; q++) {
                if (last && multi) prt_af_iterate<true, true>(A, q);
                else if (last) prt_af_iterate<true, false>(A, q);
                else if (multi) prt_af_iterate<false, true>(A, q);
                else prt_af_iterate<false, false>(A, q);
            }
            A.cin = A.cout;
            A.vin = A.vout;
            A.vinStride = 1;
        }
        if (floats && fwrite(out.data(), 4 * floats, 1, res) != 1) return 4;
    }
    fclose(in);
    return fclose(res) == 0 ? 0 : 4;
}
