// lens_main.cpp -- the arithmetic of the lens renders (prt_amd/csrc/prt_lens.h) on the CPU: a stand-alone program that prints the rays
// of a fixed table of lenses, built by tests/test_lens_cpu.py with -ffp-contract=off (and -fsanitize=address,undefined), which holds
// the numpy restatement tests/prt_lens_ref.py to its output word for word.  It links nothing of HIP and nothing of it is loaded into
// Python.  Output, per lens: a line "lens y0 y1" + the 24 words of the record, then one line of 8 words per ray, all in hex.
#include "../prt_amd/csrc/prt_lens.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

struct Entry {
    prt_lens_desc d;
    uint32_t y0, y1;
};

static prt_lens_desc lens(uint32_t model, uint32_t K, uint32_t pass, uint32_t flags)
{
    prt_lens_desc d{};
    d.model = model;
    d.width = 13;
    d.height = 7;
    d.K = K;
    d.pass = pass;
    d.jitterSeed = 0x9e3779b9u;
    d.flags = flags;
    const float pos[3] = {0.25f, 0.9f, 2.5f}, fwd[3] = {0.1f, -0.2f, -0.97f}, right[3] = {0.8f, 0.0f, 0.08f}, up[3] = {-0.01f, 0.45f, -0.09f};
    memcpy(d.pos, pos, 12);
    memcpy(d.fwd, fwd, 12);
    memcpy(d.right, right, 12);
    memcpy(d.up, up, 12);
    d.lensRadius = 0.0f;
    d.focus = 2.0f;
    d.fov = 3.14159265358979323846f;
    return d;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<Entry> table;
    for (uint32_t model = 0; model < 4; model++)
        for (uint32_t flags = 0; flags < 2; flags++) {
            table.push_back({lens(model, 3, 0, flags), 0, 7});
            table.push_back({lens(model, 1, 5, flags), 2, 5});
        }
    // the thin lens: K = 64, a late pass, one band; a basis that is not normalised
    {
        prt_lens_desc d = lens(PRT_HIP_LENS_PINHOLE, 64, 5, 0);
        d.lensRadius = 0.05f;
        table.push_back({d, 6, 7});
        d.flags = PRT_HIP_LENS_CENTRE;
        d.K = 3;
        d.right[0] = 3.0f;
        d.up[1] = 0.001f;
        table.push_back({d, 0, 7});
    }
    // hostile records: what the arithmetic gives
    {
        prt_lens_desc d = lens(PRT_HIP_LENS_PINHOLE, 3, 0, 0);
        d.lensRadius = 0.1f;
        d.up[0] = d.up[1] = d.up[2] = 0.0f; // normalize3(0): inf * 0
        table.push_back({d, 0, 7});
        d = lens(PRT_HIP_LENS_PINHOLE, 3, 0, 0);
        d.lensRadius = nan;
        table.push_back({d, 0, 7});
        d.lensRadius = -1.0f;
        d.focus = inf;
        table.push_back({d, 0, 7});
        d.lensRadius = 0.1f;
        table.push_back({d, 0, 7});
        d.focus = 0.0f;
        table.push_back({d, 0, 7});
        d = lens(PRT_HIP_LENS_EQUIRECT, 3, 0, 0);
        d.fwd[2] = 3e20f;
        d.pos[0] = nan;
        table.push_back({d, 0, 7});
        d = lens(PRT_HIP_LENS_ORTHO, 3, 0, 0);
        d.right[0] = d.right[1] = d.right[2] = 0.0f;
        d.fwd[0] = 1e-30f;
        table.push_back({d, 0, 7});
        const float fovs[4] = {0.0f, 3.14159265358979323846f, 6.28318530717958647692f, 7.0f};
        for (float fov : fovs) {
            d = lens(PRT_HIP_LENS_FISHEYE, 3, 0, 0);
            d.fov = fov;
            table.push_back({d, 0, 7});
        }
    }
    for (const Entry& e : table) {
        uint32_t w[24];
        static_assert(sizeof(prt_lens_desc) == sizeof(w), "prt_lens_desc is 96 bytes");
        memcpy(w, &e.d, sizeof(w));
        printf("lens %u %u", e.y0, e.y1);
        for (uint32_t v : w) printf(" %08x", v);
        printf("\n");
        const PrtLensFrame f = prt_lens_frame(&e.d);
        for (uint32_t y = e.y0; y < e.y1; y++)
            for (uint32_t x = 0; x < e.d.width; x++)
                for (uint32_t k = 0; k < e.d.K; k++) {
                    const PrtLensRay r = prt_lens_ray(&e.d, &f, x, y, k);
                    const float out[8] = {r.org.x, r.org.y, r.org.z, 0.0f, r.dir.x, r.dir.y, r.dir.z, 0.0f};
                    uint32_t o[8];
                    memcpy(o, out, sizeof(o));
                    o[7] = 0; // pad
                    for (uint32_t v : o) printf(" %08x", v);
                    printf("\n");
                }
    }
    return 0;
}
