// prt_envcdf.h -- the arithmetic of InfiniteAreaLight::create (light.cpp:30-84; host mirror: host/prt_host.cpp) as host / device
// functions: prt_hip_update_lights builds the two CDF tables of a new environment map on the device (prt_edit.hip), and a host
// check runs the same text (prt_hip_test_env_tables_host).  All of it is f32 without FMA, with correctly rounded / and sqrtf, and
// every sum runs in index order -- float addition is not associative, so there is no tree reduction and no parallel scan here: a
// caller hands over consecutive CHUNKS of a row (or of the column), in order, and the state travels in PrtEnvScan.
//
// The same two steps serve a row and the column: the sum of the terms in order (prt_env_sum), then the running table
// accum + inv * term (prt_env_scan), which also finds what prt_hip_upload_scene derives from host-built tables and what it
// refuses (prt_upload.hip "InfiniteAreaLight"): the first index whose value differs from its predecessor's, a table that is
// not non-decreasing, and -- rows only -- a row that starts with a NaN (an all-black row: 0 * inf, light.cpp:63-70) but is not
// NaN throughout.
#pragma once
#include <math.h>

#include "prt_devmath.h"

#define PRT_ENV_BAD_VERTICAL 1u // the vertical table is not non-decreasing
#define PRT_ENV_PARTLY_NAN 2u   // a horizontal row begins with a NaN and holds a number
#define PRT_ENV_BAD_ROW 4u      // a horizontal row is not non-decreasing
#define PRT_ENV_CHUNK 64u       // terms per chunk: one per lane of a wavefront

// length(c) (vecmath.h: sqrtf(dot(c, c)))
PRT_HD float prt_env_length(float r, float g, float b) { return sqrtf((r * r + g * g) + b * b); }

// sinPhi of row y (light.cpp:58)
PRT_HD float prt_env_sin_phi(uint32_t y, int32_t height)
{
    const float kPi = 3.14159265358979323846f; // vecmath.h:162
    float s, c;
    prt_sincosf(kPi * ((float)y + 0.5f) / (float)height, &s, &c);
    return s;
}

// sum += term[0]; sum += term[1]; ... in this order
PRT_HD float prt_env_sum(float sum, const float* term, uint32_t n)
{
    for (uint32_t k = 0; k < n; k++) sum += term[k];
    return sum;
}

struct PrtEnvScan {
    float accum, prev;
    uint32_t index;  // terms seen
    int32_t first;   // first index i >= 1 with !(p[i] - p[i - 1] == 0), -1 = none yet (light.cpp:96-98, 112-114)
    uint32_t nanRow; // p[0] is a NaN
    uint32_t flags;
};

PRT_HD PrtEnvScan prt_env_scan_begin()
{
    PrtEnvScan s;
    s.accum = 0.0f;
    s.prev = 0.0f;
    s.index = 0u;
    s.first = -1;
    s.nanRow = 0u;
    s.flags = 0u;
    return s;
}

// The next n terms of a table, replaced in place by p = accum + inv * term.  badFlag: raised where p[i] >= p[i - 1] does not hold;
// nanFlag (0 for the column, which has no such rule): a row whose p[0] is a NaN is judged by it instead -- every p must be a NaN.
PRT_HD void prt_env_scan(PrtEnvScan* s, float inv, float* term, uint32_t n, uint32_t badFlag, uint32_t nanFlag)
{
    for (uint32_t k = 0; k < n; k++) {
        const float p = s->accum + inv * term[k];
        term[k] = p;
        s->accum = p;
        if (s->index == 0u) {
            s->nanRow = (nanFlag != 0u && p != p) ? 1u : 0u;
        } else {
            if (s->first < 0 && !(p - s->prev == 0.0f)) s->first = (int32_t)s->index;
            if (s->nanRow) {
                if (p == p) s->flags |= nanFlag;
            } else if (!(p >= s->prev)) {
                s->flags |= badFlag;
            }
        }
        s->prev = p;
        s->index++;
    }
}

// firstStep of the finished table of n entries
PRT_HD int32_t prt_env_first_step(const PrtEnvScan* s, int32_t n) { return s->first < 0 ? n : s->first; }
