// prt_stats.h -- the words of a statistics copy, by name, and the hooks of the profile build (-DPRT_PROFILE, tools/role_profile.py).
//
// The context holds PRT_STAT_SHARDS copies of PRT_STAT_STRIDE 64-bit words (a workgroup adds to copy blockIdx.x % PRT_STAT_SHARDS);
// prt_hip_get_stats sums the copies.  The product writes the words PRT_STAT_*; the profile build appends the words PRT_PROF_*.
//
// The hot functions call the hooks below unconditionally, one line per site.  A hook's arguments are lane predicates and counts the
// caller has at hand; what costs something -- ballots, clock reads, LDS reads, loops -- is inside the hook.  The product build gets
// the empty twins at the end of this file and evaluates none of it.  This file holds the only test of PRT_PROFILE.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>

#define PRT_STAT_SHARDS 64 // copies of the statistics counters, summed on read-back
#define PRT_STAT_MODES 4   // traversal modes (PRT_MODE_*, prt_device.h) = ray queues of the frame kernel

enum PrtStatWord {
    // ---- the product's words (prt_hip_stats, include/prt_hip.h)
    PRT_STAT_RAYS = 0,
    PRT_STAT_OCCL = 1,           // occlusion rays (of the rays)
    PRT_STAT_BOX = 2,            // box / triangle tests, surface fetches, texture taps: counting build only
    PRT_STAT_TRI = 3,
    PRT_STAT_HIT = 4,
    PRT_STAT_TAP = 5,
    PRT_STAT_PIXELS = 6,
    PRT_STAT_STACK_OVERFLOW = 7, // launches' workgroups in which a traversal needed more than 64 stack entries
    PRT_STAT_OCCL_SKIPPED = 15,  // occlusion rays the frame kernel answered without a walk (prt_frame.h; read by the test build only)
    PRT_STAT_MODE = 16,          // + 3 * mode + PRT_STAT_MODE_*: the counting build's events per traversal mode (16 .. 27)
    // ---- the profile build's words
    PRT_PROF_SHADE_CYCLES = 8, // per wave of the frame kernel, summed: cycles in the shade role, in trace_queue, at the decision point
    PRT_PROF_TRACE_CYCLES = 9,
    PRT_PROF_IDLE_CYCLES = 10,
    PRT_PROF_SHADE_CALLS = 11,
    PRT_PROF_TRACE_CALLS = 12,
    PRT_PROF_WAVE_CYCLES = 13,
    PRT_PROF_WAVES = 14,
    // words 16 .. 27 are an OVERLAY in the profile build: + 3 * mode + PRT_PROF_LOOP_* instead of the counting build's events (the
    // host reports modeBox / modeTri / modeTap as 0 then)
    PRT_PROF_CLAIMS = 28,       // queue claims of the tracing waves, and those that got nothing
    PRT_PROF_EMPTY_CLAIMS = 29,
    PRT_PROF_SHADE_PASSES = 30, // shade passes and the groups they took
    PRT_PROF_SHADE_GROUPS = 31,
    PRT_PROF_ROUNDS = 32,       // + 8 * mode + PRT_PROF_ROUNDS_* (32 .. 63)
    PRT_PROF_SITOUT = 64,       // + 8 * mode + PRT_PROF_SITOUT_* (64 .. 95): lanes that sit a round out, by reason
    PRT_PROF_TURN = 96,         // + 4 * mode + PRT_PROF_TURN_* (96 .. 111): cycles >> 10 of the parts of a trace loop turn
    PRT_PROF_SHORT_TURNS = 112, // refills that left lanes empty; what the block looked like then, summed:
    PRT_PROF_SHORT_LANES = 113, //   the lanes left empty
    PRT_PROF_SHORT_OTHERS = 114, //  rays in the block's other queues
    PRT_PROF_SHORT_READY = 115, //   groups ready for shading
    PRT_PROF_SHORT_LOCK = 116,  //   1 when every shade role was taken
    PRT_PROF_BOUNCE_PASSES = 118, // shade passes with a bounce, and their lanes that carry a path through it
    PRT_PROF_BOUNCE_LANES = 119,
    PRT_PROF_DIRECT_INT = 120,  // node steps that leave the lane on an internal record outside the hot set: by descending / by a pop
    PRT_PROF_POP_INT = 121,
    PRT_PROF_ALPHA_ROUNDS = 122, // cooperative leaf rounds in which a candidate looked its alpha record up, and their cycles >> 10 from the
    PRT_PROF_ALPHA_CYCLES = 123, // candidate test to the end of the alpha tests
};
enum { PRT_STAT_MODE_BOX, PRT_STAT_MODE_TRI, PRT_STAT_MODE_TAP };
enum { PRT_PROF_LOOP_TURNS, PRT_PROF_LOOP_LANES, PRT_PROF_LOOP_CYCLES }; // (cycles >> 10)
enum {
    PRT_PROF_ROUNDS_NODE,       // node rounds and the lanes that stepped in them
    PRT_PROF_ROUNDS_NODE_LANES,
    PRT_PROF_ROUNDS_LEAF,       // leaf rounds and the lanes on a leaf in them
    PRT_PROF_ROUNDS_LEAF_LANES,
    PRT_PROF_ROUNDS_PAIR_LANES, // pair lanes working in the cooperative leaf rounds (serial leaf steps: lanes on a second triangle)
    PRT_PROF_ROUNDS_REFILL_LANES,
    PRT_PROF_ROUNDS_REFILLS,
    PRT_PROF_ROUNDS_POPS,       // stack pops of modes 1 .. 3 (the packet traversal pops in a loop of its own and is not counted); the
                                // word of mode 0 holds the pops of all modes that came from the spill area in HBM
};
enum {
    PRT_PROF_SITOUT_NODE_ON_LEAF,
    PRT_PROF_SITOUT_NODE_DONE,
    PRT_PROF_SITOUT_NODE_NO_RAY,
    PRT_PROF_SITOUT_LEAF_ON_NODE,
    PRT_PROF_SITOUT_LEAF_DONE,
    PRT_PROF_SITOUT_LEAF_NO_RAY,
    PRT_PROF_SITOUT_LEAF_UPDATES,  // (not lanes: hit-update turns of the leaf rounds' owners)
    PRT_PROF_SITOUT_NODE_DISTINCT, // (not lanes: distinct records the lanes of the node rounds asked for)
};
enum { PRT_PROF_TURN_REFILL, PRT_PROF_TURN_ENTER, PRT_PROF_TURN_STEP };
constexpr int prt_stat_mode(int mode, int k) { return PRT_STAT_MODE + 3 * mode + k; }
constexpr int prt_prof_rounds(int mode, int k) { return PRT_PROF_ROUNDS + 8 * mode + k; }
constexpr int prt_prof_sitout(int mode, int k) { return PRT_PROF_SITOUT + 8 * mode + k; }
constexpr int prt_prof_turn(int mode, int k) { return PRT_PROF_TURN + 4 * mode + k; }

// the copy of the statistics a workgroup adds to (PRT_STAT_STRIDE 64-bit words each: defined below, with the build it belongs to)
__device__ __forceinline__ unsigned long long* prt_stat_copy(unsigned long long* counters);

#ifdef PRT_PROFILE
#define PRT_STAT_STRIDE 128
__device__ __forceinline__ unsigned long long prof_lanes(bool p) { return (unsigned long long)__popcll(__ballot(p)); }
__device__ __forceinline__ unsigned long long prof_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t prof_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t prof_lds(const __attribute__((address_space(3))) uint32_t* p)
{
    return prof_uniform(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}

// The tallies of the traversal (a member of Traffic, prt_device.h): rounds of either kind and the lanes that took part in them
// (wave-uniform), stack pops (per lane).  The trace loop that owns the Traffic writes them out (QueueProfile::flush).
struct TraceTally {
    unsigned long long pNodeRounds, pNodeLanes, pLeafRounds, pLeafLanes, pTri2Lanes, pPops, pDeepPops;
    unsigned long long pNodeWaitLeaf, pNodeDone, pNodeNoRay, pLeafWaitNode, pLeafDone, pLeafNoRay, pLeafUpdates; // lanes that sit a round out, by reason (wave-uniform)
    unsigned long long pDirectInt, pPopInt;        // (per lane)
    unsigned long long pAlphaRounds, pAlphaCycles; // (wave-uniform)
    unsigned long long pNodeDistinct;              // (wave-uniform): the coherence of a wave's rays
    unsigned long long alpha0;                     // clock at the candidate test of the current leaf round
    int sp0;                                       // stack depth before the current node step

    __device__ __forceinline__ void pop(bool deep) // deep: the entry comes from the spill area in HBM
    {
        pPops++;
        if (deep) pDeepPops++;
    }
    // a round of the step phase is decided: nNode lanes stand on an internal node (onNode), nLeaf on a leaf (onLeaf); `finished` lanes
    // have a ray that is done with its BVH, lanes that are not `active` have none.  serialLeaves: the counting build's leaf steps
    __device__ __forceinline__ void round(bool doNode, uint32_t ref, bool onNode, bool onLeaf, bool finished, bool active, uint32_t nNode, uint32_t nLeaf,
                                          bool serialLeaves)
    {
        if (doNode) {
            { // distinct records of this round: one per group of lanes that stand on the same node
                unsigned long long m = __ballot(onNode);
                while (m) {
                    const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)ref, (int)__builtin_ctzll(m));
                    m &= ~__ballot(onNode && ref == r);
                    pNodeDistinct++;
                }
            }
            pNodeRounds++;
            pNodeLanes += nNode;
            pNodeWaitLeaf += nLeaf;
            pNodeDone += prof_lanes(finished);
            pNodeNoRay += prof_lanes(!active);
        } else {
            pLeafRounds++;
            pLeafLanes += nLeaf;
            pLeafWaitNode += nNode;
            pLeafDone += prof_lanes(finished);
            pLeafNoRay += prof_lanes(!active);
            if (serialLeaves) pTri2Lanes += prof_lanes(onLeaf && (ref & 15u) > 1u);
        }
    }
    __device__ __forceinline__ void node_begin(int sp) { sp0 = sp; }
    // coldInternal: the step has left the lane on an internal record outside the hot set
    __device__ __forceinline__ void node_end(bool coldInternal, int sp)
    {
        if (coldInternal) {
            if (sp < sp0) pPopInt++;
            else pDirectInt++;
        }
    }
    __device__ __forceinline__ void leaf_pairs(uint32_t pairs) { pTri2Lanes += pairs; }
    __device__ __forceinline__ void alpha_begin() { alpha0 = __builtin_amdgcn_s_memtime(); }
    // (called inside the pair lanes' branch: the ballot is of the lanes in it)
    __device__ __forceinline__ void alpha_end(bool candidate, bool leafHasAlpha)
    {
        if (__ballot(candidate && leafHasAlpha) != 0ull) { // some candidate lies in a leaf with alpha-tested triangles
            pAlphaRounds++;
            pAlphaCycles += __builtin_amdgcn_s_memtime() - alpha0;
        }
    }
    __device__ __forceinline__ void leaf_update() { pLeafUpdates++; }
};

// trace_queue (prt_frame.h): loop turns, claims and refills of one call, and the cycles of a turn's three parts.
struct QueueProfile {
    unsigned long long pTurns, pLanes, pClaims, pEmptyClaims, pRefills, pRefillLanes, pT0;
    unsigned long long pTRefill, pTEnter, pTStep;
    unsigned long long pShortTurns, pShortLanes, pShortOthers, pShortReady, pShortLock;
    unsigned long long pTa, pTb, pTc; // clock at the start of the turn, behind the hand-off, behind entering the BVHs

    __device__ __forceinline__ static QueueProfile start()
    {
        QueueProfile p{};
        p.pT0 = __builtin_amdgcn_s_memtime();
        return p;
    }
    __device__ __forceinline__ void turn_begin() { pTa = __builtin_amdgcn_s_memtime(); }
    // a refill is over: the lanes of `need` (the wave's mask) asked, those of them that are `active` now were served.  B: the block's
    // LDS (BlockLds, prt_frame.h)
    template <int MODE, class BL>
    __device__ __forceinline__ void refill(BL B, unsigned long long need, bool active)
    {
        const unsigned long long served = need & __ballot(active);
        { // when lanes stay empty after the refill: where is the block's work?
            const uint32_t short_ = (uint32_t)__popcll(need & ~served);
            if (short_) {
                uint32_t others = 0;
                for (int q = 0; q < PRT_STAT_MODES; q++)
                    if (q != MODE) {
                        const int32_t d = (int32_t)(prof_lds(&B->qTail[q]) - prof_lds(&B->qHead[q]));
                        others += d > 0 ? (uint32_t)d : 0u;
                    }
                pShortTurns++;
                pShortLanes += short_;
                pShortOthers += others;
                pShortReady += prof_uniform(block_ready(B));
                pShortLock += prof_uniform(block_lock_free(B) ? 0u : 1u);
            }
        }
        pClaims++;
        if (!served) pEmptyClaims++;
        else {
            pRefills++;
            pRefillLanes += (unsigned long long)__popcll(served);
        }
    }
    __device__ __forceinline__ void handed_off()
    {
        pTb = __builtin_amdgcn_s_memtime();
        pTRefill += pTb - pTa;
    }
    __device__ __forceinline__ void turn(bool active)
    {
        pTurns++;
        pLanes += prof_lanes(active);
    }
    // behind entering / leaving BVHs and behind the step phase (pass 0 of the turn's two)
    __device__ __forceinline__ void entered(int pass)
    {
        pTc = __builtin_amdgcn_s_memtime();
        if (pass == 0) pTEnter += pTc - pTb;
    }
    __device__ __forceinline__ void stepped(int pass)
    {
        if (pass == 0) pTStep += __builtin_amdgcn_s_memtime() - pTc;
    }
    template <int MODE>
    __device__ __forceinline__ void flush(unsigned long long* counters, const TraceTally& t) const
    {
        // per lane: summed over the wave by all its lanes
        const unsigned long long directInt = prof_wave_sum(t.pDirectInt), popInt = prof_wave_sum(t.pPopInt);
        const unsigned long long pops = prof_wave_sum(t.pPops), deepPops = prof_wave_sum(t.pDeepPops);
        if ((threadIdx.x & 63u) == 0u) {
            unsigned long long* C = prt_stat_copy(counters);
            if (MODE != 0) { // (the packet traversal's pops are not counted: its word holds the deep pops)
                atomicAdd(&C[prt_prof_rounds(MODE, PRT_PROF_ROUNDS_POPS)], pops);
                atomicAdd(&C[prt_prof_rounds(0, PRT_PROF_ROUNDS_POPS)], deepPops);
            }
            atomicAdd(&C[prt_prof_rounds(MODE, PRT_PROF_ROUNDS_NODE)], t.pNodeRounds);
            atomicAdd(&C[prt_prof_rounds(MODE, PRT_PROF_ROUNDS_NODE_LANES)], t.pNodeLanes);
            atomicAdd(&C[prt_prof_rounds(MODE, PRT_PROF_ROUNDS_LEAF)], t.pLeafRounds);
            atomicAdd(&C[prt_prof_rounds(MODE, PRT_PROF_ROUNDS_LEAF_LANES)], t.pLeafLanes);
            atomicAdd(&C[prt_prof_rounds(MODE, PRT_PROF_ROUNDS_PAIR_LANES)], t.pTri2Lanes);
            atomicAdd(&C[PRT_PROF_SHORT_TURNS], pShortTurns);
            atomicAdd(&C[PRT_PROF_SHORT_LANES], pShortLanes);
            atomicAdd(&C[PRT_PROF_SHORT_OTHERS], pShortOthers);
            atomicAdd(&C[PRT_PROF_SHORT_READY], pShortReady);
            atomicAdd(&C[PRT_PROF_SHORT_LOCK], pShortLock);
            atomicAdd(&C[prt_prof_turn(MODE, PRT_PROF_TURN_REFILL)], pTRefill >> 10);
            atomicAdd(&C[prt_prof_turn(MODE, PRT_PROF_TURN_ENTER)], pTEnter >> 10);
            atomicAdd(&C[prt_prof_turn(MODE, PRT_PROF_TURN_STEP)], pTStep >> 10);
            atomicAdd(&C[prt_prof_sitout(MODE, PRT_PROF_SITOUT_NODE_ON_LEAF)], t.pNodeWaitLeaf);
            atomicAdd(&C[prt_prof_sitout(MODE, PRT_PROF_SITOUT_NODE_DONE)], t.pNodeDone);
            atomicAdd(&C[prt_prof_sitout(MODE, PRT_PROF_SITOUT_NODE_NO_RAY)], t.pNodeNoRay);
            atomicAdd(&C[prt_prof_sitout(MODE, PRT_PROF_SITOUT_LEAF_ON_NODE)], t.pLeafWaitNode);
            atomicAdd(&C[prt_prof_sitout(MODE, PRT_PROF_SITOUT_LEAF_DONE)], t.pLeafDone);
            atomicAdd(&C[prt_prof_sitout(MODE, PRT_PROF_SITOUT_LEAF_NO_RAY)], t.pLeafNoRay);
            atomicAdd(&C[prt_prof_sitout(MODE, PRT_PROF_SITOUT_LEAF_UPDATES)], t.pLeafUpdates);
            atomicAdd(&C[prt_prof_sitout(MODE, PRT_PROF_SITOUT_NODE_DISTINCT)], t.pNodeDistinct);
            atomicAdd(&C[PRT_PROF_ALPHA_ROUNDS], t.pAlphaRounds);
            atomicAdd(&C[PRT_PROF_ALPHA_CYCLES], t.pAlphaCycles >> 10);
            atomicAdd(&C[PRT_PROF_DIRECT_INT], directInt);
            atomicAdd(&C[PRT_PROF_POP_INT], popInt);
            atomicAdd(&C[prt_prof_rounds(MODE, PRT_PROF_ROUNDS_REFILL_LANES)], pRefillLanes);
            atomicAdd(&C[prt_prof_rounds(MODE, PRT_PROF_ROUNDS_REFILLS)], pRefills);
            atomicAdd(&C[prt_stat_mode(MODE, PRT_PROF_LOOP_TURNS)], pTurns);
            atomicAdd(&C[prt_stat_mode(MODE, PRT_PROF_LOOP_LANES)], pLanes);
            atomicAdd(&C[prt_stat_mode(MODE, PRT_PROF_LOOP_CYCLES)], (__builtin_amdgcn_s_memtime() - pT0) >> 10);
            atomicAdd(&C[PRT_PROF_CLAIMS], pClaims);
            atomicAdd(&C[PRT_PROF_EMPTY_CLAIMS], pEmptyClaims);
        }
    }
};

// frame_body (prt_frame.h): a wave's cycles by role, and the two tallies of the shade role.
struct FrameProfile {
    unsigned long long tShade, tTrace, tIdle, nShade, nTrace, t0, tStart;

    __device__ __forceinline__ static FrameProfile start()
    {
        FrameProfile p{};
        p.tStart = p.t0 = __builtin_amdgcn_s_memtime();
        return p;
    }
    __device__ __forceinline__ void lap(unsigned long long& acc) // the cycles since the last lap go to acc
    {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        acc += t1 - t0;
        t0 = t1;
    }
    __device__ __forceinline__ void decided() { lap(tIdle); } // (the time between role calls: idle turns and the decision point)
    __device__ __forceinline__ void shaded()
    {
        lap(tShade);
        nShade++;
    }
    __device__ __forceinline__ void traced()
    {
        lap(tTrace);
        nTrace++;
    }
    __device__ __forceinline__ void flush(unsigned long long* C)
    {
        lap(tIdle);
        if ((threadIdx.x & 63u) == 0u) {
            atomicAdd(&C[PRT_PROF_SHADE_CYCLES], tShade);
            atomicAdd(&C[PRT_PROF_TRACE_CYCLES], tTrace);
            atomicAdd(&C[PRT_PROF_IDLE_CYCLES], tIdle);
            atomicAdd(&C[PRT_PROF_SHADE_CALLS], nShade);
            atomicAdd(&C[PRT_PROF_TRACE_CALLS], nTrace);
            atomicAdd(&C[PRT_PROF_WAVE_CYCLES], t0 - tStart);
            atomicAdd(&C[PRT_PROF_WAVES], 1ull);
        }
    }
    // shade_pass: the lanes of the pass that carry a path through its bounce (called inside the bounce's branch, which is per group:
    // the ballot is of the lanes in it)
    __device__ __forceinline__ static void bounce(unsigned long long* counters, bool carrying)
    {
        const unsigned long long m = __ballot(carrying);
        if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__ballot(true))) {
            unsigned long long* C = prt_stat_copy(counters);
            atomicAdd(&C[PRT_PROF_BOUNCE_PASSES], 1ull);
            atomicAdd(&C[PRT_PROF_BOUNCE_LANES], (unsigned long long)__popcll(m));
        }
    }
    // shade_role: one pass over `taken` groups
    __device__ __forceinline__ static void shade_pass_done(unsigned long long* counters, uint32_t taken)
    {
        if ((threadIdx.x & 63u) == 0u) {
            unsigned long long* C = prt_stat_copy(counters);
            atomicAdd(&C[PRT_PROF_SHADE_PASSES], 1ull);
            atomicAdd(&C[PRT_PROF_SHADE_GROUPS], (unsigned long long)taken);
        }
    }
};

// prt_hip_get_stats: the report of tools/role_profile.py, from the summed copies
inline void prt_profile_report(const unsigned long long* h)
{
    const unsigned long long waves = h[PRT_PROF_WAVES], cyc = h[PRT_PROF_WAVE_CYCLES];
    if (!waves) return;
    const auto nz = [](unsigned long long v) { return (double)(v ? v : 1); };
    fprintf(stderr, "frame profile: waves %llu, per wave: shade %.1f%% (%.0f calls) trace %.1f%% (%.0f calls) idle/decide %.1f%% of %.2f Mcycles\n", waves,
            100.0 * h[PRT_PROF_SHADE_CYCLES] / cyc, (double)h[PRT_PROF_SHADE_CALLS] / waves, 100.0 * h[PRT_PROF_TRACE_CYCLES] / cyc,
            (double)h[PRT_PROF_TRACE_CALLS] / waves, 100.0 * h[PRT_PROF_IDLE_CYCLES] / cyc, cyc / 1e6 / waves);
    for (int m = 0; m < PRT_STAT_MODES; m++) {
        const unsigned long long turns = h[prt_stat_mode(m, PRT_PROF_LOOP_TURNS)], kcyc = h[prt_stat_mode(m, PRT_PROF_LOOP_CYCLES)];
        fprintf(stderr, "  trace mode %d: %.1f M loop turns, %.1f lanes with a ray per turn, %.1f Gcycles in the loops => %.0f cycles per turn\n", m, turns / 1e6,
                (double)h[prt_stat_mode(m, PRT_PROF_LOOP_LANES)] / nz(turns), kcyc * 1024.0 / 1e9, kcyc * 1024.0 / nz(turns));
    }
    for (int m = 0; m < PRT_STAT_MODES; m++) {
        const unsigned long long* q = h + prt_prof_rounds(m, 0);
        fprintf(stderr, "  mode %d rounds: node %.1f M with %.1f lanes, leaf %.1f M with %.1f lanes on a leaf (%.1f pair lanes working; serial build: lanes on a second triangle); refills %.1f M with %.1f lanes\n", m,
                q[PRT_PROF_ROUNDS_NODE] / 1e6, (double)q[PRT_PROF_ROUNDS_NODE_LANES] / nz(q[PRT_PROF_ROUNDS_NODE]), q[PRT_PROF_ROUNDS_LEAF] / 1e6,
                (double)q[PRT_PROF_ROUNDS_LEAF_LANES] / nz(q[PRT_PROF_ROUNDS_LEAF]), (double)q[PRT_PROF_ROUNDS_PAIR_LANES] / nz(q[PRT_PROF_ROUNDS_LEAF]),
                q[PRT_PROF_ROUNDS_REFILLS] / 1e6, (double)q[PRT_PROF_ROUNDS_REFILL_LANES] / nz(q[PRT_PROF_ROUNDS_REFILLS]));
    }
    for (int m = 0; m < PRT_STAT_MODES; m++) {
        const unsigned long long* w = h + prt_prof_sitout(m, 0);
        const double nr = nz(h[prt_prof_rounds(m, PRT_PROF_ROUNDS_NODE)]), lr = nz(h[prt_prof_rounds(m, PRT_PROF_ROUNDS_LEAF)]);
        fprintf(stderr, "  mode %d lanes sitting out: node rounds %.1f on a leaf, %.1f finished, %.1f without a ray; leaf rounds %.1f on a node, %.1f finished, %.1f without a ray; %.2f hit-update turns per leaf round; %.1f distinct records per node round\n",
                m, w[PRT_PROF_SITOUT_NODE_ON_LEAF] / nr, w[PRT_PROF_SITOUT_NODE_DONE] / nr, w[PRT_PROF_SITOUT_NODE_NO_RAY] / nr, w[PRT_PROF_SITOUT_LEAF_ON_NODE] / lr,
                w[PRT_PROF_SITOUT_LEAF_DONE] / lr, w[PRT_PROF_SITOUT_LEAF_NO_RAY] / lr, w[PRT_PROF_SITOUT_LEAF_UPDATES] / lr, w[PRT_PROF_SITOUT_NODE_DISTINCT] / nr);
    }
    for (int m = 0; m < PRT_STAT_MODES; m++) {
        const unsigned long long* w = h + prt_prof_turn(m, 0);
        const double turns = nz(h[prt_stat_mode(m, PRT_PROF_LOOP_TURNS)]);
        fprintf(stderr, "  mode %d cycles per loop turn: refill + result hand-off %.0f, entering / leaving BVHs %.0f, step phase %.0f\n", m,
                w[PRT_PROF_TURN_REFILL] * 1024.0 / turns, w[PRT_PROF_TURN_ENTER] * 1024.0 / turns, w[PRT_PROF_TURN_STEP] * 1024.0 / turns);
    }
    if (const unsigned long long n = h[PRT_PROF_SHORT_TURNS])
        fprintf(stderr, "  refills that left lanes empty: %.1f M, %.1f lanes each; at that moment %.1f rays in the block's OTHER queues, %.1f groups ready for shading, shade role taken %.2f of the time\n",
                n / 1e6, (double)h[PRT_PROF_SHORT_LANES] / n, (double)h[PRT_PROF_SHORT_OTHERS] / n, (double)h[PRT_PROF_SHORT_READY] / n, (double)h[PRT_PROF_SHORT_LOCK] / n);
    if (const unsigned long long n = h[PRT_PROF_BOUNCE_PASSES])
        fprintf(stderr, "  shade passes with a bounce: %.1f M, %.1f of 64 lanes carry a path through it; the shade role is held %.2f of a block's time (sum of its waves' shade shares)\n",
                n / 1e6, (double)h[PRT_PROF_BOUNCE_LANES] / n, 4.0 * h[PRT_PROF_SHADE_CYCLES] / cyc);
    const unsigned long long direct = h[PRT_PROF_DIRECT_INT], byPop = h[PRT_PROF_POP_INT];
    fprintf(stderr, "  node steps that leave a lane on an internal record outside the hot set: %.2f G by descending from the parent, %.2f G by a pop (%.2f of them direct)\n",
            direct / 1e9, byPop / 1e9, (double)direct / nz(direct + byPop));
    fprintf(stderr, "  cooperative leaf rounds in which a candidate of a leaf with alpha-tested triangles came up: %.1f M, %.0f cycles each from the candidate test to the end of the alpha tests = %.1f Gcycles of wave time\n",
            h[PRT_PROF_ALPHA_ROUNDS] / 1e6, h[PRT_PROF_ALPHA_CYCLES] * 1024.0 / nz(h[PRT_PROF_ALPHA_ROUNDS]), h[PRT_PROF_ALPHA_CYCLES] * 1024.0 / 1e9);
    unsigned long long pops = 0;
    for (int m = 1; m < PRT_STAT_MODES; m++) pops += h[prt_prof_rounds(m, PRT_PROF_ROUNDS_POPS)];
    fprintf(stderr, "  stack pops of modes 1-3: %.1f G, of them from the spill area in HBM: %.2f G\n", pops / 1e9, h[prt_prof_rounds(0, PRT_PROF_ROUNDS_POPS)] / 1e9);
    fprintf(stderr, "  claims %.1f M, empty %.1f M; shade passes %.1f M with %.2f groups each\n", h[PRT_PROF_CLAIMS] / 1e6, h[PRT_PROF_EMPTY_CLAIMS] / 1e6,
            h[PRT_PROF_SHADE_PASSES] / 1e6, (double)h[PRT_PROF_SHADE_GROUPS] / nz(h[PRT_PROF_SHADE_PASSES]));
}
constexpr bool prt_stat_mode_words_valid = false; // words 16 .. 27 hold the loop statistics, not the counting build's events per mode

#else // the product: every hook is empty
#define PRT_STAT_STRIDE 32 // (copies 256 B apart)

// (static: an empty hook does not even take the address of its object.  With a `this` the object is a stack slot until the optimiser
// removes it, and that was enough to renumber registers in trace_queue; as it is, the product's code is that of a tree without hooks.)
struct TraceTally {
    __device__ __forceinline__ static void pop(bool) {}
    __device__ __forceinline__ static void round(bool, uint32_t, bool, bool, bool, bool, uint32_t, uint32_t, bool) {}
    __device__ __forceinline__ static void node_begin(int) {}
    __device__ __forceinline__ static void node_end(bool, int) {}
    __device__ __forceinline__ static void leaf_pairs(uint32_t) {}
    __device__ __forceinline__ static void alpha_begin() {}
    __device__ __forceinline__ static void alpha_end(bool, bool) {}
    __device__ __forceinline__ static void leaf_update() {}
};
struct QueueProfile {
    __device__ __forceinline__ static QueueProfile start() { return QueueProfile{}; }
    __device__ __forceinline__ static void turn_begin() {}
    template <int MODE, class BL>
    __device__ __forceinline__ static void refill(BL, unsigned long long, bool) {}
    __device__ __forceinline__ static void handed_off() {}
    __device__ __forceinline__ static void turn(bool) {}
    __device__ __forceinline__ static void entered(int) {}
    __device__ __forceinline__ static void stepped(int) {}
    template <int MODE>
    __device__ __forceinline__ static void flush(unsigned long long*, const TraceTally&) {}
};
struct FrameProfile {
    __device__ __forceinline__ static FrameProfile start() { return FrameProfile{}; }
    __device__ __forceinline__ static void decided() {}
    __device__ __forceinline__ static void shaded() {}
    __device__ __forceinline__ static void traced() {}
    __device__ __forceinline__ static void flush(unsigned long long*) {}
    __device__ __forceinline__ static void bounce(unsigned long long*, bool) {}
    __device__ __forceinline__ static void shade_pass_done(unsigned long long*, uint32_t) {}
};
inline void prt_profile_report(const unsigned long long*) {}
constexpr bool prt_stat_mode_words_valid = true;

#endif

__device__ __forceinline__ unsigned long long* prt_stat_copy(unsigned long long* counters)
{
    return counters + (size_t)(blockIdx.x % PRT_STAT_SHARDS) * PRT_STAT_STRIDE;
}
