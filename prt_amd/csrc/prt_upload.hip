// prt_upload.hip -- prt_hip_upload_scene: flattens a scene description into the device arrays of DevScene (prt_device.h) and decides
// where the leaves' triangles lie in them.  Host code only: no kernel is defined or launched here, so that the frame kernels' code
// objects (prt_kernels.hip) do not move when it changes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "prt_internal.h"

namespace {

int fail(int code, const std::string& msg) { return prt_fail(code, msg); }

struct HVec3 { float x, y, z; };
inline HVec3 hsub(HVec3 a, HVec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline HVec3 hcross(HVec3 a, HVec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline HVec3 hnormalize(HVec3 v) // vecmath.h:1200 -- same operations as the device's normalize3
{
    float d = v.x * v.x + v.y * v.y + v.z * v.z;
    float invlen = 1.0f / sqrtf(d);
    return {invlen * v.x, invlen * v.y, invlen * v.z};
}
inline void hsafe_normalize2(float x, float y, float* ox, float* oy) // vecmath.h:1145
{
    float len = sqrtf(x * x + y * y);
    if (len < 0.00001f) { *ox = 0.0f; *oy = 0.0f; return; }
    float invlen = 1.0f / len;
    *ox = invlen * x;
    *oy = invlen * y;
}
inline float ubits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

} // namespace

void prt_scene_view(prt_hip_ctx* c)
{
    const PrtSceneArrays& a = c->arr;
    DevScene& sc = c->sc;
    sc.wnodes = a.wnodes;
    sc.hotNodes = a.hotNodes;
    sc.tris = a.tris;
    sc.triAlpha = a.triAlpha;
    sc.triPrim = a.triPrim;
    sc.shade = a.shade;
    sc.bump = a.bump;
    sc.mats = a.mats;
    sc.alpha = a.alpha;
    sc.alphaClass = a.alphaClass;
    sc.texDesc = a.texDesc;
    sc.texels = a.texels;
    sc.envTexels = a.envTexels;
    sc.envV = a.envV;
    sc.envHor = a.envHor;
    sc.envFirstX = a.envFirstX;
}

void prt_free_scene(prt_hip_ctx* c)
{
    c->arr = PrtSceneArrays{};
    prt_refit_forget(c);
    c->qInv.release(); // the inverse triangle table is the scene's (prt_query.hip)
    c->ed = PrtEdit{};
    prt_scene_view(c); // (every pointer null)
    c->haveScene = false;
}

// Where the triangles of a mesh's leaves lie in the device arrays.  The reference keeps them in primRemapping order (leaf after leaf,
// depth first); a leaf of n triangles is n * 36 contiguous bytes here, fetched by the n pair lanes of a cooperative leaf round at
// once.  Beyond the caches such a fetch costs one DRAM row activation per 128-byte LINE it touches, whatever part of the line it
// reads (profiles/r03_rec_gather.txt), and a leaf that starts at an arbitrary multiple of 36 bytes touches more lines than
// ceil(36 n / 128) (C4's tree: 2.64 per leaf where 2.15 would do).  A leaf reference carries its first slot, so a leaf may start
// up to PRT_LEAF_PADS unused slots later when that saves it a line (two pads: 2.22 lines per leaf for 12 % more slots).  Results
// are unchanged: a hit's slot index is internal, and the shade, bump, alpha and primId records follow the slots.
// slotOf[k] = slot (within the mesh) of leaf-order index k; returns the number of slots (primCount when nothing is padded).
#ifndef PRT_LEAF_PADS
#define PRT_LEAF_PADS 2 // (C5 share 1480 -> 1408 ms, C4 834 -> 816, C3 unchanged; 0: 2.64, 1: 2.39, 2: 2.22, 3: 2.20 lines per leaf on C4's tree)
#endif
static uint32_t leaf_slots(const prt_mesh_desc& md, uint32_t triBase, std::vector<uint32_t>& slotOf)
{
    slotOf.resize(md.primCount);
    for (uint32_t k = 0; k < md.primCount; k++) slotOf[k] = k;
    if (PRT_LEAF_PADS <= 0) return md.primCount;
    std::vector<uint8_t> covered(md.primCount, 0);
    for (uint32_t i = 0; i < md.nodeCount; i++) {
        const prt_bvh_node& n = md.nodes[i];
        if (n.primCount == 0xf) continue;
        for (uint32_t t = 0; t < n.primCount; t++) {
            if (covered[n.primOrSecondNodeIndex + t]) return md.primCount; // two leaves share a triangle: keep the reference's layout
            covered[n.primOrSecondNodeIndex + t] = 1;
        }
    }
    for (uint32_t k = 0; k < md.primCount; k++)
        if (!covered[k]) return md.primCount;
    auto excess = [&](uint32_t slot, uint32_t n) { // lines touched from this slot beyond the fewest a leaf of n triangles can touch
        const uint32_t o = (uint32_t)(((uint64_t)(triBase + slot) * 36u) & 127u);
        return (o + 36u * n + 127u) / 128u - (36u * n + 127u) / 128u;
    };
    // leaves in the order of their first triangle (= depth-first order for the reference's builder)
    std::vector<std::pair<uint32_t, uint32_t>> leaves;
    for (uint32_t i = 0; i < md.nodeCount; i++)
        if (md.nodes[i].primCount != 0xf) leaves.push_back({md.nodes[i].primOrSecondNodeIndex, md.nodes[i].primCount});
    std::sort(leaves.begin(), leaves.end());
    uint32_t cursor = 0;
    for (const auto& L : leaves) {
        uint32_t best = 0, bestEx = excess(cursor, L.second);
        for (uint32_t p = 1; p <= (uint32_t)PRT_LEAF_PADS && bestEx != 0u; p++) {
            const uint32_t e = excess(cursor + p, L.second);
            if (e < bestEx) {
                best = p;
                bestEx = e;
            }
        }
        cursor += best;
        for (uint32_t t = 0; t < L.second; t++) slotOf[L.first + t] = cursor + t;
        cursor += L.second;
    }
    return cursor;
}

extern "C" {

// Flattens Scene -> Bvh -> Mesh (scene.h:61-71, bvh.h:113-119, mesh.h:87-104) into the arrays of DevScene.
int prt_hip_upload_scene(prt_hip_ctx* c, const prt_scene_desc* s)
{
    if (!c || !s) return fail(PRT_HIP_EINVAL, "NULL argument");
    if (s->meshCount == 0 || s->meshCount > PRT_MAX_BVH) return fail(PRT_HIP_EINVAL, "meshCount must be 1..8");
    HIP_TRY(hipSetDevice(c->device));
    prt_free_scene(c);
    prt_accum_forget(c); // the accumulated samples were of the old scene
    prt_denoise_forget(c);
    prt_temporal_forget(c);

    std::vector<float4> wnodes, shade, bump, mats, alpha;
    std::vector<float> tris;                 // 9 floats per triangle, leaf order
    std::vector<uint32_t> triAlpha, triPrim; // per triangle, leaf order
    std::vector<uint32_t> alphaClass;        // 2 bits per bilinear cell of every alpha-tested texture (prt_device.h DevScene::alphaClass)
    std::vector<uint32_t> classWordOf;       // per texture: first word of its cell classes in alphaClass, 0xffffffff = not built yet
    std::vector<uint4> texDesc;
    std::vector<uint8_t> texels;
    std::vector<uint32_t> slotVtx;           // 3 vertex ids per triangle slot, for prt_hip_update_meshes (prt_refit.hip)
    std::vector<PrtRefitMesh> refitMeshes;
    std::vector<uint32_t> hotOrder;
    PrtEdit ed;
    PrtSceneArrays arr; // the context's once everything is on the device: a failed upload frees what it had allocated
    DevScene sc{};      // (its pointers stay null: prt_scene_view)
    sc.bvhCount = s->meshCount;

    for (uint32_t t = 0; t < s->textureCount; t++) {
        const prt_texture_desc& td = s->textures[t];
        if (td.width <= 0 || td.height <= 0 || td.component <= 0 || !td.texels) return fail(PRT_HIP_EINVAL, "bad texture");
        size_t off = (texels.size() + 15) & ~(size_t)15;
        size_t sz = (size_t)td.width * td.height * td.component;
        texels.resize(off + sz + 16, 0);
        memcpy(&texels[off], td.texels, sz);
        texDesc.push_back(make_uint4((uint32_t)off, (uint32_t)td.width, (uint32_t)td.height, (uint32_t)td.component));
    }

    classWordOf.assign(s->textureCount, 0xffffffffu);
    // Cell classes of texture t (built when the first alpha-tested material names it).  The tap of Texture::testAlpha at a uv in cell
    // (x0, y0) blends the alpha bytes of (x0, y0), (x1, y0), (x0, y1), (x1, y1), x1 = min(x0 + 1, w - 1), with weights >= 0 that sum to 1
    // up to rounding (texture.cpp:31-100): four bytes >= 128 give more than 127 whatever the weights, four bytes <= 126 give less
    // (the blend is off 128 x sum(k) by < 1e-4); a cell with a byte of 127, or with bytes on both sides, is left to the blend itself.
    auto classWord = [&](uint32_t t) -> uint32_t {
        if (classWordOf[t] != 0xffffffffu) return classWordOf[t];
        const uint4 d = texDesc[t];
        const int32_t w = (int32_t)d.y, h = (int32_t)d.z, comp = (int32_t)d.w;
        const uint8_t* px = texels.data() + d.x;
        const uint32_t first = (uint32_t)alphaClass.size();
        alphaClass.resize(first + ((size_t)w * h + 15) / 16, 0u);
        for (int32_t y0 = 0; y0 < h; y0++) {
            const int32_t y1 = (y0 + 1 < h - 1) ? y0 + 1 : h - 1;
            for (int32_t x0 = 0; x0 < w; x0++) {
                const int32_t x1 = (x0 + 1 < w - 1) ? x0 + 1 : w - 1;
                const uint32_t a[4] = {px[comp * (x0 + y0 * w) + 3], px[comp * (x1 + y0 * w) + 3], px[comp * (x0 + y1 * w) + 3], px[comp * (x1 + y1 * w) + 3]};
                const uint32_t lo = std::min(std::min(a[0], a[1]), std::min(a[2], a[3])), hi = std::max(std::max(a[0], a[1]), std::max(a[2], a[3]));
                const uint32_t cls = lo >= 128u ? 1u : (hi <= 126u ? 2u : 0u);
                const uint32_t cell = (uint32_t)x0 + (uint32_t)y0 * (uint32_t)w;
                alphaClass[first + (cell >> 4)] |= cls << ((cell & 15u) * 2u);
            }
        }
        return classWordOf[t] = first;
    };

    bool anyBump = false;
    for (uint32_t m = 0; m < s->meshCount; m++)
        for (uint32_t k = 0; k < s->meshes[m].materialCount; k++)
            if (s->meshes[m].materials[k].bumpMap >= 0) anyBump = true;

    for (uint32_t m = 0; m < s->meshCount; m++) {
        const prt_mesh_desc& md = s->meshes[m];
        if (!md.nodes || !md.primRemapping || !md.indices || !md.positions || !md.primMaterial || !md.materials || md.nodeCount == 0)
            return fail(PRT_HIP_EINVAL, "mesh descriptor has NULL arrays");
        const uint32_t triBase = (uint32_t)(tris.size() / 9);
        const uint32_t primBase = (uint32_t)(shade.size() / 4), matBase = (uint32_t)(mats.size() / PRT_MAT_STRIDE);
        sc.primBase[m] = primBase;
        ed.meshes.push_back(PrtEditMesh{matBase, std::vector<prt_material>(md.materials, md.materials + md.materialCount)});
        sc.hasNormals[m] = md.normals ? 1u : 0u;
        auto P = [&](uint32_t v) { return HVec3{md.positions[3 * v], md.positions[3 * v + 1], md.positions[3 * v + 2]}; };
        for (uint32_t k = 0; k < md.materialCount; k++) {
            const prt_material& mt = md.materials[k];
            if (mt.diffuseMap >= (int32_t)s->textureCount || mt.bumpMap >= (int32_t)s->textureCount)
                return fail(PRT_HIP_EINVAL, "material texture index out of range");
            if (mt.alphaTest && mt.diffuseMap < 0) return fail(PRT_HIP_EINVAL, "alphaTest material without a diffuse map");
            float4 record[PRT_MAT_STRIDE]; // (prt_internal.h: the one writer of a material record)
            prt_material_record(mt, texDesc, record);
            mats.insert(mats.end(), record, record + PRT_MAT_STRIDE);
        }
        std::vector<uint32_t> slotOf, kOfSlot; // leaf-order index <-> slot in the device arrays (leaf_slots)
        uint32_t slotCount = md.primCount;
        // Wide records: one per internal node, in the reference's DFS order.  wideIndex[i] = record of node i.
        {
            std::vector<uint32_t> wideIndex(md.nodeCount, 0);
            uint32_t nextWide = (uint32_t)(wnodes.size() / 4);
            for (uint32_t i = 0; i < md.nodeCount; i++) {
                const prt_bvh_node& n = md.nodes[i];
                if (n.primCount == 0xf) {
                    if (n.primOrSecondNodeIndex >= md.nodeCount || n.primOrSecondNodeIndex <= i || i + 1 >= md.nodeCount)
                        return fail(PRT_HIP_EINVAL, "bad child index");
                    wideIndex[i] = nextWide++;
                } else if (n.primCount == 0 || n.primCount > 8 || n.primOrSecondNodeIndex + n.primCount > md.primCount) {
                    return fail(PRT_HIP_EINVAL, "bad leaf range");
                }
            }
            if ((size_t)triBase + md.primCount >= (1u << PRT_COOP_TRI_BITS) || nextWide >= (1u << 30)) return fail(PRT_HIP_EINVAL, "scene too large for 32-bit child references"); // (a pair-table word holds a triangle index in 26 bits)
            slotCount = leaf_slots(md, triBase, slotOf);
            if ((size_t)triBase + slotCount >= (1u << PRT_COOP_TRI_BITS)) return fail(PRT_HIP_EINVAL, "scene too large for 32-bit child references");
            kOfSlot.assign(slotCount, 0xffffffffu); // (an unused slot between two leaves: no leaf reference reaches it)
            for (uint32_t k = 0; k < md.primCount; k++) kOfSlot[slotOf[k]] = k;
            auto refOf = [&](uint32_t i) -> uint32_t {
                const prt_bvh_node& n = md.nodes[i];
                if (n.primCount == 0xf) return wideIndex[i];
                bool anyAlpha = false; // some triangle of the leaf is alpha-tested: its candidates look their alpha record up
                for (uint32_t k = 0; k < n.primCount; k++) {
                    const uint32_t prim = md.primRemapping[n.primOrSecondNodeIndex + k];
                    if (prim < md.primCount && md.primMaterial[prim] < md.materialCount && md.materials[md.primMaterial[prim]].alphaTest) anyAlpha = true;
                }
                return PRT_REF_LEAF | ((triBase + slotOf[n.primOrSecondNodeIndex]) << 4) | (anyAlpha ? PRT_LEAF_ALPHA : 0u) | (n.primCount - 1u);
            };
            for (uint32_t i = 0; i < md.nodeCount; i++) {
                const prt_bvh_node& n = md.nodes[i];
                if (n.primCount != 0xf) continue;
                const prt_bvh_node& c0 = md.nodes[i + 1];
                const prt_bvh_node& c1 = md.nodes[n.primOrSecondNodeIndex];
                wnodes.push_back(make_float4(c0.lower[0], c0.upper[0], c0.lower[1], c0.upper[1])); // x and y of child 0
                wnodes.push_back(make_float4(c0.lower[2], c0.upper[2], c1.lower[2], c1.upper[2])); // z of both children
                wnodes.push_back(make_float4(c1.lower[0], c1.upper[0], c1.lower[1], c1.upper[1])); // x and y of child 1
                wnodes.push_back(make_float4(ubits(refOf(i + 1)), ubits(refOf(n.primOrSecondNodeIndex)), ubits(n.splitAxis & 3u), 0.0f));
            }
            sc.rootRef[m] = refOf(0);
            memcpy(&sc.rootBox[m][0], md.nodes[0].lower, 12);
            memcpy(&sc.rootBox[m][3], md.nodes[0].upper, 12);
        }
        // leaf triangles in primRemapping order (TriangleVector, bvh.cpp:245-296), leaf blocks placed by leaf_slots
        for (uint32_t slot = 0; slot < slotCount; slot++) {
            if (kOfSlot[slot] == 0xffffffffu) {
                tris.insert(tris.end(), 9, 0.0f);
                triAlpha.push_back(0u);
                triPrim.push_back(0u);
                slotVtx.insert(slotVtx.end(), 3, 0xffffffffu);
                continue;
            }
            uint32_t prim = md.primRemapping[kOfSlot[slot]];
            if (prim >= md.primCount) return fail(PRT_HIP_EINVAL, "bad primRemapping");
            uint32_t v0 = md.indices[3 * prim], v1 = md.indices[3 * prim + 1], v2 = md.indices[3 * prim + 2];
            if (v0 >= md.vertexCount || v1 >= md.vertexCount || v2 >= md.vertexCount) return fail(PRT_HIP_EINVAL, "bad vertex index");
            if (md.primMaterial[prim] >= md.materialCount) return fail(PRT_HIP_EINVAL, "bad material index");
            const prt_material& mt = md.materials[md.primMaterial[prim]];
            uint32_t alphaRef = 0;
            if (mt.alphaTest) {
                // leaf uv are the mesh texcoord buffer by vertex index (bvh.cpp:266-269), zero if there is none
                float u[6] = {0, 0, 0, 0, 0, 0};
                if (md.texcoords) {
                    u[0] = md.texcoords[2 * v0]; u[1] = md.texcoords[2 * v0 + 1];
                    u[2] = md.texcoords[2 * v1]; u[3] = md.texcoords[2 * v1 + 1];
                    u[4] = md.texcoords[2 * v2]; u[5] = md.texcoords[2 * v2 + 1];
                }
                const uint4 ad = texDesc[mt.diffuseMap];
                alpha.push_back(make_float4(u[0], u[1], u[2], u[3]));
                alpha.push_back(make_float4(u[4], u[5], ubits((uint32_t)mt.diffuseMap), ubits(classWord((uint32_t)mt.diffuseMap))));
                alpha.push_back(make_float4(ubits(ad.x), ubits(ad.y), ubits(ad.z), ubits(ad.w)));
                alphaRef = (uint32_t)(alpha.size() / 3);
            }
            HVec3 p0 = P(v0), p1 = P(v1), p2 = P(v2);
            const float corners[9] = {p0.x, p0.y, p0.z, p1.x, p1.y, p1.z, p2.x, p2.y, p2.z};
            tris.insert(tris.end(), corners, corners + 9);
            slotVtx.insert(slotVtx.end(), {v0, v1, v2});
            triAlpha.push_back(alphaRef);
            triPrim.push_back(prim);
        }
        {
            PrtRefitMesh rm;
            rm.slotBase = triBase;
            rm.slotCount = slotCount;
            rm.vertexCount = md.vertexCount;
            rm.primCount = md.primCount;
            rm.hasNormals = md.normals ? 1u : 0u;
            // Mesh::calculateBounds (mesh.cpp:302-309): over ALL vertices, for the radius of prt_hip_deform_meshes (prt_deform.hip)
            for (int j = 0; j < 3; j++) {
                rm.vbox[j] = std::numeric_limits<float>::max();
                rm.vbox[3 + j] = std::numeric_limits<float>::lowest();
            }
            for (uint32_t v = 0; v < md.vertexCount; v++)
                for (int j = 0; j < 3; j++) {
                    rm.vbox[j] = std::fmin(rm.vbox[j], md.positions[3 * v + j]);
                    rm.vbox[3 + j] = std::fmax(rm.vbox[3 + j], md.positions[3 * v + j]);
                }
            rm.vboxValid = true;
            refitMeshes.push_back(std::move(rm));
        }
        // shading records (Mesh::getSurfaceProperties, mesh.cpp:311-364) in LEAF order, like the triangles: a hit names its
        // triangle by that index
        for (uint32_t slot = 0; slot < slotCount; slot++) {
            if (kOfSlot[slot] == 0xffffffffu) {
                shade.insert(shade.end(), 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
                if (anyBump) bump.insert(bump.end(), 3, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
                continue;
            }
            const uint32_t prim = md.primRemapping[kOfSlot[slot]];
            uint32_t v0 = md.indices[3 * prim], v1 = md.indices[3 * prim + 1], v2 = md.indices[3 * prim + 2];
            HVec3 p0 = P(v0), p1 = P(v1), p2 = P(v2);
            HVec3 n0, n1{0, 0, 0}, n2{0, 0, 0};
            if (md.normals) {
                n0 = {md.normals[3 * v0], md.normals[3 * v0 + 1], md.normals[3 * v0 + 2]};
                n1 = {md.normals[3 * v1], md.normals[3 * v1 + 1], md.normals[3 * v1 + 2]};
                n2 = {md.normals[3 * v2], md.normals[3 * v2 + 1], md.normals[3 * v2 + 2]};
            } else {
                n0 = hnormalize(hcross(hsub(p1, p0), hsub(p2, p0))); // mesh.cpp:335
            }
            float t[6] = {0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f}; // mesh.cpp:351-353
            if (md.texcoords) {
                t[0] = md.texcoords[2 * v0]; t[1] = md.texcoords[2 * v0 + 1];
                t[2] = md.texcoords[2 * v1]; t[3] = md.texcoords[2 * v1 + 1];
                t[4] = md.texcoords[2 * v2]; t[5] = md.texcoords[2 * v2 + 1];
            }
            shade.push_back(make_float4(n0.x, n0.y, n0.z, ubits(matBase + md.primMaterial[prim])));
            shade.push_back(make_float4(n1.x, n1.y, n1.z, t[0]));
            shade.push_back(make_float4(n2.x, n2.y, n2.z, t[1]));
            shade.push_back(make_float4(t[2], t[3], t[4], t[5]));
            if (anyBump) {
                HVec3 dp01 = hnormalize(hsub(p1, p0)), dp02 = hnormalize(hsub(p2, p0)); // mesh.cpp:360-361
                float d01x, d01y, d02x, d02y;
                hsafe_normalize2(t[2] - t[0], t[3] - t[1], &d01x, &d01y);
                hsafe_normalize2(t[4] - t[0], t[5] - t[1], &d02x, &d02y);
                bump.push_back(make_float4(dp01.x, dp01.y, dp01.z, d01x));
                bump.push_back(make_float4(dp02.x, dp02.y, dp02.z, d01y));
                bump.push_back(make_float4(d02x, d02y, 0.0f, 0.0f));
            }
        }
    }
    // The PRT_HOT_NODES records nearest to the roots, breadth first over the BVHs in order; references to them become
    // PRT_REF_HOT | slot everywhere (parents' records, root references), and `hot` holds copies of the rewritten records.
    std::vector<float4> hot((size_t)PRT_HOT_NODES * 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    {
        auto bitsOf = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
        std::vector<uint32_t> order; // record indices, breadth first
        for (uint32_t m = 0; m < sc.bvhCount; m++)
            if (!(sc.rootRef[m] & PRT_REF_LEAF)) order.push_back(sc.rootRef[m]);
        for (size_t head = 0; head < order.size() && order.size() < PRT_HOT_NODES; head++) {
            const float4& refs = wnodes[(size_t)order[head] * 4 + 3];
            for (uint32_t r : {bitsOf(refs.x), bitsOf(refs.y)})
                if (!(r & PRT_REF_LEAF) && order.size() < PRT_HOT_NODES) order.push_back(r);
        }
        std::vector<uint32_t> slotOf(wnodes.size() / 4, 0xffffffffu);
        for (size_t k = 0; k < order.size(); k++) slotOf[order[k]] = (uint32_t)k;
        auto hotRef = [&](uint32_t r) { return (!(r & PRT_REF_LEAF) && slotOf[r] != 0xffffffffu) ? (PRT_REF_HOT | slotOf[r]) : r; };
        for (size_t rec = 0; rec < wnodes.size() / 4; rec++) {
            float4& refs = wnodes[rec * 4 + 3];
            refs.x = ubits(hotRef(bitsOf(refs.x)));
            refs.y = ubits(hotRef(bitsOf(refs.y)));
        }
        for (uint32_t m = 0; m < sc.bvhCount; m++) sc.rootRef[m] = hotRef(sc.rootRef[m]);
        for (size_t k = 0; k < order.size(); k++) memcpy(&hot[k * 4], &wnodes[(size_t)order[k] * 4], 4 * sizeof(float4));
        hotOrder = order;
    }
    sc.hasLight = s->hasDirectionalLight ? 1u : 0u;
    memcpy(sc.lightDir, s->lightDir, 12);
    memcpy(sc.lightIntensity, s->lightIntensity, 12);
    sc.radius = s->radius;

    int rc;
    // InfiniteAreaLight: texels + CDF tables as they are, plus the "first index that differs from its predecessor" constants
    // of the bisection (prt_device.h cdf_find).  The bisection needs non-decreasing tables: running sums of non-negative terms
    // are, unless the image holds negative, infinite or NaN radiance -- refuse those.
    sc.hasEnv = 0;
    if (s->hasInfiniteAreaLight) {
        const int32_t W = s->envWidth, H = s->envHeight;
        if (W <= 0 || H <= 0 || !s->envTexels || !s->envVerticalP || !s->envHorizontalP) return fail(PRT_HIP_EINVAL, "incomplete environment light");
        if ((int64_t)W * H > (1 << 28)) return fail(PRT_HIP_EINVAL, "environment map too large");
        auto firstStep = [](const float* cdf, int32_t n) {
            for (int32_t i = 1; i < n; i++) {
                float pdf = cdf[i] - cdf[i - 1];
                if (!(pdf == 0.0f)) return i; // light.cpp:96-98, 112-114
            }
            return n;
        };
        auto monotone = [](const float* cdf, int32_t n) {
            for (int32_t i = 1; i < n; i++)
                if (!(cdf[i] >= cdf[i - 1])) return false;
            return true;
        };
        if (!monotone(s->envVerticalP, H)) return fail(PRT_HIP_EINVAL, "environment light: vertical CDF is not non-decreasing (negative or non-finite radiance?)");
        std::vector<int32_t> firstX((size_t)H);
        for (int32_t y = 0; y < H; y++) {
            const float* row = s->envHorizontalP + (size_t)y * W;
            const bool allNaN = row[0] != row[0]; // an all-black row: 0 * inf (light.cpp:63-70); never selected, never exceeds u
            if (allNaN) {
                for (int32_t x = 0; x < W; x++)
                    if (row[x] == row[x]) return fail(PRT_HIP_EINVAL, "environment light: partly NaN CDF row");
            } else if (!monotone(row, W)) {
                return fail(PRT_HIP_EINVAL, "environment light: horizontal CDF is not non-decreasing (negative or non-finite radiance?)");
            }
            firstX[y] = firstStep(row, W);
        }
        std::vector<float4> tex((size_t)W * H);
        memcpy(tex.data(), s->envTexels, tex.size() * sizeof(float4));
        std::vector<float> vp(s->envVerticalP, s->envVerticalP + H), hp(s->envHorizontalP, s->envHorizontalP + (size_t)W * H);
        if ((rc = prt_upload(arr.envTexels, tex, c->stream))) return rc;
        if ((rc = prt_upload(arr.envV, vp, c->stream))) return rc;
        if ((rc = prt_upload(arr.envHor, hp, c->stream))) return rc;
        if ((rc = prt_upload(arr.envFirstX, firstX, c->stream))) return rc;
        sc.envW = W;
        sc.envH = H;
        sc.envFirstY = firstStep(s->envVerticalP, H);
        sc.hasEnv = 1;
    }
    // every texture descriptor a kernel can reach lies inside the texel array (checked here, on the host, once per upload)
    for (const uint4& d : texDesc)
        if ((size_t)d.x + (size_t)d.y * d.z * d.w > texels.size()) return fail(PRT_HIP_EINVAL, "internal: texture descriptor outside the texel array");
    for (size_t k = 0; k + PRT_MAT_STRIDE <= mats.size(); k += PRT_MAT_STRIDE)
        for (int j = 3; j <= 4; j++) {
            const float4& f = mats[k + j];
            uint32_t off, w, h, comp;
            memcpy(&off, &f.x, 4); memcpy(&w, &f.y, 4); memcpy(&h, &f.z, 4); memcpy(&comp, &f.w, 4);
            if ((size_t)off + (size_t)w * h * comp > texels.size()) return fail(PRT_HIP_EINVAL, "internal: material map descriptor outside the texel array");
        }
    if (mats.size() % PRT_MAT_STRIDE != 0) return fail(PRT_HIP_EINVAL, "internal: material table is not a whole number of records");
    if ((rc = prt_upload(arr.wnodes, wnodes, c->stream))) return rc;
    if ((rc = prt_upload(arr.hotNodes, hot, c->stream))) return rc;
    if ((rc = prt_upload(arr.tris, tris, c->stream))) return rc;
    if ((rc = prt_upload(arr.triAlpha, triAlpha, c->stream))) return rc;
    if ((rc = prt_upload(arr.triPrim, triPrim, c->stream))) return rc;
    if ((rc = prt_upload(arr.shade, shade, c->stream))) return rc;
    if ((rc = prt_upload(arr.bump, bump, c->stream))) return rc;
    if ((rc = prt_upload(arr.mats, mats, c->stream))) return rc;
    if ((rc = prt_upload(arr.alpha, alpha, c->stream))) return rc;
    if ((rc = prt_upload(arr.alphaClass, alphaClass, c->stream))) return rc;
    if ((rc = prt_upload(arr.texDesc, texDesc, c->stream))) return rc;
    if ((rc = prt_upload(arr.texels, texels, c->stream))) return rc;
    for (uint32_t m = 0; m < sc.bvhCount; m++) refitMeshes[m].rootKid = sc.rootRef[m];
    if ((rc = prt_refit_build(c, wnodes, hotOrder, std::move(refitMeshes), slotVtx))) {
        prt_refit_forget(c); // (whatever part of it was built)
        return rc;
    }
    c->arr = std::move(arr);
    c->sc = sc;
    prt_scene_view(c);
    ed.texDesc = std::move(texDesc);
    ed.classWordOf = std::move(classWordOf);
    c->ed = std::move(ed);
    c->haveScene = true;
    return PRT_HIP_OK;
}

} // extern "C"
