// ref_glue.cpp -- lets the compiled reference's path_tracer.cpp / scene.cpp / bvh.cpp run end to end WITHOUT its texture.cpp,
// material.cpp, mesh.cpp and image.cpp (ref_path, ref_path_stats), and hands scenes and images over in both builds.
//
// TEST INFRASTRUCTURE ONLY.  The members below "forwarding members" have the reference's declarations and forward to the ORACLE's
// restatement (prt_oracle.c) -- this file contains no reference code.  A `ref_path render` therefore pins the oracle's bounce loop,
// traversal, camera and RNG against the reference's compiled code while surface fetch and material / texture sampling in that run are
// the oracle's own.  With -DREF_REAL_TUS (ref_path_real, oracle/Makefile) those members are compiled out and the reference's own four
// objects -- built against the stand-in declarations of oracle/shim/ext/ -- serve the render: rows a12 / a14 are then the reference's
// too, and tests/test_hostile_taps_cpu.py checks that the committed fixtures come out the same.  The bookkeeping above the switch
// (the hand-made Image, the mesh registry the forwarding getSurfaceProperties looks its oracle mesh up in) stays in both.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <cmath>
#include <vector>
#include <string>
#include <atomic>
#include <deque>
#include <mutex>
#include <condition_variable>
#include <functional>
#include <thread>
#include <random>
#include <limits>
#include <map>

#define private public
#define protected public
#include "vecmath.h"
#include "ray.h"
#include "mesh.h"
#include "material.h"
#include "texture.h"
#include "bvh.h"
#include "image.h"
#undef private
#undef protected

#include "ref_glue.h"

namespace {
std::map<const void*, const orc_mesh*> g_meshByPositions; // Mesh objects move; their position buffer does not
}

void refGlueRegister(const std::vector<prt::Bvh*>& bvhs, const std::vector<orc_mesh*>& omeshes)
{
    for (size_t i = 0; i < bvhs.size(); i++) g_meshByPositions[(const void*)bvhs[i]->m_mesh.m_positions] = omeshes[i];
}

prt::Image* refGlueMakeImage(uint32_t width, uint32_t height, float exposure)
{
    // Image's constructor and virtual destructor live in image.cpp; build the object by hand.
    prt::Image* im = (prt::Image*)calloc(1, sizeof(prt::Image));
    im->m_pixels = (float*)calloc((size_t)width * height * 3, sizeof(float));
    im->m_width = width;
    im->m_height = height;
    im->m_tonemap = true;
    im->m_exposure = exposure;
    return im;
}

const float* refGlueImagePixels(const prt::Image* image) { return image->m_pixels; }

#ifndef REF_REAL_TUS // ---- the forwarding members; compiled out where the reference's own four TUs are linked (ref_path_real)
namespace prt {

// image.cpp:44-50
void Image::writePixel(uint32_t x, uint32_t y, const Vector3f& color)
{
    float* p = m_pixels + ((size_t)x + (size_t)y * m_width) * 3;
    p[0] = m_exposure * color.x;
    p[1] = m_exposure * color.y;
    p[2] = m_exposure * color.z;
}

// mesh.cpp:311-370 -> oracle get_surface
template<>
void Mesh::getSurfaceProperties<SurfaceProperties, RayHit>(SurfaceProperties& prop, const RayHit& hit) const
{
    auto it = g_meshByPositions.find((const void*)m_positions);
    if (it == g_meshByPositions.end()) { fprintf(stderr, "ref_glue: unregistered mesh\n"); abort(); }
    uint32_t mat = 0;
    orc_x_get_surface(it->second, hit.primId, hit.i, hit.j, hit.k, &prop.normal.x, &mat, &prop.uv.x, &prop.duv01.x,
                      &prop.duv02.x, &prop.dp01.x, &prop.dp02.x);
    prop.material = &m_materials[mat];
}

// material.cpp:87-96
Vector3f Material::sampleDiffuse(const Vector2f& uv) const
{
    Vector3f out;
    orc_x_sample_diffuse(&diffuse.x, diffuseMap.width, diffuseMap.height, diffuseMap.component,
                         (const uint8_t*)diffuseMap.texels, uv.x, uv.y, &out.x);
    return out;
}

// material.cpp:98-114
Vector3f Material::sampleBump(const SurfaceProperties& prop) const
{
    Vector3f out;
    orc_x_sample_bump(&prop.normal.x, bumpMap.width, bumpMap.height, bumpMap.component, (const uint8_t*)bumpMap.texels,
                      &prop.uv.x, &prop.duv01.x, &prop.duv02.x, &prop.dp01.x, &prop.dp02.x, &out.x);
    return out;
}

// texture.cpp:142-156
bool Texture::testAlpha(const Vector2f& uv) const
{
    return orc_x_tex_test_alpha(width, height, component, (const uint8_t*)texels, uv.x, uv.y, 0) != 0;
}

// texture.cpp:158-183
SoaMask Texture::testAlpha(const SoaMask& mask, const SoaVector2f& uv) const
{
    int32_t bits = mask.ballot(), res = 0;
    for (int l = 0; l < SoaConstants::kLaneCount; l++) {
        if (!((bits >> l) & 1)) continue;
        Vector2f v = uv.getLane(l);
        if (orc_x_tex_test_alpha(width, height, component, (const uint8_t*)texels, v.x, v.y, 1)) res |= 1 << l;
    }
    return SoaMask(res);
}

// ---- what light.cpp (built from the reference, InfiniteAreaLight::create/sample) needs from texture.cpp
// texture.cpp:88-139, k32Float branch
template <>
Vector3f Texture::sample<Vector3f>(const Vector2f& uv) const
{
    if (channel != TextureChannel::k32Float) { fprintf(stderr, "ref_glue: sample<Vector3f> on a non-float texture\n"); abort(); }
    Vector3f out;
    orc_x_tex_sample3f(width, height, component, (const float*)texels, uv.x, uv.y, &out.x);
    return out;
}

// texture.cpp:256-310 decodes an OpenEXR file with tinyexr (not in this image).  The harness hands the float RGBA texels
// over in a raw file instead -- "PRTE", i32 width, i32 height, width*height*4 f32 -- and this keeps the field bookkeeping
// of :303-310 (component 4, k32Float).
void Texture::loadExr(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "ref_glue: cannot open %s\n", path); abort(); }
    char magic[4];
    int32_t w = 0, h = 0;
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "PRTE", 4) || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1) abort();
    float* p = (float*)malloc((size_t)w * h * 16);
    if (fread(p, 16, (size_t)w * h, f) != (size_t)w * h) abort();
    fclose(f);
    texels = p;
    component = 4;
    width = w;
    height = h;
    format = 0;
    channel = TextureChannel::k32Float;
}

// ---- what sample_models.cpp needs to hand over the Cornell box data (mesh.cpp:23-104, 302-309;
// material.cpp:30-43; texture.cpp:202-210): allocation and field bookkeeping only.
void Texture::init()
{
    width = 0; height = 0; format = 0; component = 0;
    channel = TextureChannel::k8Unorm;
    texels = nullptr;
}

void Material::init()
{
    diffuse = Vector3f(0.0f); ambient = Vector3f(0.0f); specular = Vector3f(0.0f); emissive = Vector3f(0.0f);
    diffuseMap.init(); ambientMap.init(); specularMap.init(); emissiveMap.init(); bumpMap.init();
    reflectionType = ReflectionType::kDiffuse;
    alphaTest = false;
}

Mesh::Mesh(Mesh&& m) { memcpy((void*)this, (void*)&m, sizeof(Mesh)); memset((void*)&m, 0, sizeof(Mesh)); }
Mesh& Mesh::operator=(Mesh&& m)
{
    // keep this object's vptr; take the fields
    memcpy((char*)this + sizeof(void*), (char*)&m + sizeof(void*), sizeof(Mesh) - sizeof(void*));
    memset((char*)&m + sizeof(void*), 0, sizeof(Mesh) - sizeof(void*));
    return m;
}
Mesh::~Mesh() {}

void Mesh::create(uint32_t primCount, uint32_t vertexCount, uint32_t materialCount, bool hasVertexNormal)
{
    m_indexCount = primCount * kVertexCountPerPrim;
    m_indices = new uint32_t[m_indexCount];
    m_texcoordIndices = new uint32_t[m_indexCount];
    m_positions = new Vector3f[vertexCount];
    m_texcoords = new Vector2f[vertexCount];
    if (hasVertexNormal) m_normals = new Vector3f[vertexCount];
    m_primMaterial = new uint32_t[primCount];
    m_materials = (Material*)calloc(materialCount, sizeof(Material));
    m_vertexCount = vertexCount;
    m_materialCount = materialCount;
    m_hasVertexNormal = hasVertexNormal;
}

void Mesh::calculateBounds()
{
    BBox bbox = BBox::init();
    for (uint32_t i = 0; i < m_vertexCount; i++) bbox.merge(m_positions[i]);
    m_bbox = bbox;
}

} // namespace prt
#endif // REF_REAL_TUS
