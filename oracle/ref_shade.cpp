// ref_shade.cpp -- row-level driver of the COMPILED REFERENCE's texture.cpp, material.cpp, mesh.cpp and image.cpp (rows a12 / a14 of
// SURVEY.md 8(a)): Texture::sample / testAlpha / load / loadExr / isAlphaTestRequired, convertNormalToBump, Material::sampleDiffuse /
// sampleBump, Mesh::getSurfaceProperties, Image::savePpm.  It links the reference's real objects (built by oracle/Makefile against the
// stand-in declarations of oracle/shim/ext/) and NONE of ref_glue.cpp's forwarding members: what it writes is the reference's answer.
//
// TEST INFRASTRUCTURE ONLY.  This file contains no reference code.  It includes ref_harness.cpp for the PRTS scene reader and the
// mesh bookkeeping (fillMesh), not for its commands.
//
//   taps    <scene> <rec> <out>   rec: N x {u32 material of mesh 0, f32 u, f32 v, u32 flags}; N a multiple of 8, 8 consecutive records
//                                 name one material.  flags 1: uv finite (the single flavours are defined), 2: the map has 4
//                                 components (the alpha tests are defined).  out: N x 12 words:
//                                 [0..2] diffuseMap.sample<Vector3f>  [3] bumpMap.sample<float>  [4] testAlpha(uv)
//                                 [5] testAlpha(full mask, packet of the 8 records) bit of this lane  [6..8] sampleDiffuse  [9..11] 0
//   tapsf   <prte> <rec> <out>    Texture::loadExr, then sample<Vector3f> of N x {f32 u, v} -> N x 3 f32
//   bump    <scene> <rec> <out>   rec: N x 16 words {u32 material of mesh 0, normal[3], uv[2], duv01[2], duv02[2], dp01[3], dp02[3]} -> N x 3 f32
//   surface <scene> <rec> <out>   rec: N x {u32 mesh, u32 prim, f32 i, j, k}; out: N x 20 words: normal[3] uv[2] material index
//                                 duv01[2] duv02[2] dp01[3] dp02[3], sampleBump's normal [3], 0
//   ppm     <w> <h> <tonemap> <in: f32 rgb> <out.ppm>      Image::savePpm of a float image
//   load    <prti> <bump 0|1> <out>   Texture::load through the raw-texel stbi_load of ref_stubs.cpp; out: i32 width, height, component,
//                                 isAlphaTestRequired (0 unless component is 4), then the texels
//   bump24  <out>                 convertNormalToBump on the 4096 x 4096 image of all RGB triples (texel r + 256 g + 65536 b) -> 2^24 bytes
#define REF_HARNESS_NO_MAIN
#define REF_WITH_GLUE
#include "ref_harness.cpp"

namespace prt { void convertNormalToBump(uint8_t* bump, const uint8_t* normal, uint32_t width, uint32_t height); } // texture.cpp:185

static std::vector<uint32_t> readWords(const char* path)
{
    auto f = readFloats(path);
    std::vector<uint32_t> w(f.size());
    if (!w.empty()) memcpy(w.data(), f.data(), w.size() * 4);
    return w;
}
static float asF(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t asU(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static void put3(uint32_t* q, const Vector3f& v) { q[0] = asU(v.x); q[1] = asU(v.y); q[2] = asU(v.z); }

// the scene's meshes as reference Mesh objects (no BVH: nothing here traces)
static std::vector<Mesh*> meshesOf(FScene& fs)
{
    std::vector<Mesh*> out;
    for (auto& fm : fs.meshes) {
        Mesh* m = (Mesh*)calloc(1, sizeof(Mesh));
        fillMesh(m, fm, fs);
        out.push_back(m);
    }
    return out;
}

static int cmdTaps(const char* scenePath, const char* in, const char* out)
{
    FScene fs = loadScene(scenePath);
    auto meshes = meshesOf(fs);
    auto rec = readWords(in);
    const size_t n = rec.size() / 4;
    if (n % 8) { fprintf(stderr, "taps: record count is no multiple of 8\n"); return 2; }
    std::vector<uint32_t> o(n * 12, 0u);
    for (size_t g = 0; g < n; g += 8) {
        const uint32_t mat = rec[g * 4];
        if (mat >= meshes[0]->getMaterialCount()) { fprintf(stderr, "taps: bad material\n"); return 2; }
        const Material& m = meshes[0]->getMaterial(mat);
        Vector2f uvs[8];
        bool alphaOk = true;
        for (int l = 0; l < 8; l++) {
            const uint32_t* r = &rec[(g + l) * 4];
            if (r[0] != mat) { fprintf(stderr, "taps: a packet names two materials\n"); return 2; }
            uvs[l] = Vector2f(asF(r[1]), asF(r[2]));
            alphaOk = alphaOk && (r[3] & 2u);
        }
        int32_t bits = 0;
        if (alphaOk) {
            SoaMask all; all.setAll(true);
            bits = m.testAlpha(all, SoaVector2f(uvs)).ballot();
        }
        for (int l = 0; l < 8; l++) {
            const uint32_t flags = rec[(g + l) * 4 + 3];
            uint32_t* q = &o[(g + l) * 12];
            if (flags & 1u) {
                put3(q, m.diffuseMap.sample<Vector3f>(uvs[l]));
                q[3] = asU(m.bumpMap.sample<float>(uvs[l]));
                if (flags & 2u) q[4] = m.testAlpha(uvs[l]) ? 1u : 0u;
                put3(q + 6, m.sampleDiffuse(uvs[l]));
            }
            if (flags & 2u) q[5] = (uint32_t)(bits >> l) & 1u;
        }
    }
    writeAll(out, o.data(), o.size() * 4);
    return 0;
}

static int cmdTapsF(const char* prte, const char* in, const char* out)
{
    Texture t;
    t.init();
    t.loadExr(prte);
    if (!t.isValid()) return 2;
    auto uv = readFloats(in);
    std::vector<uint32_t> o(uv.size() / 2 * 3);
    for (size_t i = 0; i < uv.size() / 2; i++) put3(&o[i * 3], t.sample<Vector3f>(Vector2f(uv[2 * i], uv[2 * i + 1])));
    writeAll(out, o.data(), o.size() * 4);
    return 0;
}

static int cmdBump(const char* scenePath, const char* in, const char* out)
{
    FScene fs = loadScene(scenePath);
    auto meshes = meshesOf(fs);
    auto rec = readWords(in);
    const size_t n = rec.size() / 16;
    std::vector<uint32_t> o(n * 3);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* r = &rec[i * 16];
        if (r[0] >= meshes[0]->getMaterialCount()) return 2;
        const Material& m = meshes[0]->getMaterial(r[0]);
        SurfaceProperties p;
        p.material = &m;
        p.normal = Vector3f(asF(r[1]), asF(r[2]), asF(r[3]));
        p.uv = Vector2f(asF(r[4]), asF(r[5]));
        p.duv01 = Vector2f(asF(r[6]), asF(r[7]));
        p.duv02 = Vector2f(asF(r[8]), asF(r[9]));
        p.dp01 = Vector3f(asF(r[10]), asF(r[11]), asF(r[12]));
        p.dp02 = Vector3f(asF(r[13]), asF(r[14]), asF(r[15]));
        put3(&o[i * 3], m.sampleBump(p));
    }
    writeAll(out, o.data(), o.size() * 4);
    return 0;
}

static int cmdSurface(const char* scenePath, const char* in, const char* out)
{
    FScene fs = loadScene(scenePath);
    auto meshes = meshesOf(fs);
    auto rec = readWords(in);
    const size_t n = rec.size() / 5;
    std::vector<uint32_t> o(n * 20, 0u);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* r = &rec[i * 5];
        if (r[0] >= meshes.size() || r[1] >= meshes[r[0]]->getPrimCount()) return 2;
        const Mesh& mesh = *meshes[r[0]];
        RayHit hit;
        hit.t = 1.0f; hit.i = asF(r[2]); hit.j = asF(r[3]); hit.k = asF(r[4]);
        hit.primId = r[1]; hit.meshId = r[0];
        SurfaceProperties p;
        mesh.getSurfaceProperties(p, hit);
        uint32_t* q = &o[i * 20];
        put3(q, p.normal);
        q[3] = asU(p.uv.x); q[4] = asU(p.uv.y);
        q[5] = (uint32_t)(p.material - &mesh.getMaterial(0));
        q[6] = asU(p.duv01.x); q[7] = asU(p.duv01.y); q[8] = asU(p.duv02.x); q[9] = asU(p.duv02.y);
        put3(q + 10, p.dp01);
        put3(q + 13, p.dp02);
        put3(q + 16, p.material->sampleBump(p));
    }
    writeAll(out, o.data(), o.size() * 4);
    return 0;
}

static int cmdPpm(uint32_t w, uint32_t h, bool tonemap, const char* in, const char* out)
{
    auto px = readFloats(in);
    if (px.size() != (size_t)w * h * 3) return 2;
    Image image(w, h, tonemap, 1.0f);
    memcpy(image.m_pixels, px.data(), px.size() * 4);
    image.savePpm(out);
    return 0;
}

static int cmdLoad(const char* path, bool bump, const char* out)
{
    Texture t;
    t.init();
    t.load(path, bump);
    if (!t.isValid()) return 2;
    int32_t hdr[4] = {t.width, t.height, t.component, (t.component == 4 && t.isAlphaTestRequired()) ? 1 : 0};
    std::vector<uint8_t> buf((const uint8_t*)hdr, (const uint8_t*)hdr + 16);
    buf.insert(buf.end(), (const uint8_t*)t.texels, (const uint8_t*)t.texels + (size_t)t.width * t.height * t.component);
    writeAll(out, buf.data(), buf.size());
    return 0;
}

static int cmdBump24(const char* out)
{
    std::vector<uint8_t> rgba((size_t)4 << 24), b((size_t)1 << 24);
    for (uint32_t i = 0; i < (1u << 24); i++) {
        rgba[4 * (size_t)i] = (uint8_t)i; rgba[4 * (size_t)i + 1] = (uint8_t)(i >> 8); rgba[4 * (size_t)i + 2] = (uint8_t)(i >> 16); rgba[4 * (size_t)i + 3] = 255;
    }
    prt::convertNormalToBump(b.data(), rgba.data(), 4096, 4096);
    writeAll(out, b.data(), b.size());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 5 && !strcmp(argv[1], "taps")) return cmdTaps(argv[2], argv[3], argv[4]);
    if (argc >= 5 && !strcmp(argv[1], "tapsf")) return cmdTapsF(argv[2], argv[3], argv[4]);
    if (argc >= 5 && !strcmp(argv[1], "bump")) return cmdBump(argv[2], argv[3], argv[4]);
    if (argc >= 5 && !strcmp(argv[1], "surface")) return cmdSurface(argv[2], argv[3], argv[4]);
    if (argc >= 7 && !strcmp(argv[1], "ppm")) return cmdPpm((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), atoi(argv[4]) != 0, argv[5], argv[6]);
    if (argc >= 5 && !strcmp(argv[1], "load")) return cmdLoad(argv[2], atoi(argv[3]) != 0, argv[4]);
    if (argc >= 3 && !strcmp(argv[1], "bump24")) return cmdBump24(argv[2]);
    fprintf(stderr, "usage: %s taps|bump|surface <scene> <rec> <out> | tapsf <prte> <rec> <out> | ppm w h tonemap <in> <out> | load <prti> bump <out> | bump24 <out>\n", argv[0]);
    return 1;
}
