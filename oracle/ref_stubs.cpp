// ref_stubs.cpp -- definitions for the stand-in declarations under oracle/shim/ext/, so that the reference's texture.cpp, material.cpp,
// mesh.cpp and image.cpp link (ref_shade, ref_path_real; oracle/Makefile).
//
// TEST INFRASTRUCTURE ONLY.  No decoder, encoder or parser lives here and nothing is taken from stb, tinyexr or tinyobjloader:
//   * stbi_info / stbi_load read the raw texel file the tests write -- "PRTI", i32 width, height, comp, width*height*comp bytes -- and
//     hand over req_comp bytes per texel (3 -> 4 appends alpha 255, as an image without an alpha channel is opaque);
//   * LoadEXRFromMemory reads the raw float image the tests write -- "PRTE", i32 width, height, width*height*4 f32;
//   * SaveEXRImageToFile and ObjReader::ParseFromFile fail.
// The image and OBJ decoders themselves therefore stay unpinned by the reference.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "../ext/stb/stb_image.h"
#include "../ext/tinyexr/tinyexr.h"
#include "../ext/tinyobjloader/tiny_obj_loader.h"

static const char* g_reason = "no error";

static FILE* openRaw(const char* path, int32_t hdr[3])
{
    FILE* f = fopen(path, "rb");
    char magic[4];
    if (!f) { g_reason = "cannot open"; return nullptr; }
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "PRTI", 4) || fread(hdr, 4, 3, f) != 3) { g_reason = "not a PRTI file"; fclose(f); return nullptr; }
    return f;
}

extern "C" int stbi_info(const char* path, int* w, int* h, int* comp)
{
    int32_t hdr[3];
    FILE* f = openRaw(path, hdr);
    if (!f) return 0;
    fclose(f);
    *w = hdr[0]; *h = hdr[1]; *comp = hdr[2];
    return 1;
}

extern "C" stbi_uc* stbi_load(const char* path, int* w, int* h, int* comp, int req_comp)
{
    int32_t hdr[3];
    FILE* f = openRaw(path, hdr);
    if (!f) return nullptr;
    const size_t n = (size_t)hdr[0] * hdr[1];
    const int c = hdr[2];
    stbi_uc* src = (stbi_uc*)malloc(n * c + 1);
    stbi_uc* dst = (stbi_uc*)malloc(n * req_comp + 1);
    if (fread(src, 1, n * c, f) != n * c || !(c == req_comp || (c == 3 && req_comp == 4))) {
        g_reason = "short or unsupported PRTI file";
        fclose(f); free(src); free(dst);
        return nullptr;
    }
    fclose(f);
    if (c == req_comp) memcpy(dst, src, n * c);
    else
        for (size_t i = 0; i < n; i++) { dst[4 * i] = src[3 * i]; dst[4 * i + 1] = src[3 * i + 1]; dst[4 * i + 2] = src[3 * i + 2]; dst[4 * i + 3] = 255; }
    free(src);
    *w = hdr[0]; *h = hdr[1]; *comp = c;
    return dst;
}

extern "C" void stbi_image_free(void* p) { free(p); }
extern "C" const char* stbi_failure_reason(void) { return g_reason; }

void InitEXRHeader(EXRHeader* header) { memset(header, 0, sizeof(*header)); }
void InitEXRImage(EXRImage* image) { memset(image, 0, sizeof(*image)); }
void FreeEXRErrorMessage(const char*) {}

int LoadEXRFromMemory(float** rgba, int* width, int* height, const unsigned char* memory, size_t size, const char** err)
{
    int32_t wh[2];
    if (size < 12 || memcmp(memory, "PRTE", 4)) { if (err) *err = "not a PRTE file"; return -1; }
    memcpy(wh, memory + 4, 8);
    const size_t bytes = (size_t)wh[0] * wh[1] * 16;
    if (size < 12 + bytes) { if (err) *err = "short PRTE file"; return -1; }
    *rgba = (float*)malloc(bytes);
    memcpy(*rgba, memory + 12, bytes);
    *width = wh[0]; *height = wh[1];
    return TINYEXR_SUCCESS;
}

int SaveEXRImageToFile(const EXRImage*, const EXRHeader*, const char*, const char** err)
{
    if (err) *err = "no OpenEXR writer in this build";
    return -1;
}

namespace tinyobj {
bool ObjReader::ParseFromFile(const std::string&) { return false; }
const attrib_t& ObjReader::GetAttrib() const { return attrib_; }
const std::vector<shape_t>& ObjReader::GetShapes() const { return shapes_; }
const std::vector<material_t>& ObjReader::GetMaterials() const { return materials_; }
}
