// Stand-in for stb_image.h: declarations of the four functions and two constants texture.cpp names, so that the reference's
// texture.cpp compiles where the library itself is absent.  TEST INFRASTRUCTURE ONLY; no decoder, nothing taken from the library.
// oracle/ref_stubs.cpp defines the functions (a raw-texel reader the tests feed).
#pragma once
typedef unsigned char stbi_uc;
enum { STBI_grey = 1, STBI_rgb_alpha = 4 };
extern "C" {
int stbi_info(const char* path, int* w, int* h, int* comp);
stbi_uc* stbi_load(const char* path, int* w, int* h, int* comp, int req_comp);
void stbi_image_free(void* p);
const char* stbi_failure_reason(void);
}
