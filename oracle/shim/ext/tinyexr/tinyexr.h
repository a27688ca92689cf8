// Stand-in for tinyexr.h: the names texture.cpp and image.cpp use, declared only, so that the reference's two files compile where
// the library itself is absent.  TEST INFRASTRUCTURE ONLY; no codec, nothing taken from the library.  oracle/ref_stubs.cpp defines
// the functions: the loader reads the raw "PRTE" float image the tests write, the writer refuses.
#pragma once
#include <stddef.h>
enum { TINYEXR_SUCCESS = 0, TINYEXR_PIXELTYPE_HALF = 1, TINYEXR_PIXELTYPE_FLOAT = 2 };
struct EXRChannelInfo { char name[256]; };
struct EXRHeader { int num_channels; EXRChannelInfo* channels; int* pixel_types; int* requested_pixel_types; };
struct EXRImage { unsigned char** images; int width, height, num_channels; };
void InitEXRHeader(EXRHeader* header);
void InitEXRImage(EXRImage* image);
int LoadEXRFromMemory(float** rgba, int* width, int* height, const unsigned char* memory, size_t size, const char** err);
int SaveEXRImageToFile(const EXRImage* image, const EXRHeader* header, const char* path, const char** err);
void FreeEXRErrorMessage(const char* msg);
