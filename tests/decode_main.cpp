// decode_main.cpp -- the host asset readers (prt_amd/csrc/host: PNM / TGA / PNG / JPEG textures, OBJ / MTL, OpenEXR / PFM environment
// maps) on files from a user's disk: a stand-alone program that enters them through the public classes of host/prt.h only, built by
// tests/test_hostile_files_cpu.py from host/prt_models.cpp, prt_host.cpp and prt_bvh.cpp with g++, once with
// -fsanitize=address,undefined and once plain (to run under an address-space limit).  It links nothing of HIP (tests/decode_stubs.cpp
// stands in for the prt_hip_* calls prt_host.cpp refers to) and nothing of it is loaded into Python.
//
//   decode_main tex FILE...   Mesh::loadObj on a generated OBJ + MTL next to FILE, with FILE as map_Kd and as map_bump
//   decode_main obj FILE...   Mesh::loadObj(FILE)
//   decode_main env FILE...   Scene::setInfiniteAreaLight(FILE)
//
// One line per file on stdout, "@ NAME ..." with NAME = FILE as given (the readers' own messages carry no such prefix):
//   tex:  @ NAME kd RESULT bump RESULT     RESULT = refused | loaded W H C DIGEST
//   obj:  @ NAME refused | @ NAME loaded PRIMS VERTICES MATERIALS DIGEST    (indices, then positions)
//   env:  @ NAME refused | @ NAME loaded W H 4 DIGEST
// DIGEST is the 64-bit FNV-1a of the bytes.  Exit status 0 = every file was answered.
#include "../prt_amd/csrc/host/prt.h"

#include <cstdio>
#include <cstring>
#include <string>

using namespace prt;

static uint64_t fnv(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ull)
{
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

static void split(const std::string& path, std::string& dir, std::string& name)
{
    const size_t slash = path.find_last_of('/');
    dir = slash == std::string::npos ? "." : path.substr(0, slash);
    name = slash == std::string::npos ? path : path.substr(slash + 1);
}

static void printTexture(const char* role, const Texture& t)
{
    if (!t.isValid()) printf(" %s refused", role);
    else printf(" %s loaded %u %u %u %016llx", role, (unsigned)t.width, (unsigned)t.height, (unsigned)t.component,
                (unsigned long long)fnv(t.texels->data(), t.texels->size()));
}

static bool writeText(const std::string& path, const std::string& text)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    return fclose(f) == 0 && ok;
}

static int tex(const std::string& path)
{
    std::string dir, name;
    split(path, dir, name);
    const std::string obj = dir + "/_decode_main.obj";
    if (!writeText(dir + "/_decode_main.mtl", "newmtl a\nKd 1 1 1\nmap_Kd " + name + "\nmap_bump " + name + "\n") ||
        !writeText(obj, "mtllib _decode_main.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\n"))
        return 1;
    Mesh mesh;
    mesh.loadObj(obj.c_str());
    if (mesh.getPrimCount() != 1 || mesh.getMaterialCount() != 1) return 1; // the generated OBJ itself always loads
    printf("@ %s", path.c_str());
    printTexture("kd", mesh.getMaterial(0).diffuseMap);
    printTexture("bump", mesh.getMaterial(0).bumpMap);
    printf("\n");
    return 0;
}

static int obj(const std::string& path)
{
    Mesh mesh;
    mesh.loadObj(path.c_str());
    if (mesh.getPrimCount() == 0) { // prt_host_mesh_load_obj's failure value
        printf("@ %s refused\n", path.c_str());
        return 0;
    }
    uint64_t h = fnv(mesh.getIndexBuffer(), (size_t)mesh.getIndexCount() * 4);
    h = fnv(mesh.getPositionBuffer(), (size_t)mesh.getVertexCount() * sizeof(Vector3f), h);
    printf("@ %s loaded %u %u %u %016llx\n", path.c_str(), mesh.getPrimCount(), mesh.getVertexCount(), mesh.getMaterialCount(), (unsigned long long)h);
    return 0;
}

static int env(const std::string& path)
{
    Scene scene;
    scene.init();
    scene.setInfiniteAreaLight(path.c_str());
    const InfiniteAreaLight& l = scene.getInfiniteAreaLight();
    if (!scene.isLightAvailable(LightType::kInfiniteArea) || !l.isValid()) { // prt_host_scene_load_env_light's failure value
        printf("@ %s refused\n", path.c_str());
        return 0;
    }
    printf("@ %s loaded %d %d 4 %016llx\n", path.c_str(), l.getWidth(), l.getHeight(),
           (unsigned long long)fnv(l.getTexels().data(), l.getTexels().size() * sizeof(float)));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    int (*fn)(const std::string&) = mode == "tex" ? tex : mode == "obj" ? obj : mode == "env" ? env : nullptr;
    if (!fn) return 2;
    for (int i = 2; i < argc; i++) {
        if (fn(argv[i]) != 0) return 1;
        fflush(stdout);
    }
    return 0;
}
