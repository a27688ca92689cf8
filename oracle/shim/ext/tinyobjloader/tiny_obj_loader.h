// Stand-in for tiny_obj_loader.h: the types and members mesh.cpp and material.cpp name, declared only, so that the reference's two
// files compile where the library itself is absent.  TEST INFRASTRUCTURE ONLY; no parser, nothing taken from the library.
// oracle/ref_stubs.cpp defines ObjReader's members: a reader that fails (the harnesses hand meshes over through Mesh::create).
#pragma once
#include <string>
#include <vector>
namespace tinyobj {
struct material_t {
    std::string name;
    float ambient[3], diffuse[3], specular[3], emission[3];
    std::string ambient_texname, diffuse_texname, specular_texname, emissive_texname, bump_texname;
};
struct index_t { int vertex_index, normal_index, texcoord_index; };
struct mesh_t { std::vector<index_t> indices; std::vector<int> material_ids; };
struct shape_t { std::string name; mesh_t mesh; };
struct attrib_t { std::vector<float> vertices, normals, texcoords; };
class ObjReader {
public:
    bool ParseFromFile(const std::string& path);
    const attrib_t& GetAttrib() const;
    const std::vector<shape_t>& GetShapes() const;
    const std::vector<material_t>& GetMaterials() const;
private:
    attrib_t attrib_;
    std::vector<shape_t> shapes_;
    std::vector<material_t> materials_;
};
}
