"""Geometry updates without a GPU (include/prt_hip.h "geometry updates"): the refit rule restated in numpy (prt_refit_ref.py)
reproduces the builders' own node boxes, Scene.update_positions is that rule byte for byte, and the rigid moves the GPU suite
pins to the oracle at tolerance 0 really do leave the builder's topology alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_testlib as T
from prt_refit_ref import RIGID_MOVES, atrium_scene, bend, no_negative_zero, refit_nodes, teapot_scene



@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


def single_mesh_oracle(mesh):
    o = T.OracleScene(T.SceneDesc([mesh], cam_pos=(0, 0.965, 2.6), cam_dir=(0, 0, -1.0), width=16, height=16))
    return o.nodes(0), o.prim_remap(0), o.radius()


def test_numpy_refit_of_the_builders_nodes_is_the_identity():
    """A builder sets every node's box to the min / max over the vertices below it, so refitting its nodes with unchanged
    positions changes no byte: the oracle's builder on the teapot, the compiled reference's nodes on both golden meshes."""
    tea = T.load_teapot_mesh()
    assert no_negative_zero(tea.positions)
    nodes, remap, _ = single_mesh_oracle(tea)
    assert refit_nodes(nodes, remap, tea.indices, tea.positions).tobytes() == nodes.tobytes()
    z = np.load(os.path.join(T.GOLDEN, "bvh_cornell_teapot.npz"))
    for i, mesh in enumerate((T.load_cornell_mesh(), tea)):
        assert no_negative_zero(mesh.positions)
        ref = z[f"nodes{i}"].view(T.NODE_DTYPE).reshape(-1)
        assert refit_nodes(ref, z[f"remap{i}"], mesh.indices, mesh.positions).tobytes() == ref.tobytes(), i


def test_rigid_moves_rebuild_to_the_refitted_tree():
    """The precondition of the GPU suite's oracle parity: for each rigid move it uses, the oracle's REBUILD of the moved teapot has
    the old topology and remapping and exactly the refit's boxes."""
    tea = T.load_teapot_mesh()
    nodes, remap, _ = single_mesh_oracle(tea)
    for name, move in RIGID_MOVES.items():
        P = move(tea.positions)
        assert no_negative_zero(P), name
        moved = T.MeshDesc(tea.indices, P, tea.prim_material, tea.materials, texcoords=tea.texcoords)
        rnodes, rremap, _ = single_mesh_oracle(moved)
        assert (rremap == remap).all(), name
        assert rnodes.tobytes() == refit_nodes(nodes, remap, tea.indices, P).tobytes(), name


@pytest.mark.parametrize("which", ["teapot", "atrium"])
def test_scene_update_positions_is_the_numpy_refit(L, which):
    scene, camera, _ = teapot_scene() if which == "teapot" else atrium_scene()
    m = 1 if which == "teapot" else 0
    before = scene.arrays()
    mesh0 = before["meshes"][m]
    if which == "atrium":
        mats = mesh0["materials"]
        assert (mats["bumpMap"] >= 0).any() and (mats["alphaTest"] != 0).any()
    rev_desc_before = scene.describe().contents.meshes[m].vertexCount
    for name, move in list(RIGID_MOVES.items())[2:] + [("bend", bend)]:
        P = move(mesh0["positions"])
        assert no_negative_zero(P), name
        scene.update_positions(m, P)
        a = scene.arrays()
        got = a["meshes"][m]
        assert scene.describe().contents.meshes[m].vertexCount == rev_desc_before
        assert got["positions"].tobytes() == P.tobytes(), name
        assert got["normals"].tobytes() == mesh0["normals"].tobytes(), name  # kept
        assert (got["remap"] == mesh0["remap"]).all() and (got["indices"] == mesh0["indices"]).all()
        assert got["nodes"].tobytes() == refit_nodes(mesh0["nodes"], mesh0["remap"], mesh0["indices"], P).tobytes(), name
        for other in range(len(a["meshes"])):
            if other != m:
                assert a["meshes"][other]["nodes"].tobytes() == before["meshes"][other]["nodes"].tobytes()
        # bounds over every vertex of every mesh; the radius as the oracle computes it for a scene built from the moved arrays
        allP = np.concatenate([mm["positions"] for mm in a["meshes"]])
        assert scene.bbox().tobytes() == np.concatenate([allP.min(axis=0), allP.max(axis=0)]).astype(np.float32).tobytes(), name
        o = T.OracleScene(T.scene_desc_from_product(scene, camera))
        assert np.float32(a["radius"]).tobytes() == np.float32(o.radius()).tobytes(), name
    # new vertex normals are stored as given
    N = np.ascontiguousarray(mesh0["normals"][::-1])
    scene.update_positions(m, mesh0["positions"], N)
    a = scene.arrays()
    assert a["meshes"][m]["normals"].tobytes() == N.tobytes()
    assert a["meshes"][m]["nodes"].tobytes() == mesh0["nodes"].tobytes()  # back at the original positions: the builder's boxes again
    assert np.float32(a["radius"]).tobytes() == np.float32(before["radius"]).tobytes()


def test_scene_update_positions_refusals(L):
    scene, _, _ = teapot_scene()
    a = scene.arrays()
    box, tea = a["meshes"][0], a["meshes"][1]
    assert box["normals"] is None and tea["normals"] is not None
    with pytest.raises(prt_amd.PrtError):
        scene.update_positions(2, tea["positions"])  # no such mesh
    with pytest.raises(prt_amd.PrtError):
        scene.update_positions(1, tea["positions"][:-1])  # another vertex count
    with pytest.raises(prt_amd.PrtError):
        scene.update_positions(0, box["positions"], np.zeros_like(box["positions"]))  # normals for a mesh without
    with pytest.raises(prt_amd.PrtError):
        scene.update_positions(1, tea["positions"], tea["normals"][:-1])
    after = scene.arrays()
    for i in range(2):
        assert after["meshes"][i]["positions"].tobytes() == a["meshes"][i]["positions"].tobytes()
        assert after["meshes"][i]["nodes"].tobytes() == a["meshes"][i]["nodes"].tobytes()


def test_update_entry_point_is_exported_declared_and_refuses_without_a_context(L):
    assert "prt_hip_update_meshes" in prt_amd.EXPORTS and "prt_host_scene_update_positions" in prt_amd.EXPORTS
    hdr = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    assert re.search(r"int prt_hip_update_meshes\(prt_hip_ctx\* ctx, uint32_t count, const prt_mesh_update\* updates, void\* stream\);", hdr)
    # the struct the Python side binds has the header's fields, in order
    body = re.search(r"typedef struct \{([^}]*)\} prt_mesh_update;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+);", body)
    assert fields == [n for n, _ in prt_amd.MeshUpdate._fields_], fields
    syms = subprocess.check_output(["nm", "-D", "--defined-only", prt_amd.LIB_PATH]).decode()
    assert " T prt_hip_update_meshes" in syms and "prt_hip_test" not in syms
    assert "prt_hip_test_scene_arrays" in prt_amd.TEST_EXPORTS and hasattr(prt_amd.test_lib(), "prt_hip_test_scene_arrays")
    # reachable without a device: no context
    up = prt_amd.MeshUpdate()
    assert L.prt_hip_update_meshes(None, 1, C.byref(up), None) == -2  # PRT_HIP_EINVAL
    assert L.prt_hip_last_error()
    from prt_amd import _build as B
    assert "prt_refit.hip" in B.SOURCES
