"""Geometry updates from device memory, without a GPU (include/prt_hip.h): the per-vertex walk of tests/prt_deform_ref.py IS
Mesh::calculateVertexNormals -- bit for bit against the oracle's sequential loop and the product's host code, on a mesh built to break
it -- the radius restatement is Scene::updatePositions', and the new entry points are exported, declared and bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import prt_amd
import prt_deform_ref as D
import prt_testlib as T
from prt_refit_ref import RIGID_MOVES, atrium_scene, bend, teapot_scene

F = np.float32


@pytest.fixture(scope="module")
def L():
    prt_amd.build()
    return prt_amd.lib()


def hostile_desc():
    idx, P = D.hostile_mesh()
    mats = np.array([T.make_material(diffuse=(0.7, 0.6, 0.5))], dtype=T.MATERIAL_DTYPE)
    return T.MeshDesc(idx, P, np.zeros(len(idx), np.uint32), mats)


def cases():
    tea = T.load_teapot_mesh()
    bent = T.MeshDesc(tea.indices, bend(tea.positions), tea.prim_material, tea.materials, texcoords=tea.texcoords)
    return {"hostile": hostile_desc(), "teapot": tea, "teapot_bent": bent}


def test_hostile_mesh_holds_what_it_promises():
    idx, P = D.hostile_mesh()
    off, face = D.csr(idx, len(P))
    valence = off[1:] - off[:-1]
    assert valence.max() == 300 and (valence == 0).sum() == 1 and len(face) == 3 * len(idx)
    fn = D.face_normals(idx, P)
    assert (fn == 0).all(axis=1).sum() >= 4  # equal positions, a vertex named twice, underflow, denormal
    assert np.signbit(P[P == 0]).any()
    n = D.vertex_normals(idx, P)
    assert np.isnan(n).all(axis=1).sum() >= 4  # the unused vertex, and the vertices whose faces are all degenerate
    # the coincident pair: the second face would cancel the first, and is skipped
    pair = np.nonzero((np.sort(idx, axis=1)[:, None, :] == np.sort(idx, axis=1)[None, :, :]).all(-1).sum(1) == 2)[0]
    assert len(pair) == 2 and (fn[pair[0]] == -fn[pair[1]]).all() and D.bits_equal(n[idx[pair[0]]], np.tile(D._normalize(fn[pair[1]]), (3, 1)))
    # the list is in the reference's order: faces descending per vertex
    for v in (0, 21, int(np.argmax(valence))):
        assert (np.diff(face[off[v]:off[v + 1]]) <= 0).all()


@pytest.mark.parametrize("which", ["hostile", "teapot", "teapot_bent"])
def test_walk_is_the_sequential_loop(L, which):
    mesh = cases()[which]
    want = T.oracle_vertex_normals(mesh).normals
    got = D.vertex_normals(mesh.indices, mesh.positions)
    assert D.bits_equal(got, want), f"{which}: {(~(np.isnan(got) & np.isnan(want)) & (got.view(np.uint32) != want.view(np.uint32))).sum()} words differ"
    # ... and the product's own host code
    pm = prt_amd.Mesh.from_arrays(mesh.indices, mesh.positions, mesh.prim_material, mesh.materials.view(prt_amd.MATERIAL_DTYPE))
    pm.calculate_vertex_normals()
    scene = prt_amd.Scene()
    scene.add(pm)
    assert D.bits_equal(scene.arrays()["meshes"][0]["normals"], got), which


@pytest.mark.parametrize("which", ["teapot", "atrium"])
def test_radius_restatement_is_update_positions(L, which):
    scene, camera, _ = teapot_scene() if which == "teapot" else atrium_scene()
    m = 1 if which == "teapot" else 0
    a = scene.arrays()
    P0 = a["meshes"][m]["positions"]
    assert F(a["radius"]).tobytes() == D.radius([D.vertex_box(mm["positions"]) for mm in a["meshes"]]).tobytes()
    for name, move in list(RIGID_MOVES.items()) + [("bend", bend)]:
        scene.update_positions(m, move(P0))
        a = scene.arrays()
        boxes = [D.vertex_box(mm["positions"]) for mm in a["meshes"]]
        assert F(scene.describe().contents.radius).tobytes() == D.radius(boxes).tobytes(), name
        assert scene.bbox().tobytes() == D.vertex_box(np.concatenate([mm["positions"] for mm in a["meshes"]])).tobytes()


def test_sah_restatement_on_a_hand_made_tree():
    nodes = np.zeros(3, dtype=T.NODE_DTYPE)
    nodes["lower"] = [(0, 0, 0), (0, 0, 0), (1, 0, 0)]
    nodes["upper"] = [(2, 1, 1), (1, 1, 1), (2, 1, 0.5)]
    nodes["primCount"] = [0xF, 2, 3]
    s = D.sah(nodes)
    assert s["internalArea"] == 10.0 and s["leafArea"] == 2 * 6.0 + 3 * 4.0 and s["rootArea"] == 10.0
    assert s["sahCost"] == (0.125 * 10.0 + 24.0) / 10.0 and (s["internalNodes"], s["leaves"]) == (1, 2)


def header_fields(hdr, name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"\[\d+\]", "", w.strip().split()[-1].lstrip("*")) for w in decl.split(",")]
    return out


def test_entry_points_are_exported_declared_and_bound(L):
    names = ("prt_hip_deform_meshes", "prt_hip_get_mesh_vertices", "prt_hip_mesh_info")
    hdr = open(os.path.join(T.ROOT, "include", "prt_hip.h")).read()
    assert "geometry updates from device memory" in hdr
    assert re.search(r"int prt_hip_deform_meshes\(prt_hip_ctx\* ctx, uint32_t count, const prt_mesh_deform\* deforms, uint32_t flags, void\* stream\);", hdr)
    assert re.search(r"int prt_hip_get_mesh_vertices\(prt_hip_ctx\* ctx, uint32_t mesh, float\* positions, float\* normals, uint32_t flags, void\* stream\);", hdr)
    assert re.search(r"int prt_hip_mesh_info\(prt_hip_ctx\* ctx, uint32_t mesh, prt_mesh_info\* out\);", hdr)
    for macro, value in (("PRT_HIP_NORMALS_KEEP", 0), ("PRT_HIP_NORMALS_GIVEN", 1), ("PRT_HIP_NORMALS_RECOMPUTE", 2), ("PRT_HIP_DEFORM_HOST", 1),
                         ("PRT_HIP_DEFORM_RADIUS_AUTO", 2)):
        assert re.search(r"#define " + macro + r"\s+" + str(value) + "u", hdr), macro
    M = prt_amd.MeshDeform
    assert (M.NORMALS_KEEP, M.NORMALS_GIVEN, M.NORMALS_RECOMPUTE, M.HOST, M.RADIUS_AUTO) == (0, 1, 2, 1, 2)
    assert header_fields(hdr, "prt_mesh_deform") == [n for n, _ in prt_amd.MeshDeform._fields_]
    assert header_fields(hdr, "prt_mesh_info") == [n for n, _ in prt_amd.MeshInfo._fields_]
    assert C.sizeof(prt_amd.MeshDeform) == 32 and C.sizeof(prt_amd.MeshInfo) == 104
    syms = subprocess.check_output(["nm", "-D", "--defined-only", prt_amd.LIB_PATH]).decode()
    for n in names:
        assert n in prt_amd.EXPORTS and f" T {n}" in syms and hasattr(L, n), n
    assert "prt_hip_test" not in syms
    assert "prt_hip_test_deform_profile" in prt_amd.TEST_EXPORTS and hasattr(prt_amd.test_lib(), "prt_hip_test_deform_profile")
    for n in ("deform_meshes", "mesh_vertices", "mesh_info"):
        assert callable(getattr(prt_amd.PathTracer, n)), n
    # reachable without a device: no context
    d, info = prt_amd.MeshDeform(), prt_amd.MeshInfo()
    assert L.prt_hip_deform_meshes(None, 1, C.byref(d), 0, None) == -2  # PRT_HIP_EINVAL
    assert L.prt_hip_get_mesh_vertices(None, 0, None, None, 0, None) == -2
    assert L.prt_hip_mesh_info(None, 0, C.byref(info)) == -2 and L.prt_hip_last_error()
    from prt_amd import _build as B
    assert "prt_deform.hip" in B.SOURCES and "prt_deform.hip" not in B.KERNEL_HEADERS
    # the frame kernel's translation unit does not see the new file
    for f in ("prt_kernels.hip", "prt_frame.h", "prt_device.h", "prt_lanes.h"):
        assert "prt_deform" not in open(os.path.join(B.CSRC, f)).read(), f
