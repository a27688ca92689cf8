"""The host asset readers (prt_amd/csrc/host: PNM / TGA / PNG / JPEG textures, OBJ / MTL, OpenEXR / PFM environment maps) on hostile
files: a reader refuses, it never aborts, never reads or writes out of bounds, never allocates on a header's word.

tests/decode_main.cpp, a stand-alone program, enters the readers through the public classes; it is built twice under tests/_build/:
with AddressSanitizer and UBSan (every family of tests/prt_hostile_files.py runs through that one), and plain (that one runs under
an address-space limit, which ASan's own reservations rule out).  Nothing sanitized is loaded into Python.  The readers' output on
the smallest valid shapes is held to Pillow's, through the product library as the other loader tests do."""
import io
import os
import resource
import struct
import subprocess
import sys

import numpy as np
import pytest

import prt_hostile_files as H

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "prt_amd", "csrc", "host")
BUILD = os.path.join(HERE, "_build")
LIMIT = 2 << 30  # RLIMIT_AS of the plain harness and of the Python child: a condition, not a measurement (every valid file loads under it)
BATCH = 300


def _build(name, extra):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    srcs = [os.path.join(HERE, "decode_main.cpp"), os.path.join(HERE, "decode_stubs.cpp")] + \
        [os.path.join(HOST, f) for f in ("prt_models.cpp", "prt_host.cpp", "prt_bvh.cpp")]
    deps = srcs + [os.path.join(HOST, "prt.h"), os.path.join(HOST, "cornell_data.inc"), os.path.join(ROOT, "include", "prt_hip.h")]
    exe = os.path.join(BUILD, name)
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return None, exe
    os.makedirs(BUILD, exist_ok=True)
    tmp = f"{exe}.tmp.{os.getpid()}"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-pthread"] + extra + srcs + ["-o", tmp]
    return (subprocess.Popen(cmd), tmp), exe


@pytest.fixture(scope="session")
def harness():
    """{"san": ..., "plain": ...}: the two builds of tests/decode_main.cpp (rebuilt when a source is newer)."""
    # the sanitizers' runtimes are linked statically: the program is complete in itself, whatever else the process environment loads
    jobs = {"san": _build("decode_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]),
            "plain": _build("decode_main_plain", [])}
    out = {}
    for key, (job, exe) in jobs.items():
        if job:
            assert job[0].wait() == 0, f"{key} harness does not compile"
            os.replace(job[1], exe)
        out[key] = exe
    return out


def _limit():
    resource.setrlimit(resource.RLIMIT_AS, (LIMIT, LIMIT))


def run(exe, mode, directory, names, limited=False):
    """The harness over `names` (relative to `directory`) in batches: {name: answer}, answer = the words after the name."""
    answers = {}
    for i in range(0, len(names), BATCH):
        batch = names[i:i + BATCH]
        r = subprocess.run([exe, mode] + batch, cwd=directory, capture_output=True, timeout=600, preexec_fn=_limit if limited else None)
        err = r.stderr.decode(errors="replace")
        seen = [line.split() for line in r.stdout.decode(errors="replace").splitlines() if line.startswith("@ ")]
        last = seen[-1][1] if seen else "(none)"
        assert r.returncode == 0, f"exit status {r.returncode} after {last} (batch {batch[0]} .. {batch[-1]})\n{err[-3000:]}"
        assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]
        for words in seen:
            answers[words[1]] = words[2:]
        for n in batch:
            assert n in answers, f"no answer for {n}"
            a = answers[n]
            if mode == "tex":
                assert a[0] == "kd" and a[1] in ("refused", "loaded") and "bump" in a and a[a.index("bump") + 1] in ("refused", "loaded"), (n, a)
            else:
                assert a[0] in ("refused", "loaded"), (n, a)
    return answers


def write(directory, files):
    """files: [(name, bytes)]; names that occur twice (two edits that give the same file) are written once."""
    names = []
    for name, data in dict(files).items():
        with open(os.path.join(str(directory), name), "wb") as f:
            f.write(data)
        names.append(name)
    return names


def tex(answer):
    """(kd, bump) of a tex answer: None = refused, else (W, H, C, digest)."""
    def one(words):
        return None if words[0] == "refused" else (int(words[1]), int(words[2]), int(words[3]), words[4])
    b = answer.index("bump")
    return one(answer[1:b]), one(answer[b + 1:])


def refused(mode, answer):
    return tex(answer) == (None, None) if mode == "tex" else answer[0] == "refused"


@pytest.fixture(scope="session")
def src(tmp_path_factory):
    return H.sources(tmp_path_factory.mktemp("hostile_sources"))


SOURCES = ["tga_raw", "tga_rle", "tga_grey_rle", "ppm", "pgm", "pam", "png_rgba", "png_palette", "png_adam7_16", "png_pillow_64", "jpeg_420",
           "jpeg_grey_restart", "jpeg_progressive", "exr_raw", "exr_rle", "exr_zip"]
EDITS = {"tga": ("tex", lambda s: H.field_edits_tga(s)), "pnm": ("tex", lambda s: H.field_edits_pnm()), "png": ("tex", lambda s: H.field_edits_png(s)),
         "png_zlib": ("tex", lambda s: H.field_edits_png_zlib()), "jpeg": ("tex", lambda s: H.field_edits_jpeg(s)), "exr": ("env", lambda s: H.field_edits_exr(s))}


def test_the_sources_are_the_ones_the_tests_name(src):
    assert sorted(src) == sorted(SOURCES)


# ------------------------------------------------------------------------------------------------------------- nothing crashes
@pytest.mark.parametrize("name", SOURCES)
def test_truncations_under_the_sanitizers_and_the_truncation_property(harness, src, tmp_path, name):
    """Every prefix (a seeded sample past the headers of the larger sources) is answered under ASan + UBSan, and:
    a strict prefix of a PNM or raw TGA file is refused; a PNG cut before its last IDAT chunk is complete is refused; a prefix of a JPEG
    or of a run-length TGA is refused or loads with the source's own width, height and components.  No prefix of anything changes them."""
    kind, data = src[name]
    mode = H.MODE[kind]
    names = write(tmp_path, H.truncations(kind, data, seed=SOURCES.index(name)) + [("whole" + H.EXT[kind], data)])
    got = run(harness["san"], mode, str(tmp_path), names)
    whole = got["whole" + H.EXT[kind]]
    assert not refused(mode, whole), "the source itself does not load"
    if kind == "png":
        chunks = H._png_chunks(data)
        o, _, n = [c for c in chunks if c[1] == b"IDAT"][-1]
        idat_end = o + 12 + n
    for n_ in names:
        if not n_.startswith("cut"):
            continue
        k, a = int(n_[3:8]), got[n_]
        if kind == "pnm" or name == "tga_raw":
            assert refused(mode, a), f"{name}: a prefix of {k} of {len(data)} bytes loads"
        elif kind == "png" and k < idat_end:
            assert refused(mode, a), f"{name}: a prefix of {k} bytes, cut before the last IDAT ends at {idat_end}, loads"
        elif mode == "tex":
            for got_one, whole_one in zip(tex(a), tex(whole)):
                assert got_one is None or got_one[:3] == whole_one[:3], f"{name}: a prefix of {k} bytes loads as {got_one[:3]}, the file as {whole_one[:3]}"
        else:
            assert a[0] == "refused" or a[1:4] == whole[1:4], f"{name}: a prefix of {k} bytes loads as {a[1:4]}, the file as {whole[1:4]}"


@pytest.mark.parametrize("name", SOURCES)
def test_byte_mutations_under_the_sanitizers(harness, src, tmp_path, name):
    """1500 seeded mutants of one to three bytes per source: each is answered, the sanitizers report nothing."""
    kind, data = src[name]
    names = write(tmp_path, H.byte_mutations(kind, data, seed=100 + SOURCES.index(name)))
    assert len(names) > 1400
    run(harness["san"], H.MODE[kind], str(tmp_path), names)


@pytest.mark.parametrize("fmt", sorted(EDITS))
def test_field_edits_under_the_sanitizers(harness, src, tmp_path, fmt):
    """Every size, count, length and selector field of a format at 0, 1, its maximum, maximum - 1 and its sign bit, and the malformed
    structures prt_hostile_files.py lists per format."""
    mode, make = EDITS[fmt]
    files = make(src)
    assert len(files) >= 25
    run(harness["san"], mode, str(tmp_path), write(tmp_path, files))


def test_oversize_claims_under_the_sanitizers(harness, tmp_path):
    files = H.oversize_claims()
    for mode in ("tex", "env"):
        names = write(tmp_path, [(n, b) for n, k, b in files if H.MODE[k] == mode] + ([("idat_64mb.png", H.png_with_64mb_idat())] if mode == "tex" else []))
        got = run(harness["san"], mode, str(tmp_path), names)
        assert all(refused(mode, got[n]) for n in names if n != "idat_64mb.png")


def _write_obj_cases(tmp_path):
    paths = []
    for case, files, load in H.obj_cases():
        os.mkdir(tmp_path / case)
        write(tmp_path / case, list(files.items()))
        paths.append(f"{case}/{load}")
    return paths


def test_obj_and_mtl_under_the_sanitizers(harness, tmp_path):
    """Hostile OBJ / MTL text: every case is answered; what must load loads as the mesh it describes, what must not is refused."""
    got = run(harness["san"], "obj", str(tmp_path), _write_obj_cases(tmp_path))
    g = {k.split("/")[0]: v for k, v in got.items()}
    one_triangle = g["valid"]
    assert one_triangle[:4] == ["loaded", "1", "3", "1"]
    for case in ("index_negative_valid", "face_1_slash_slash", "face_trailing_slash", "usemtl_without_mtllib", "mtllib_missing", "mtllib_is_the_obj",
                 "mtl_empty", "mtl_newmtl_without_name", "mtl_map_kd_without_file", "mtl_map_bump_bm_without_value", "mtl_map_kd_is_the_mtl", "crlf",
                 "crlf_with_mtl", "no_final_newline", "long_line", "tabs", "leading_spaces", "faces_before_vertices_negative"):
        if case == "faces_before_vertices_negative":
            assert g[case] == ["refused"], case  # -1 names the last vertex READ SO FAR: there is none yet
        else:
            assert g[case] == one_triangle, (case, g[case])  # the same triangle: same counts, same digest
    for idx in ("0", "-9", "4", "-4", "4294967297", "4294967296", "2147483649", "-4294967295", "18446744073709551617", "99999999999999999999",
                "-99999999999999999999", "9223372036854775807", "-9223372036854775808"):
        assert g[f"index_{idx}"] == ["refused"] and g[f"index_{idx}_first"] == ["refused"], idx
        assert g[f"vt_index_{idx}"][:4] == ["loaded", "1", "3", "1"], idx  # a texture coordinate out of range reads as (0, 0), as before
    for case in ("empty", "only_newlines", "faces_before_vertices", "face_0_corners", "face_1_corner", "face_2_corners", "nul_only", "binary", "face_letters"):
        assert g[case] == ["refused"], (case, g[case])
    assert g["face_2_corners_bad_index"][:4] == ["loaded", "1", "3", "1"]  # a face of two corners makes no triangle: its indices are never used
    assert g["face_60000_corners"][:3] == ["loaded", "59998", "60000"]
    assert g["face_quad_and_pentagon"][:3] == ["loaded", "5", "5"]
    for val in ("nan", "inf", "-inf", "1e999"):
        assert g[f"coordinate_{val}"][:3] == ["loaded", "1", "3"], val  # the numbers strtod reads: the mesh carries them


def test_smallest_valid_shapes_under_the_sanitizers(harness, tmp_path):
    files = H.smallest_valid(tmp_path)
    names = write(tmp_path, [(n, b) for n, _, b in files])
    got = run(harness["san"], "tex", str(tmp_path), names)
    assert all(tex(got[n])[0] is not None for n in names), [n for n in names if tex(got[n])[0] is None]


# ---------------------------------------------------------------------------------------- nothing is allocated on a header's word
def test_every_valid_file_loads_under_the_address_space_limit(harness, src, tmp_path):
    files = [(n + H.EXT[k], k, b) for n, (k, b) in src.items()] + H.smallest_valid(tmp_path)
    for mode in ("tex", "env"):
        names = write(tmp_path, [(n, b) for n, k, b in files if H.MODE[k] == mode])
        got = run(harness["plain"], mode, str(tmp_path), names, limited=True)
        assert not [n for n in names if refused(mode, got[n])]


def test_oversize_claims_are_refused_under_the_address_space_limit(harness, tmp_path):
    """Header-only files that declare 65535 x 65535 (and 65535 x 1, 1 x 65535), a JPEG frame of that size over one coded MCU, OpenEXR data
    windows up to 2^31 - 1: each is refused, with exit status 0, by a process that may map 2 GB.  A reader that sized a buffer by the
    header before looking at the data ends in std::bad_alloc here (exit status 134)."""
    files = H.oversize_claims()
    assert len(files) >= 40
    for mode in ("tex", "env"):
        names = write(tmp_path, [(n, b) for n, k, b in files if H.MODE[k] == mode])
        got = run(harness["plain"], mode, str(tmp_path), names, limited=True)
        assert not [n for n in names if not refused(mode, got[n])]


def test_an_idat_that_inflates_to_64_mb_is_cut_at_the_image(harness, tmp_path):
    """An 8 x 8 grey PNG needs 72 bytes of scanlines.  Its IDAT inflates to 64 MB of zeros: the inflate stops at the 72 bytes the header
    asks for and the file loads as the 8 x 8 image those bytes are (libpng ignores the excess too) -- `loaded 8 8 1`, all texels 0; it
    does so under a limit that the 64 MB, inflated into a growing vector, would still fit: what is pinned is the answer."""
    names = write(tmp_path, [("idat_64mb.png", H.png_with_64mb_idat()), ("zeros.png", H.png(8, 8, 8, 0, bytes(72)))])
    got = run(harness["plain"], "tex", str(tmp_path), names, limited=True)
    kd, bump = tex(got["idat_64mb.png"])
    assert kd is not None and kd[:3] == (8, 8, 1) and bump[:3] == (8, 8, 1)
    assert (kd, bump) == tex(got["zeros.png"])


# -------------------------------------------------------------------------------------------------------------- stated refusals
def test_stated_refusals(harness, src, tmp_path):
    """Files that are wrong in a way the reader can see are refused, not decoded to something: an OBJ face index beyond 2^32 (it once
    wrapped to vertex 0), a JPEG scan on a quantisation table no DQT defined, PNG filter type 5, a palette index beyond the PLTE chunk,
    an over-subscribed Huffman table in a DHT."""
    os.mkdir(tmp_path / "o")
    (tmp_path / "o" / "m.obj").write_text(H.TRIANGLE + "f 1 2 4294967297\n")
    assert run(harness["san"], "obj", str(tmp_path), ["o/m.obj"])["o/m.obj"] == ["refused"]
    files = {}
    for name in ("jpeg_420", "jpeg_grey_restart", "jpeg_progressive"):
        data = src[name][1]
        segs = H.jpeg_segments(data)
        sof = next(o for m, o, n in segs if m in (0xc0, 0xc2))
        # the first component's Tq -> 3: a table that no DQT of the file defines
        assert not any(data[o + 4] & 15 == 3 for m, o, n in segs if m == 0xdb)
        files[f"{name}_undefined_tq.jpg"] = H._set(data, sof + 12, 1, 3)
        # every DQT removed
        cut = data
        for m, o, n in reversed(segs):
            if m == 0xdb:
                cut = cut[:o] + cut[o + 2 + n:]
        files[f"{name}_no_dqt.jpg"] = cut
        sos = next(o for m, o, n in segs if m == 0xda)
        for counts in ([3] + [0] * 15, [0, 5] + [0] * 14, [2, 1] + [0] * 14):
            seg = bytes([0x00] + counts) + bytes(range(sum(counts)))
            files[f"{name}_dht_oversubscribed_{counts[0]}_{counts[1]}.jpg"] = data[:sos] + b"\xff\xc4" + struct.pack(">H", len(seg) + 2) + seg + data[sos:]
    grey8 = b"".join(bytes([0]) + bytes(range(8 * y, 8 * y + 8)) for y in range(8))
    files["filter_5.png"] = H.png(8, 8, 8, 0, bytes([5]) + grey8[1:])
    files["filter_5_last_row.png"] = H.png(8, 8, 8, 0, grey8[:63] + bytes([5]) + grey8[64:])
    idx = bytes([0, 0, 1, 2, 3, 0, 4, 5, 6, 7, 0, 8, 9, 1, 10])
    files["index_10_of_10.png"] = H.png(4, 3, 8, 3, idx, before=H.chunk(b"PLTE", bytes(range(30))))
    files["index_2_of_2_1bit.png"] = H.png(8, 1, 2, 3, bytes([0, 0x12, 0x00]), before=H.chunk(b"PLTE", bytes(range(6))))
    files["index_9_of_10.png"] = H.png(4, 3, 8, 3, idx[:-1] + bytes([9]), before=H.chunk(b"PLTE", bytes(range(30))))
    names = write(tmp_path, list(files.items()))
    got = run(harness["san"], "tex", str(tmp_path), names)
    assert tex(got["index_9_of_10.png"])[0][:3] == (4, 3, 4)  # the control: the last index inside the palette loads
    assert not [n for n in names if n != "index_9_of_10.png" and not refused("tex", got[n])]


# ------------------------------------------------------------------------------------------- differential on the smallest shapes
def _product_texels(tmp_path, name):
    import prt_amd
    (tmp_path / "q.mtl").write_text(f"newmtl a\nKd 1 1 1\nmap_Kd {name}\n")
    (tmp_path / "q.obj").write_text("mtllib q.mtl\n" + H.TRIANGLE + "usemtl a\nf 1/1 2/2 3/3\n")
    sc = prt_amd.Scene()
    sc.add(prt_amd.Mesh.load_obj(str(tmp_path / "q.obj")))
    textures = sc.arrays()["textures"]
    assert len(textures) == 1, f"{name} did not load"
    return textures[0]


def _as_loaded(a):
    """Texture::load (texture.cpp:218-249): one channel for a grey file; grey + alpha becomes (g, g, g, a); RGB gets alpha 255."""
    a = np.asarray(a)
    if a.ndim == 2: return a[..., None].astype(np.uint8)
    if a.shape[2] == 1: return a.astype(np.uint8)
    if a.shape[2] == 2: return np.dstack([a[..., 0]] * 3 + [a[..., 1]]).astype(np.uint8)
    if a.shape[2] == 3: return np.dstack([a, np.full(a.shape[:2], 255)]).astype(np.uint8)
    return a.astype(np.uint8)


def _pillow_expectation(name, data):
    """What the product documents for the file, from Pillow's decoding of it."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    key = im.info.get("transparency")
    if name.endswith(".png"):
        if im.mode == "P" or im.mode == "PA":
            return np.asarray(im.convert("RGBA"))
        if im.mode.startswith("I;16") or im.mode == "I":
            # 16-bit grey: Pillow hands out the samples as stored.  decodePng keeps the HIGH BYTE (stb_image's conversion), and a colour
            # key is compared with the 16-bit sample
            raw = np.asarray(im).astype(np.uint32)
            g = (raw >> 8).astype(np.uint8)
            return g[..., None] if key is None else np.dstack([g, g, g, np.where(raw == key, 0, 255)]).astype(np.uint8)
        if im.mode == "1":
            return (np.asarray(im).astype(np.uint8) * 255)[..., None]
        a = np.asarray(im)
        if key is not None and im.mode == "L":
            return np.dstack([a, a, a, np.where(a == key, 0, 255)]).astype(np.uint8)
        if key is not None and im.mode == "RGB":
            # (16-bit RGB reaches Pillow as its high bytes, the product's rule; the key is compared at the precision Pillow kept, which
            # tells the one keyed pixel of these seeded files from the others as the 16-bit comparison does)
            k = np.array([v >> 8 if max(key) > 255 else v for v in key])
            return np.dstack([a, np.where((a == k).all(-1), 0, 255)]).astype(np.uint8)
        return _as_loaded(a)
    return _as_loaded(np.asarray(im))


@pytest.fixture(scope="module")
def smallest(tmp_path_factory):
    d = tmp_path_factory.mktemp("smallest")
    files = H.smallest_valid(d)
    write(d, [(n, b) for n, _, b in files])
    return d, files


def test_png_tga_and_pnm_texels_equal_pillows_on_the_smallest_shapes(smallest):
    """1 x 1, 1 x N, N x 1 in every format; PNG at bit depths 1, 2, 4 and 16 with and without Adam7 (passes of no pixels), palettes and
    colour keys; TGA in all four orientations, raw and with packets that cross row ends; PAM of depth 2 and 4: byte for byte what Pillow decodes, after
    the conversions the product documents (the high byte of 16-bit samples, grey + alpha to (g, g, g, a), alpha 255 where there is none).
    Pillow reads no PAM: those are held to the samples they were written from."""
    pytest.importorskip("PIL.Image")
    d, files = smallest
    checked = 0
    for name, kind, data in files:
        if kind == "jpeg":
            continue
        got = _product_texels(d, name)
        if name.startswith("tga_packets_cross_rows_"):
            # Pillow refuses a run-length packet that crosses a row end (TGA 2.0 advises writers against them; readers meet them):
            # the reference is Pillow's decoding of the SAME pixels stored raw, in the same orientation
            raw_name = name.replace("tga_packets_cross_rows_", "tga_raw_")
            want = _pillow_expectation(raw_name, next(b for n, _, b in files if n == raw_name))
        elif name.endswith(".pam"):
            hd = data.index(b"ENDHDR\n") + 7
            w, h, depth = (int(data[:hd].split(key)[1].split()[0]) for key in (b"WIDTH", b"HEIGHT", b"DEPTH"))
            want = _as_loaded(np.frombuffer(data[hd:], np.uint8).reshape(h, w, depth))
        else:
            want = _pillow_expectation(name, data)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got, want), name
        checked += 1
    assert checked >= 150


# test_png_and_jpeg_files_written_by_an_independent_library's bounds for two conforming decoders (stb_image's integer IDCT, resamplers
# and fixed-point YCbCr, which decodeJpeg restates, against libjpeg's): the largest difference of a sample per chroma sampling, and the
# mean.  4:4:0 halves the chroma in one direction as 4:2:2 does, 4:1:1 quarters it as 4:2:0 does: they take those bounds.
JPEG_MAX = {"444": 3, "422": 6, "420": 8, "grey": 2, "440": 6, "411": 8}
JPEG_MEAN = {False: 0.8, True: 0.9}  # baseline, progressive


def test_jpeg_texels_stay_within_the_two_decoder_bound_on_the_smallest_shapes(smallest):
    """1 x 1, 9 x 17 and 17 x 9 (one MCU, and ragged against 8 and 16) at 4:4:4, 4:2:2, 4:2:0, 4:4:0, 4:1:1 and grey, baseline and
    progressive, with and without restart intervals, against Pillow (libjpeg).  The mean is taken over all files of a sampling: one
    pixel has no mean to speak of."""
    pytest.importorskip("PIL.Image")
    d, files = smallest
    pooled = {}
    for name, kind, data in files:
        if kind != "jpeg":
            continue
        sampling = name.split("_")[1]
        got = _product_texels(d, name).astype(np.int32)
        want = _pillow_expectation(name, data).astype(np.int32)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        diff = np.abs(got - want)[..., :3]
        if sampling == "422" and diff.shape[1] > 2:
            # as in that test: stb_image's horizontal 2x resampler weighs the last pair of a row the other way round than libjpeg's
            assert diff[:, -2:].max() <= 128, name
            diff = diff[:, :-2]
        print(f"{name}: max {int(diff.max())} mean {float(diff.mean()):.3f}")
        assert diff.max() <= JPEG_MAX[sampling], (name, int(diff.max()))
        pooled.setdefault((sampling, "_prog1_" in name), []).append(diff.reshape(-1))
    assert len(pooled) >= 10
    for (sampling, progressive), diffs in pooled.items():
        mean = float(np.concatenate(diffs).mean())
        assert mean < JPEG_MEAN[progressive], (sampling, progressive, mean)


# ------------------------------------------------------------------------------------------------------------- the C boundary
CHILD = r"""
import sys
import numpy as np
import prt_amd
mesh = prt_amd.Mesh.load_obj(sys.argv[1])          # must return: the texture is unreadable, the mesh is not
scene = prt_amd.Scene()
scene.add(mesh)
a = scene.arrays()
mats = a["meshes"][0]["materials"]
assert len(a["textures"]) == 0 and int(mats["diffuseMap"][0]) == -1 and int(mats["bumpMap"][0]) == -1, "the material kept a map"
for path in sys.argv[2:]:
    try:
        scene.set_infinite_area_light(path)
    except prt_amd.PrtError:
        pass
    else:
        raise AssertionError(path + " loaded")
    assert scene.arrays()["env"] is None
print("boundary ok")
"""


def test_no_exception_crosses_the_c_boundary(tmp_path):
    """Mesh.load_obj on an OBJ whose MTL names header-only 65535 x 65535 files, and Scene.set_infinite_area_light on oversize OpenEXR and
    PFM files, in a fresh Python process that may map 2 GB: the calls return, the material keeps no map, the light raises PrtError, the
    child exits with status 0.  (An exception that leaves prt_host_mesh_load_obj ends the interpreter: extern "C" has nowhere to
    pass it.)"""
    files = {n: b for n, k, b in H.oversize_claims()}
    for n in ("header_only_65535x65535.tga", "header_only_65535x65535.png", "window_65536x65536.exr", "window_2_31_minus_1.exr", "header_only_65535x65535.pfm"):
        (tmp_path / n).write_bytes(files[n])
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 1 1 1\nmap_Kd header_only_65535x65535.tga\nmap_bump header_only_65535x65535.png\n")
    (tmp_path / "m.obj").write_text("mtllib m.mtl\n" + H.TRIANGLE + "usemtl a\nf 1/1 2/2 3/3\n")
    env = dict(os.environ)  # as it is: nothing is added to it but the tree's own path
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "m.obj"), str(tmp_path / "window_65536x65536.exr"),
                        str(tmp_path / "window_2_31_minus_1.exr"), str(tmp_path / "header_only_65535x65535.pfm")],
                       capture_output=True, text=True, env=env, timeout=300, preexec_fn=_limit)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    assert "boundary ok" in r.stdout
