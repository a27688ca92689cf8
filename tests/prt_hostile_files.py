"""Hostile files for the host asset readers (prt_amd/csrc/host: PNM / TGA / PNG / JPEG textures, OBJ / MTL, OpenEXR / PFM environment
maps): a seeded, deterministic corpus, generated at test time from small valid files that Pillow and the test-side writers of
prt_images.py produce.  Nothing is read from outside the test tree and nothing is committed.

Seven families, each a function that returns a list of (file name, bytes) -- or, for OBJ, (case name, {file name: bytes}):
truncations, field_edits_*, byte_mutations, oversize_claims, obj_cases, and smallest_valid (the differential test's shapes).
sources() gives the valid files the first three start from: {name: (kind, bytes)}, kind in tga / pnm / png / jpeg / exr."""
import io
import os
import struct
import zlib

import numpy as np

from prt_images import _jpeg, _png, _png_general, _tga, _write_exr

MODE = {"tga": "tex", "pnm": "tex", "png": "tex", "jpeg": "tex", "exr": "env", "pfm": "env"}  # the harness mode that reads a kind
EXT = {"tga": ".tga", "pnm": ".ppm", "png": ".png", "jpeg": ".jpg", "exr": ".exr", "pfm": ".pfm"}


def _via(tmp, name, writer, *a, **kw):
    p = os.path.join(str(tmp), name)
    writer(p, *a, **kw)
    with open(p, "rb") as f:
        return f.read()


def _pil(arr, mode, fmt, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr, mode).save(b, fmt, **kw)
    return b.getvalue()


def _pattern(h, w, ch, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 9 + yy * 5 + 40 * c) % 256 for c in range(ch)], axis=2)
    img = np.clip(base + rng.integers(-12, 13, base.shape), 0, 255).astype(np.uint8)
    img[h // 3:h // 3 + 2] = img[h // 3, 0]  # runs, for the run-length and LZ77 paths
    return img if ch > 1 else img[..., 0]


def pnm(magic, w, h, body, maxval=255):
    return f"{magic}\n{w} {h}\n{maxval}\n".encode() + body


def pam(w, h, depth, body, maxval=255, endhdr=True):
    return (f"P7\nWIDTH {w}\nHEIGHT {h}\nDEPTH {depth}\nMAXVAL {maxval}\nTUPLTYPE X\n" + ("ENDHDR\n" if endhdr else "")).encode() + body


def sources(tmp):
    """Small valid files: {name: (kind, bytes)}.  The largest is 64 x 64."""
    s = {}
    rgba = _pattern(6, 9, 4, 1)
    s["tga_raw"] = ("tga", _via(tmp, "s.tga", _tga, rgba, False, False))
    s["tga_rle"] = ("tga", _via(tmp, "s.tga", _tga, rgba, True, True))
    s["tga_grey_rle"] = ("tga", _via(tmp, "s.tga", _tga, _pattern(5, 7, 1, 2), True, False))
    s["ppm"] = ("pnm", pnm("P6", 7, 5, _pattern(5, 7, 3, 3).tobytes()))
    s["pgm"] = ("pnm", pnm("P5", 7, 5, _pattern(5, 7, 1, 4).tobytes()))
    s["pam"] = ("pnm", pam(5, 4, 4, _pattern(4, 5, 4, 5).tobytes()))
    s["png_rgba"] = ("png", _via(tmp, "s.png", _png, _pattern(13, 11, 4, 6)))
    rng = np.random.default_rng(7)
    s["png_palette"] = ("png", _via(tmp, "s.png", _png, rng.integers(0, 7, (6, 4), dtype=np.uint8), palette=rng.integers(0, 256, (7, 3)),
                                    trns=[255, 0, 128]))
    s["png_adam7_16"] = ("png", _via(tmp, "s.png", _png_general, rng.integers(0, 65536, (11, 13, 2)), 16, 4, True))
    s["png_pillow_64"] = ("png", _pil(_pattern(64, 64, 3, 8), "RGB", "PNG"))
    s["jpeg_420"] = ("jpeg", _pil(_pattern(17, 9, 3, 9), "RGB", "JPEG", quality=85, subsampling=2))
    s["jpeg_grey_restart"] = ("jpeg", _pil(_pattern(17, 20, 1, 10), "L", "JPEG", quality=90, restart_marker_blocks=1))
    s["jpeg_progressive"] = ("jpeg", _pil(_pattern(17, 9, 3, 11), "RGB", "JPEG", quality=80, subsampling=1, progressive=True))
    f = np.random.default_rng(12).random((20, 9)).astype(np.float32)
    chans = {"R": f, "G": (f * 2).astype(np.float16), "B": (f * 3).astype(np.float32), "A": np.full((20, 9), 0.5, np.float32)}
    for comp, name in ((0, "exr_raw"), (1, "exr_rle"), (3, "exr_zip")):
        s[name] = ("exr", _via(tmp, "s.exr", _write_exr, chans, 3, 5, comp))
    return s


# ----------------------------------------------------------------------------------------------------------------- 1. truncations
def header_length(kind, data):
    """Bytes up to where the samples (or the entropy-coded / compressed data) begin."""
    if kind == "tga":
        return 18 + data[0]
    if kind == "pnm":
        return (data.index(b"ENDHDR\n") + 7) if data[:2] == b"P7" else len(b"\n".join(data.split(b"\n", 3)[:3])) + 1
    if kind == "png":
        return data.index(b"IDAT") + 4
    if kind == "jpeg":
        i = data.index(b"\xff\xda")
        return i + 4 + struct.unpack_from(">H", data, i + 2)[0]
    if kind == "exr":
        return exr_table(data) + 8
    raise ValueError(kind)


def truncations(kind, data, seed, sample=160):
    """Every strict prefix of a source under about 700 bytes; of a larger one every length through the headers, then a seeded sample."""
    n = len(data)
    if n <= 700:
        lengths = range(n)
    else:
        hd = min(header_length(kind, data) + 16, n)
        rng = np.random.default_rng(seed)
        lengths = sorted(set(range(hd)) | set(int(x) for x in rng.integers(hd, n, sample)) | {n - 1, n - 2})
    return [(f"cut{k:05d}{EXT[kind]}", data[:k]) for k in lengths]


# ----------------------------------------------------------------------------------------------------------------- 2. field edits
def _values(nbytes):
    top = (1 << (8 * nbytes)) - 1
    return [0, 1, top, top - 1, 1 << (8 * nbytes - 1)]


def _set(data, off, nbytes, value, big=False):
    b = bytearray(data)
    b[off:off + nbytes] = int(value).to_bytes(nbytes, "big" if big else "little")
    return bytes(b)


def field_edits_tga(src):
    """src: {name: (kind, bytes)} of sources()."""
    out = []
    for name in ("tga_raw", "tga_rle", "tga_grey_rle"):
        data = src[name][1]
        for field, off, nb in (("idLength", 0, 1), ("colorMapType", 1, 1), ("type", 2, 1), ("width", 12, 2), ("height", 14, 2), ("bpp", 16, 1),
                               ("descriptor", 17, 1)):
            for v in _values(nb) + ([2, 3, 9, 10, 11] if field == "type" else []) + ([8, 16, 24, 32] if field == "bpp" else []) + \
                    ([0x10, 0x20, 0x30] if field == "descriptor" else []):
                out.append((f"{name}_{field}_{v}.tga", _set(data, off, nb, v)))
    # run-length packets that cross the end of the image: 3 x 2 pixels, a run / a literal packet of 128 as the last one, and as the only one
    hd = struct.pack("<BBBHHBHHHHBB", 0, 0, 10, 0, 0, 0, 0, 0, 3, 2, 24, 0)
    out.append(("rle_run_past_end.tga", hd + bytes([0x84]) + b"abc" + bytes([0xff]) + b"xyz"))
    out.append(("rle_literal_past_end.tga", hd + bytes([0x04]) + b"abc" * 5 + bytes([0x7f]) + b"xyz" * 128))
    out.append(("rle_one_packet_past_end.tga", hd + bytes([0xff]) + b"abc"))
    out.append(("rle_exact.tga", hd + bytes([0x85]) + b"abc"))
    return out


def field_edits_pnm():
    body3, body1 = bytes(range(7 * 5 * 3)), bytes(range(35))
    numbers = [0, 1, 65535, 65534, 65536, 2147483647, 2147483648, -1, -2147483648, 99999999999999999999]
    out = []
    for v in numbers:
        out.append((f"ppm_width_{v}.ppm", pnm("P6", v, 5, body3)))
        out.append((f"ppm_height_{v}.ppm", pnm("P6", 7, v, body3)))
        out.append((f"pgm_width_{v}.ppm", pnm("P5", v, 5, body1)))
        out.append((f"pam_width_{v}.ppm", pam(v, 5, 3, body3)))
        out.append((f"pam_height_{v}.ppm", pam(7, v, 3, body3)))
        out.append((f"pam_depth_{v}.ppm", pam(7, 5, v, body3)))
    for v in (0, 1, 254, 255, 256, 65535, 32768, -1):
        out.append((f"ppm_maxval_{v}.ppm", pnm("P6", 7, 5, body3, v)))
        out.append((f"pam_maxval_{v}.ppm", pam(7, 5, 3, body3, v)))
    for d in (0, 1, 2, 3, 4, 5, 255):
        out.append((f"pam_depth{d}_sized.ppm", pam(7, 5, d, bytes(7 * 5 * max(d, 1)))))
    out.append(("pam_no_endhdr.ppm", pam(7, 5, 3, body3, endhdr=False)))
    out.append(("pam_header_only.ppm", pam(7, 5, 3, b"")))
    out.append(("ppm_header_only.ppm", pnm("P6", 7, 5, b"")))
    out.append(("ppm_magic_only.ppm", b"P6"))
    out.append(("pam_magic_only.ppm", b"P7\n"))
    out.append(("pam_key_without_value.ppm", b"P7\nWIDTH"))
    out.append(("ppm_words.ppm", b"P6\nseven five 255\n" + body3))
    out.append(("p4.ppm", b"P4\n7 5\n" + bytes(5)))
    return out


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


PNG_SIG = b"\x89PNG\r\n\x1a\n"


def png(w, h, bits, ctype, raw=None, z=None, interlace=0, before=b"", idats=1, comp=0, filt=0):
    """A PNG around filtered scanline bytes `raw` (deflated here) or a ready zlib stream `z`; `before`: chunks between IHDR and IDAT."""
    if z is None:
        z = zlib.compress(raw, 6)
    cut = [len(z) * k // idats for k in range(idats + 1)]
    return PNG_SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bits, ctype, comp, filt, interlace)) + before + \
        b"".join(chunk(b"IDAT", z[a:b]) for a, b in zip(cut, cut[1:])) + chunk(b"IEND", b"")


def _png_chunks(data):
    """[(offset of the length field, tag, length)]."""
    out, o = [], 8
    while o + 12 <= len(data):
        n = struct.unpack_from(">I", data, o)[0]
        out.append((o, data[o + 4:o + 8], n))
        o += 12 + n
    return out


def field_edits_png(src):
    out = []
    grey8 = b"".join(bytes([0]) + bytes(range(8 * y, 8 * y + 8)) for y in range(8))  # 8 x 8, 8-bit grey, filter 0
    for name in ("png_rgba", "png_palette", "png_adam7_16"):
        data = src[name][1]
        ihdr = data.index(b"IHDR") + 4
        for k in range(13):  # every IHDR byte
            for v in _values(1) + [2, 3, 4, 6, 8, 16]:
                out.append((f"{name}_ihdr{k:02d}_{v}.png", _set(data, ihdr + k, 1, v)))
        for o, tag, n in _png_chunks(data):  # chunk lengths
            for v in (0, 1, n - 1 if n else 2, n + 1, 0x7fffffff, 0x80000000, 0xffffffff):
                out.append((f"{name}_{tag.decode()}{o}_len_{v}.png", _set(data, o, 4, v, big=True)))
        first = data.index(b"IDAT") - 4
        out.append((f"{name}_no_ihdr.png", data[:8] + data[8 + 25:]))
        out.append((f"{name}_idat_before_ihdr.png", data[:8] + data[first:-12] + data[8:8 + 25] + data[-12:]))
        out.append((f"{name}_no_idat.png", data[:first] + data[-12:]))
        out.append((f"{name}_no_iend.png", data[:-12]))
        out.append((f"{name}_two_ihdr.png", data[:8 + 25] + chunk(b"IHDR", struct.pack(">IIBBBBB", 4096, 4096, 16, 6, 0, 0, 0)) + data[8 + 25:]))
    idx = bytes([0, 0, 1, 2, 3, 0, 4, 5, 6, 7, 0, 8, 9, 200, 255])  # 3 rows of 4 indices, filter 0
    pal = bytes(range(30))
    for n in (0, 1, 2, 3, 4, 29, 30):  # a short PLTE, and palette indices beyond it (the last row names entries 200 and 255)
        out.append((f"plte_{n}_bytes.png", png(4, 3, 8, 3, idx, before=chunk(b"PLTE", pal[:n]))))
    out.append(("plte_missing.png", png(4, 3, 8, 3, idx)))
    out.append(("plte_index_inside.png", png(4, 3, 8, 3, idx[:10] + bytes([0, 8, 9, 1, 2]), before=chunk(b"PLTE", pal))))
    for bits in (1, 2, 4):  # every index of a 2-entry palette and beyond, packed
        out.append((f"plte_2_entries_{bits}bit.png", png(8, 1, bits, 3, bytes([0]) + bytes([0xe4] * bits), before=chunk(b"PLTE", pal[:6]))))
    for n in range(8):  # tRNS of every length 0 to 7 on grey, RGB and palette files
        t = chunk(b"tRNS", bytes([0, 9, 0, 10, 0, 11, 0][:n]))
        out.append((f"trns_{n}_grey.png", png(8, 8, 8, 0, grey8, before=t)))
        out.append((f"trns_{n}_grey16.png", png(4, 8, 16, 0, grey8, before=t)))
        out.append((f"trns_{n}_rgb.png", png(4, 2, 8, 2, bytes([0]) + bytes(range(9, 21)) + bytes([0]) + bytes(12), before=t)))
        out.append((f"trns_{n}_palette.png", png(4, 3, 8, 3, idx[:10] + bytes([0, 8, 9, 1, 2]), before=chunk(b"PLTE", pal) + t)))
        out.append((f"trns_{n}_grey_alpha.png", png(4, 8, 8, 4, grey8, before=t)))
    for ft in (5, 6, 255):  # filter types beyond Paeth, in the first row and in a later one
        out.append((f"filter_{ft}_first_row.png", png(8, 8, 8, 0, bytes([ft]) + grey8[1:])))
        out.append((f"filter_{ft}_later_row.png", png(8, 8, 8, 0, grey8[:27] + bytes([ft]) + grey8[28:])))
    # Adam7 passes of zero width or height: valid files (1 x 1, 1 x 5, 5 x 1, 2 x 2) and the same with too little data
    for w, h in ((1, 1), (1, 5), (5, 1), (2, 2), (3, 9)):
        rows = _adam7_rows(np.arange(w * h, dtype=np.uint8).reshape(h, w, 1) + 7, 8)
        out.append((f"adam7_{w}x{h}.png", png(w, h, 8, 0, rows, interlace=1)))
        out.append((f"adam7_{w}x{h}_short.png", png(w, h, 8, 0, rows[:-1], interlace=1)))
    out.append(("interlace_2.png", png(8, 8, 8, 0, grey8, interlace=2)))
    out.append(("idat_empty.png", png(8, 8, 8, 0, z=b"")))
    out.append(("idat_two_bytes.png", png(8, 8, 8, 0, z=b"\x78\x9c")))
    out.append(("idat_in_9_chunks.png", png(8, 8, 8, 0, grey8, idats=9)))
    return out


def _adam7_rows(samples, bits):
    """Filter-0 scanlines of the seven passes of an (h, w, ch) 8-bit image."""
    out = bytearray()
    for x0, y0, dx, dy in zip((0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1), (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)):
        sub = samples[y0::dy, x0::dx]
        if sub.size:
            for row in sub:
                out += bytes([0]) + row.astype(np.uint8).tobytes()
    return bytes(out)


class Bits:
    """Deflate's bit order: fields least significant bit first, Huffman codes most significant bit first."""

    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits += [(v >> k) & 1 for k in range(n)]
        return self

    def code(self, v, n):
        self.bits += [(v >> k) & 1 for k in range(n - 1, -1, -1)]
        return self

    def fixed(self, sym):  # RFC 1951 3.2.6
        if sym < 144: return self.code(0x30 + sym, 8)
        if sym < 256: return self.code(0x190 + sym - 144, 9)
        if sym < 280: return self.code(sym - 256, 7)
        return self.code(0xc0 + sym - 280, 8)

    def bytes(self, pad=0):
        b = self.bits + [pad] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def zlib_streams():
    """{name: zlib stream} of malformed deflate data, for an image that needs 72 bytes (8 x 8 grey)."""
    raw = b"".join(bytes([0]) + bytes(range(8 * y, 8 * y + 8)) for y in range(8))
    hd = b"\x78\x01"
    s = {}
    s["stored_len_past_data"] = hd + bytes([1]) + struct.pack("<HH", 1000, 1000 ^ 0xffff) + raw
    s["stored_len_65535"] = hd + bytes([1]) + struct.pack("<HH", 65535, 0) + raw
    s["stored_nlen_wrong"] = hd + bytes([1]) + struct.pack("<HH", 72, 0x1234) + raw
    s["stored_cut_in_len"] = hd + bytes([1, 72])
    s["block_type_3"] = hd + bytes([7]) + raw

    def dynamic(hlit, hdist, cl, syms, tail=b"\xff" * 8):
        """cl: {symbol of the code-length alphabet: (code, length)}; syms: [(symbol, extra value, extra bits)]."""
        b = Bits().put(1, 1).put(2, 2).put(hlit, 5).put(hdist, 5).put(15, 4)
        for k in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
            b.put(cl[k][1] if k in cl else 0, 3)
        for sym, extra, n in syms:
            b.code(*cl[sym])
            b.put(extra, n)
        return hd + b.bytes() + tail

    two = {8: (0, 1), 16: (1, 1)}         # a complete code of two symbols: 8 -> "0", 16 -> "1"
    three = {8: (0, 1), 16: (2, 2), 18: (3, 2)}
    s["hlit_hdist_max"] = dynamic(31, 31, two, [(8, 0, 0)] * 320)                      # 288 + 32 lengths, every one 8
    s["hlit_max_hdist_30"] = dynamic(31, 29, two, [(8, 0, 0)] * 318)
    s["repeat_16_first"] = dynamic(0, 0, two, [(16, 0, 2)] + [(8, 0, 0)] * 255)
    s["repeat_past_table"] = dynamic(0, 0, three, [(8, 0, 0)] * 250 + [(18, 127, 7)])   # 250 + 138 > 258
    s["repeat_16_past_table"] = dynamic(0, 0, three, [(8, 0, 0)] * 256 + [(16, 3, 2)])  # 256 + 6 > 258
    s["code_lengths_oversubscribed"] = dynamic(0, 0, {1: (0, 1), 16: (1, 1)}, [(1, 0, 0)] * 258)  # 257 literal codes of one bit
    s["code_lengths_incomplete"] = dynamic(0, 0, {0: (0, 1), 2: (1, 1)}, [(2, 0, 0)] + [(0, 0, 0)] * 257, tail=b"\x00" * 8)
    s["code_lengths_all_zero"] = dynamic(0, 0, {0: (0, 1), 2: (1, 1)}, [(0, 0, 0)] * 258)
    s["code_length_code_oversubscribed"] = dynamic(0, 0, {0: (0, 1), 8: (1, 1), 16: (0, 1), 17: (1, 1)}, [(8, 0, 0)] * 258)
    s["code_length_code_empty"] = dynamic(0, 0, {}, [])

    def fixed(*ops, end=True, tail=b""):
        b = Bits().put(1, 1).put(1, 2)
        for op in ops:
            if op[0] == "lit":
                for v in op[1]:
                    b.fixed(v)
            else:  # ("match", length symbol, extra, extra bits, distance symbol, extra, extra bits)
                b.fixed(op[1]).put(op[2], op[3]).code(op[4], 5).put(op[5], op[6])
        if end:
            b.fixed(256)
        return hd + b.bytes() + tail
    s["distance_beyond_output"] = fixed(("lit", raw[:1]), ("match", 257, 0, 0, 4, 0, 1), ("lit", raw))
    s["distance_at_start"] = fixed(("match", 257, 0, 0, 0, 0, 0), ("lit", raw))
    s["distance_32768"] = fixed(("lit", raw[:40]), ("match", 285, 0, 0, 29, 8191, 13), ("lit", raw))
    for d in (30, 31):
        s[f"distance_symbol_{d}"] = fixed(("lit", raw[:9]), ("match", 257, 0, 0, d, 0, 0), ("lit", raw))
    for sym in (286, 287):
        s[f"length_symbol_{sym}"] = fixed(("lit", raw[:9]), ("match", sym, 0, 0, 0, 0, 0), ("lit", raw))
    s["no_end_of_block"] = fixed(("lit", raw), end=False)
    s["no_end_of_block_short"] = fixed(("lit", raw[:50]), end=False)
    s["match_fills_the_image"] = fixed(("lit", bytes([0])), ("match", 285, 0, 0, 0, 0, 0), tail=b"\x00" * 4)  # 1 + 258 zeros: more than 72
    s["valid_fixed"] = fixed(("lit", raw), tail=struct.pack(">I", zlib.adler32(raw)))
    return s


def field_edits_png_zlib():
    return [(f"z_{name}.png", png(8, 8, 8, 0, z=z)) for name, z in zlib_streams().items()]


def jpeg_segments(data):
    """[(marker, offset of the marker's 0xff, length field)] up to and including SOS."""
    out, o = [], 2
    while o + 4 <= len(data):
        assert data[o] == 0xff
        m, n = data[o + 1], struct.unpack_from(">H", data, o + 2)[0]
        out.append((m, o, n))
        if m == 0xda:
            break
        o += 2 + n
    return out


def field_edits_jpeg(src):
    out = []
    for name in ("jpeg_420", "jpeg_grey_restart", "jpeg_progressive"):
        data = src[name][1]
        segs = jpeg_segments(data)
        at = {}
        for m, o, n in segs:
            at.setdefault(m, o)
        sof = at[0xc2] if 0xc2 in at else at[0xc0]
        ncomp = data[sof + 9]

        def add(what, b):
            out.append((f"{name}_{what}.jpg", bytes(b)))
        for field, off, nb in (("height", 5, 2), ("width", 7, 2)):
            for v in _values(nb):
                add(f"sof_{field}_{v}", _set(data, sof + off, nb, v, big=True))
        for v in _values(1) + [8, 12, 16]:
            add(f"sof_precision_{v}", _set(data, sof + 4, 1, v))
        for v in _values(1) + [2, 3, 4]:
            add(f"sof_components_{v}", _set(data, sof + 9, 1, v))
        for c in range(ncomp):
            for v in (0x00, 0x01, 0x10, 0x15, 0x51, 0x55, 0x11, 0x12, 0x21, 0x22, 0x33, 0x34, 0x44, 0xff):  # sampling factors 0 and 5, and pairs that do not divide
                add(f"sof_c{c}_sampling_{v:02x}", _set(data, sof + 11 + 3 * c, 1, v))
            for v in (0, 1, 2, 3, 4, 255):
                add(f"sof_c{c}_tq_{v}", _set(data, sof + 12 + 3 * c, 1, v))
            for v in _values(1):
                add(f"sof_c{c}_id_{v}", _set(data, sof + 10 + 3 * c, 1, v))
        for m, o, n in segs:  # marker lengths 0, 1 and 65535, and off by one
            for v in (0, 1, 2, n - 1, n + 1, 65535):
                add(f"{m:02x}at{o}_length_{v}", _set(data, o + 2, 2, v, big=True))
        for m, o, n in segs:  # a segment missing (DQT, DHT, SOF, ...), and twice
            add(f"{m:02x}at{o}_missing", data[:o] + data[o + 2 + n:])
            add(f"{m:02x}at{o}_twice", data[:o] + data[o:o + 2 + n] * 2 + data[o + 2 + n:])
        for m, o, n in segs:
            if m == 0xdb:
                for v in (0x00, 0x01, 0x03, 0x04, 0x0f, 0x10, 0x20, 0xf0):  # DQT precision 1 and 2, table ids up to 15
                    add(f"dqt{o}_pq_tq_{v:02x}", _set(data, o + 4, 1, v))
            if m == 0xc4:
                for v in (0x00, 0x03, 0x04, 0x10, 0x13, 0x14, 0x20, 0xff):
                    add(f"dht{o}_tc_th_{v:02x}", _set(data, o + 4, 1, v))
                for k in range(16):
                    for v in (0, 1, 255, 254, 128):
                        add(f"dht{o}_count{k:02d}_{v}", _set(data, o + 5 + k, 1, v))
        # DHT totals of 256 and 257, and over-subscribed counts
        for total in (255, 256, 257):
            counts = [0] * 7 + [max(0, total - 255)] + [0] * 7 + [min(total, 255)]  # 8-bit and 16-bit codes
            seg = bytes([0x00] + counts) + bytes(range(256))[:total] + bytes(max(0, total - 256))
            add(f"dht_total_{total}", data[:at[0xda]] + b"\xff\xc4" + struct.pack(">H", len(seg) + 2) + seg + data[at[0xda]:])
        for counts in ([3] + [0] * 15, [2, 1] + [0] * 14, [0, 5] + [0] * 14, [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3]):
            seg = bytes([0x00] + counts) + bytes(range(sum(counts)))
            add("dht_oversubscribed_" + "_".join(map(str, counts[:3])) + f"_{counts[15]}",
                data[:at[0xda]] + b"\xff\xc4" + struct.pack(">H", len(seg) + 2) + seg + data[at[0xda]:])
        sos = at[0xda]
        ns = data[sos + 4]
        for v in _values(1) + [2, 3, 4]:
            add(f"sos_components_{v}", _set(data, sos + 4, 1, v))
        for c in range(ns):
            for v in _values(1) + [9]:
                add(f"sos_c{c}_id_{v}", _set(data, sos + 5 + 2 * c, 1, v))
            for v in (0x00, 0x11, 0x22, 0x33, 0x04, 0x40, 0x44, 0xff):
                add(f"sos_c{c}_tables_{v:02x}", _set(data, sos + 6 + 2 * c, 1, v))
        tail = sos + 5 + 2 * ns
        for k, field in enumerate(("Ss", "Se", "AhAl")):
            for v in (0, 1, 5, 62, 63, 64, 255, 254, 128, 0x0d, 0x0e, 0xd0, 0xe0, 0x10, 0x01):
                add(f"sos_{field}_{v}", _set(data, tail + k, 1, v))
        if 0xdd in at:
            for v in _values(2) + [2, 3]:
                add(f"dri_interval_{v}", _set(data, at[0xdd] + 4, 2, v, big=True))
        else:
            for v in _values(2) + [2, 3]:
                add(f"dri_added_{v}", data[:sos] + b"\xff\xdd\x00\x04" + struct.pack(">H", v) + data[sos:])
        for L in (0, 2, 3, 5, 6):
            add(f"dri_length_{L}", data[:sos] + b"\xff\xdd" + struct.pack(">H", L) + b"\x00\x01\x00\x00"[:max(0, L - 2)] + data[sos:])
        add("second_sof_larger", data[:sos] + b"\xff\xc0" + struct.pack(">HBHHB", 11, 8, 4096, 4096, 1) + bytes([data[sof + 10], 0x11, 0]) + data[sos:])
        add("second_sof_same", data[:sos] + data[sof:sof + 2 + struct.unpack_from(">H", data, sof + 2)[0]] + data[sos:])
        add("eoi_before_sos", data[:sos] + b"\xff\xd9" + data[sos:])
        add("sof3_lossless", _set(data, sof + 1, 1, 0xc3))
        add("sof9_arithmetic", _set(data, sof + 1, 1, 0xc9))
        ecs = sos + 2 + struct.unpack_from(">H", data, sos + 2)[0]
        for k in (0, 1, 2, 3, 5, 9):  # entropy-coded data that ends in the middle of a block, with and without EOI
            add(f"entropy_{k}_bytes", data[:ecs + k])
            add(f"entropy_{k}_bytes_eoi", data[:ecs + k] + b"\xff\xd9")
        add("entropy_all_ones", data[:ecs] + b"\xff\x00" * 40 + b"\xff\xd9")
        add("entropy_all_zeros", data[:ecs] + b"\x00" * 80 + b"\xff\xd9")
    # a progressive file whose first scan is an AC scan (the second scan moved in front of the DC scan)
    data = src["jpeg_progressive"][1]
    scans = [i for i in range(len(data) - 1) if data[i] == 0xff and data[i + 1] == 0xda]
    if len(scans) >= 3:
        a, b, c = scans[0], scans[1], scans[2]
        # the DHT segments that precede a scan travel with it
        out.append(("jpeg_progressive_second_scan_first.jpg", data[:a] + data[b:c] + data[a:b] + data[c:]))
    return out


def exr_table(data):
    """Offset of the scan-line offset table: what follows the header's attributes (name, type, size, payload) and their terminating NUL."""
    pos = 8
    while data[pos]:
        pos = data.index(b"\0", pos) + 1           # name
        pos = data.index(b"\0", pos) + 1           # type
        pos += 4 + struct.unpack_from("<i", data, pos)[0]
    return pos + 1


def _exr_attr(data, name, typ):
    key = name + b"\0" + typ + b"\0"
    return data.index(key) + len(key) + 4


def field_edits_exr(src):
    out = []
    for name in ("exr_raw", "exr_rle", "exr_zip"):
        data = src[name][1]
        table = exr_table(data)
        for bad in (0xFFFFFFFFFFFFFFFC, 0xFFFFFFFFFFFFFFF8, len(data) - 4, len(data) + 1000, 0, 1, 1 << 63, table):  # the first four: the cases the suite has
            out.append((f"{name}_offset_{bad:x}.exr", _set(data, table, 8, bad)))
        out.append((f"{name}_channel_list_cut.exr", data[:_exr_attr(data, b"channels", b"chlist") + 2 + 4 + 2]))
        dw = _exr_attr(data, b"dataWindow", b"box2i")
        x0, y0, x1, y1 = struct.unpack_from("<iiii", data, dw)
        for k, field in enumerate(("x0", "y0", "x1", "y1")):  # negative and huge data windows
            for v in (0, 1, -1, 0x7fffffff, 0x7ffffffe, -0x80000000, 65535, 65536, (x0, y0, x1, y1)[k] + 1, (x0, y0, x1, y1)[k] - 1):
                out.append((f"{name}_window_{field}_{v}.exr", _set(data, dw + 4 * k, 4, v & 0xffffffff)))
        out.append((f"{name}_window_negative.exr", data[:dw] + struct.pack("<iiii", -9, -20, -1, -1) + data[dw + 16:]))
        out.append((f"{name}_window_whole_range.exr", data[:dw] + struct.pack("<iiii", -0x80000000, -0x80000000, 0x7fffffff, 0x7fffffff) + data[dw + 16:]))
        ch = _exr_attr(data, b"channels", b"chlist")
        size = struct.unpack_from("<i", data, ch - 4)[0]
        out.append((f"{name}_channel_list_without_terminator.exr", _set(data, ch + size - 1, 1, ord("Z"))))
        out.append((f"{name}_channel_list_size_0.exr", _set(data, ch - 4, 4, 0)))
        out.append((f"{name}_channel_list_size_negative.exr", _set(data, ch - 4, 4, 0xffffffff)))
        out.append((f"{name}_channel_list_size_huge.exr", _set(data, ch - 4, 4, 0x7fffffff)))
        for v in (0, 1, 2, 3, 255, 0x80000000):
            out.append((f"{name}_channel_type_{v}.exr", _set(data, ch + 2, 4, v)))   # the first channel is "A\0"
            out.append((f"{name}_channel_xsampling_{v}.exr", _set(data, ch + 10, 4, v)))
        co = _exr_attr(data, b"compression", b"compression")
        for v in range(0, 11):
            out.append((f"{name}_compression_{v}.exr", _set(data, co, 1, v)))
        for v in (0, 1, 2, 0x202, 0x802, 0x1002, 0xffffffff):
            out.append((f"{name}_version_{v:x}.exr", _set(data, 4, 4, v)))
        first = struct.unpack_from("<Q", data, table)[0]
        bsize = struct.unpack_from("<i", data, first + 4)[0]
        for v in (0, 1, bsize - 1, bsize + 1, len(data), 0x7fffffff, 0x80000000, 0xffffffff):  # a block size beyond the file, and off by one
            out.append((f"{name}_block_size_{v}.exr", _set(data, first + 4, 4, v)))
        for v in (y0 - 1, y1 + 1, 0x7fffffff, -0x80000000, y1):
            out.append((f"{name}_block_y_{v}.exr", _set(data, first, 4, v & 0xffffffff)))
    # a ZIP block that inflates to the wrong size: the LAST block of the ZIP file replaced (no offset moves)
    data = src["exr_zip"][1]
    table = exr_table(data)
    blocks = []
    k = table
    while struct.unpack_from("<Q", data, k)[0] > k:
        blocks.append(struct.unpack_from("<Q", data, k)[0])
        k += 8
        if k + 8 > blocks[0]:
            break
    last = max(blocks)
    y = data[last:last + 4]
    for what, payload in (("short", zlib.compress(bytes(100))), ("one_short", None), ("long", zlib.compress(bytes(1 << 16))), ("huge", zlib.compress(bytes(1 << 26), 9)),
                          ("empty", zlib.compress(b""))):
        if payload is None:
            good = zlib.decompress(data[last + 8:])
            payload = zlib.compress(good[:-1])
        out.append((f"exr_zip_block_inflates_{what}.exr", data[:last] + y + struct.pack("<i", len(payload)) + payload))
    # an RLE block that unpacks to too much
    data = src["exr_rle"][1]
    table = exr_table(data)
    first = struct.unpack_from("<Q", data, table)[0]
    bsize = struct.unpack_from("<i", data, first + 4)[0]
    runs = bytes([127, 7]) * (bsize // 2) + bytes([0] * (bsize % 2))
    out.append(("exr_rle_block_all_runs.exr", data[:first + 8] + runs + data[first + 8 + bsize:]))
    out.append(("exr_rle_block_literal_past_end.exr", data[:first + 8] + bytes([0x81]) * bsize + data[first + 8 + bsize:]))
    return out


# --------------------------------------------------------------------------------------------------------------- 3. byte mutations
def byte_mutations(kind, data, seed, count=1500):
    """One to three bytes of the source set to one of {0, 1, 0x7f, 0x80, 0xff, random}."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        b = bytearray(data)
        for _ in range(int(rng.integers(1, 4))):
            pos = int(rng.integers(0, len(b)))
            b[pos] = (0, 1, 0x7f, 0x80, 0xff, int(rng.integers(0, 256)))[int(rng.integers(0, 6))]
        out.append((f"mut{k:04d}{EXT[kind]}", bytes(b)))
    return out


# --------------------------------------------------------------------------------------------------------------- 4. oversize claims
def oversize_claims():
    """[(file name, kind, bytes)]: files whose headers claim far more than the bytes behind them."""
    out = []
    grey1 = _pil(np.full((8, 8), 99, np.uint8), "L", "JPEG", quality=90)  # a complete scan of one MCU
    sof = grey1.index(b"\xff\xc0")
    exr = _exr_small()
    dw = _exr_attr(exr, b"dataWindow", b"box2i")
    for w, h in ((65535, 65535), (65535, 1), (1, 65535)):
        tag = f"{w}x{h}"
        out.append((f"header_only_{tag}.tga", "tga", struct.pack("<BBBHHBHHHHBB", 0, 0, 2, 0, 0, 0, 0, 0, w, h, 32, 8)))
        out.append((f"header_only_rle_{tag}.tga", "tga", struct.pack("<BBBHHBHHHHBB", 0, 0, 10, 0, 0, 0, 0, 0, w, h, 32, 8)))
        out.append((f"header_only_{tag}.ppm", "pnm", pnm("P6", w, h, b"")))
        out.append((f"header_only_{tag}.pam", "pnm", pam(w, h, 4, b"")))
        empty = zlib.compress(b"")  # a complete zlib stream of no bytes: IHDR + this IDAT + IEND is 65 bytes
        out.append((f"header_only_{tag}.png", "png", png(w, h, 16, 6, z=empty)))
        out.append((f"header_only_8bit_grey_{tag}.png", "png", png(w, h, 8, 0, z=empty)))
        out.append((f"header_only_adam7_{tag}.png", "png", png(w, h, 16, 6, z=empty, interlace=1)))
        out.append((f"header_only_no_idat_bytes_{tag}.png", "png", png(w, h, 16, 6, z=b"")))
        for m in (0xc0, 0xc2):
            out.append((f"header_only_sof{m - 0xc0}_{tag}.jpg", "jpeg",
                        b"\xff\xd8\xff" + bytes([m]) + struct.pack(">HBHHB", 17, 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]) + b"\xff\xd9"))
        out.append((f"one_mcu_{tag}.jpg", "jpeg", grey1[:sof + 5] + struct.pack(">HH", h, w) + grey1[sof + 9:]))
        out.append((f"window_{tag}.exr", "exr", exr[:dw] + struct.pack("<iiii", 0, 0, w - 1, h - 1) + exr[dw + 16:]))
        out.append((f"header_only_{tag}.pfm", "pfm", f"PF\n{w} {h}\n-1.0\n".encode()))
    out.append(("window_65536x65536.exr", "exr", exr[:dw] + struct.pack("<iiii", 0, 0, 65535, 65535) + exr[dw + 16:]))
    for comp in (0, 1, 2, 3):
        co = _exr_attr(exr, b"compression", b"compression")
        out.append((f"window_65536x65536_compression_{comp}.exr", "exr", _set(exr[:dw] + struct.pack("<iiii", 0, 0, 65535, 65535) + exr[dw + 16:], co, 1, comp)))
    out.append(("window_2_31_minus_1.exr", "exr", exr[:dw] + struct.pack("<iiii", 0, 0, 0x7fffffff - 1, 0x7fffffff - 1) + exr[dw + 16:]))
    out.append(("window_x1_2_31_minus_1.exr", "exr", exr[:dw] + struct.pack("<iiii", 0, 0, 0x7fffffff, 3) + exr[dw + 16:]))
    out.append(("window_y1_2_31_minus_1.exr", "exr", exr[:dw] + struct.pack("<iiii", 0, 0, 3, 0x7fffffff) + exr[dw + 16:]))
    out.append(("header_only_2_31_minus_1.pfm", "pfm", b"PF\n2147483647 2147483647\n-1.0\n"))
    return out


def _exr_small():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        return _via(d, "s.exr", _write_exr, {"R": np.ones((4, 4), np.float32)}, 0, 0, 0)


def png_with_64mb_idat():
    """An 8 x 8 grey PNG (72 bytes of scanlines) whose IDAT inflates to 64 MB: about 65 KB."""
    return png(8, 8, 8, 0, z=zlib.compress(bytes(64 << 20), 9))


# ------------------------------------------------------------------------------------------------------------------ 5. OBJ and MTL
TRIANGLE = "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\n"


def obj_cases():
    """[(case name, {file name: bytes}, the file to load)]."""
    c = []

    def add(name, obj, **more):
        files = {"m.obj": obj, **more}
        c.append((name, {k: (v if isinstance(v, bytes) else v.encode()) for k, v in files.items()}, "m.obj"))
    add("empty", "")
    add("only_newlines", "\n\n\n")
    add("valid", TRIANGLE + "f 1/1 2/2 3/3\n")
    add("faces_before_vertices", "f 1 2 3\n" + TRIANGLE)
    add("faces_before_vertices_negative", "f -1 -2 -3\n" + TRIANGLE)
    for idx in ("0", "-9", "4", "-4", "4294967297", "4294967296", "2147483649", "-4294967295", "18446744073709551617", "99999999999999999999",
                "-99999999999999999999", "9223372036854775807", "-9223372036854775808"):
        add(f"index_{idx}", TRIANGLE + f"f 1 2 {idx}\n")
        add(f"index_{idx}_first", TRIANGLE + f"f {idx} 2 3\n")
        add(f"vt_index_{idx}", TRIANGLE + f"f 1/1 2/2 3/{idx}\n")
    add("index_negative_valid", TRIANGLE + "f -3 -2 -1\n")
    add("face_0_corners", TRIANGLE + "f\nf \n")
    add("face_1_corner", TRIANGLE + "f 1\n")
    add("face_2_corners", TRIANGLE + "f 1 2\n")
    add("face_2_corners_bad_index", TRIANGLE + "f 1 4294967297\nf 1 2 3\n")
    add("face_1_slash_slash", TRIANGLE + "f 1// 2// 3//\n")
    add("face_2_four_slashes", TRIANGLE + "f 1 2//// 3\n")
    add("face_3_a_b", TRIANGLE + "f 1 2 3/a/b\n")
    add("face_letters", TRIANGLE + "f a b c\n")
    add("face_trailing_slash", TRIANGLE + "f 1/ 2/ 3/\n")
    add("face_quad_and_pentagon", TRIANGLE + "v 1 1 0\nv 2 2 0\nf 1 2 4 3\nf 1 2 5 4 3\n")
    for val in ("nan", "inf", "-inf", "1e999", "-1e999", "1e-999", "0x1p3", "nan(0x7)"):
        add(f"coordinate_{val}", TRIANGLE.replace("v 1 0 0", f"v {val} {val} {val}") + "f 1 2 3\n")
        add(f"texcoord_{val}", TRIANGLE.replace("vt 1 0", f"vt {val} {val}") + "f 1/1 2/2 3/3\n")
    add("v_two_numbers", "v 0 0\nv 1\nv\nv 0 1 0\nf 1 2 4\n")
    add("v_words", "v a b c\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    add("usemtl_without_mtllib", TRIANGLE + "usemtl a\nf 1 2 3\n")
    add("usemtl_without_name", TRIANGLE + "usemtl\nf 1 2 3\nusemtl \nf 1 2 3\n")
    add("mtllib_missing", "mtllib nowhere.mtl\n" + TRIANGLE + "usemtl a\nf 1 2 3\n")
    add("mtllib_without_name", "mtllib\n" + TRIANGLE + "usemtl a\nf 1 2 3\n")
    add("mtllib_is_the_obj", "mtllib m.obj\n" + TRIANGLE + "usemtl a\nf 1 2 3\n")
    add("mtllib_is_the_directory", "mtllib .\n" + TRIANGLE + "usemtl a\nf 1 2 3\n")
    tri = "mtllib m.mtl\n" + TRIANGLE + "usemtl a\nf 1/1 2/2 3/3\n"
    add("mtl_empty", tri, **{"m.mtl": ""})
    add("mtl_newmtl_without_name", tri, **{"m.mtl": "newmtl\nKd 1 0 0\nnewmtl \nKd 0 1 0\n"})
    add("mtl_map_kd_without_file", tri, **{"m.mtl": "newmtl a\nmap_Kd\nmap_Kd \n"})
    add("mtl_map_bump_bm_without_value", tri, **{"m.mtl": "newmtl a\nmap_bump -bm\nbump -bm\n"})
    add("mtl_map_kd_is_the_mtl", tri, **{"m.mtl": "newmtl a\nmap_Kd m.mtl\nmap_bump m.mtl\n"})
    add("mtl_map_kd_is_the_obj", tri, **{"m.mtl": "newmtl a\nmap_Kd m.obj\n"})
    add("mtl_map_kd_is_the_directory", tri, **{"m.mtl": "newmtl a\nmap_Kd .\nmap_bump ..\n"})
    add("mtl_map_kd_missing", tri, **{"m.mtl": "newmtl a\nmap_Kd nowhere.png\n"})
    add("mtl_kd_words", tri, **{"m.mtl": "newmtl a\nKd a b c\nKe nan inf 1e999\nKa\nKs 1\n"})
    add("mtl_keys_before_newmtl", tri, **{"m.mtl": "Kd 1 1 1\nmap_Kd m.mtl\nnewmtl a\n"})
    add("mtl_unknown_material", tri, **{"m.mtl": "newmtl b\nKd 1 1 1\n"})
    add("mtl_same_material_twice", tri, **{"m.mtl": "newmtl a\nKd 1 0 0\nnewmtl a\nKd 0 1 0\n"})
    n = 60000  # a 60 000-corner face
    ring = "".join(f"v {np.cos(k * 1e-4):.6f} {np.sin(k * 1e-4):.6f} 0\n" for k in range(n))
    add("face_60000_corners", ring + "f " + " ".join(str(k + 1) for k in range(n)) + "\n")
    add("crlf", (TRIANGLE + "usemtl a\nf 1/1 2/2 3/3\n").replace("\n", "\r\n"))
    add("crlf_with_mtl", tri.replace("\n", "\r\n"), **{"m.mtl": "newmtl a\r\nKd 1 0 0\r\nmap_Kd nowhere.png\r\n"})
    add("cr_only", (TRIANGLE + "f 1 2 3\n").replace("\n", "\r"))
    add("embedded_nul", (TRIANGLE + "f 1 2 3\n").encode().replace(b"v 1 0 0", b"v 1\0 0 0"))
    add("embedded_nul_in_face", (TRIANGLE + "f 1 2 3\n").encode().replace(b"f 1 2 3", b"f 1 2\0 3"))
    add("nul_only", b"\0" * 64)
    add("no_final_newline", TRIANGLE + "f 1 2 3")
    add("long_line", "# " + "x" * 300000 + "\n" + TRIANGLE + "f 1 2 3\n")
    add("binary", bytes(np.random.default_rng(5).integers(0, 256, 4096, dtype=np.uint8)))
    add("tabs", "v\t0\t0\t0\nv\t1\t0\t0\nv\t0\t1\t0\nf\t1\t2\t3\n")
    add("leading_spaces", "  v 0 0 0\n  v 1 0 0\n  v 0 1 0\n  f 1 2 3\n")
    return c


# ----------------------------------------------------------------------------------------------------- 6. the smallest valid shapes
def smallest_valid(tmp):
    """[(file name, kind, bytes)]: valid files at the sizes where decoders go wrong, each one readable by Pillow."""
    out = []
    rng = np.random.default_rng(31)
    sizes = ((1, 1), (1, 7), (7, 1))  # (h, w)
    for h, w in sizes + ((6, 9),):
        tag = f"{w}x{h}"
        rgb, rgba, grey = (rng.integers(0, 256, (h, w, c), dtype=np.uint8) for c in (3, 4, 1))
        grey = grey[..., 0]
        if w > 2:
            rgba[h // 2, :w - 1] = rgba[h // 2, 0]  # a run
            grey[0, 1:] = grey[0, 1]
        out.append((f"ppm_{tag}.ppm", "pnm", pnm("P6", w, h, rgb.tobytes())))
        out.append((f"pgm_{tag}.ppm", "pnm", pnm("P5", w, h, grey.tobytes())))
        out.append((f"pam_depth4_{tag}.pam", "pnm", pam(w, h, 4, rgba.tobytes())))
        out.append((f"pam_depth2_{tag}.pam", "pnm", pam(w, h, 2, rgba[..., :2].tobytes())))
        for mode, arr in (("RGB", rgb), ("RGBA", rgba), ("L", grey), ("LA", rgba[..., :2])):
            out.append((f"png_{mode}_{tag}.png", "png", _pil(arr, mode, "PNG")))
            if mode != "LA":
                out.append((f"tga_{mode}_{tag}.tga", "tga", _pil(arr, mode, "TGA")))
                out.append((f"tga_rle_{mode}_{tag}.tga", "tga", _pil(arr, mode, "TGA", compression="tga_rle")))
        for rle in (False, True):
            for top in (False, True):
                out.append((f"tga_own_rle{int(rle)}_top{int(top)}_{tag}.tga", "tga", _via(tmp, "v.tga", _tga, rgba, rle, top)))
    # TGA: run-length packets that cross row ends (a 5 x 4 image as one run of 7, literals of 6, a run of 7), both row orders, and
    # with the right-to-left bit
    px = [b"\x10\x20\x30"] * 7 + [bytes([k, 2 * k, 255 - k]) for k in range(6)] + [b"\x90\xa0\xb0"] * 7
    body = bytes([0x86]) + px[0] + bytes([0x05]) + b"".join(px[7:13]) + bytes([0x86]) + px[13]
    for desc in (0x00, 0x20, 0x10, 0x30):
        out.append((f"tga_packets_cross_rows_desc{desc:02x}.tga", "tga", struct.pack("<BBBHHBHHHHBB", 0, 0, 10, 0, 0, 0, 0, 0, 5, 4, 24, desc) + body))
        out.append((f"tga_raw_desc{desc:02x}.tga", "tga", struct.pack("<BBBHHBHHHHBB", 0, 0, 2, 0, 0, 0, 0, 0, 5, 4, 24, desc) + b"".join(px)))
    # PNG: 7 x 5 and 3 x 1 at bit depths 1, 2 and 4, grey and palette, with and without Adam7 (some passes are empty); 16 bits with tRNS
    for h, w in ((5, 7), (1, 3), (1, 1)):
        for bits in (1, 2, 4):
            v = rng.integers(0, 1 << bits, (h, w, 1))
            pal = rng.integers(0, 256, (1 << bits, 3))
            for inter in (False, True):
                tag = f"{w}x{h}_{bits}bit_adam7{int(inter)}"
                out.append((f"png_grey_{tag}.png", "png", _via(tmp, "v.png", _png_general, v, bits, 0, inter)))
                out.append((f"png_palette_{tag}.png", "png", _via(tmp, "v.png", _png_general, v, bits, 3, inter, palette=pal)))
                out.append((f"png_palette_trns_{tag}.png", "png", _via(tmp, "v.png", _png_general, v, bits, 3, inter, palette=pal, trns=bytes([0, 200]))))
        for inter in (False, True):
            g = rng.integers(0, 65536, (h, w, 1))
            g[0, 0] = 0x1234
            out.append((f"png_grey16_trns_{w}x{h}_adam7{int(inter)}.png", "png", _via(tmp, "v.png", _png_general, g, 16, 0, inter, trns=struct.pack(">H", 0x1234))))
            c = rng.integers(0, 65536, (h, w, 3))
            c[0, w - 1] = (0x0102, 0x0304, 0x0506)
            out.append((f"png_rgb16_trns_{w}x{h}_adam7{int(inter)}.png", "png", _via(tmp, "v.png", _png_general, c, 16, 2, inter, trns=struct.pack(">HHH", 0x0102, 0x0304, 0x0506))))
            for ch, ctype in ((2, 4), (4, 6)):
                out.append((f"png_16bit_ctype{ctype}_{w}x{h}_adam7{int(inter)}.png", "png", _via(tmp, "v.png", _png_general, rng.integers(0, 65536, (h, w, ch)), 16, ctype, inter)))
            k8 = rng.integers(0, 256, (h, w, 3))
            k8[0, 0] = (10, 200, 30)
            out.append((f"png_rgb8_trns_{w}x{h}_adam7{int(inter)}.png", "png", _via(tmp, "v.png", _png_general, k8, 8, 2, inter, trns=struct.pack(">HHH", 10, 200, 30))))
    # JPEG: 1 x 1, 9 x 17 and 17 x 9; 4:4:4, 4:2:2, 4:2:0 (Pillow's "4:1:1" is its old name for 4:2:0: it writes no 4:1:1 file) and grey,
    # baseline and progressive, with and without restart intervals; 4:4:0 and 4:1:1 from the test-side baseline writer
    for h, w in ((1, 1), (17, 9), (9, 17)):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 11 + yy * 3) % 256, (yy * 13 + 60) % 256, ((xx + yy) * 7 + 120) % 256], axis=2).astype(np.uint8)
        for prog in (False, True):
            for rst in (0, 1):
                kw = dict(progressive=prog, **({"restart_marker_blocks": 1} if rst else {}))
                tag = f"{w}x{h}_prog{int(prog)}_rst{rst}"
                for ss, name in ((0, "444"), (1, "422"), (2, "420")):
                    out.append((f"jpeg_{name}_{tag}.jpg", "jpeg", _pil(img, "RGB", "JPEG", quality=90, subsampling=ss, **kw)))
                out.append((f"jpeg_grey_{tag}.jpg", "jpeg", _pil(img[..., 0], "L", "JPEG", quality=90, **kw)))
        planes = [np.ascontiguousarray(img[..., k]) for k in range(3)]
        for samp, name in (([(1, 2), (1, 1), (1, 1)], "440"), ([(4, 1), (1, 1), (1, 1)], "411")):
            for rst in (0, 2):
                out.append((f"jpeg_{name}_{w}x{h}_own_rst{rst}.jpg", "jpeg", _via(tmp, "v.jpg", _jpeg, planes, samp, 2, rst)))
    return out
