"""Writers of the TGA and PNG files the OBJ / MTL reader's tests feed it."""
import numpy as np


def _tga(path, img, rle=False, top_down=False):
    """Write an 8-bit grey (h, w) or true-colour (h, w, 3|4) image as a TGA file."""
    import struct
    h, w = img.shape[:2]
    depth = 1 if img.ndim == 2 else img.shape[2]
    px = img.reshape(h, w, depth)
    if depth >= 3:
        px = px[..., [2, 1, 0] + ([3] if depth == 4 else [])]  # stored BGR(A)
    rows = px if top_down else px[::-1]
    flat = np.ascontiguousarray(rows).reshape(-1, depth)
    typ = (3 if depth == 1 else 2) + (8 if rle else 0)
    body = bytearray()
    if rle:
        i, n = 0, len(flat)
        while i < n:
            run = 1
            while i + run < n and run < 128 and (flat[i + run] == flat[i]).all():
                run += 1
            if run >= 2:
                body += bytes([0x80 | (run - 1)]) + flat[i].tobytes()
                i += run
            else:
                lit = 1
                while i + lit < n and lit < 128 and not (i + lit + 1 < n and (flat[i + lit] == flat[i + lit + 1]).all()):
                    lit += 1
                body += bytes([lit - 1]) + flat[i:i + lit].tobytes()
                i += lit
    else:
        body += flat.tobytes()
    with open(path, "wb") as f:
        f.write(struct.pack("<BBBHHBHHHHBB", 3, 0, typ, 0, 0, 0, 0, 0, w, h, 8 * depth, (0x20 if top_down else 0) | (8 if depth == 4 else 0)))
        f.write(b"id!")
        f.write(bytes(body))


def _png(path, img, level=6, strategy=0, palette=None, trns=None):
    """Write an 8-bit PNG (grey, grey+alpha, RGB, RGBA or palette) cycling through the five scanline filters."""
    import struct
    import zlib
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    ctype = 3 if palette is not None else {1: 0, 2: 4, 3: 2, 4: 6}[ch]
    rows = img.reshape(h, w * ch).astype(np.int32)
    out = bytearray()
    for y in range(h):
        ft = y % 5
        cur, up = rows[y], (rows[y - 1] if y else np.zeros(w * ch, dtype=np.int32))
        a = np.concatenate([np.zeros(ch, dtype=np.int32), cur[:-ch]])
        c = np.concatenate([np.zeros(ch, dtype=np.int32), up[:-ch]])
        if ft == 0: pred = 0
        elif ft == 1: pred = a
        elif ft == 2: pred = up
        elif ft == 3: pred = (a + up) // 2
        else:
            p = a + up - c
            pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        out += bytes([ft]) + ((cur - pred) & 0xff).astype(np.uint8).tobytes()
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    z = co.compress(bytes(out)) + co.flush()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)))
        if palette is not None:
            f.write(chunk(b"PLTE", np.asarray(palette, dtype=np.uint8).tobytes()))
            if trns is not None:
                f.write(chunk(b"tRNS", np.asarray(trns, dtype=np.uint8).tobytes()))
        half = len(z) // 2
        f.write(chunk(b"IDAT", z[:half]) + chunk(b"IDAT", z[half:]) + chunk(b"IEND", b""))
