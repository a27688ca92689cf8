"""Writers of the TGA, PNG, JPEG and OpenEXR files the asset readers' tests feed them."""
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


def _png_general(path, samples, bits, ctype, interlace=False, palette=None, trns=None):
    """Write a PNG of any colour type / bit depth, optionally Adam7-interlaced.  samples: (h, w, channels) integers < 2**bits."""
    import struct
    import zlib
    h, w, ch = samples.shape
    bpp = max(1, ch * bits // 8)

    def pack_rows(sub):
        ph, pw, _ = sub.shape
        out = bytearray()
        prev = np.zeros(((pw * ch * bits + 7) // 8,), dtype=np.int32)
        for y in range(ph):
            flat = sub[y].reshape(-1).astype(np.uint32)
            if bits == 16:
                row = np.stack([flat >> 8, flat & 255], axis=1).reshape(-1)
            elif bits == 8:
                row = flat
            else:
                per = 8 // bits
                padded = np.concatenate([flat, np.zeros((-len(flat)) % per, dtype=np.uint32)]).reshape(-1, per)
                row = sum(padded[:, k] << (8 - bits * (k + 1)) for k in range(per))
            cur = row.astype(np.int32)
            ft = (y + pw) % 5
            a = np.concatenate([np.zeros(bpp, dtype=np.int32), cur[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
            c = np.concatenate([np.zeros(bpp, dtype=np.int32), prev[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
            if ft == 0: pred = 0
            elif ft == 1: pred = a
            elif ft == 2: pred = prev
            elif ft == 3: pred = (a + prev) // 2
            else:
                pp = a + prev - c
                pa, pb, pc = abs(pp - a), abs(pp - prev), abs(pp - c)
                pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
            out += bytes([ft]) + ((cur - pred) & 0xff).astype(np.uint8).tobytes()
            prev = cur
        return bytes(out)

    if interlace:
        x0s, y0s, dxs, dys = (0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1), (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)
        body = b"".join(pack_rows(samples[y0::dy, x0::dx]) for x0, y0, dx, dy in zip(x0s, y0s, dxs, dys) if samples[y0::dy, x0::dx].size)
    else:
        body = pack_rows(samples)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bits, ctype, 0, 0, 1 if interlace else 0)))
        if palette is not None:
            f.write(chunk(b"PLTE", palette.astype(np.uint8).tobytes()))
        if trns is not None:
            f.write(chunk(b"tRNS", bytes(trns)))
        f.write(chunk(b"IDAT", zlib.compress(body, 6)) + chunk(b"IEND", b""))


_ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50,
       43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _jpeg(path, planes, sampling, q=2, restart=0):
    """A baseline (SOF0) JPEG writer for the tests: planes = list of 2-D uint8 arrays at FULL resolution (Y or Y, Cb, Cr);
    sampling = [(h, v), ...]; chroma planes are box-filtered down.  Own Huffman tables (every code 4 bits for the 12 DC
    categories, 8 bits for the 162 AC symbols) and a flat quantiser q.  Returns the planes the decoder should reconstruct
    BEFORE upsampling (i.e. after subsampling + quantisation round trip is not modelled: the test compares with a tolerance)."""
    import struct
    from scipy.fft import dctn
    H, W = planes[0].shape
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    mcuw, mcuh = 8 * hmax, 8 * vmax
    mx, my = (W + mcuw - 1) // mcuw, (H + mcuh - 1) // mcuh
    comps = []
    for p, (sh, sv) in zip(planes, sampling):
        fx, fy = hmax // sh, vmax // sv
        pad = np.pad(p.astype(np.float64), ((0, my * mcuh - H), (0, mx * mcuw - W)), mode="edge")
        sub = pad.reshape(pad.shape[0] // fy, fy, pad.shape[1] // fx, fx).mean(axis=(1, 3))
        comps.append(sub)
    ac_syms = [0x00, 0xf0] + [(r << 4) | z for r in range(16) for z in range(1, 11)]
    dc_code = {c: (c, 4) for c in range(12)}
    ac_code = {sym: (i, 8) for i, sym in enumerate(ac_syms)}
    bits = []

    def put(v, n):
        for k in range(n - 1, -1, -1):
            bits.append((v >> k) & 1)

    def cat(v):
        a = abs(int(v))
        return a.bit_length()

    def put_val(v, n):
        v = int(v)
        put(v if v >= 0 else v + (1 << n) - 1, n)

    pred = [0] * len(comps)
    out_bytes = bytearray()

    def flush_bits():
        while len(bits) % 8:
            bits.append(1)
        for i in range(0, len(bits), 8):
            b = 0
            for k in range(8):
                b = (b << 1) | bits[i + k]
            out_bytes.append(b)
            if b == 0xff:
                out_bytes.append(0)
        bits.clear()

    def encode_block(ci, blk):
        co = np.round(dctn(blk - 128.0, norm="ortho") / q).astype(np.int64).reshape(-1)
        zz = [int(co[k]) for k in _ZZ]
        diff = zz[0] - pred[ci]
        pred[ci] = zz[0]
        n = cat(diff)
        put(*dc_code[n])
        if n:
            put_val(diff, n)
        run = 0
        last = max([k for k in range(1, 64) if zz[k]] + [0])
        for k in range(1, last + 1):
            if zz[k] == 0:
                run += 1
                continue
            while run > 15:
                put(*ac_code[0xf0])
                run -= 16
            n = cat(zz[k])
            put(*ac_code[(run << 4) | n])
            put_val(zz[k], n)
            run = 0
        if last < 63:
            put(*ac_code[0x00])

    count = 0
    rst = 0
    for j in range(my):
        for i in range(mx):
            for ci, (sh, sv) in enumerate(sampling):
                for y in range(sv):
                    for x in range(sh):
                        by, bx = (j * sv + y) * 8, (i * sh + x) * 8
                        encode_block(ci, comps[ci][by:by + 8, bx:bx + 8])
            count += 1
            if restart and count % restart == 0 and not (j == my - 1 and i == mx - 1):
                flush_bits()
                out_bytes += bytes([0xff, 0xd0 + rst])
                rst = (rst + 1) & 7
                pred = [0] * len(comps)
    flush_bits()

    def seg(marker, data):
        return bytes([0xff, marker]) + struct.pack(">H", len(data) + 2) + data
    with open(path, "wb") as f:
        f.write(b"\xff\xd8")
        f.write(seg(0xdb, bytes([0]) + bytes([q] * 64)))
        f.write(seg(0xc0, struct.pack(">BHHB", 8, H, W, len(comps)) + b"".join(bytes([k + 1, (sh << 4) | sv, 0]) for k, (sh, sv) in enumerate(sampling))))
        f.write(seg(0xc4, bytes([0x00] + [0, 0, 0, 12] + [0] * 12 + list(range(12)))))
        f.write(seg(0xc4, bytes([0x10] + [0] * 7 + [162] + [0] * 8 + ac_syms)))
        if restart:
            f.write(seg(0xdd, struct.pack(">H", restart)))
        f.write(seg(0xda, bytes([len(comps)]) + b"".join(bytes([k + 1, 0x00]) for k in range(len(comps))) + bytes([0, 63, 0])))
        f.write(bytes(out_bytes) + b"\xff\xd9")


def _write_exr(path, channels, x0, y0, compression):
    """Test-side OpenEXR writer: `channels` = {name: (h, w) array of float16 / float32 / uint32}; scan lines, compression 0 (none),
    1 (RLE), 2 (ZIPS) or 3 (ZIP); the data window starts at (x0, y0)."""
    import struct
    import zlib
    names = sorted(channels)
    h, w = channels[names[0]].shape
    types = {np.dtype(np.uint32): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}
    hd = struct.pack("<ii", 20000630, 2)

    def attr(name, typ, payload):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(payload)) + payload
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iBBBBii", types[channels[n].dtype], 0, 0, 0, 0, 1, 1) for n in names) + b"\0"
    hd += attr("channels", "chlist", chlist) + attr("compression", "compression", bytes([compression]))
    hd += attr("dataWindow", "box2i", struct.pack("<iiii", x0, y0, x0 + w - 1, y0 + h - 1))
    hd += attr("displayWindow", "box2i", struct.pack("<iiii", 0, 0, x0 + w - 1, y0 + h - 1))
    hd += attr("lineOrder", "lineOrder", b"\0") + attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    hd += attr("screenWindowCenter", "v2f", struct.pack("<ff", 0, 0)) + attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    per = 16 if compression == 3 else 1
    blocks = []
    for b0 in range(0, h, per):
        raw = b"".join(channels[n][y].tobytes() for y in range(b0, min(h, b0 + per)) for n in names)
        data = raw
        if compression:
            a = np.frombuffer(raw, dtype=np.uint8)
            sh = np.concatenate([a[0::2], a[1::2]]).astype(np.int32)
            sh[1:] = (sh[1:] - sh[:-1] + 128) & 255
            pre = sh.astype(np.uint8).tobytes()
            if compression == 1:  # RLE: runs of >= 3 equal bytes as (count - 1, byte), everything else as negative-count literals
                out, i = bytearray(), 0
                while i < len(pre):
                    j = i
                    while j + 1 < len(pre) and pre[j + 1] == pre[i] and j - i < 127:
                        j += 1
                    if j - i >= 2:
                        out += bytes([j - i, pre[i]])
                        i = j + 1
                    else:
                        k = i
                        while k < len(pre) and k - i < 127 and not (k + 2 < len(pre) and pre[k] == pre[k + 1] == pre[k + 2]):
                            k += 1
                        out += bytes([(256 - (k - i)) & 255]) + pre[i:k]
                        i = k
                packed = bytes(out)
            else:
                packed = zlib.compress(pre, 6)
            data = packed if len(packed) < len(raw) else raw
        blocks.append(struct.pack("<ii", y0 + b0, len(data)) + data)
    off = len(hd) + 8 * len(blocks)
    table = b""
    for blk in blocks:
        table += struct.pack("<Q", off)
        off += len(blk)
    open(path, "wb").write(hd + table + b"".join(blocks))
