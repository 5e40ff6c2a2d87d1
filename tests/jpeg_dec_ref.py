"""Python-integer restatement of the baseline JPEG decoder (asva_amd/csrc/jpeg.hip: avsd_jpeg_decode_scan,
avsd_jpeg_idct_rgb_u8; asva_amd/video_io.py: decode_jpeg_frames), written from the standard (ITU-T T.81 Annex B, F) and from
libjpeg's default decompression path (jidctint.c "islow", jdsample.c h2v2 fancy upsampling, jdcolor.c), with nothing imported
from the package: the marker parser, the sequential Huffman decoder, dequantisation, the integer IDCT, the triangle chroma
upsampling of 4:2:0 and the fixed-point colour conversion.  Its contract is the bytes PIL returns for the same stream."""
import numpy as np

# natural (row-major) index of the coefficient at each zigzag position (T.81 figure A.6)
ZIGZAG = []
for _s in range(15):
    _d = [(i, _s - i) for i in range(8) if 0 <= _s - i < 8]
    ZIGZAG += [r * 8 + c for r, c in (_d[::-1] if _s % 2 == 0 else _d)]
ZIGZAG = np.array(ZIGZAG)


class Unsupported(ValueError):
    pass


def parse(data):
    """-> dict(H, W, sampling '444' | '420', qtabs [3] of 64 ints in zigzag order, dc [3] / ac [3] of (bits, vals), scan: the
    entropy-coded bytes with the stuffing removed).  Raises Unsupported for everything but baseline, 8-bit, three components,
    4:4:4 or 4:2:0, one interleaved scan, no restart interval."""
    if data[:2] != b"\xff\xd8":
        raise Unsupported("no SOI")
    p, dqt, dht, frame, scan = 2, {}, {}, None, None
    while scan is None:
        if data[p] != 0xFF:
            raise Unsupported(f"byte {data[p]:#x} where a marker was expected")
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        n = int.from_bytes(data[p + 2:p + 4], "big")
        seg = data[p + 4:p + 2 + n]
        if 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                if seg[q] >> 4:
                    raise Unsupported("16-bit quantisation table")
                dqt[seg[q] & 15] = list(seg[q + 1:q + 65])
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                bits = list(seg[q + 1:q + 17])
                dht[seg[q]] = (bits, list(seg[q + 17:q + 17 + sum(bits)]))
                q += 17 + sum(bits)
        elif m == 0xC0:
            if seg[0] != 8 or seg[5] != 3:
                raise Unsupported(f"{seg[0]}-bit samples, {seg[5]} components")
            frame = (int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), [tuple(seg[6 + 3 * i:9 + 3 * i]) for i in range(3)])
        elif m == 0xDD:
            if int.from_bytes(seg[:2], "big"):
                raise Unsupported("restart interval")
        elif m == 0xDA:
            if frame is None or seg[0] != 3 or tuple(seg[7:10]) != (0, 63, 0):
                raise Unsupported("not one interleaved sequential scan")
            sel = [seg[2 + 2 * i] for i in range(3)]
            scan = p + 2 + n
        else:
            raise Unsupported(f"marker {m:#x}")
        p += 2 + n
    H, W, comps = frame
    samp = tuple(c[1] for c in comps)
    if samp not in ((0x11, 0x11, 0x11), (0x22, 0x11, 0x11)):
        raise Unsupported(f"sampling factors {samp}")
    end = scan
    while not (data[end] == 0xFF and data[end + 1] not in (0x00, 0xFF)):
        end += 1
    if data[end + 1] != 0xD9:
        raise Unsupported(f"marker {data[end + 1]:#x} inside the scan")
    return {"H": H, "W": W, "sampling": "444" if samp[0] == 0x11 else "420", "qtabs": [dqt[c[2]] for c in comps],
            "dc": [dht[s >> 4] for s in sel], "ac": [dht[0x10 | (s & 15)] for s in sel],
            "scan": bytes(data[scan:end]).replace(b"\xff\x00", b"\xff")}


def _decode_table(spec):
    """{(length, code): symbol} by the procedure of Annex C"""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def blocks_per_mcu(sampling):
    return 3 if sampling == "444" else 6


def component_of_block(sampling):
    return (0, 1, 2) if sampling == "444" else (0, 0, 0, 0, 1, 2)


def decode_scan(info):
    """-> int64 (blocks, 64): zigzag order, blocks in scan order, DC values absolute.  Sequential, bit by bit (F.2.2)."""
    H, W = info["H"], info["W"]
    mcu = 8 if info["sampling"] == "444" else 16
    n_mcu = -(-H // mcu) * -(-W // mcu)
    comp_of = component_of_block(info["sampling"])
    dc, ac = [_decode_table(t) for t in info["dc"]], [_decode_table(t) for t in info["ac"]]
    scan = info["scan"]
    acc, nbits = int.from_bytes(scan, "big"), 8 * len(scan)
    pos = 0

    def take(n):
        nonlocal pos
        if pos + n > nbits:
            raise ValueError("the scan ends inside a symbol")
        v = (acc >> (nbits - pos - n)) & ((1 << n) - 1)
        pos += n
        return v

    def symbol(table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | take(1)
            if (length, code) in table:
                return table[(length, code)]
        raise ValueError("a code no table assigns")

    def value(size):
        if size == 0:
            return 0
        v = take(size)
        return v if v >> (size - 1) else v - (1 << size) + 1

    out = np.zeros((n_mcu * len(comp_of), 64), dtype=np.int64)
    pred = [0, 0, 0]
    for m in range(n_mcu):
        for b, c in enumerate(comp_of):
            blk = out[m * len(comp_of) + b]
            pred[c] += value(symbol(dc[c]))
            blk[0] = pred[c]
            k = 1
            while k < 64:
                rs = symbol(ac[c])
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        break
                    k += 16
                    continue
                k += r
                blk[k] = value(s)
                k += 1
    left = nbits - pos
    if left >= 8 or (left and take(left) != (1 << left) - 1):
        raise ValueError("bits left over behind the last block")
    return out


def _descale(x, s):
    return (x + (1 << (s - 1))) >> s


def _wrap16(x):
    return ((np.asarray(x) + 32768) & 0xFFFF) - 32768


def _sat16(x):
    return np.clip(x, -32768, 32767)


def _idct_1d(i, s):
    """jidctint.c: i = the eight inputs (arrays), 13-bit constants, result descaled by s bits.  The _wrap16 / _sat16 calls are
    libjpeg-turbo's 16-bit vector layout of the same arithmetic (inputs, the sums i0 +- i4, z3 and z4 are 16-bit lanes that wrap;
    results are packed with signed saturation): no-ops for every stream an encoder makes from pixels, and what PIL returns for
    streams built from extreme coefficients."""
    z1 = (i[2] + i[6]) * 4433
    t2 = z1 - i[6] * 15137
    t3 = z1 + i[2] * 6270
    t0 = _wrap16(i[0] + i[4]) << 13
    t1 = _wrap16(i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, _wrap16(a0 + a2), _wrap16(a1 + a3)
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return [_sat16(_descale(x, s)) for x in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)]


def idct_blocks(coef, qtab):
    """coef (n, 64) zigzag, qtab 64 zigzag -> (n, 8, 8) samples 0..255"""
    nat = np.zeros((coef.shape[0], 64), dtype=np.int64)
    nat[:, ZIGZAG] = _wrap16(np.asarray(coef, dtype=np.int64) * np.asarray(qtab, dtype=np.int64))
    w = nat.reshape(-1, 8, 8)
    cols = np.stack(_idct_1d([w[:, r, :] for r in range(8)], 11), axis=1)            # down the columns: (n, 8 rows, 8)
    # a block whose rows 1..7 are all zero takes the vector code's shortcut: every row is row 0 << 2, in 16 bits (the same value
    # as the full pass unless it leaves int16, where this wraps and the full pass saturates)
    flat = ~w[:, 1:, :].any(axis=(1, 2))
    cols[flat] = np.repeat(_wrap16(w[flat, :1, :] << 2), 8, axis=1)
    rows = np.stack(_idct_1d([cols[:, :, c] for c in range(8)], 18), axis=2)         # along the rows
    return np.clip(rows + 128, 0, 255)


def planes(info, coef):
    """-> [Y, Cb, Cr] as decoded, padded to whole MCUs"""
    H, W = info["H"], info["W"]
    s = 1 if info["sampling"] == "444" else 2
    mh, mw = -(-H // (8 * s)), -(-W // (8 * s))
    bpm = blocks_per_mcu(info["sampling"])
    coef = np.asarray(coef).reshape(mh, mw, bpm, 64)
    out = []
    for c in range(3):
        if c == 0 and s == 2:
            px = idct_blocks(coef[:, :, :4].reshape(-1, 64), info["qtabs"][0]).reshape(mh, mw, 2, 2, 8, 8)
            out.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(mh * 16, mw * 16))
        else:
            px = idct_blocks(coef[:, :, bpm - 3 + c].reshape(-1, 64), info["qtabs"][c]).reshape(mh, mw, 8, 8)
            out.append(px.transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8))
    return out


def upsample_fancy(c, H, W):
    """jdsample.c h2v2_fancy_upsample over the ceil(H/2) x ceil(W/2) real samples, cropped to H x W"""
    ch, cw = -(-H // 2), -(-W // 2)
    c = np.asarray(c[:ch, :cw], dtype=np.int64)
    up, down = np.vstack([c[:1], c[:-1]]), np.vstack([c[1:], c[-1:]])
    v = np.empty((2 * ch, cw), dtype=np.int64)
    v[0::2], v[1::2] = 3 * c + up, 3 * c + down
    left, right = np.hstack([v[:, :1], v[:, :-1]]), np.hstack([v[:, 1:], v[:, -1:]])
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * v + left + 8) >> 4, (3 * v + right + 7) >> 4
    return out[:H, :W]


def to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pixels(info, coef):
    H, W = info["H"], info["W"]
    y, cb, cr = planes(info, coef)
    if info["sampling"] == "420":
        cb, cr = upsample_fancy(cb, H, W), upsample_fancy(cr, H, W)
    return to_rgb(y[:H, :W], cb[:H, :W], cr[:H, :W])


def decode(data):
    """a complete JPEG file -> uint8 (H, W, 3)"""
    info = parse(data)
    return pixels(info, decode_scan(info))
