"""Float64 / Python-integer restatement of the baseline JPEG encoder (asva_amd/csrc/jpeg.hip, asva_amd/video_io.py:
encode_jpeg_frames), written from the standard (ITU-T T.81 Annex A, C, F, K; JFIF 1.01) and libjpeg's quality scaling, with
nothing imported from the package: JFIF colour matrix, orthonormal 8 x 8 DCT-II, true division with rounding half away from
zero, zigzag, the sequential Huffman coder on Python integers, the markers, and the float64 inverse for reconstruction.
4:4:4 only: one MCU is one Y, one Cb and one Cr block."""
import numpy as np

# natural (row-major) index of the coefficient at each zigzag position (T.81 figure A.6)
ZIGZAG = []
for _s in range(15):
    _d = [(i, _s - i) for i in range(8) if 0 <= _s - i < 8]
    ZIGZAG += [r * 8 + c for r, c in (_d[::-1] if _s % 2 == 0 else _d)]
ZIGZAG = np.array(ZIGZAG)

# T.81 tables K.1 and K.2, natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                      100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32)

# T.81 tables K.3 - K.6: (BITS, HUFFVAL)
_AC_TAIL = [(r << 4) | s for r in range(16) for s in range(1, 11)]
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
            0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
            0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
            0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
            0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
            0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
            0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
            0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
              0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
              0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
              0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
              0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
              0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
              0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
              0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
assert sorted(AC_LUMA[1]) == sorted(AC_CHROMA[1]) == sorted([0x00, 0xf0] + _AC_TAIL) and sum(AC_LUMA[0]) == sum(AC_CHROMA[0]) == 162

TIE_WINDOW = 4e-3          # worst-case f32 error of a 64-term sum of values up to 1024 at a table entry of 1: 64 x 1024 x 2^-24


def tables(quality):
    """libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (force_baseline): natural-order (luma, chroma)"""
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (BASE_LUMA, BASE_CHROMA))


def huff_codes(spec):
    """T.81 Annex C: {symbol: (code, length)}"""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


_CODES = {"dc": (huff_codes(DC_LUMA), huff_codes(DC_CHROMA)), "ac": (huff_codes(AC_LUMA), huff_codes(AC_CHROMA))}

# C[u][x] = c(u) / 2 cos((2x + 1) u pi / 16)
DCT = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) / 2.0 * np.cos((2 * x + 1) * u * np.pi / 16.0) for x in range(8)] for u in range(8)])


def rgb_to_ycc(rgb):
    """(..., 3) -> (..., 3) float64, full range, NOT level-shifted"""
    rgb = np.asarray(rgb, dtype=np.float64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return np.stack([0.299 * r + 0.587 * g + 0.114 * b, -0.168735892 * r - 0.331264108 * g + 0.5 * b + 128.0,
                     0.5 * r - 0.418687589 * g - 0.081312411 * b + 128.0], axis=-1)


def ycc_to_rgb(ycc):
    y, cb, cr = ycc[..., 0], ycc[..., 1] - 128.0, ycc[..., 2] - 128.0
    return np.stack([y + 1.402 * cr, y - 0.344136286 * cb - 0.714136286 * cr, y + 1.772 * cb], axis=-1)


def _blocks(plane3):
    """(H, W, 3) -> (H/8, W/8, 3, 8, 8)"""
    H, W, _ = plane3.shape
    return plane3.reshape(H // 8, 8, W // 8, 8, 3).transpose(0, 2, 4, 1, 3)


def quotients(frame, qy, qc):
    """(H, W, 3) uint8 -> the pre-rounding quotients F / Q, float64 (H/8, W/8, 3, 64) in zigzag order"""
    H, W, _ = frame.shape
    assert H % 8 == 0 and W % 8 == 0
    f = _blocks(rgb_to_ycc(frame) - 128.0)
    F = np.einsum("ux,...xy,vy->...uv", DCT, f, DCT).reshape(H // 8, W // 8, 3, 64)
    Q = np.stack([np.asarray(qy), np.asarray(qc), np.asarray(qc)]).astype(np.float64)       # (3, 64) natural
    return (F / Q)[..., ZIGZAG]


def round_half_away(x):
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def near_tie(quot):
    """where rounding the quotient is decided by less than TIE_WINDOW"""
    frac = np.abs(quot) - np.floor(np.abs(quot))
    return np.abs(frac - 0.5) <= TIE_WINDOW


def quantize(frame, qy, qc):
    return round_half_away(quotients(frame, qy, qc))


def _category(v):
    return int(abs(int(v))).bit_length()


def encode_scan(coef):
    """coef int (n_mcu, 3, 64) zigzag (any leading shape that reshapes to it) -> (bytes unstuffed and padded with 1-bits, bit length)"""
    coef = np.asarray(coef).reshape(-1, 3, 64)
    acc, nbits = 0, 0

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | (code & ((1 << length) - 1))
        nbits += length

    def put_value(v, size):
        put(v if v >= 0 else v - 1, size)

    pred = [0, 0, 0]
    for mcu in coef:
        for comp in range(3):
            tab = 0 if comp == 0 else 1
            blk = [int(x) for x in mcu[comp]]
            diff = blk[0] - pred[comp]
            pred[comp] = blk[0]
            size = _category(diff)
            put(*_CODES["dc"][tab][size])
            put_value(diff, size)
            run = 0
            for k in range(1, 64):
                if blk[k] == 0:
                    run += 1
                    continue
                while run > 15:
                    put(*_CODES["ac"][tab][0xF0])
                    run -= 16
                size = _category(blk[k])
                put(*_CODES["ac"][tab][(run << 4) | size])
                put_value(blk[k], size)
                run = 0
            if run:
                put(*_CODES["ac"][tab][0x00])
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((nbits + pad) // 8, "big"), nbits


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def headers(H, W, qy, qc):
    """SOI, APP0 (JFIF 1.01), DQT x 2, SOF0, DHT x 4, SOS"""
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((qy, qc)):
        out += _seg(0xDB, [i] + [int(np.asarray(q)[n]) for n in ZIGZAG])
    out += _seg(0xC0, [8] + list(H.to_bytes(2, "big")) + list(W.to_bytes(2, "big")) + [3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _seg(0xC4, [tc_th] + spec[0] + spec[1])
    return out + _seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


def stuff(scan):
    return scan.replace(b"\xff", b"\xff\x00")


def jpeg_from_coefficients(coef, H, W, qy, qc):
    return headers(H, W, qy, qc) + stuff(encode_scan(coef)[0]) + b"\xff\xd9"


def encode(frame, quality):
    qy, qc = tables(quality)
    H, W, _ = frame.shape
    return jpeg_from_coefficients(quantize(frame, qy, qc), H, W, qy, qc)


def reconstruct(coef, qy, qc):
    """coef (H/8, W/8, 3, 64) zigzag -> (H, W, 3) float64 RGB of the exact inverse (dequantise, inverse DCT, +128, inverse colour
    matrix), clipped to [0, 255] as any decoder's output is, not rounded"""
    coef = np.asarray(coef)
    hb, wb = coef.shape[:2]
    nat = np.zeros(coef.shape, dtype=np.float64)
    nat[..., ZIGZAG] = coef
    Q = np.stack([np.asarray(qy), np.asarray(qc), np.asarray(qc)]).astype(np.float64)
    F = (nat * Q).reshape(hb, wb, 3, 8, 8)
    f = np.einsum("ux,...uv,vy->...xy", DCT, F, DCT) + 128.0
    ycc = f.transpose(0, 3, 1, 4, 2).reshape(hb * 8, wb * 8, 3)
    return np.clip(ycc_to_rgb(ycc), 0.0, 255.0)


def psnr(a, b):
    mse = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


# ---- the inputs the tests share ---------------------------------------------------------------------------------------------
def smooth_image(H=48, W=64, seed=3):
    """smooth colour gradients plus 3 % noise, in gamut"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 90 * np.sin(x / 11.0 + 0.3) * np.cos(y / 17.0), 128 + 80 * np.cos(x / 23.0 - y / 9.0),
                     128 + 70 * np.sin((x + y) / 15.0)], axis=-1)
    return np.clip(np.rint(base + rng.normal(0.0, 0.03 * 255.0, base.shape)), 0, 255).astype(np.uint8)


def named_frames():
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:16, 0:16]
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    return {
        "mcu": rng.integers(0, 256, (8, 8, 3), dtype=np.uint8),
        "noise": rng.integers(0, 256, (16, 24, 3), dtype=np.uint8),
        "smooth": smooth_image(),
        "flat": np.full((8, 16, 3), 200, dtype=np.uint8),
        "checker": checker,
    }


def clip_frames():
    """(3, 48, 64, 3): the smooth image, uniform noise, the smooth image of another seed - a T = 3 clip for the end-to-end tests"""
    noise = np.random.default_rng(21).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    return np.stack([smooth_image(), noise, smooth_image(seed=8)])


def quantize_cases():
    """(name, quality): every named frame at 100, 95, 75, the checkerboard not at 100 (2.1 % of its quotients sit inside the tie
    window there, above the 2 % cap)"""
    return [(n, q) for n in ("mcu", "noise", "smooth", "flat", "checker") for q in (100, 95, 75) if not (n == "checker" and q == 100)]


def handmade_coefficients():
    """{name: int16 (mcu_rows, mcu_cols, 3, 64)}: the coder's corner cases on 1 x 1, 1 x 3 and 2 x 3 MCU grids"""
    out = {}

    def grid(r, c):
        return np.zeros((r, c, 3, 64), dtype=np.int16)

    out["all_zero"] = grid(1, 1)
    g = grid(1, 3)
    g[0, :, :, 0] = [[5, -3, 2], [5, -3, 2], [-100, 7, 0]]
    out["dc_only"] = g
    g = grid(1, 3)
    g[0, :, :, 0] = [[1023] * 3, [-1024] * 3, [1023] * 3]                 # differences of +1023, -2047, +2047: categories 10, 11, 11
    out["dc_extremes"] = g
    g = grid(1, 3)
    g[0, 0, 0, 1:64] = 1023
    g[0, 1, 1, 1:64] = -1023
    g[0, 2, 2, 1:64:2] = 1023
    g[0, 2, 2, 2:64:2] = -1023
    out["ac_extremes"] = g                                                 # also the longest block: every coefficient at 26 bits
    g = grid(1, 1)
    g[0, 0, :, 63] = [1, -1, 7]
    g[0, 0, :, 5] = [3, 0, -2]
    out["no_eob"] = g
    g = grid(2, 3)
    for i, (idx, val) in enumerate(((17, 1), (33, -2), (48, 5), (16, -1), (50, 9), (63, -1))):
        g[i // 3, i % 3, :, idx] = val                                     # runs of 16, 32, 47, 15, 49 zeros, and 62 zeros before index 63
        g[i // 3, i % 3, :, 0] = i - 2
    out["zero_runs"] = g
    g = grid(1, 1)
    g[0, 0, 0, 63] = 4
    out["only_63"] = g
    return out


def residue_sweep():
    """single-MCU frames, DC-only with growing values, until the reference's bit lengths have hit all eight residues mod 8"""
    out, seen = [], set()
    for v in range(0, 64):
        c = np.zeros((1, 1, 3, 64), dtype=np.int16)
        c[0, 0, 0, 0] = v
        c[0, 0, 1, 1] = v // 3
        n = encode_scan(c)[1] % 8
        if n not in seen:
            seen.add(n)
            out.append(c)
        if len(seen) == 8:
            break
    return out
