"""Exact-integer GEMM problems in framed buffers: the helpers of tests/test_gemm_exact_gpu.py, checked without a device by
tests/test_gemm_exact_cpu.py.

Operands are small integers (A, A2 in [-3, 3], W in [-2, 2], bias / rowvec / residuals integers, alpha in {1, 0.5, 2}): exact in bfloat16 and
IEEE half, every partial sum of |a| |w| far below 2^24, so the f32 result of avsd_gemm_bf16 is THE value whatever the K order, the split-K
slicing or the three-pass splitting — the comparison needs no tolerance.  The reference is the float64 statement of the operation on the CPU.

Every tensor a launch writes is a view inside a larger buffer pre-filled with a bit pattern (Frame), every tensor it reads a slice of a
wider buffer whose surroundings hold SENTINEL (embed): a store outside the view changes the pattern, a load outside the slice moves the
result by >= 4096 (0 x SENTINEL stays 0: a tile that zero-fills one operand of a K tail is correct; NaN is deliberately not used).
"""
import functools
import math

import torch
import torch.nn.functional as F

SENTINEL = 4096.0
GUARD = 4096          # elements before and after a contiguous framed view
ROWS = 2              # rows above and below a column-slice view
COLS = 8              # columns left and right of a column-slice view (16-byte alignment of every row start is kept)
PAT16 = 0x5A5A        # fill of 16-bit buffers (bf16 1.5e16, fp16 203.25: neither is a value these problems produce)
PAT32 = 0x5A5A5A5A    # fill of f32 buffers (1.5e16)
FORMS = ("flat", "cols")
PLAIN, TMIX, CONV3 = 0, 1, 2


# ---- problems ------------------------------------------------------------------------------------------------------------------------
def ints(shape, lo, hi, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


class Problem:
    """operands as float64 CPU tensors in the layout ops.gemm takes them, and the exact result `ref` [rows out, columns out]"""

    def __init__(self, **kw):
        self.a2 = self.bias = self.rowvec = self.res1 = self.res2 = None
        self.rows_per_vec, self.alpha, self.kw = 0, 1.0, {}
        self.__dict__.update(kw)

    def abs_bound(self):
        """largest sum of |terms| of any output element: bounds every partial sum in any order"""
        a = self.a_full.abs() @ self.w_full.abs().T * max(self.alpha, 1.0)
        for t in self.terms:
            a = a + t.abs()
        return float(a.max())


def _epilogue(p, M, N, epi, seed, small):
    """adds the linear epilogue terms named in `epi` to p.ref (= A' . W^T so far): 'bias', 'rowvec', 'res1', 'res2', 'alpha:<v>'"""
    r = 4 if small else 64
    p.rowvec_rows = None
    for e in epi:
        if e.startswith("alpha:"):
            p.alpha = float(e[6:])
    assert p.alpha in (1.0, 0.5, 2.0)
    p.ref = p.alpha * p.ref
    if "bias" in epi:
        p.bias = ints((N,), -16 if not small else -4, 16 if not small else 4, seed + 11)
        p.ref = p.ref + p.bias
    if "rowvec" in epi:
        p.rows_per_vec = max(1, (M + 2) // 3)             # three vectors, the last one shorter
        nv = (M + p.rows_per_vec - 1) // p.rows_per_vec
        p.rowvec = ints((nv, N), -r // 4, r // 4, seed + 12)
        p.rowvec_rows = p.rowvec.repeat_interleave(p.rows_per_vec, 0)[:M]
        p.ref = p.ref + p.rowvec_rows
    if "res1" in epi:
        p.res1 = ints((M, N), -r, r, seed + 13)
        p.ref = p.ref + p.res1
    if "res2" in epi:
        p.res2 = ints((M, N), -r, r, seed + 14)
        p.ref = p.ref + p.res2
    p.terms = [t for t in (p.bias, p.rowvec_rows, p.res1, p.res2) if t is not None]      # each broadcasts against a_full . w_full^T
    return p


@functools.lru_cache(maxsize=None)
def plain(M, N, K, k1=0, epi=(), seed=0, small=False):
    """out = alpha [a | a2] . w^T + ...; k1 > 0: two sources split at k1.  small: |v| <= 512 for the row statistics"""
    am, wm = (1, 1) if small else (3, 2)
    a, w = ints((M, K), -am, am, seed + 1), ints((N, K), -wm, wm, seed + 2)
    p = Problem(mode=PLAIN, a=a[:, :k1] if k1 else a, a2=a[:, k1:] if k1 else None, w=w, a_full=a, w_full=w, ref=a @ w.T, M=M, N=N, K=K)
    return _epilogue(p, M, N, epi, seed, small)


@functools.lru_cache(maxsize=None)
def batched(B, M, N, K, epi=(), seed=0):
    """out[b] = alpha a[b] . w[b]^T + bias"""
    a, w = ints((B, M, K), -3, 3, seed + 1), ints((B, N, K), -2, 2, seed + 2)
    p = Problem(mode=PLAIN, a=a, w=w, a_full=a.reshape(B * M, K), w_full=w.reshape(B * N, K), ref=torch.einsum("bmk,bnk->bmn", a, w), M=M, N=N, K=K)
    for e in epi:
        if e.startswith("alpha:"):
            p.alpha = float(e[6:])
    p.ref = p.alpha * p.ref
    p.terms = []
    if "bias" in epi:
        p.bias = ints((N,), -16, 16, seed + 11)
        p.ref = p.ref + p.bias
        p.terms = [p.bias.repeat(B)]
    return p


def tmix_rows(y, B, Fr, hw):
    """the temporal mix's A operand: row (b, f, s) = [frame 0 | frame max(f - 1, 0) | frame f] of pixel s"""
    C = y.shape[1]
    y5 = y.reshape(B, Fr, hw, C)
    prev = torch.cat([y5[:, :1], y5[:, :-1]], 1)
    return torch.cat([y5[:, :1].expand_as(y5), prev, y5], -1).reshape(B * Fr * hw, 3 * C)


@functools.lru_cache(maxsize=None)
def tmix(B, Fr, hw, C, N, epi=(), seed=0):
    M = B * Fr * hw
    y, w = ints((M, C), -3, 3, seed + 1), ints((N, 3 * C), -2, 2, seed + 2)
    cat = tmix_rows(y, B, Fr, hw)
    p = Problem(mode=TMIX, a=y, w=w, a_full=cat, w_full=w, ref=cat @ w.T, M=M, N=N, K=3 * C, kw=dict(tmix=(hw, Fr)))
    return _epilogue(p, M, N, epi, seed, False)


def conv_out_hw(hs, ws, stride, ups):
    hin, win = hs << ups, ws << ups
    return (hin + 2 - 3) // stride + 1, (win + 2 - 3) // stride + 1


def subpixel_weights(wf):
    """asva_amd.weights.subpixel_conv3x3 restated in float64: [cout, 3, 3, cin] -> [4 cout, 4 cin], the three kernel rows (columns) folded
    onto the two input rows (columns) each output-pixel parity sees"""
    cout, _, _, cin = wf.shape
    sets = (((0,), (1, 2)), ((0, 1), (2,)))
    out = torch.zeros((2, 2, cout, 2, 2, cin), dtype=wf.dtype)
    for dy in range(2):
        for dx in range(2):
            for i in range(2):
                for j in range(2):
                    for ky in sets[dy][i]:
                        for kx in sets[dx][j]:
                            out[dy, dx, :, i, j, :] += wf[:, ky, kx, :]
    return out.reshape(4 * cout, 4 * cin)


def im2col(x, n_img, hs, ws, stride, ups, pad):
    """[n_img hs ws, cin] -> [M, 9 cin] in the tap-major order of the packed weights: what the CONV3 loader presents as A"""
    cin = x.shape[1]
    xi = x.reshape(n_img, hs, ws, cin).permute(0, 3, 1, 2)
    if ups:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    xi = F.pad(xi, (1, 1, 1, 1) if pad else (0, 1, 0, 1))
    ho, wo = conv_out_hw(hs, ws, stride, 1 if ups else 0)
    cols = F.unfold(xi, 3, stride=stride)                       # [n, cin * 9, L], channel-major
    assert cols.shape[2] == ho * wo, (cols.shape, ho, wo)
    return cols.reshape(n_img, cin, 9, ho * wo).permute(0, 3, 2, 1).reshape(n_img * ho * wo, 9 * cin)


@functools.lru_cache(maxsize=None)
def conv(n_img, hs, ws, cin, cout, stride=1, ups=0, pad=1, k1=0, epi=(), seed=0, small=False):
    """3x3 convolution on channels-last rows; ups = 1: behind a nearest 2x upsample; ups = 2: the same in the sub-pixel form (four 2x2
    convolutions, summed weights up to 4 x 2); pad = 0: stride 2 over F.pad(x, (0, 1, 0, 1)).  Reference: F.conv2d in float64."""
    am, wm = (1, 1) if small else (3, 2)
    x = ints((n_img * hs * ws, cin), -am, am, seed + 1)
    w4 = ints((cout, cin, 3, 3), -wm, wm, seed + 2)
    xi = x.reshape(n_img, hs, ws, cin).permute(0, 3, 1, 2)
    if ups:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    if pad == 0:
        assert stride == 2 and ups == 0 and hs % 2 == 0 and ws % 2 == 0
        ref = F.conv2d(F.pad(xi, (0, 1, 0, 1)), w4, stride=2)
    else:
        ref = F.conv2d(xi, w4, stride=stride, padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, cout)
    M = ref.shape[0]
    wl = w4.permute(0, 2, 3, 1).contiguous()                      # [cout, 3, 3, cin]
    w9 = wl.reshape(cout, 9 * cin)
    w = subpixel_weights(wl) if ups == 2 else w9
    a_full = im2col(x, n_img, hs, ws, stride, ups, pad)
    assert torch.equal(a_full @ w9.T, ref)                        # (the im2col statement and F.conv2d agree: both exact)
    p = Problem(mode=CONV3, a=x[:, :k1] if k1 else x, a2=x[:, k1:] if k1 else None, w=w, a_full=a_full, w_full=w9, ref=ref, M=M, N=cout, K=w.shape[1],
                kw=dict(conv=(n_img, hs, ws, stride, ups) + ((0,) if pad == 0 else ())))
    p = _epilogue(p, M, cout, epi, seed, small)
    if ups == 2 and p.bias is not None:
        p.bias = p.bias.repeat(4)                                 # once per output-pixel parity
    return p


def check_problem(p, small=False):
    """the properties the exact comparison rests on; raises AssertionError.  Returns (bound on any partial sum, max |value|)."""
    bound, top = p.abs_bound(), float(p.ref.abs().max())
    assert bound < 2 ** 24 and top < 2 ** 15 and top <= bound, (bound, top)
    if small:
        assert top <= 512, top
    # the float64 reference against an f32 product summed in two different K orders: ascending in blocks of 8 columns, and the columns
    # taken descending in steps of 7, again 8 at a time
    a, w = p.a_full.float(), p.w_full.float()
    K = a.shape[1]
    order = torch.tensor([k for s in range(7) for k in range(K - 1 - s, -1, -7)])
    assert sorted(order.tolist()) == list(range(K))
    fwd, rev = torch.zeros(a.shape[0], w.shape[0]), torch.zeros(a.shape[0], w.shape[0])
    for k in range(0, K, 8):
        fwd += a[:, k:k + 8] @ w[:, k:k + 8].T
        rev += a[:, order[k:k + 8]] @ w[:, order[k:k + 8]].T
    assert fwd.dtype == torch.float32 and torch.equal(fwd, rev)
    lin = p.alpha * fwd
    for t in p.terms:
        lin = lin + t.float()
    assert lin.dtype == torch.float32
    if p.a.dim() == 2:
        assert torch.equal(lin.double(), p.ref)
    else:                                   # batched: the block diagonal of the flattened product
        B, M, N = p.ref.shape
        for b in range(B):
            assert torch.equal(lin[b * M:(b + 1) * M, b * N:(b + 1) * N].double(), p.ref[b])
    # operands survive both storage types
    for t in (p.a, p.a2, p.w, p.res1, p.res2):
        if t is not None:
            assert torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)
    for t in (p.bias, p.rowvec):
        if t is not None:
            assert torch.equal(t.float().double(), t)
    return bound, top


# ---- storage ---------------------------------------------------------------------------------------------------------------------------
def round16(v, dtype):
    """float64 -> the 16-bit storage type, round to nearest even (|v| < 2^24 integers or halves: the f32 step in between is exact)"""
    return v.float().to(dtype)


def _ints_of(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _pad8(n):
    return (n + 7) // 8 * 8


class Frame:
    """an output view of `shape` (2-D, or 3-D [B, M, N]) inside a larger pattern-filled buffer.
      flat: contiguous (ld == N), GUARD elements before and after — catches stores before row 0 / past row M
      cols: buf[ROWS:ROWS + M, COLS:COLS + N] of a buffer 2 COLS columns wider (ld == N + 16) — catches stores past column N
    planes = 2: a twin allocation [2, n]: `view` in the first half and `rest` at the same offset in the second (split-precision storage,
    or the explicit (main, rest) pair of AVSD_GEMM_OUT_REST)."""

    def __init__(self, shape, dtype, form, device, planes=1):
        assert form in FORMS
        self.shape, self.dtype, self.form, self.planes = tuple(int(s) for s in shape), dtype, form, planes
        *lead, M, N = self.shape
        B = lead[0] if lead else 1
        if form == "flat":
            self.full = None
            n = 2 * GUARD + _pad8(B * M * N)
        else:
            self.full = (B, M + 2 * ROWS, N + 2 * COLS)
            n = _pad8(math.prod(self.full))
        self.buf = torch.empty((planes, n), dtype=dtype, device=device)
        _ints_of(self.buf).fill_(PAT16 if self.buf.element_size() == 2 else PAT32)
        self.view = self._view(0)
        self.rest = self._view(1) if planes == 2 else None
        assert self.view.data_ptr() % 16 == 0 and self.view.shape == self.shape

    def _view(self, plane):
        *lead, M, N = self.shape
        B = lead[0] if lead else 1
        if self.form == "flat":
            v = self.buf[plane, GUARD:GUARD + B * M * N].view(B, M, N)
        else:
            v = self.buf[plane, :math.prod(self.full)].view(self.full)[:, ROWS:ROWS + M, COLS:COLS + N]
        return v if lead else v[0]

    def untouched(self):
        """True while every element of the buffer still holds the fill pattern"""
        return bool((_ints_of(self.buf) == (PAT16 if self.buf.element_size() == 2 else PAT32)).all())

    def check(self, want, want_rest=None, what=""):
        """the view holds `want` (and the rest plane `want_rest`) exactly, and nothing around them was written.  `want` None: frame only.
        Destructive: the views are re-filled with the pattern to compare the whole buffer in one pass."""
        assert want is None or (want_rest is not None) == (self.planes == 2), "a twin frame is checked plane by plane"
        got = self.view.clone()
        got_rest = self.rest.clone() if self.rest is not None else None
        pat = PAT16 if self.buf.element_size() == 2 else PAT32
        _ints_of(self.view).fill_(pat)
        if self.rest is not None:
            _ints_of(self.rest).fill_(pat)
        bad = _ints_of(self.buf) != pat
        if bool(bad.any()):
            at = bad.nonzero()[:8].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} element(s) outside the {self.form} view of {self.shape} were written, first at (plane, offset) {at}"
                                 f" (view starts at offset {self.view.storage_offset()}, row stride {self.view.stride(-2)})")
        if want is None:
            return
        for name, g, w in (("out", got, want), ("rest plane", got_rest, want_rest)):
            if w is None:
                continue
            w = w.to(g.device)
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
            if not torch.equal(g, w):
                ne = (g != w).reshape(-1, g.shape[-1]) if g.dim() > 1 else (g != w)[None]
                at = ne.nonzero()[:6].tolist()
                raise AssertionError(f"{what}: {name} differs from the exact value in {int(ne.sum())} of {g.numel()} elements, first at (row, column) {at}: "
                                     f"got {[float(g.reshape(-1, g.shape[-1])[r, c]) for r, c in at]}, want {[float(w.reshape(-1, w.shape[-1])[r, c]) for r, c in at]}")


def embed(t, dtype, device, twin=False):
    """a 2-D / 3-D float64 tensor in storage type `dtype` as a slice of a wider SENTINEL-filled buffer (ROWS rows above and below, COLS
    columns left and right; 1-D: COLS elements either side).  twin: the main plane of a split-precision twin allocation; the values are
    exact in 16 bits, so the rest plane holds zeros inside the slice (and SENTINEL around it)."""
    if t is None:
        return None
    if t.dim() == 1:
        buf = torch.full((t.numel() + 2 * COLS,), SENTINEL, dtype=dtype, device=device)
        buf[COLS:COLS + t.numel()] = t.to(dtype)
        return buf[COLS:COLS + t.numel()]
    *lead, M, K = t.shape
    B = lead[0] if lead else 1
    full = (B, M + 2 * ROWS, K + 2 * COLS)
    n = _pad8(math.prod(full))
    buf = torch.full((2 if twin else 1, n), SENTINEL, dtype=dtype, device=device)
    view = buf[0, :math.prod(full)].view(full)[:, ROWS:ROWS + M, COLS:COLS + K]
    view.copy_(t.reshape(B, M, K).to(dtype))
    if twin:
        buf[1, :math.prod(full)].view(full)[:, ROWS:ROWS + M, COLS:COLS + K].zero_()
    return view if lead else view[0]


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------
PRECS = ("bf16", "fp16", "bf16x2")
# hand-scheduled tiles (csrc/gemm4.hip avsd_gemm_dispatch_asm: launch4<FM, FN> is a 64 FM x 64 FN block), the N-streaming tile's band of
# 96 rows and 8 fragments of 32 columns per wave set (csrc/nstream.hip), the resident convolution tiles' column widths (ops._CONV3R*_BN)
ASM_BLOCK = {60: (256, 256), 61: (256, 128), 62: (128, 256), 63: (128, 128), 64: (128, 64), 65: (64, 128), 66: (64, 64), 67: (128, 320)}
ASM_X2 = (63, 64, 65, 66)
ASM_TMIX = (61, 62, 63, 64, 65, 66, 67)
NSTREAM_BLOCK = (96, 256)
IMAGES = ((1, 3, 5), (2, 4, 4), (3, 8, 12))          # (n_img, hs, ws)


def built_tiles():
    """{family: {tile id: (BM, BN)}} of every tile the library builds, from the dispatchers tests/test_tile_choice_cpu.py parses"""
    from asva_amd import ops
    from tests.test_tile_choice_cpu import _dispatcher

    one, x2 = _dispatcher("dispatch_tile"), _dispatcher("dispatch_tile_x2")
    assert set(ASM_BLOCK) == set(ops.ASM_TILES)
    r1 = {t: (0, ops._CONV3R_BN[t - 40]) for t in ops.CONV3R_TILES}
    r2 = {t: (0, ops._CONV3R2D_BN[t]) for t in ops.CONV3R2D_TILES}
    return {"one": one, "x2": x2, "subpix": _dispatcher("avsd_gemm_dispatch_subpix"), "subpix_x2": _dispatcher("avsd_gemm_dispatch_x2_subpix"),
            "asm": dict(ASM_BLOCK), "nstream": {ops.NSTREAM_TILE: NSTREAM_BLOCK}, "resident": {**r1, **r2}}


class Launch:
    """one ops.gemm / ops.gemm_batched call of the matrix: which problem (builder name + arguments), on which tile, what it writes"""

    def __init__(self, build, args, tile, form, *, epi=(), out="16", r1="16", r2="16", master=False, out_rest=False, rowstats=False, split_k=1,
                 nonlinear=None, small=False):
        self.build, self.tile, self.form, self.epi, self.out, self.r1, self.r2 = build, tile, form, tuple(epi), out, r1, r2
        self.master, self.out_rest, self.rowstats, self.split_k, self.nonlinear, self.small = master, out_rest, rowstats, split_k, nonlinear, small
        kw = dict(args)
        kw["epi"] = self.epi
        if small:
            kw["small"] = True
        self.key = (build, tuple(sorted(kw.items())))

    def problem(self):
        return globals()[self.build](**dict(self.key[1]))

    def __repr__(self):
        opts = [f"out={self.out}", f"form={self.form}"] + [k for k in ("master", "out_rest", "rowstats") if getattr(self, k)]
        opts += [f"split_k={self.split_k}"] if self.split_k > 1 else []
        opts += [self.nonlinear] if self.nonlinear else []
        return f"{self.build}{dict(self.key[1])} tile {self.tile} " + " ".join(opts)


# the linear epilogue terms, spread over four launches per shape: every term alone and together, both residuals in both types, every output
RECIPES = (
    dict(epi=()),
    dict(epi=("bias", "res1")),
    dict(epi=("bias", "rowvec", "res1", "res2", "alpha:0.5"), r1="f32", master=True),
    dict(epi=("rowvec", "res1", "res2", "alpha:2"), out="f32", r2="f32"),
)
REST_RECIPE = dict(epi=("bias", "res2"), r2="f32", out_rest=True)          # the IEEE-half library only (AVSD_GEMM_OUT_REST)
STATS_RECIPE = dict(epi=("bias", "res1"), rowstats=True, small=True)


def _recipe(rec, prec):
    rec = dict(rec)
    if prec == "bf16x2":
        rec.pop("master", None)          # split precision has no f32 master: refused, asserted once by the GPU file
    return rec


def _tmix_geom(m_big):
    """(B, frames, hw) with 3 frames and the fewest rows above m_big"""
    return (1, 3, m_big // 3 + 1)


def plan_plain(tile, bm, bn, prec, fam):
    """fam: 'v1' register-staged, 'lds' LDS-direct (also 34-36 under split precision), 'asm', 'nstream'"""
    Ks = {"asm": (64, 192, 576), "nstream": (320, 640)}.get(fam, (8, 72, 200, 576))
    Ns = (32, bn + 32) if fam == "nstream" else (4, bn + 4)
    shapes = [(M, N, K) for M in (7, bm + 1) for N in Ns for K in Ks]
    if fam != "nstream":
        shapes.append((bm + 1, bn + 8, Ks[1]))        # ld % 8 == 0: the 16-byte store form up to the last column fragment
    for i, (M, N, K) in enumerate(shapes):          # two recipes per shape: over the K values every (M, N) meets each recipe in both frame forms
        for f, j in enumerate((i % 4, (i + 2) % 4)):
            yield Launch("plain", dict(M=M, N=N, K=K), tile, FORMS[(i // 4 + f) % 2], **_recipe(RECIPES[j], prec))
        if prec == "fp16" and fam != "nstream" and i % 2 == 0:
            yield Launch("plain", dict(M=M, N=N, K=K), tile, FORMS[(i // 2) % 2], **REST_RECIPE)
    # row statistics of the stored output
    for i, (M, N) in enumerate((M, N) for M in (7, bm + 1) for N in (32, bn + 32)):
        yield Launch("plain", dict(M=M, N=N, K=Ks[1]), tile, FORMS[i % 2], **STATS_RECIPE)
    # split-K: even and uneven slices, a slice that is the K tail alone
    splits = {"lds": ((72, 2), (200, 2), (576, 2), (576, 5)), "asm": ((192, 2), (576, 2), (576, 5))}.get(fam, ())
    for i, ((K, sk), M, N) in enumerate((s, M, N) for s in splits for M in (7, bm + 1) for N in Ns):
        yield Launch("plain", dict(M=M, N=N, K=K), tile, FORMS[(i // 2) % 2], split_k=sk, **_recipe(RECIPES[2 + i % 2], prec))


def plan_two_source(tile, bm, bn, prec, fam):
    """k_split on a 64 boundary (LDS-direct tiles switch buffers per K tile) and the unaligned 160 + 160 form (register-staged tiles)"""
    if fam == "lds":
        for i, (M, N, (k1, K)) in enumerate((M, N, kk) for M in (7, bm + 1) for N in (4, bn + 4) for kk in ((64, 72), (128, 200))):
            for j in (1, 3):
                yield Launch("plain", dict(M=M, N=N, K=K, k1=k1), tile, FORMS[(i + j) % 2], **_recipe(RECIPES[j], prec))
        for i, (M, N) in enumerate((M, N) for M in (7, bm + 1) for N in (4, bn + 4)):
            yield Launch("plain", dict(M=M, N=N, K=200, k1=128), tile, FORMS[i % 2], split_k=2, **_recipe(RECIPES[3], prec))
    else:       # v1 tiles, and tile 0 (the dispatcher's own fall-back to them; split precision: ops.gemm's two-launch form)
        for i, (M, N) in enumerate((M, N) for M in (7, bm + 1) for N in (4, bn + 4)):
            for j in (1, 3):
                rec = _recipe(RECIPES[j], prec)
                if prec == "bf16x2" and j == 3:
                    rec = dict(epi=("rowvec", "res1", "alpha:2"), out="f32", r1="f32")        # (that form takes one residual)
                yield Launch("plain", dict(M=M, N=N, K=320, k1=160), tile, FORMS[(i + j) % 2], **rec)


def plan_tmix(tile, bm, bn, prec, fam):
    Cs = (64, 192) if fam == "asm" else (8, 24, 72, 192)
    geoms = ((1, 7, 1), _tmix_geom(bm))
    shapes = [(g, N, C) for g in geoms for N in (4, bn + 4) for C in Cs]
    for i, ((B, Fr, hw), N, C) in enumerate(shapes):
        for j in (1, 3):
            yield Launch("tmix", dict(B=B, Fr=Fr, hw=hw, C=C, N=N), tile, FORMS[(i + j) % 2], **_recipe(RECIPES[j], prec))
    # K slices that start inside a segment (C = 72: slice 1 starts at k = 128 of segment [72, 144); C = 192: at 320 of [192, 384))
    splits = () if fam == "v1" else ((64, 2), (192, 2)) if fam == "asm" else ((72, 2), (192, 2))
    for i, ((C, sk), (B, Fr, hw), N) in enumerate((s, g, N) for s in splits for g in geoms for N in (4, bn + 4)):
        yield Launch("tmix", dict(B=B, Fr=Fr, hw=hw, C=C, N=N), tile, FORMS[i % 2], split_k=sk, **_recipe(RECIPES[2 + i % 2], prec))


CONV_FORMS = ((1, 0, 1), (2, 0, 1), (1, 1, 1), (2, 1, 1), (2, 0, 0))          # (stride, ups, pad); pad 0: the asymmetric form, even images


def plan_conv(tile, bm, bn, prec, fam):
    """the tap-major 3x3 convolution"""
    i = 0
    for n_img, hs, ws in IMAGES:
        for stride, ups, pad in CONV_FORMS:
            if pad == 0 and (hs % 2 or ws % 2):
                continue
            for cin in (8, 64):
                for cout in (4, bn + 4):
                    n = 1 if ups else n_img          # (an upsampled 8 x 12 image is 384 rows already)
                    yield Launch("conv", dict(n_img=n, hs=hs, ws=ws, cin=cin, cout=cout, stride=stride, ups=ups, pad=pad), tile, FORMS[(i // 4 + i) % 2],
                                 **_recipe(RECIPES[i % 4], prec))
                    i += 1
    if fam == "lds":
        for i, (sk, cout) in enumerate((sk, c) for sk in (2, 5) for c in (4, bn + 4)):
            yield Launch("conv", dict(n_img=2, hs=4, ws=4, cin=64, cout=cout), tile, FORMS[i % 2], split_k=sk, **_recipe(RECIPES[2 + i % 2], prec))


def plan_subpix(tile, bm, bn, prec, fam):
    """ups = 2: whole column tiles per output-pixel parity (cout % BN == 0, cout % 64 == 0); bias / master / rest plane only"""
    cout = bn * 64 // math.gcd(bn, 64)
    recs = (dict(epi=("bias",), out="f32"), dict(epi=("bias",), master=True, out_rest=prec != "bf16x2"), dict(epi=()))
    i = 0
    for n_img, hs, ws in IMAGES:
        for rec in recs:
            for form in FORMS:
                yield Launch("conv", dict(n_img=n_img, hs=hs, ws=ws, cin=64, cout=cout, ups=2), tile, form, split_k=2 if i % 3 == 2 else 1, **_recipe(rec, prec))
                i += 1


def plan_resident(tile, bn, supported):
    """LDS-resident 3x3 convolutions (one-pass libraries): the images of IMAGES the tile admits plus the smallest it is built for (4 x 4
    in whole images, 8 x 32 / 4 x 32 for the rectangular tiles); supported(tile, hs, ws, cin) -> rows per tile, 0 = refused"""
    images = IMAGES + ((6, 4, 4), (17, 4, 4), (1, 8, 32), (3, 4, 32), (2, 8, 32))
    i = 0
    for n_img, hs, ws in images:
        for cin, k1 in ((64, 0), (128, 0), (128, 64)):
            if not supported(tile, hs, ws, cin):
                continue
            for cout in (4, bn + 4):
                for sk in (1, 2) if cin == 128 else (1,):
                    rec = dict(RECIPES[i % 4])
                    if i % 5 == 4:
                        rec = dict(STATS_RECIPE)
                        cout = bn + 32 if cout > 4 else 32
                    yield Launch("conv", dict(n_img=n_img, hs=hs, ws=ws, cin=cin, cout=cout, k1=k1), tile, FORMS[(i // 4 + i) % 2], split_k=sk, **rec)
                    i += 1


def plan_batched(tile, bm, bn, prec, fam):
    recs = (dict(epi=("alpha:0.5", "bias")), dict(epi=("alpha:2",), out="f32"))
    for i, (M, N, K) in enumerate((M, N, K) for M in (7, bm + 1) for N in (4, bn + 4) for K in (8, 200)):
        for j, rec in enumerate(recs):
            yield Launch("batched", dict(B=3, M=M, N=N, K=K), tile, FORMS[(i + j) % 2], **rec)


def plan_nonlinear(tile, bm, bn, prec, fam):
    """GELU, GEGLU, the LayerNorm fold, and GEGLU behind the fold (tile 70's written-out form): the frame check only"""
    K = 320 if fam == "nstream" else 64
    for i, (M, N) in enumerate((M, N) for M in (7, bm + 1) for N in (32, bn + 32)):
        for j, kind in enumerate(("gelu", "geglu", "ln", "geglu_ln")):
            for f, form in enumerate(FORMS):
                yield Launch("plain", dict(M=M, N=N, K=K), tile, form, epi=("bias",), nonlinear=kind, out="f32" if (i + j + f) % 4 == 3 else "16")


def families(prec):
    """(family, {tile: (BM, BN)}) pairs that run under `prec`: ids 34-36 under split precision only, the N-streaming and resident tiles in
    the one-pass libraries only, the hand-scheduled tiles 63-66 in all three"""
    t = built_tiles()
    if prec == "bf16x2":
        return {"lds": t["x2"], "asm": {k: v for k, v in t["asm"].items() if k in ASM_X2}, "subpix": t["subpix_x2"]}
    return {"v1": {k: v for k, v in t["one"].items() if k < 4}, "lds": {k: v for k, v in t["one"].items() if k >= 4}, "asm": t["asm"],
            "nstream": t["nstream"], "subpix": t["subpix"], "resident": t["resident"]}


PLANS = {"plain": (plan_plain, ("v1", "lds", "asm", "nstream")), "two_source": (plan_two_source, ("v1", "lds")),
         "tmix": (plan_tmix, ("v1", "lds", "asm")), "conv": (plan_conv, ("v1", "lds")), "subpix": (plan_subpix, ("subpix",)),
         "batched": (plan_batched, ("v1", "lds")), "nonlinear": (plan_nonlinear, ("v1", "lds", "asm", "nstream"))}


def matrix(prec):
    """[(plan name, family, tile, BM, BN)] of everything test_gemm_exact_gpu.py runs under `prec` through PLANS"""
    out = []
    fams = families(prec)
    for name, (_, fs) in PLANS.items():
        for fam in fs:
            for tile, (bm, bn) in sorted(fams.get(fam, {}).items()):
                if name == "tmix" and fam == "asm" and tile not in ASM_TMIX:
                    continue
                out.append((name, fam, tile, bm, bn))
    # the unaligned two-source form on tile 0: the dispatcher's own fall-back to a register-staged tile / split precision's two launches
    out.append(("two_source", "v1", 0, 64, 64))
    return out


def launches(prec, name, fam, tile, bm, bn):
    return list(PLANS[name][0](tile, bm, bn, prec, fam))


def all_problem_keys(resident_supported=lambda tile, hs, ws, cin: 1):
    """every distinct generator configuration of the matrix (resident convolutions: with a permissive geometry predicate, a superset)"""
    keys = {}
    for prec in PRECS:
        for row in matrix(prec):
            for L in launches(prec, *row):
                keys.setdefault(L.key, L)
        for tile, (_, bn) in families(prec).get("resident", {}).items():
            for L in plan_resident(tile, bn, resident_supported):
                keys.setdefault(L.key, L)
    return keys
