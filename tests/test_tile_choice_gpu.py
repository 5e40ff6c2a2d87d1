"""The tile that `ops.gemm(tile=0)` picks BY RULE, launched (-m gpu).  tests/test_ops_gpu.py, test_split_gpu.py and test_planes_gpu.py run
every built tile id by number; their tile = 0 cases are small enough (M <= ~3000) that the rule ends in its 64 x 64 / 128 x 64 branches
or the committed table answers.  Here the table is emptied for each test, the measuring tuner is off, and a spy on the two rules
(_heuristic_tile / _heuristic_tile_x2) states which branch each case started from (tests/test_tile_choice_cpu.py pins the same points
without a device), so a later change of the rule cannot quietly turn a case into a repeat of another.

References are float64 statements of the same operation on the values the kernel reads.  Tolerances (rel-L2 over the whole output) are
the constants of the files above for the same operations:
  bf16: 16-bit outputs 4e-3, f32 outputs 2e-5 (test_ops_gpu.py)         split precision: 3e-5 / 2e-5, GEGLU 2 x, LayerNorm fold 5e-5
  explicit (main, rest) planes, three passes: 3e-5 (test_ops_gpu.py, test_planes_gpu.py)            (test_split_gpu.py)
  fp16 16-bit outputs: 5e-4 = the bf16 bound / 8 (11 significand bits against 8; the products and f32 sums are the same)
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_blocks_gpu import TOL as BLOCK_TOL, _pack, _rows, _state, _video, gold, prec  # noqa: F401  (gold, prec: fixtures)

pytestmark = pytest.mark.gpu

TOL_BF16 = 4e-3
TOL_FP16 = TOL_BF16 / 8
TOL_F32 = 2e-5
TOL_X2_16 = 3e-5
TOL_X2_32 = 2e-5
TOL_PLANES = 3e-5
TOL_X2_LNFOLD = 5e-5


def dev():
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rndf(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dev())


def act(*shape, seed=0, scale=1.0, shift=0.0):
    """seeded tensor in the storage type of the active precision (two planes in split mode) + the float64 values a kernel reads from it"""
    from asva_amd import ops

    t = ops.to_act(rndf(*shape, seed=seed, scale=scale, shift=shift))
    return t, ops.from_act(t).double()


def packed(wf):
    """f32 weights -> (storage tensor, the float64 values a kernel reads from it)"""
    from asva_amd.weights import from_act, to_act

    t = to_act(wf)
    return t, from_act(t).double()


def tol16(prec):
    return {"bf16": TOL_BF16, "fp16": TOL_FP16, "bf16x2": TOL_X2_16}[prec]


def tol32(prec):
    return TOL_X2_32 if prec == "bf16x2" else TOL_F32


class _Spy:
    def __init__(self):
        self.rule = []          # (which rule, (M, N, K, geglu, splitk_ok), (tile, split_k))
        self.subpix = []        # (rule tile, cout, x2, final tile)

    def last(self, which):
        assert self.rule and self.rule[-1][0] == which, self.rule[-1:]
        return self.rule[-1][2]


@pytest.fixture
def rule(monkeypatch, prec):
    """empties the tile table, checks that the tuner is off, and records what the two rules and the sub-pixel repair return"""
    from asva_amd import ops

    assert ops._AUTOTUNE is False
    monkeypatch.setattr(ops, "_TILE_CACHE", {})
    spy = _Spy()

    def wrap(name, fn):
        def f(M, N, K, geglu, splitk_ok):
            r = fn(M, N, K, geglu, splitk_ok)
            spy.rule.append((name, (M, N, K, geglu, splitk_ok), r))
            return r
        return f

    def subpix(tile, cout, x2, fn=ops._subpix_tile):
        r = fn(tile, cout, x2)
        spy.subpix.append((tile, cout, bool(x2), r))
        return r

    monkeypatch.setattr(ops, "_heuristic_tile", wrap("one", ops._heuristic_tile))
    monkeypatch.setattr(ops, "_heuristic_tile_x2", wrap("x2", ops._heuristic_tile_x2))
    monkeypatch.setattr(ops, "_subpix_tile", subpix)
    return spy


# (the precision fixture of tests/test_blocks_gpu.py, narrowed to the builds in which a form exists)
one_pass_builds = pytest.mark.parametrize("prec", ["bf16", "fp16"], indirect=True)
split_build = pytest.mark.parametrize("prec", ["bf16x2"], indirect=True)


# ---- a. sub-pixel upsample convolution (AVSD_GEMM_CONV3 with ups = 2) at widths that are no multiple of 128 --------------------------
# (n_img, hs, ws, cin, cout) -> rule tile in one pass, rule tile of the three-pass forms; every one is repaired to 128 x 64 (tile 24):
# the rule's 256 x 128 / 128 x 128 picks would straddle two output-pixel parities (cout % 128 != 0, gemm.hip launch2), and 12 is not built
# for this loader.  (6, .., 128, 320) is the small-M control; (62, 8, 12, ..) a non-square image; (56, .., 64, 64) fails in the three-pass
# forms only (one pass starts from tile 12 there, which always mapped to 24).
SUBPIX = [((23, 16, 16, 64, 320), 14, 11), ((23, 16, 16, 256, 320), 20, 11), ((14, 16, 16, 256, 448), 30, 11), ((23, 16, 16, 64, 192), 11, 11),
          ((6, 16, 16, 128, 320), 12, 24), ((62, 8, 12, 64, 320), 14, 11)]
SUBPIX_X2_ONLY = [((56, 16, 16, 64, 64), 12, 11)]


def _ups_conv_ref(xv, w, b, n_img, hs, ws):
    """nearest 2x upsample + 3x3 convolution in float64; xv [n_img * hs * ws, cin], w [cout, cin, 3, 3] -> [n_img * 2 hs * 2 ws, cout]"""
    xi = F.interpolate(xv.reshape(n_img, hs, ws, -1).permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    return F.conv2d(xi, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def _tap_exact(xv, wq, b, n_img, hs, ws, cout):
    """the four per-parity 2x2 convolutions on the PACKED weights wq [4 cout, 4 cin] (float64 of what the kernel multiplies): a wrong tap,
    parity or output pixel is an O(1) error"""
    cin = xv.shape[1]
    xp = F.pad(xv.reshape(n_img, hs, ws, cin), (0, 0, 1, 1, 1, 1))
    want = torch.zeros(n_img, 2 * hs, 2 * ws, cout, dtype=torch.float64, device=dev())
    for dy in range(2):
        for dx in range(2):
            taps = torch.cat([xp[:, dy + i:dy + i + hs, dx + j:dx + j + ws] for i in range(2) for j in range(2)], -1).reshape(-1, 4 * cin)
            par = 2 * dy + dx
            want[:, dy::2, dx::2] = (taps @ wq[par * cout:(par + 1) * cout].T + b.double()).reshape(n_img, hs, ws, cout)
    return want.reshape(-1, cout)


def _subpix_operands(n_img, hs, ws, cin, cout):
    from asva_amd.weights import subpixel_conv3x3

    w = rndf(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5)
    return w, rndf(cout, seed=3), subpixel_conv3x3(w.permute(0, 2, 3, 1).contiguous())


@one_pass_builds
@pytest.mark.parametrize("shape,want_one,want_x2", SUBPIX)
def test_subpixel_upsample_by_rule_one_pass(rule, prec, shape, want_one, want_x2):
    """f32 output against the float64 upsampled convolution and against the tap-exact restatement; 16-bit output + rest plane + f32 master
    through the same scatter, bit for bit"""
    from asva_amd import ops, precision as P

    n_img, hs, ws, cin, cout = shape
    M = n_img * hs * ws
    x, xv = act(M, cin, seed=1)
    w, b, wm = _subpix_operands(*shape)
    wp, wq = packed(wm)
    conv = dict(bias=b.repeat(4), mode=ops.CONV3, conv=(n_img, hs, ws, 1, 2))
    o32 = ops.gemm(x, wp, out_f32=True, **conv)
    assert rule.last("one") == (want_one, 1) and rule.subpix[-1] == (want_one, cout, False, 24)
    assert o32.shape == (4 * M, cout)
    e_ref, e_tap = rel_l2(o32, _ups_conv_ref(xv, w, b, n_img, hs, ws)), rel_l2(o32, _tap_exact(xv, wq, b, n_img, hs, ws, cout))
    print(f"ups=2 {shape} [{prec}]: rule tile {want_one} -> {rule.subpix[-1][3]}; f32 output vs float64 conv {e_ref:.3e}, vs tap-exact {e_tap:.3e}")
    assert e_ref < TOL_BF16 and e_tap < TOL_F32
    out, rest = ops.alloc_planes((4 * M, cout), dev())
    master = torch.empty((4 * M, cout), dtype=torch.float32, device=dev())
    ops.gemm(x, wp, out=out, out_rest=rest, master=master, **conv)
    assert rule.last("one") == (want_one, 1) and rule.subpix[-1][3] == 24
    assert torch.equal(master, o32) and torch.equal(out, master.to(P.ACT)) and torch.equal(rest, (master - out.float()).to(P.ACT))


@one_pass_builds
@pytest.mark.parametrize("shape,want_one,want_x2", SUBPIX + SUBPIX_X2_ONLY)
def test_subpixel_upsample_by_rule_three_pass_planes(rule, prec, shape, want_one, want_x2):
    """explicit (main, rest) planes of the input and of the summed weights (the per-layer precision plan's samplers)"""
    from asva_amd import ops, precision as P

    n_img, hs, ws, cin, cout = shape
    M = n_img * hs * ws
    w, b, wm = _subpix_operands(*shape)
    pw, pwr = ops.alloc_planes(tuple(wm.shape), dev())
    pw.copy_(wm.to(P.ACT)), pwr.copy_((wm - wm.to(P.ACT).float()).to(P.ACT))
    xf = rndf(M, cin, seed=1)
    px, pxr = ops.alloc_planes(tuple(xf.shape), dev())
    px.copy_(xf.to(P.ACT)), pxr.copy_((xf - xf.to(P.ACT).float()).to(P.ACT))
    o3 = ops.gemm(px, pw, bias=b.repeat(4), mode=ops.CONV3, conv=(n_img, hs, ws, 1, 2), out_f32=True, a_rest=pxr, w_rest=pwr)
    assert rule.last("x2") == (want_x2, 1) and rule.subpix[-1] == (want_x2, cout, True, 24)
    xv, wq = px.double() + pxr.double(), pw.double() + pwr.double()
    e_ref, e_tap = rel_l2(o3, _ups_conv_ref(xv, w, b, n_img, hs, ws)), rel_l2(o3, _tap_exact(xv, wq, b, n_img, hs, ws, cout))
    print(f"ups=2 {shape} [{prec} planes]: rule tile {want_x2} -> {rule.subpix[-1][3]}; vs float64 conv {e_ref:.3e}, vs tap-exact {e_tap:.3e}")
    assert e_ref < TOL_PLANES and e_tap < TOL_F32


@split_build
@pytest.mark.parametrize("shape,want_one,want_x2", SUBPIX + SUBPIX_X2_ONLY)
def test_subpixel_upsample_by_rule_split_precision(rule, prec, shape, want_one, want_x2):
    from asva_amd import ops

    n_img, hs, ws, cin, cout = shape
    M = n_img * hs * ws
    x, xv = act(M, cin, seed=1)
    w, b, wm = _subpix_operands(*shape)
    wp, wq = packed(wm)
    conv = dict(bias=b.repeat(4), mode=ops.CONV3, conv=(n_img, hs, ws, 1, 2))
    o32 = ops.gemm(x, wp, out_f32=True, **conv)
    assert rule.last("x2") == (want_x2, 1) and rule.subpix[-1] == (want_x2, cout, True, 24)
    ref, tap = _ups_conv_ref(xv, w, b, n_img, hs, ws), _tap_exact(xv, wq, b, n_img, hs, ws, cout)
    o16 = ops.gemm(x, wp, **conv)
    assert o16.shape == (4 * M, cout) and rule.subpix[-1][3] == 24
    errs = rel_l2(o32, tap), rel_l2(ops.from_act(o16), tap), rel_l2(ops.from_act(o16), ref)
    print(f"ups=2 {shape} [split]: rule tile {want_x2} -> 24; f32 vs tap-exact {errs[0]:.3e}, two planes vs tap-exact {errs[1]:.3e}, vs float64 conv {errs[2]:.3e}")
    assert errs[0] < TOL_X2_32 and errs[1] < TOL_X2_16 and errs[2] < TOL_X2_16      # (the last: summed weights rounded to 2^-17)
    assert rel_l2(o16, ref) > 5e-4                                                   # ... and the main plane alone would not do


# ---- b. one launch per branch of each rule, for the other A loaders ------------------------------------------------------------------
# (M, N, K) -> (tile, split_k) by _heuristic_tile, by _heuristic_tile_x2: between them every `return` of either rule
PLAIN_POINTS = [
    ((14336, 512, 1024), (20, 1), (11, 1)), ((14336, 512, 256), (14, 1), (11, 1)), ((7168, 512, 512), (30, 1), (11, 1)),
    ((7168, 512, 256), (11, 1), (11, 1)), ((5760, 320, 1024), (24, 1), (24, 1)), ((5760, 320, 256), (12, 1), (24, 1)),
    ((3584, 320, 512), (25, 1), (25, 1)), ((1280, 320, 256), (13, 1), (13, 1)), ((1280, 320, 512), (25, 2), (25, 2)),
    ((256, 320, 4096), (25, 8), (25, 8)), ((14336, 320, 512), (12, 1), (34, 1)),
]


def _want(rule, prec, one, x2):
    return ("x2", x2) if prec == "bf16x2" else ("one", one)


@pytest.mark.parametrize("mnk,one,x2", PLAIN_POINTS)
def test_plain_bias_residual_by_rule(rule, prec, mnk, one, x2):
    from asva_amd import ops

    which, want = _want(rule, prec, one, x2)
    M, N, K = mnk
    a, av = act(M, K, seed=1)
    w, wv = act(N, K, seed=2, scale=K ** -0.5)
    bias = rndf(N, seed=3)
    res, rv = act(M, N, seed=4)
    ref = av @ wv.T + bias.double() + rv
    out = ops.gemm(a, w, bias=bias, res1=res)
    assert rule.last(which) == want
    o32 = ops.gemm(a, w, bias=bias, res1=res, out_f32=True)
    assert rule.last(which) == want and out.shape == (M, N)
    e16, e32 = rel_l2(ops.from_act(out), ref), rel_l2(o32, ref)
    print(f"PLAIN {mnk} [{prec}]: rule {want}; 16-bit {e16:.3e}, f32 {e32:.3e}")
    assert e16 < tol16(prec) and e32 < tol32(prec)


# two-source A (the UNet's skip concat): k_split on a K-tile boundary, and inside a K tile — there C runs the register-staged tiles in one
# pass (no split-K: splitk_ok is False) and split precision runs two launches, the first leaving its f32 partial for the second
@pytest.mark.parametrize("mnk,k1,one,x2", [
    ((14336, 512, 1024), 512, (20, 1), (11, 1)), ((7168, 512, 512), 256, (30, 1), (11, 1)), ((1280, 320, 512), 256, (25, 2), (25, 2)),
    ((14336, 512, 1024), 488, (20, 1), (11, 1)), ((1280, 320, 512), 232, (25, 1), (13, 1))])
def test_plain_two_source_by_rule(rule, prec, mnk, k1, one, x2):
    from asva_amd import ops

    M, N, K = mnk
    a1, a1v = act(M, k1, seed=1)
    a2, a2v = act(M, K - k1, seed=2)
    w, wv = act(N, K, seed=3, scale=K ** -0.5)
    bias = rndf(N, seed=4)
    ref = torch.cat([a1v, a2v], 1) @ wv.T + bias.double()
    out = ops.gemm(a1, w, a2=a2, bias=bias, out_f32=True)
    if k1 % 64 == 0:
        which, want = _want(rule, prec, one, x2)
        assert rule.last(which) == want and rule.rule[-1][1] == (M, N, K, False, True)
    elif prec == "bf16x2":          # two launches, each placed by the x2 rule on its own K
        assert [r[1][:3] for r in rule.rule] == [(M, N, k1), (M, N, K - k1)] and [r[2] for r in rule.rule] == [x2, x2]
    else:
        assert rule.last("one") == one and rule.rule[-1][1] == (M, N, K, False, False)
    e32 = rel_l2(out, ref)
    print(f"PLAIN two-source {mnk} k_split {k1} [{prec}]: rule {[r[2] for r in rule.rule]}; f32 {e32:.3e}")
    assert e32 < tol32(prec)


@pytest.mark.parametrize("mnk,one,x2", [((14336, 512, 256), (14, 1), (11, 1)), ((7168, 512, 512), (30, 1), (11, 1)), ((1280, 320, 512), (25, 1), (25, 1))])
def test_geglu_by_rule(rule, prec, mnk, one, x2):
    """N counts value and gate columns; the last point would split K were it not a GEGLU product"""
    from asva_amd import ops
    from asva_amd.weights import pack_geglu

    which, want = _want(rule, prec, one, x2)
    M, N, K = mnk
    a, av = act(M, K, seed=1)
    wf, b = rndf(N, K, seed=2, scale=K ** -0.5), rndf(N, seed=3)
    wp, bp = pack_geglu(wf, b)
    _, wv = packed(wf)
    h = av @ wv.T + b.double()
    ref = h[:, :N // 2] * F.gelu(h[:, N // 2:])
    out = ops.gemm(a, wp, bias=bp, geglu=True)
    assert rule.last(which) == want and rule.rule[-1][1][3] is True and out.shape == (M, N // 2)
    e16 = rel_l2(ops.from_act(out), ref)
    print(f"GEGLU {mnk} [{prec}]: rule {want}; 16-bit {e16:.3e}")
    assert e16 < (2 * TOL_X2_16 if prec == "bf16x2" else tol16(prec))          # (split: erf from a 1.5e-7 polynomial, as test_split_gpu.py)


@pytest.mark.parametrize("mnk,one,x2", [((5760, 320, 1024), (24, 1), (24, 1)), ((5760, 320, 256), (12, 1), (24, 1)), ((7168, 512, 512), (30, 1), (11, 1)),
                                        ((256, 320, 4096), (25, 8), (25, 8))])
def test_layernorm_fused_plain_by_rule(rule, prec, mnk, one, x2):
    """Linear(LayerNorm(a)) on the raw a (AVSD_GEMM_LNFUSE): (sum, sumsq) per 32 columns of a, the gain in the weights, their column sums
    carrying the mean; the last point also splits K eight ways.  Reference: float64 on the folded weights the kernel multiplies by."""
    from asva_amd import ops

    which, want = _want(rule, prec, one, x2)
    M, N, K = mnk
    a, av = act(M, K, seed=1, shift=0.5)
    blk = av.reshape(M, K // 32, 32)
    stats = torch.stack([blk.sum(-1), (blk * blk).sum(-1)], -1).float().contiguous()
    g, be = 1.0 + 0.2 * rndf(K, seed=2), 0.3 * rndf(K, seed=3)
    w, b = rndf(N, K, seed=4, scale=K ** -0.5), rndf(N, seed=5)
    wf, wfv = packed(w * g)
    bias2 = (w @ be + b).contiguous()
    out = ops.gemm(a, wf, bias=bias2, ln=(stats, wfv.sum(1).float().contiguous(), 1e-5))
    assert rule.last(which) == want
    norm = (av - av.mean(-1, keepdim=True)) * torch.rsqrt(av.var(-1, unbiased=False, keepdim=True) + 1e-5)
    e16 = rel_l2(ops.from_act(out), norm @ wfv.T + bias2.double())
    print(f"LNFUSE {mnk} [{prec}]: rule {want}; 16-bit {e16:.3e}")
    assert e16 < (TOL_X2_LNFOLD if prec == "bf16x2" else tol16(prec))


# temporal mix (A' = [frame 0 | previous frame | this frame], K = 3 C): C with 3 C next to the K of the PLAIN point on the same side of
# the rule's K thresholds (64 K-tiles-of-64: 16 for the deep rings, 8 for 128 x 128 x 4 and for split-K)
@pytest.mark.parametrize("B,Fr,hw,C,N,one,x2", [
    (56, 4, 64, 344, 512, (20, 1), (11, 1)), (56, 4, 64, 88, 512, (14, 1), (11, 1)), (28, 4, 64, 168, 512, (30, 1), (11, 1)),
    (30, 4, 48, 344, 320, (24, 1), (24, 1)), (5, 4, 64, 168, 320, (25, 2), (25, 2)), (56, 4, 64, 168, 320, (12, 1), (34, 1))])
def test_tmix_by_rule(rule, prec, B, Fr, hw, C, N, one, x2):
    from asva_amd import ops

    which, want = _want(rule, prec, one, x2)
    M = B * Fr * hw
    y, yv = act(M, C, seed=1)
    w, wv = act(N, 3 * C, seed=2, scale=(3 * C) ** -0.5)
    bias = rndf(N, seed=3)
    res, rv = act(M, N, seed=4)
    y4 = yv.reshape(B, Fr, hw, C)
    cat = torch.cat([y4[:, :1].expand_as(y4), torch.cat([y4[:, :1], y4[:, :-1]], 1), y4], -1).reshape(M, 3 * C)
    ref = cat @ wv.T + bias.double() + rv
    out = ops.gemm(y, w, bias=bias, res1=res, mode=ops.TMIX, tmix=(hw, Fr))
    assert rule.last(which) == want and rule.rule[-1][1][:3] == (M, N, 3 * C)
    e16 = rel_l2(ops.from_act(out), ref)
    print(f"TMIX M {M} N {N} K {3 * C} [{prec}]: rule {want}; 16-bit {e16:.3e}")
    assert e16 < tol16(prec)


# 3x3 convolutions, K = 9 cin, M = n_img * ho * wo: stride 1 (tap-major LDS-direct tiles: the table is empty, so no resident tile), stride 2
# and the 9-tap upsample fold (ups = 1); (n_img, output side, cin, cout)
CONV_POINTS = [((56, 16, 112, 512), (20, 1), (11, 1)), ((56, 16, 24, 512), (14, 1), (11, 1)), ((28, 16, 56, 512), (30, 1), (11, 1)),
               ((10, 24, 112, 320), (24, 1), (24, 1)), ((5, 16, 56, 320), (25, 2), (25, 2))]


@pytest.mark.parametrize("stride,ups", [(1, 0), (2, 0), (1, 1)])
@pytest.mark.parametrize("pt,one,x2", CONV_POINTS)
def test_conv3_by_rule(rule, prec, pt, one, x2, stride, ups):
    from asva_amd import ops
    from asva_amd.weights import pack_conv3x3

    which, want = _want(rule, prec, one, x2)
    n_img, so, cin, cout = pt
    hs = ws = so * stride >> ups
    x, xv = act(n_img * hs * ws, cin, seed=1)
    wf = rndf(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5)
    b = rndf(cout, seed=3)
    wp = pack_conv3x3(wf)
    _, wq = packed(wf)
    xi = xv.reshape(n_img, hs, ws, cin).permute(0, 3, 1, 2)
    if ups:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xi, wq, b.double(), stride=stride, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    out = ops.gemm(x, wp, bias=b, mode=ops.CONV3, conv=(n_img, hs, ws, stride, ups))
    assert rule.last(which) == want and rule.rule[-1][1][:3] == (n_img * so * so, cout, 9 * cin) and not rule.subpix
    assert out.shape == ref.shape
    e16 = rel_l2(ops.from_act(out), ref)
    print(f"CONV3 {pt} stride {stride} ups {ups} [{prec}]: rule {want}; 16-bit {e16:.3e}")
    assert e16 < tol16(prec)


# ---- c. the upsampler of a 320-channel block, as the UNet packs and runs it -------------------------------------------------------
def test_upsampler_320_at_large_batch_matches_reference(rule, prec, gold):
    """_Sampler(320) in its sub-pixel form (the UNet packs every upsampler so, precision.SUBPIXEL_UPS) on the up_320 golden's input
    replicated along the batch axis until the convolution's GEMM has >= 5888 rows: clips are independent, so every replica must match the
    same golden output of the reference's module.  With 2 clips (512 rows) the rule ends in its 128 x 64 branch; here it starts from
    256 x 128 (split precision: 128 x 128), whose column tiles do not divide 320."""
    from asva_amd.unet import AudioUNet3DConditionModel as M, _Act, _Sampler

    reps = 12
    root = _pack(_Sampler(320), "blk.up_320.", lambda pr, h: pr.ffconv(h.conv, subpixel=True))
    assert root.p.subpixel
    st = _state(gold, False)
    st.B = gold["B"] * reps
    rows = _rows(gold["in"]["x320"].repeat(reps, 1, 1, 1, 1))
    assert rows.shape[0] == reps * 512 >= 5888
    out = M._ffconv(st, _Act(rows), root.p, (gold["H"], gold["W"]), ups=1)
    which, start = ("x2", 11) if prec == "bf16x2" else ("one", 20)
    assert rule.subpix == [(start, 320, prec == "bf16x2", 24)] and rule.rule[0][0] == which and rule.rule[0][2] == (start, 1)
    ref = gold["up_320"].float()
    got = _video(out.lo, st.B, gold["F"], ref.shape[-2], ref.shape[-1])
    errs = [rel_l2(got[i * gold["B"]:(i + 1) * gold["B"]], ref) for i in range(reps)]
    print(f"up_320 x {reps} [{prec}]: rule tile {start} -> 24; rel-L2 vs reference {min(errs):.3e} .. {max(errs):.3e}")
    assert max(errs) < BLOCK_TOL[prec]["conv"]
