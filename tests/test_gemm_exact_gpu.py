"""avsd_gemm_bf16's store paths, exactly (-m gpu): every tile the library builds, every A-operand mode and every linear epilogue term on
small-integer operands whose product is exact in f32 — outputs are compared with torch.equal against the float64 statement of the operation
(16-bit outputs: its round-to-nearest-even), and every tensor a launch writes is a view inside a pattern-filled buffer that is compared bit
for bit afterwards (tests/gemm_exact.py, whose generator and comparison tests/test_gemm_exact_cpu.py checks without a device).

The matrix (gemm_exact.matrix / plan_*): shapes M in {7, BM + 1}, N in {4, BN + 4} ({32, BN + 32} for row statistics, GEGLU and tile 70; one
N = BN + 8 whose leading dimension admits the 16-byte store form), K from one vector to a wrapped LDS ring, in bf16, in the IEEE-half
library and in split precision.  GELU, GEGLU and the LayerNorm fold get the frame check only.  A (tile, mode, precision) combination the
library refuses is asserted refused (test_refused_*), never skipped.
"""
import pytest
import torch

from tests import gemm_exact as G
from tests.test_blocks_gpu import prec  # noqa: F401  (fixture: switches the storage precision, restores bf16)

pytestmark = pytest.mark.gpu

F32 = torch.float32
CASES = [(p,) + row for p in G.PRECS for row in G.matrix(p)]
_DEV = {}


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def ops(prec):  # noqa: F811
    from asva_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module", autouse=True)
def _drop_device_operands():
    yield
    _DEV.clear()


def operands(prec, L):
    """the problem's operands on the device in the active storage type, each a slice of a SENTINEL-filled buffer; shared by every launch
    that reads the same problem (they are never written)"""
    from asva_amd import precision as P

    key = (L.key, prec, L.r1, L.r2)
    if key not in _DEV:
        p, twin = L.problem(), prec == "bf16x2"
        res = lambda t, kind: G.embed(t, F32 if kind == "f32" else P.ACT, dev(), twin and kind != "f32")      # noqa: E731
        _DEV[key] = dict(a=G.embed(p.a, P.ACT, dev(), twin), a2=G.embed(p.a2, P.ACT, dev(), twin), w=G.embed(p.w, P.ACT, dev(), twin),
                         bias=G.embed(p.bias, F32, dev()), rowvec=G.embed(p.rowvec, F32, dev()), res1=res(p.res1, L.r1), res2=res(p.res2, L.r2))
    return _DEV[key]


def gemm_kwargs(ops, L, p, o):
    kw = dict(a2=o["a2"], bias=o["bias"], rowvec=o["rowvec"], rows_per_vec=p.rows_per_vec, res1=o["res1"], res2=o["res2"], alpha=p.alpha,
              tile=L.tile, split_k=L.split_k, mode=(ops.PLAIN, ops.TMIX, ops.CONV3)[p.mode], **p.kw)
    if L.tile == ops.NSTREAM_TILE:
        from asva_amd.weights import pack_frag

        kw["w_frag"] = pack_frag(o["w"].contiguous())
    return kw


def frames(prec, L, shape):
    """(out, master, rowstats) frames of a launch; the master takes the other frame form than the output"""
    from asva_amd import precision as P

    f32 = L.out == "f32"
    out = G.Frame(shape, F32 if f32 else P.ACT, L.form, dev(), planes=2 if not f32 and (prec == "bf16x2" or L.out_rest) else 1)
    master = G.Frame(shape, F32, G.FORMS[1 - G.FORMS.index(L.form)], dev()) if L.master else None
    stats = G.Frame((shape[0], shape[1] // 32, 2), F32, "flat", dev()) if L.rowstats else None
    return out, master, stats


def run_linear(ops, prec, L):
    from asva_amd import precision as P

    p, o = L.problem(), operands(prec, L)
    out, master, stats = frames(prec, L, tuple(p.ref.shape))
    what = f"[{prec}] {L!r}"
    if L.build == "batched":
        got = ops.gemm_batched(o["a"], o["w"], alpha=p.alpha, out_f32=L.out == "f32", bias=o["bias"], tile=L.tile, out=out.view)
    else:
        got = ops.gemm(o["a"], o["w"], out=out.view, out_f32=L.out == "f32", master=None if master is None else master.view,
                       out_rest=out.rest if L.out_rest else None, rowstats=None if stats is None else stats.view, **gemm_kwargs(ops, L, p, o))
    assert got.data_ptr() == out.view.data_ptr()
    v = p.ref
    if L.out == "f32":
        out.check(v.float(), what=what)
    else:
        main = G.round16(v, P.ACT)
        rest = G.round16(v - main.double(), P.ACT) if out.planes == 2 else None
        stored = main.double() + (rest.double() if prec == "bf16x2" else 0.0)
        if prec == "bf16x2":
            assert torch.equal(stored, v), "the problem does not fit the two planes"
            assert torch.equal(ops.from_act(out.view).double().cpu(), v), what
        out.check(main, rest, what=what)
        if stats is not None:
            blk = stored.reshape(v.shape[0], v.shape[1] // 32, 32)
            stats.check(torch.stack([blk.sum(-1), (blk * blk).sum(-1)], -1).float(), what=what + " rowstats")
    if master is not None:
        master.check(v.float(), what=what + " master")


def run_nonlinear(ops, prec, L):
    """GELU / GEGLU / LayerNorm fold (/ both): nothing outside the output view is written; the values stay with the per-kernel tests"""
    from asva_amd.weights import pack_frag, pack_geglu

    p, o = L.problem(), operands(prec, L)
    a, w, bias = o["a"], o["w"], o["bias"]
    kw = dict(tile=L.tile, out_f32=L.out == "f32")
    n_out = p.N
    if L.nonlinear in ("geglu", "geglu_ln"):
        w, bias = pack_geglu(ops.from_act(w).contiguous(), bias)
        kw["geglu"], n_out = True, p.N // 2
    else:
        kw["gelu"] = L.nonlinear == "gelu"
    if L.nonlinear in ("ln", "geglu_ln"):
        blk = ops.from_act(a).reshape(p.M, p.K // 32, 32)
        kw["ln"] = (torch.stack([blk.sum(-1), (blk * blk).sum(-1)], -1).contiguous(), ops.from_act(w).sum(1).contiguous(), 1e-5)
    if L.tile == ops.NSTREAM_TILE:
        kw["w_frag"] = pack_frag(w.contiguous())
    out, _, _ = frames(prec, L, (p.M, n_out))
    ops.gemm(a, w, bias=bias, out=out.view, **kw)
    vals = ops.from_act(out.view) if L.out != "f32" else out.view
    assert bool(torch.isfinite(vals).all()), f"[{prec}] {L!r}"
    out.check(None, what=f"[{prec}] {L!r}")


def run(ops, prec, L):
    """one launch and its checks.  A device fault is not a test failure: nothing more is started on the device in this session."""
    try:
        (run_nonlinear if L.nonlinear else run_linear)(ops, prec, L)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"device fault in [{prec}] {L!r}: {e}", returncode=3)
        raise


@pytest.mark.parametrize("prec,name,fam,tile,bm,bn", CASES, indirect=["prec"], ids=[f"{c[0]}-{c[1]}-{c[3]}" for c in CASES])
def test_exact(ops, prec, name, fam, tile, bm, bn):
    for L in G.launches(prec, name, fam, tile, bm, bn):
        run(ops, prec, L)


def _supported(tile, hs, ws, cin):
    from asva_amd import _lib, ops as _ops

    f = _lib.lib().avsd_gemm_conv3r2d_supported if tile in _ops.CONV3R2D_TILES else _lib.lib().avsd_gemm_conv3r_supported
    return f(tile, hs, ws, cin)


RESIDENT = sorted(G.built_tiles()["resident"].items())


@pytest.mark.parametrize("prec", ["bf16", "fp16"], indirect=True)
@pytest.mark.parametrize("tile,bn", [(t, b[1]) for t, b in RESIDENT])
def test_exact_resident_convolution(ops, prec, tile, bn):
    """LDS-resident 3x3 convolutions on the geometries avsd_gemm_conv3r*_supported admits: one and two sources, channel-chunk split-K, full
    epilogue, row statistics; the other geometries of the matrix are refused at the C ABI with the output untouched"""
    ran = 0
    for L in G.plan_resident(tile, bn, _supported):
        run(ops, prec, L)
        ran += 1
    assert ran >= 8, f"tile {tile}: no geometry of the matrix runs it"
    for n_img, hs, ws in G.IMAGES:
        if _supported(tile, hs, ws, 64):
            continue
        L = G.Launch("conv", dict(n_img=n_img, hs=hs, ws=ws, cin=64, cout=4), tile, "cols")
        p, o = L.problem(), operands(prec, L)
        out, _, _ = frames(prec, L, tuple(p.ref.shape))
        with pytest.raises(RuntimeError, match="gemm/conv3r"):
            ops.gemm(o["a"], o["w"], out=out.view, **gemm_kwargs(ops, L, p, o))
        assert out.untouched()


def _refused(ops, prec, L, exc, match):
    """the launch raises and writes nothing"""
    p, o = L.problem(), operands(prec, L)
    out, master, stats = frames(prec, L, tuple(p.ref.shape))
    with pytest.raises(exc, match=match):
        ops.gemm(o["a"], o["w"], out=out.view, out_f32=L.out == "f32", master=None if master is None else master.view,
                 out_rest=out.rest if L.out_rest else None, **gemm_kwargs(ops, L, p, o))
    torch.cuda.synchronize()
    assert out.untouched() and (master is None or master.untouched()), f"[{prec}] {L!r}: a refused launch wrote"


@pytest.mark.parametrize("prec", ["bf16", "fp16"], indirect=True)
def test_refused_one_pass(ops, prec):
    """what the one-pass libraries refuse of the matrix: the rest-plane store in the bfloat16 build (outside ups = 2) and on the tiles that
    have none, TMIX / two sources / K tails on the hand-scheduled tiles, ups = 2 outside its loader's tiles, tile 70 without its operands"""
    plain = dict(M=7, N=4, K=64)
    if prec == "bf16":
        for tile in sorted(G.families(prec)["lds"]) + sorted(G.ASM_BLOCK):
            _refused(ops, prec, G.Launch("plain", plain, tile, "cols", **G.REST_RECIPE), RuntimeError, "OUT_REST is compiled into the IEEE-half build only")
    else:
        _refused(ops, prec, G.Launch("plain", dict(M=7, N=32, K=320), 70, "cols", **G.REST_RECIPE), RuntimeError, "OUT_REST is for one-pass 16-bit outputs")
    for tile in G.ASM_BLOCK:
        _refused(ops, prec, G.Launch("plain", dict(M=7, N=4, K=72), tile, "cols"), RuntimeError, "asm tiles")
        _refused(ops, prec, G.Launch("plain", dict(M=7, N=4, K=128, k1=64), tile, "cols"), RuntimeError, "asm tiles")
        _refused(ops, prec, G.Launch("tmix", dict(B=1, Fr=7, hw=1, C=8, N=4), tile, "cols"), RuntimeError, "asm tiles")
    _refused(ops, prec, G.Launch("tmix", dict(B=1, Fr=7, hw=1, C=64, N=4), 60, "cols"), RuntimeError, "no TMIX form")
    _refused(ops, prec, G.Launch("plain", dict(M=7, N=32, K=64), 70, "cols"), ValueError, "tile 70 needs")
    _refused(ops, prec, G.Launch("plain", dict(M=7, N=32, K=320), 70, "cols", split_k=2), ValueError, "tile 70 needs")
    subpix = G.built_tiles()["subpix"]
    for tile in sorted(set(G.families(prec)["lds"]) - set(subpix)) + [1, 63, 40]:
        _refused(ops, prec, G.Launch("conv", dict(n_img=1, hs=3, ws=5, cin=64, cout=64, ups=2), tile, "cols"), RuntimeError, "ups = 2 runs on")
    for tile in (t for t, (_, bn) in subpix.items() if bn > 64):
        _refused(ops, prec, G.Launch("conv", dict(n_img=1, hs=3, ws=5, cin=64, cout=64, ups=2), tile, "cols"), RuntimeError, "whole column tiles per output-pixel parity")
    for tile in (1, 2, 3):
        _refused(ops, prec, G.Launch("plain", dict(M=7, N=4, K=200), tile, "cols", out="f32", split_k=2), RuntimeError, "split_k needs an LDS-direct tile")


@pytest.mark.parametrize("prec", ["bf16x2"], indirect=True)
def test_refused_split_precision(ops, prec):
    """what split precision refuses of the matrix: the one-pass tiles outside dispatch_tile_x2, the hand-scheduled tiles without a
    three-pass form, the N-streaming and resident tiles, an f32 master and an explicit rest plane (the planes are the output)"""
    t = G.built_tiles()
    plain = dict(M=7, N=4, K=64)
    for tile in sorted(set(t["one"]) - set(t["x2"])):
        _refused(ops, prec, G.Launch("plain", plain, tile, "cols"), RuntimeError, "AVSD_GEMM_X2 runs on tiles")
        _refused(ops, prec, G.Launch("tmix", dict(B=1, Fr=7, hw=1, C=8, N=4), tile, "cols"), RuntimeError, "AVSD_GEMM_X2 runs on tiles")
        _refused(ops, prec, G.Launch("conv", dict(n_img=1, hs=3, ws=5, cin=8, cout=4), tile, "cols"), RuntimeError, "AVSD_GEMM_X2 runs on tiles")
    for tile in sorted(set(G.ASM_BLOCK) - set(G.ASM_X2)):
        _refused(ops, prec, G.Launch("plain", plain, tile, "cols"), RuntimeError, "no split-precision form")
    _refused(ops, prec, G.Launch("plain", dict(M=7, N=32, K=320), 70, "cols"), ValueError, "tile 70 needs")
    for tile, _ in RESIDENT:
        _refused(ops, prec, G.Launch("conv", dict(n_img=2, hs=4, ws=4, cin=64, cout=4), tile, "cols"), RuntimeError, "gemm/conv3r")
    _refused(ops, prec, G.Launch("plain", plain, 11, "cols", master=True), ValueError, "no f32 master")
    L = G.Launch("plain", plain, 11, "cols")
    p, o = L.problem(), operands(prec, L)
    out, _, _ = frames(prec, L, (7, 4))
    with pytest.raises(ValueError, match="out_rest goes with"):
        ops.gemm(o["a"], o["w"], out=out.view, out_rest=out.rest, tile=11)
    assert out.untouched()
