"""The AVSync classifier on a matrix of pairs on the MI355X (csrc/avsync_pairs.hip, asva_amd/avsync.py), in both builds of the library.

Bounds (none comes from what the kernels give):
  * exact integers: embeddings, W1 (16 non-zeros per row), W2 and w3 in {-1, 0, 1}, integer biases in [-16, 16] -> |h1| <= 32,
    |h2| <= 32 * 512 + 16, |s| <= 16400 * 256 + 16 < 4.3e6 < 2^24: every partial sum in any order is an exact f32 integer, so the
    scores EQUAL the float64 result;
  * real inputs: three products in series on v_mfma_f32_32x32x2_f32, inside the 1e-5 (1 + |s|) that tests/test_avsync_gpu.py derives
    for the whole classifier (about twenty products); the materialised route lies within the same bound, so the two routes lie within
    2e-5 (1 + |s|) of each other;
  * cross-entropy moves at most twice the largest logit error: trainer losses within 2e-5 (1 + max |s|) / tau; the line losses of
    avsd_pair_xent_f32 on GIVEN scores within 1e-5 (1 + |loss|) (f32 exp / log and a fixed-tree f32 sum of at most 64 terms);
  * an argmax is compared only where the float64 top-2 margin exceeds 4e-5 (1 + max |s|), twice the distance two f32 routes can lie
    apart; the margin is asserted, not skipped on.
Measured on MI355X: tests/golden/avsync_pairs_measured.json.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import avsync_pairs_ref as PR
from tests import avsync_ref as R
from tests import gemm_exact as GX
from tests.helpers import ROOT, load_golden, load_shapes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEASURED = {}


@pytest.fixture(params=["bf16", "fp16"])
def build(request):
    """the library the test runs in; only a library that is not built may skip"""
    from asva_amd import _lib, precision

    if not os.path.isfile(_lib.LIB_PATHS[request.param]):
        pytest.skip(f"the {request.param} library is not built")
    precision.set_precision(request.param)
    yield request.param
    precision.set_precision("bf16")


def _in_build(name, fn):
    from asva_amd import precision

    precision.set_precision(name)
    try:
        return fn()
    finally:
        precision.set_precision("bf16")


def _both_built():
    from asva_amd import _lib

    if not all(os.path.isfile(p) for p in _lib.LIB_PATHS.values()):
        pytest.skip("needs both the bf16 and the fp16 library")


def _record(key, value):
    """keeps the largest figure per key; written out at the end of the module when $AVSD_PAIRS_MEASURED names a file"""
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _write_measured():
    yield
    path = os.environ.get("AVSD_PAIRS_MEASURED")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump({"gpu": {k: MEASURED[k] for k in sorted(MEASURED)}}, f, indent=1)
            f.write("\n")


@functools.lru_cache(maxsize=None)
def _dev_head(kind, dim, seed):
    """(state dict, packed head on the device) of an FCHead(dim): kind "int" exact-integer weights, "real" seeded N(0, 1 / fan_in)"""
    from asva_amd import avsync as A

    sd = PR.integer_head(dim, seed) if kind == "int" else PR.draw_head(dim, seed)
    head = A.FCHead(dim=dim).eval()
    head.load_state_dict(sd)
    pk = A.fold_head(head)
    for layer in pk:
        layer.w, layer.bias = layer.w.to(DEV), layer.bias.to(DEV)
    return sd, pk


@functools.lru_cache(maxsize=None)
def _int_problem(shape):
    G, P, Q = shape
    sd, _ = _dev_head("int", 512, 3)
    a, v = PR.integer_embeddings(G, P, Q, 512, 100 + G * 10000 + P * 100 + Q)
    want = PR.pair_scores64(sd, a, v)
    assert float(want.abs().max()) < 2 ** 24 and torch.equal(want, want.round()) and float(want.abs().max()) > 0
    return a, v, want


@functools.lru_cache(maxsize=None)
def _real_problem(shape, dim, seed=0):
    G, P, Q = shape
    sd, _ = _dev_head("real", dim, 11 + dim)
    a, v = PR.draw_embeddings(G, P, Q, dim, 5 + seed)
    return a, v, PR.pair_scores64(sd, a, v)


def _fused(pk, a, v, out=None):
    """the three launches of run_pair_head, with the scores written into `out` when given"""
    from asva_amd import avsync as A, ops

    G, P, D = a.shape
    Q = v.shape[1]
    assert ops.pair_head_supported(D, pk[0].cout, pk[1].cout)
    u = A._Hip.half(a.reshape(G * P, D), pk[0], 0, None).view(G, P, -1)
    vh = A._Hip.half(v.reshape(G * Q, D), pk[0], D, pk[0].bias).view(G, Q, -1)
    return ops.pair_head_f32(u, vh, pk[1].w, pk[1].bias, pk[2].w, pk[2].bias, out=out)


# ---- avsd_pair_head_f32: exact integers in a framed buffer ----------------------------------------------------------------------------------
EXACT_SHAPES = [(1, 1, 1), (2, 3, 3), (1, 1, 31), (1, 31, 1), (3, 5, 7), (2, 33, 33)]


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=["x".join(map(str, s)) for s in EXACT_SHAPES])
def test_pair_head_exact_integers_in_a_frame(build, shape):
    from asva_amd import avsync as A

    a, v, want = _int_problem(shape)
    _, pk = _dev_head("int", 512, 3)
    frame = GX.Frame(shape, torch.float32, "flat", DEV)
    out = _fused(pk, a.to(DEV), v.to(DEV), out=frame.view)
    assert out.data_ptr() == frame.view.data_ptr()
    frame.check(want.float(), what=f"pair_head_f32 {shape} [{build}]")            # equality, and nothing outside G P Q floats written
    assert torch.equal(A.run_pair_head(pk, a.to(DEV), v.to(DEV)).cpu().double(), want)
    if shape[1] == shape[2] and shape[1] > 1:
        assert not torch.equal(want, want.transpose(1, 2))                         # the problem can tell p from q


# ---- against float64, and against the materialised route ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    g = load_golden("avsync_tiny.pt")
    sd = R.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), g["seed"])
    R.check_draw(sd, g["probe"])
    g["sd"] = sd
    return g


@pytest.fixture(scope="module")
def net(fixture):
    from asva_amd import avsync as A

    m = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()
    m.load_state_dict(fixture["sd"])
    return m.to(DEV)


def _within(got, want, rel):
    got, want = got.double().cpu(), want.double().cpu()
    err = ((got - want).abs() / (1.0 + want.abs())).max().item()
    assert err <= rel, (err, rel)
    return err


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 33), (2, 1, 31), (2, 31, 1)], ids=["3x5x7", "2x33x33", "2x1x31", "2x31x1"])
def test_pair_scores_against_float64_and_score_embeddings(build, net, fixture, shape):
    G, P, Q = shape
    sd = R._sub(fixture["sd"], "head.")
    a, v = PR.draw_embeddings(G, P, Q, 512, 9)
    want = PR.pair_scores64(sd, a, v)
    ad, vd = a.to(DEV), v.to(DEV)
    got = net.pair_scores(ad, vd)
    assert got.shape == (G, P, Q) and got.dtype == torch.float32 and got.is_contiguous()
    e64 = _within(got, want, 1e-5)
    rows_a = ad[:, :, None, :].expand(G, P, Q, 512).reshape(-1, 512).contiguous()
    rows_v = vd[:, None, :, :].expand(G, P, Q, 512).reshape(-1, 512).contiguous()
    mat = net.score_embeddings(rows_a, rows_v).view(G, P, Q)
    emat = _within(got, mat, 2e-5)
    print(f"pair_scores {shape} [{build}]: vs float64 {e64:.3e} (bound 1e-5), vs score_embeddings on materialised pairs {emat:.3e} (bound 2e-5)")
    _record("pair_scores_vs_float64_rel", e64)
    _record("pair_scores_vs_score_embeddings_rel", emat)
    if P == Q:
        assert ((got.double().cpu().transpose(1, 2) - want).abs() / (1.0 + want.abs())).max().item() > 1e-3       # a transposed matrix fails


@pytest.mark.parametrize("dim", [64, 192, 48], ids=["dim64_kernel", "dim192_kernel", "dim48_fallback"])
def test_other_head_sizes(build, dim, monkeypatch):
    """dim 64 (H2 = 32: one fragment, one wave busy) and dim 192 (H2 = 96: three of four waves) through the kernel, dim 48 through the
    materialised fallback; the route is asserted by counting pair_head_f32 launches"""
    from asva_amd import avsync as A, ops

    shape = (3, 5, 7)
    a, v, want = _real_problem(shape, dim)
    _, pk = _dev_head("real", dim, 11 + dim)
    calls = []
    real = ops.pair_head_f32
    monkeypatch.setattr(ops, "pair_head_f32", lambda *args, **kw: calls.append(1) or real(*args, **kw))
    got = A.run_pair_head(pk, a.to(DEV), v.to(DEV))
    assert len(calls) == (0 if dim == 48 else 1)
    e = _within(got, want, 1e-5)
    print(f"pair_scores dim {dim} {shape} [{build}]: vs float64 {e:.3e}")
    _record(f"pair_scores_dim{dim}_vs_float64_rel", e)


def test_pair_head_refuses_bad_arguments(build):
    from asva_amd import _lib, ops

    _, pk = _dev_head("real", 64, 75)
    u, vh = torch.zeros(2, 3, 64, device=DEV), torch.zeros(2, 4, 64, device=DEV)
    good = ops.pair_head_f32(u, vh, pk[1].w, pk[1].bias, pk[2].w, pk[2].bias)
    assert good.shape == (2, 3, 4)
    with pytest.raises(ValueError):
        ops.pair_head_f32(u, vh[:1], pk[1].w, pk[1].bias, pk[2].w, pk[2].bias)                    # G differs
    with pytest.raises(ValueError):
        ops.pair_head_f32(u, vh, pk[1].w, pk[1].bias, pk[2].w, pk[2].bias, out=torch.zeros(2, 4, 3, device=DEV))
    with pytest.raises(_lib.AvsdError, match="H1"):
        ops.pair_head_f32(u[:, :, :48].contiguous(), vh[:, :, :48].contiguous(), pk[1].w, pk[1].bias, pk[2].w, pk[2].bias)
    w2 = torch.zeros(48, 64, device=DEV)
    with pytest.raises(_lib.AvsdError, match="H2"):
        ops.pair_head_f32(u, vh, w2, None, torch.zeros(1, 48, device=DEV), None)
    with pytest.raises(_lib.AvsdError, match="H2"):
        ops.pair_head_f32(u, vh, torch.zeros(288, 64, device=DEV), None, torch.zeros(1, 288, device=DEV), None)
    with pytest.raises(ValueError):
        ops.convnd_f32(u.view(6, 1, 1, 1, 64), pk[0].w, (1, 1, 1), (1, 1, 1), (0, 0, 0), w_col=96)      # columns 96 .. 160 of 128


# ---- invariance ------------------------------------------------------------------------------------------------------------------------------------
def _single_pairs(pk, ad, vd, picks):
    return torch.stack([_fused(pk, ad[g:g + 1, p:p + 1].contiguous(), vd[g:g + 1, q:q + 1].contiguous())[0, 0, 0] for g, p, q in picks])


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 33)], ids=["3x5x7", "2x33x33"])
def test_a_score_is_a_function_of_its_pair(build, shape):
    """bit for bit the (1, 1, 1) call on that pair, whatever (G, P, Q) and wherever the pair sits in a 32-row tile; two calls agree"""
    G, P, Q = shape
    a, v, _ = _real_problem(shape, 512, seed=3)
    _, pk = _dev_head("real", 512, 11 + 512)
    ad, vd = a.to(DEV), v.to(DEV)
    full = _fused(pk, ad, vd)
    assert torch.equal(full, _fused(pk, ad, vd))
    if G * P * Q <= 128:
        picks = [(g, p, q) for g in range(G) for p in range(P) for q in range(Q)]
    else:       # rows 0, 31, 32 of the tiles around the group boundary (pair 1089 = tile 34, row 1) and the corners
        flat = sorted({0, 1, 31, 32, 33, 63, 64, 1055, 1056, 1087, 1088, 1089, 1090, 1119, 1120, 2143, 2144, 2175, 2176, 2177, P * Q - 1, 17 * Q + 5})
        picks = [(m // (P * Q), (m % (P * Q)) // Q, m % Q) for m in flat]
    singles = _single_pairs(pk, ad, vd, picks)
    want = torch.stack([full[g, p, q] for g, p, q in picks])
    assert torch.equal(singles, want), (singles - want).abs().max()
    # the same pair inside another problem: group 0 alone, and one row against all columns
    assert torch.equal(_fused(pk, ad[:1].contiguous(), vd[:1].contiguous()), full[:1])
    assert torch.equal(_fused(pk, ad[:, 1:2].contiguous(), vd), full[:, 1:2])
    assert torch.equal(_fused(pk, ad, vd[:, Q - 1:].contiguous()), full[:, :, Q - 1:])


def test_both_builds_agree_bit_for_bit(net):
    from asva_amd import ops

    _both_built()
    a, v, _ = _real_problem((3, 5, 7), 512, seed=3)
    ad, vd = a.to(DEV), v.to(DEV)
    s = torch.randn(2, 31, 31, generator=torch.Generator().manual_seed(1)).to(DEV)

    def run():
        x = ops.pair_xent_f32(s, 0.07)
        return [net.pair_scores(ad, vd).clone()] + [x[k].clone() for k in sorted(x)]

    for x, y in zip(_in_build("bf16", run), _in_build("fp16", run)):
        assert torch.equal(x, y)


# ---- avsd_pair_xent_f32 --------------------------------------------------------------------------------------------------------------------------------
XENT_SHAPES = [(1, 1, 1), (2, 3, 3), (8, 31, 31), (1, 64, 64)]


def _check_xent(r, scores, tau, tag):
    row, col, ram, cam = PR.line_losses64(scores, tau)
    G, P, Q = scores.shape
    worst = 0.0
    for name, want in (("row_loss", row), ("col_loss", col)):
        if want is None:
            assert name not in r
            continue
        got = r[name].double().cpu()
        assert bool(torch.isfinite(got).all())
        err = ((got - want).abs() / (1.0 + want.abs())).max().item()
        assert err <= 1e-5, (tag, name, err)
        worst = max(worst, err)
    assert r["row_argmax"].dtype == torch.int32 and torch.equal(r["row_argmax"].cpu().long(), ram)
    assert torch.equal(r["col_argmax"].cpu().long(), cam)
    if P == Q:
        want = PR.contrastive64(scores, tau)
        for k, w in zip(("av_loss", "va_loss", "av_acc", "va_acc"), want):
            assert r[k].dim() == 0 and r[k].dtype == torch.float32
            err = abs(float(r[k]) - float(w)) / (1.0 + abs(float(w)))
            assert err <= 1e-5, (tag, k, float(r[k]), float(w))
            worst = max(worst, err)
    return worst


@pytest.mark.parametrize("tau", [1.0, 0.07])
@pytest.mark.parametrize("shape", XENT_SHAPES, ids=["x".join(map(str, s)) for s in XENT_SHAPES])
def test_pair_xent_against_float64(build, shape, tau):
    from asva_amd import ops

    g = torch.Generator().manual_seed(shape[0] * 1000 + shape[1])
    scores = torch.randn(shape, generator=g) * 0.7 - 0.3
    assert PR.top2_margin(scores) > 0 and PR.top2_margin(scores.transpose(1, 2)) > 0         # f32 inputs: an argmax is exact
    r = ops.pair_xent_f32(scores.to(DEV), tau)
    worst = _check_xent(r, scores, tau, (shape, tau))
    print(f"pair_xent_f32 {shape} tau {tau} [{build}]: max |d| / (1 + |loss|) {worst:.3e}")
    _record("pair_xent_loss_rel", worst)
    if shape == (1, 1, 1):
        assert float(r["row_loss"]) == 0.0 and float(r["col_loss"]) == 0.0 and float(r["av_loss"]) == 0.0 and float(r["av_acc"]) == 1.0
    again = ops.pair_xent_f32(scores.to(DEV), tau)
    assert all(torch.equal(r[k], again[k]) for k in r)
    if shape[0] > 1:                 # an example's lines do not depend on the batch it sits in
        one = ops.pair_xent_f32(scores[1:2].contiguous().to(DEV), tau)
        assert torch.equal(one["row_loss"], r["row_loss"][1:2]) and torch.equal(one["col_argmax"], r["col_argmax"][1:2])


def test_pair_xent_large_scores_ties_and_arguments(build):
    from asva_amd import ops

    s = torch.full((2, 5, 5), -1000.0)
    s[0] += 2000.0 * torch.eye(5)
    s[1, :, 0] = 1000.0
    for tau in (1.0, 0.07):
        r = ops.pair_xent_f32(s.to(DEV), tau)
        worst = _check_xent(r, s, tau, ("large", tau))
        assert all(bool(torch.isfinite(r[k]).all()) for k in ("row_loss", "col_loss", "av_loss", "va_loss"))
        _record("pair_xent_loss_rel", worst)
    # ties go to the lowest index: this kernel's own contract
    t = torch.zeros(2, 4, 70)
    t[0, 1, 5] = t[0, 1, 69] = t[0, 1, 64] = 2.0
    t[1, 2, 3] = t[1, 3, 3] = 1.0
    r = ops.pair_xent_f32(t.to(DEV), 1.0)
    ram, cam = r["row_argmax"].cpu(), r["col_argmax"].cpu()
    assert ram[0].tolist() == [0, 5, 0, 0] and ram[1].tolist() == [0, 0, 3, 3]
    assert cam[0, 5] == 1 and cam[0, 64] == 1 and cam[0, 0] == 0 and cam[1, 3] == 2 and int(cam.sum()) == 1 + 1 + 1 + 2
    with pytest.raises(ValueError):
        ops.pair_xent_f32(s.to(DEV), 0.0)
    with pytest.raises(ValueError):
        ops.pair_xent_f32(s.to(DEV)[:, :, :3], 1.0)


@pytest.mark.parametrize("shape", [(2, 3, 7), (2, 7, 3), (3, 1, 31), (3, 31, 1)], ids=["2x3x7", "2x7x3", "3x1x31", "3x31x1"])
def test_pair_xent_writes_only_what_is_defined(build, shape):
    """P != Q: the argmax arrays and the loss whose labels exist; the other loss and the means stay untouched (pattern-filled buffers)"""
    from asva_amd import _lib, ops

    G, P, Q = shape
    scores = torch.randn(shape, generator=torch.Generator().manual_seed(2))
    sd = scores.to(DEV)
    n = G * max(P, Q) + 64
    bufs = {k: torch.empty(n, dtype=torch.int32, device=DEV).fill_(GX.PAT32) for k in ("row_loss", "col_loss", "row_argmax", "col_argmax", "means")}
    ops.check(_lib.lib().avsd_pair_xent_f32(sd.data_ptr(), 1.0, bufs["row_loss"].data_ptr(), bufs["col_loss"].data_ptr(), bufs["row_argmax"].data_ptr(),
                                            bufs["col_argmax"].data_ptr(), bufs["means"].data_ptr(), G, P, Q, torch.cuda.current_stream().cuda_stream),
              "avsd_pair_xent_f32")
    row, col, ram, cam = PR.line_losses64(scores, 1.0)
    written = {"row_argmax": G * P, "col_argmax": G * Q, "row_loss": G * P if P <= Q else 0, "col_loss": G * Q if Q <= P else 0, "means": 0}
    for k, cnt in written.items():
        assert bool((bufs[k][cnt:] == GX.PAT32).all()), k
    assert torch.equal(bufs["row_argmax"][:G * P].cpu().long().view(G, P), ram) and torch.equal(bufs["col_argmax"][:G * Q].cpu().long().view(G, Q), cam)
    for k, want in (("row_loss", row), ("col_loss", col)):
        if want is not None:
            got = bufs[k][:want.numel()].view(torch.float32).cpu().double().view(want.shape)
            assert ((got - want).abs() / (1.0 + want.abs())).max().item() <= 1e-5
    r = ops.pair_xent_f32(sd, 1.0)
    assert ("row_loss" in r) == (P <= Q) and ("col_loss" in r) == (Q <= P) and "av_loss" not in r


# ---- end to end on the tiny fixture ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_reference():
    g = load_golden("avsync_tiny.pt")
    sd = R.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), g["seed"])
    audios, videos = PR.tiny_clips(g["audio"])
    a64, v64 = PR.tiny_reference(sd, audios, videos)
    return audios, videos, a64, v64, PR.pair_scores64(R._sub(sd, "head."), a64, v64)


@pytest.mark.parametrize("tau", [1.0, 0.07])
def test_trainer_end_to_end(build, net, tau):
    from asva_amd import avsync as A

    audios, videos, a64, v64, s64 = _tiny_reference()
    top = float(s64.abs().max())
    trainer = A.AVSyncContrastiveTrainer(net.audio_encoder, net.video_encoder, net.head, tau=tau)
    got = trainer(audios.to(DEV), videos.to(DEV))
    assert all(t.dim() == 0 and t.dtype == torch.float32 and t.is_cuda and not t.requires_grad for t in got)
    want = PR.contrastive64(s64, tau)
    bound = 2e-5 * (1.0 + top) / tau
    errs = [abs(float(got[i]) - float(want[i])) for i in (0, 1)]
    print(f"trainer tau {tau} [{build}]: |av_loss - ref| {errs[0]:.3e}, |va_loss - ref| {errs[1]:.3e} (bound {bound:.3e}); losses {float(want[0]):.6f} {float(want[1]):.6f}")
    _record(f"trainer_loss_abs_tau{tau}", max(errs))
    assert max(errs) <= bound
    assert abs(float(want[0]) - float(want[1])) > 10 * bound                       # av and va are not interchangeable on these inputs
    margin = min(PR.top2_margin(s64), PR.top2_margin(s64.transpose(1, 2)))
    assert margin > 4e-5 * (1.0 + top), (margin, top)                             # chosen on the CPU; a too-small margin fails here
    assert float(got[2]) == float(want[2].float()) and float(got[3]) == float(want[3].float())


def test_shift_accuracy_end_to_end(build, net, fixture):
    from asva_amd import avsync as A

    audios, videos, a64, v64, _ = _tiny_reference()
    want = PR.shift_eval64(R._sub(fixture["sd"], "head."), a64, v64, 0)
    top = max(float(want["av_scores"].abs().max()), float(want["va_scores"].abs().max()))
    margin = min(PR.top2_margin(want["av_scores"]), PR.top2_margin(want["va_scores"]))
    assert margin > 4e-5 * (1.0 + top), (margin, top)
    got = A.shift_accuracy(net, audios.to(DEV), videos.to(DEV), tolerate_range=0)
    for k in ("av_pred", "va_pred", "av_hit", "va_hit"):
        assert got[k].cpu().tolist() == want[k].tolist(), (k, got[k], want[k])
    assert got["av_pred"].dtype == torch.int64 and got["av_hit"].dtype == torch.bool
    wide = A.shift_accuracy(net, audios.to(DEV), videos.to(DEV), tolerate_range=1)
    assert bool(wide["av_hit"].all()) and bool(wide["va_hit"].all())               # k = 3: every prediction lies within 1 of the centre
    r = A.evaluate_shift_accuracy(net, [{"index": torch.tensor([5, 6]), "audio": audios.to(DEV), "video": videos.to(DEV)},
                                        {"index": torch.tensor([6, 5]), "audio": audios.flip(0).to(DEV), "video": videos.flip(0).to(DEV)}], tolerate_range=0)
    assert r["valid_examples"] == 2 and r["av_acc"] == float(want["av_hit"].double().mean()) and r["va_acc"] == float(want["va_hit"].double().mean())


# ---- shifted_pairs ---------------------------------------------------------------------------------------------------------------------------------------------
def test_shifted_pairs(build, monkeypatch):
    from asva_amd import avsync as A, ops
    from asva_amd.audio_features import waveform_to_melspectrogram

    fps, sr, k, shift = 24, 16000, 5, 0.04
    frames = R.u8_to_unit(R.grating_video_u8(3 * fps, 60, 72, 0.7, 0.13, 23.0)).permute(1, 0, 2, 3).contiguous()      # (72, 3, 60, 72)
    stamps = np.arange(3 * fps, dtype=np.float64) / fps
    t = torch.arange(3 * sr, dtype=torch.float32) / sr
    wave = (0.3 * torch.sin(2 * torch.pi * 440.0 * t) * (1.0 + torch.sin(2 * torch.pi * 3.0 * t)))[None]
    resizes = []
    real = ops.resize_aa_normalize_f32
    monkeypatch.setattr(ops, "resize_aa_normalize_f32", lambda x, *a, **kw: resizes.append(x.shape[0]) or real(x, *a, **kw))
    counts = {}
    audios, videos = A.shifted_pairs(frames, stamps, wave, sr, num_clips=k, shift_time=shift, counts=counts)
    assert audios.shape == (k, 1, 128, 204) and videos.shape == (k, 3, 12, 224, 224) and audios.is_cuda and videos.is_cuda
    # the clip times in closed form: 3 s recording, 2 s clips, 5 clips 0.04 s apart, centred -> first start (1 - 0.16) / 2 = 0.42
    starts = 0.42 + shift * np.arange(k)
    want_idx = [[int(np.floor((s + (1e-4 if f == 0 else 0.0) + f / 6.0) * fps + 0.5)) for f in range(12)] for s in starts]
    distinct = sorted({i for row in want_idx for i in row})
    assert resizes == [len(distinct)] and counts["frames_resized"] == len(distinct) < k * 12        # one launch, every distinct frame once
    monkeypatch.undo()
    c = k // 2                                                                                           # the clip at shift 0 from the centre
    direct_v = A.preprocess_videos(frames[want_idx[c]].permute(1, 0, 2, 3)[None].to(DEV))[0]
    assert torch.equal(videos[c], direct_v)
    lo, hi = int(round((starts[c] + 1e-4) * sr)), int(round((starts[c] + 2.0 - 1e-4) * sr))
    assert torch.equal(audios[c], waveform_to_melspectrogram(wave[:, lo:hi], device=DEV))
    assert not torch.equal(videos[0], videos[k - 1]) and not torch.equal(audios[0], audios[k - 1])
    with pytest.raises(ValueError, match="too short"):
        A.shifted_pairs(frames, stamps, wave, sr, num_clips=31, shift_time=0.04)                        # 2 + 1.2 s > 3 s


# ---- the tool ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_avsync_eval_tool_runs():
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "avsync_eval.py"), "--synthetic", "2"],
                       capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "mean nothing" in r.stdout and "av_acc" in r.stdout and "va_acc" in r.stdout and "launches" in r.stdout


# ---- the file source, and the tool on files -----------------------------------------------------------------------------------------------------------------------
def test_avi_source_and_tool_on_files(build, tmp_path):
    """two short recordings written with the project's own Motion-JPEG writer: `shifted_pairs_from_avi` equals `shifted_pairs` on the
    decoded frames and audio bit for bit, and tools/avsync_eval.py runs its --checkpoint / --example_list_path branch on them"""
    from asva_amd import avsync as A
    from asva_amd.video_io import read_mjpeg_avi, write_mjpeg_avi

    fps, sr, k = 24, 16000, 5
    t = torch.arange(3 * sr, dtype=torch.float32) / sr
    for i, name in enumerate(("a.avi", "b.avi")):
        clip = R.grating_video_u8(3 * fps, 64, 72, 0.7 + i, 0.13, 23.0 - 6 * i).permute(1, 2, 3, 0).contiguous()          # (72, 64, 72, 3) uint8
        wave = (0.3 * torch.sin(2 * torch.pi * (440.0 + 200 * i) * t) * (1.0 + torch.sin(2 * torch.pi * 3.0 * t)))[None]
        write_mjpeg_avi(str(tmp_path / name), clip, fps, wave, sr, encoder="host")
    audios, videos = A.shifted_pairs_from_avi(str(tmp_path / "a.avi"), num_clips=k)
    assert audios.shape == (k, 1, 128, 204) and videos.shape == (k, 3, 12, 224, 224)
    video, got_fps, audio, audio_fps = read_mjpeg_avi(str(tmp_path / "a.avi"))
    assert got_fps == fps and audio_fps == sr and video.shape == (3 * fps, 64, 72, 3)
    frames = video.permute(0, 3, 1, 2).float() / 255.0
    a2, v2 = A.shifted_pairs(frames, np.arange(3 * fps, dtype=np.float64) / fps, audio, sr, num_clips=k)
    assert torch.equal(audios, a2) and torch.equal(videos, v2)
    with pytest.raises(ValueError, match="empty"):
        A.shifted_pairs(frames[:0], np.zeros(0), audio, sr, num_clips=k)
    if build != "bf16":
        return                    # the tool picks its own library: one run
    # the tool: a checkpoint folder in the layout load_avsync_model reads, a list of the two files
    A.AVSyncContrastiveTrainer(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).save_pretrained(str(tmp_path / "modules"))
    (tmp_path / "list.txt").write_text("a.avi\nb.avi\n")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "avsync_eval.py"), "--checkpoint", str(tmp_path / "modules"),
                        "--data_root", str(tmp_path), "--example_list_path", str(tmp_path / "list.txt"), "--num_clips", str(k)],
                       capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "valid examples = 2" in r.stdout and "mean nothing" not in r.stdout and "av_acc" in r.stdout
