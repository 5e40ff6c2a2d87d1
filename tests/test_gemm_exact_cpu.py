"""tests/gemm_exact.py without a device: every generator configuration tests/test_gemm_exact_gpu.py launches is exact (the float64
reference equals an f32 product in two K orders, every partial sum stays below 2^24 and every value below 2^15 — 512 where row statistics
are taken — and the operands survive bfloat16 and IEEE half), and the comparison fails on one ulp and on one frame element."""
import pytest
import torch

from tests import gemm_exact as G


def test_matrix_covers_every_built_tile():
    t = G.built_tiles()
    one_pass = {row[2] for row in G.matrix("bf16")} | set(t["resident"])
    assert one_pass >= (set(t["one"]) | set(t["asm"]) | set(t["nstream"]) | set(t["subpix"]) | set(t["resident"]))
    assert {row[2] for row in G.matrix("fp16")} == {row[2] for row in G.matrix("bf16")}
    split = {row[2] for row in G.matrix("bf16x2")}
    assert split >= set(t["x2"]) | set(G.ASM_X2) | set(t["subpix_x2"]) and {34, 35, 36} <= split
    assert not {34, 35, 36} & one_pass              # (ids above AVSD_GEMM_MAX_TILE: split precision only)
    # every mode and every epilogue term appears on every LDS-direct tile
    for prec in G.PRECS:
        for tile in G.families(prec)["lds"]:
            seen, epi, outs = set(), set(), set()
            for row in G.matrix(prec):
                if row[2] != tile:
                    continue
                seen.add(row[0])
                for L in G.launches(prec, *row):
                    epi |= set(L.epi) | ({f"res1:{L.r1}"} if "res1" in L.epi else set()) | ({f"res2:{L.r2}"} if "res2" in L.epi else set())
                    outs |= {L.out, L.form} | {k for k in ("master", "out_rest", "rowstats") if getattr(L, k)} | ({"split_k"} if L.split_k > 1 else set())
            assert seen >= {"plain", "two_source", "tmix", "conv", "batched", "nonlinear"}, (prec, tile, seen)
            assert epi >= {"bias", "rowvec", "res1", "res2", "alpha:0.5", "alpha:2", "res1:16", "res1:f32", "res2:16", "res2:f32"}, (prec, tile, epi)
            want = {"16", "f32", "flat", "cols", "rowstats", "split_k"} | ({"master"} if prec != "bf16x2" else set()) | ({"out_rest"} if prec == "fp16" else set())
            assert outs >= want, (prec, tile, outs)


def test_every_generator_configuration_is_exact():
    keys = G.all_problem_keys()
    assert len(keys) > 500
    top_all = 0.0
    for L in keys.values():
        p = L.problem()
        bound, top = G.check_problem(p, small=L.small)
        top_all = max(top_all, top)
        if L.rowstats:
            assert L.small and top <= 512
    assert top_all > 256          # (values beyond 8 significant bits: the 16-bit outputs really are rounded)


def _filled(form, dtype, planes, want, rest):
    f = G.Frame(tuple(want.shape), dtype, form, "cpu", planes=planes)
    assert f.untouched()
    f.view.copy_(want)
    if planes == 2:
        f.rest.copy_(rest)
    return f


@pytest.mark.parametrize("form", G.FORMS)
@pytest.mark.parametrize("dtype,planes", [(torch.bfloat16, 1), (torch.float16, 1), (torch.bfloat16, 2), (torch.float32, 1)])
@pytest.mark.parametrize("shape", [(7, 12), (3, 7, 12)])
def test_frame_check_fails_on_one_ulp_and_on_one_frame_element(form, dtype, planes, shape):
    v = G.ints(shape, -3000, 3000, seed=5) + 0.5
    want = v.float() if dtype == torch.float32 else G.round16(v, dtype)
    rest = G.round16(v - want.double(), dtype) if planes == 2 else None
    _filled(form, dtype, planes, want, rest).check(want, rest)                       # the exact value in an untouched frame passes
    if dtype != torch.float32:
        assert not torch.equal(want.double(), v)                                      # (the cast rounded)
        assert torch.equal(want, v.to(dtype))                                         # round16 is the float64 reference cast to the storage type
    # one element off by one unit in the last place of the storage type
    ulp = want.clone()
    bits = ulp.view(torch.int16 if ulp.element_size() == 2 else torch.int32)
    bits.view(-1)[17] += 1
    assert (ulp != want).sum() == 1
    with pytest.raises(AssertionError, match="differs from the exact value in 1 of"):
        _filled(form, dtype, planes, ulp, rest).check(want, rest)
    if planes == 2:
        r2 = rest.clone()
        r2.view(torch.int16).view(-1)[3] += 1
        with pytest.raises(AssertionError, match="rest plane differs"):
            _filled(form, dtype, planes, want, r2).check(want, rest)
    # one frame element changed: just before the view, just after it, and (column slice) the first element right of a row
    f = _filled(form, dtype, planes, want, rest)
    n = f.buf.shape[1]
    first = f.view.storage_offset()
    last = first + sum((s - 1) * st for s, st in zip(f.view.shape, f.view.stride()))
    spots = [first - 1, last + 1, 0, n - 1] + ([first + shape[-1]] if form == "cols" else [])
    for plane in range(planes):
        for at in spots:
            g = _filled(form, dtype, planes, want, rest)
            g.buf[plane, at] = 1.0
            with pytest.raises(AssertionError, match="1 element\\(s\\) outside"):
                g.check(want, rest)
            g = _filled(form, dtype, planes, want, rest)
            g.buf[plane, at] = 1.0
            with pytest.raises(AssertionError, match="outside"):
                g.check(None)                                                         # the frame-only check of the non-linear epilogues
            assert not g.untouched()


def test_embed_surrounds_operands_with_the_sentinel():
    t = G.ints((5, 24), -3, 3, seed=1)
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for twin in (False, True) if dtype != torch.float32 else (False,):
            e = G.embed(t, dtype, "cpu", twin)
            assert torch.equal(e.double(), t) and e.stride() == (24 + 2 * G.COLS, 1) and e.storage_offset() % 8 == 0
            base = torch.as_strided(e, (e.untyped_storage().nbytes() // e.element_size(),), (1,), 0)
            full = base[:(5 + 2 * G.ROWS) * (24 + 2 * G.COLS)].view(5 + 2 * G.ROWS, 24 + 2 * G.COLS).clone()
            assert float(full.double().sum()) == float(t.sum()) + G.SENTINEL * (full.numel() - t.numel())
            if twin:
                half = base.numel() // 2
                rest = torch.as_strided(e, e.shape, e.stride(), e.storage_offset() + half)
                assert not rest.any() and float(base[half:half + full.numel()].double().sum()) == G.SENTINEL * (full.numel() - t.numel())
    b = G.embed(G.ints((12,), -16, 16, seed=2), torch.float32, "cpu")
    assert b.storage_offset() == G.COLS and b.numel() == 12
    e3 = G.embed(G.ints((3, 5, 8), -3, 3, seed=3), torch.bfloat16, "cpu")
    assert e3.shape == (3, 5, 8) and e3.stride() == ((5 + 2 * G.ROWS) * (8 + 2 * G.COLS), 8 + 2 * G.COLS, 1)
    # what a load outside the slice does to a product, and what a zero-filled operand does not
    assert G.SENTINEL * 1 >= 4096 and G.SENTINEL * 0 == 0
