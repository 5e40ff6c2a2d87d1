"""The device's counter-based normal generator on the MI355X (-m gpu): its Philox words against tests/philox_ref.py bit for bit, its
normals against the float64 construction within a bound derived from the math library's specified accuracy, their moments,
partition independence bit for bit, indices past 2^34, and DeviceGenerator."""
import numpy as np
import pytest
import torch

from tests import philox_ref

pytestmark = pytest.mark.gpu

# Bound on |device - float64| / max(|z|, 2^-10) for one normal z = r * c, r = sqrtf(-2 logf(u)), (s, c) = sincospif(2 v), from the
# accuracy the device's math library is specified to (the OpenCL 3.0 full-profile table its f32 functions are written to meet:
# log <= 3 ulp, sqrt <= 3 ulp, sinpi / cospi <= 4 ulp; a product is correctly rounded, 0.5 ulp), one ulp being at most 2^-23
# relative.  u and v are exact in f32 and 2 v and -2 log u are exact scalings, so nothing else rounds:
#   log:   3 ulp on log u; the square root halves a relative error         -> 1.5 ulp on r
#   sqrt:  3 ulp                                                            -> 4.5 ulp on r
#   sincospi: 4 ulp on c (or s), relative to c itself, also next to its zeros
#   product r * c: 0.5 ulp                                                  -> 9 ulp on z, to first order
# The reference's own float64 error is 1e-15 relative, except next to a zero of cos / sin, where rounding 2 pi v leaves an absolute
# 6e-15 that the floor 2^-10 of the metric turns into 6e-12: 1e-10 covers both and the second-order terms.
NORMAL_BOUND = 9 * 2.0 ** -23 + 1e-10          # 1.073e-6; measured maximum: profiles/stochastic.md


def _metric(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 2.0 ** -10)))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- raw words ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,stream,step,first,n", [(0, 0, 0, 0, 4096 + 3), (2 ** 64 - 1, 0xffffffff, 0xffffffff, 0, 1026),
                                                      (1234, 3, 17, 2 ** 34 - 6, 64), (77, 1, 2, 5, 1)])
def test_philox_words_equal_the_reference(seed, stream, step, first, n):
    """all zeros (whose first block is Random123's known answer), all ones, a word range whose block index crosses 2^32, and a
    single word in the middle of a block"""
    from asva_amd import ops

    got = _u32(ops.philox_u32(n, seed, stream, step, first))
    np.testing.assert_array_equal(got, philox_ref.words(n, seed, stream, step, first))
    if seed == 0:
        assert [f"{int(v):08x}" for v in got[:4]] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]


# ---- normals -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def million():
    """2^20 normals of (seed 1234, stream 0, step 0): the device's f32 and the float64 reference from the same words"""
    from asva_amd import ops

    n = 1 << 20
    return ops.randn_philox(n, 1234).cpu().numpy(), philox_ref.normals(n, 1234)


def test_normals_match_float64_within_the_derived_bound(million):
    """the bound is NORMAL_BOUND above, derived from the specified ulp errors of logf, sqrtf, sincospif and the product"""
    got, want = million
    err = _metric(got, want)
    print(f"randn_philox, n = 2^20: max |delta| / max(|z|, 2^-10) = {err:.3e} = {err / 2.0 ** -23:.2f} ulp; bound {NORMAL_BOUND:.3e}")
    assert got.dtype == np.float32 and np.isfinite(got).all() and np.abs(got).max() <= 5.77
    assert err < NORMAL_BOUND


def test_normals_have_normal_moments(million):
    m = philox_ref.moments(million[0])
    print("device normals, n = 2^20: standardised mean, variance, excess kurtosis, lag-1 correlation", m)
    assert all(abs(v) < 5 for v in m)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 515])
def test_partition_independence_is_bit_exact(k):
    from asva_amd import ops

    whole = ops.randn_philox(1001, 99, 2, 5)
    part = ops.randn_philox(1001 - k, 99, 2, 5, first=k)
    assert torch.equal(whole[k:], part)
    # a destination that is only 4-byte aligned, and a preallocated one of another shape
    buf = torch.full((1001 - k + 1,), 7.0, device="cuda")
    ops.randn_philox(1001 - k, 99, 2, 5, first=k, out=buf[1:])
    assert torch.equal(buf[1:], part) and float(buf[0]) == 7.0


def test_normals_past_2_to_the_34():
    from asva_amd import ops

    first = 2 ** 34 - 6
    got = ops.randn_philox(64, 5, 1, 2, first=first).cpu().numpy()
    assert _metric(got, philox_ref.normals(64, 5, 1, 2, first=first)) < NORMAL_BOUND
    guard = torch.full((64 + 8,), 3.0, device="cuda")
    ops.randn_philox(64, 5, 1, 2, first=first, out=guard[4:68])
    assert np.array_equal(guard[4:68].cpu().numpy(), got) and bool((guard[:4] == 3.0).all()) and bool((guard[68:] == 3.0).all())


def test_device_generator_on_the_device():
    from asva_amd.rng import DeviceGenerator

    g = DeviceGenerator(42)
    a, b = g.normal((2, 3, 5, 7), "cuda"), g.normal((2, 3, 5, 7), "cuda")
    assert a.shape == (2, 3, 5, 7) and a.dtype == torch.float32 and not torch.equal(a, b) and g.streams == 2
    assert torch.equal(DeviceGenerator(42).normal((2, 3, 5, 7), "cuda"), a)
    assert _metric(a.cpu().numpy().reshape(-1), philox_ref.normals(210, 42, 0, 0)) < NORMAL_BOUND
    assert torch.equal(g.normal((2, 3, 5, 7), "cuda", stream=0), a) and g.streams == 2
    with pytest.raises(ValueError):
        from asva_amd import ops

        ops.randn_philox(-1, 1)
