"""The device's counter-based normal generator on CPU (-m "not gpu"): the Philox / Box-Muller reference (tests/philox_ref.py)
against the Random123 known answers and its documented layout, DeviceGenerator's state on an emulated `ops.randn_philox`, and the
argument checks of the two entry points.  The stochastic samplers this generator was written for (DDIM eta > 0, SDE-DPM-Solver++)
are not in the tree yet."""
import math

import numpy as np
import pytest
import torch

from tests import philox_ref


def randn_philox(n, seed, stream=0, step=0, first=0, device="cpu", out=None):
    """ops.randn_philox's contract on the float64 reference, rounded to f32"""
    z = torch.from_numpy(philox_ref.normals(n, seed, stream, step, first).copy()).float()
    return z if out is None else out.copy_(z.reshape(out.shape))


class _RngOps:
    randn_philox = staticmethod(randn_philox)


@pytest.fixture
def emu_rng(monkeypatch):
    import asva_amd.rng as rng

    monkeypatch.setattr(rng, "ops", _RngOps)


# ---- the generator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_reference_gives_the_random123_known_answers(counter, key, want):
    assert " ".join(f"{int(v):08x}" for v in philox_ref.philox4x32_10(counter, key)) == want


def test_reference_layout_and_moments():
    """seed 1234, stream 0, step 0, n = 65536: standardised mean 0.95, variance 0.52, lag-1 correlation -0.52 with exactly this
    layout (key = seed words, counter = (block lo, block hi, step, stream), lanes as documented); the excess kurtosis is -1.13
    when standardised by sqrt(n / 24), its asymptotic deviation.  Each is within 4, and |z| <= 5.77 by construction."""
    z = philox_ref.normals(65536, 1234)
    m = philox_ref.moments(z)
    print("moments", m, "max |z|", np.abs(z).max())
    assert all(abs(v) < 4 for v in m)
    assert [round(float(v), 2) for v in (m[0], m[1], m[3])] == [0.95, 0.52, -0.52]
    assert np.abs(z).max() <= 5.77
    # the layout: words of block b are the counter (b lo, b hi, step, stream) under the key (seed lo, seed hi)
    seed, b = 0x0123456789abcdef, (1 << 32) + 5
    w = philox_ref.philox4x32_10((b & 0xffffffff, b >> 32, 7, 9), (seed & 0xffffffff, seed >> 32))
    np.testing.assert_array_equal(philox_ref.words(4, seed, stream=9, step=7, first=4 * b), np.array(w, dtype=np.uint32).reshape(-1))
    # any partition of a range gives the same items
    np.testing.assert_array_equal(philox_ref.normals(1001, 5)[515:], philox_ref.normals(1001 - 515, 5, first=515))
    # the extreme uniform: word 0 -> u = 2^-24 -> the bound on |z|
    assert math.sqrt(-2.0 * math.log(2.0 ** -24)) <= 5.77


def test_device_generator_state(emu_rng):
    from asva_amd.rng import DeviceGenerator

    g = DeviceGenerator(5)
    a = g.normal((2, 3), "cpu")
    b = g.normal((2, 3), "cpu")
    assert g.streams == 2 and not torch.equal(a, b)
    assert torch.equal(g.normal((2, 3), "cpu", stream=0), a) and g.streams == 2      # a named stream does not advance the count
    assert torch.equal(g.manual_seed(5).normal((2, 3), "cpu"), a) and g.next_stream() == 1
    assert not torch.equal(DeviceGenerator(6).normal((2, 3), "cpu"), a)
    assert a.dtype == torch.float32 and torch.equal(g.normal(6, "cpu", stream=0).reshape(2, 3), a)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            DeviceGenerator(bad)


def test_new_entry_points_report_argument_errors_without_a_device():
    from asva_amd import _lib

    h = _lib.lib()
    assert h.avsd_randn_philox_f32(None, 16, 1, 0, 0, 0, None) == -1 and b"randn_philox_f32" in h.avsd_last_error()
    assert h.avsd_randn_philox_f32(None, -1, 1, 0, 0, 0, None) == -1
    assert h.avsd_philox4x32_u32(None, 4, 1, 0, 0, -4, None) == -1 and b"philox4x32_u32" in h.avsd_last_error()
    assert h.avsd_randn_philox_f32(None, 0, 1, 0, 0, 0, None) == 0                      # nothing to do, nothing launched


def test_recorder_takes_unsigned_arguments():
    """asva_amd/plan.py records a 64-bit seed as the 'i' tag's signed 64 bits; csrc/plan.hip casts them back"""
    import ctypes as C

    from asva_amd import _lib, plan

    args = plan._Proxy._convert("avsd_randn_philox_f32", _lib.SIGNATURES["avsd_randn_philox_f32"][1],
                                (256, 8, 2 ** 64 - 1, 2 ** 32 - 1, 3, 2 ** 34, 0))
    assert args == [("p", 256), ("i", 8), ("i", -1), ("i", 2 ** 32 - 1), ("i", 3), ("i", 2 ** 34), ("S",)]
    assert C.c_uint64(-1 & (2 ** 64 - 1)).value == 2 ** 64 - 1
