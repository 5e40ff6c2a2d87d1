"""The inputs of the probability-tail case of tests/test_kernels_prec_gpu.py, checked WITHOUT a device: the float64 reference and its
rounding emulations (tests/attn_prec_ref.py) alone must satisfy what the GPU test relies on, so the operands cannot silently stop
discriminating between a kernel that keeps subnormal probabilities and one that flushes them.
"""
import pytest
import torch

from tests import attn_prec_ref as R


@pytest.mark.parametrize("dom", [0, 700])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_tail_case_discriminates(dtype, dom):
    q, k, v = (t.to(dtype) for t in R.tail_operands(dom))
    f = R.tail_figures(q, k, v, dom, dtype)
    tol = R.TOL16[dtype]
    print(f"tail dom={dom} [{dtype}]: tail mass {f['tail_mass']:.3f}, ideal rounding {f['e_ideal']:.3e}, e_grad {f['e_grad']:.3e}, "
          f"flushed {f['e_flush']:.3e}")
    assert f["e_grad"] <= tol / 1.5              # the documented roundings leave the whole-tensor bound in force ...
    assert R.bound16(dtype, f["e_grad"]) == tol
    if dtype == torch.float16:
        assert f["e_flush"] >= 10 * tol          # ... and a kernel that loses the subnormal tail misses it by far
    assert f["tail_mass"] >= 0.15


@pytest.mark.parametrize("gap,fp16_worse", [(16.0, False), (18.0, True)])
def test_wider_gaps_are_measurement_only(gap, fp16_worse):
    """profiles/kernels_fp16.md: at an 18-bit gap the rounding of P costs IEEE half more than bfloat16 on this input"""
    e = {}
    for dtype in (torch.float16, torch.bfloat16):
        q, k, v = (t.to(dtype) for t in R.tail_operands(0, gap_bits=gap))
        e[dtype] = R.tail_figures(q, k, v, 0, dtype)["e_grad"]
    print(f"tail gap {gap:.0f} bits: e_grad fp16 {e[torch.float16]:.3e}, bf16 {e[torch.bfloat16]:.3e}")
    assert (e[torch.float16] > e[torch.bfloat16]) == fp16_worse
