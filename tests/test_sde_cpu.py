"""The two stochastic samplers on CPU (-m "not gpu"): DDIM with eta > 0 and SDE-DPM-Solver++ (asva_amd/schedulers.py), whose noise
the step kernels evaluate themselves (avsd_guided_step_sde / avsd_guided_multistep_sde).  The plans against exact identities on
point-mass data and against the order of convergence on Gaussian data, the object protocol against the plan-driven float64
contract (tests/sde_contract.py) with one DeviceGenerator, the cases that must not change, the refused ones, the step tables, and
the entry points' argument checks."""
import ctypes
import itertools
import struct

import pytest
import torch

from tests import sde_contract as K
from tests.test_stochastic_cpu import emu_rng  # noqa: F401  (fixture: ops.randn_philox on tests/philox_ref.py)


def _sde(**kw):
    from asva_amd.schedulers import SDEDPMSolverMultistepScheduler

    return SDEDPMSolverMultistepScheduler(**kw)


def _ddim(eta=0.0):
    from asva_amd.schedulers import DDIMScheduler

    return DDIMScheduler().set_eta(eta)


STEPS_SDE = (3, 4, 5, 7, 10, 14, 15, 20, 50, 200)
STEPS_DDIM = (3, 4, 5, 10, 20, 50, 100, 250)


# ---- exact identities on point-mass data --------------------------------------------------------------------------------------
def test_sde_plans_carry_the_marginals_of_point_mass_data():
    """eps = (x - alpha_s x0) / sigma_s: every step maps mean alpha_s x0 to alpha_t x0 and variance sigma_s^2 to sigma_t^2, i.e.
    ca alpha_s + c_cur + sum w = alpha_t and ca^2 sigma_s^2 + c_noise^2 = sigma_t^2.  Relative residual < 1e-12 in float64 (the
    formulas give at most 6.7e-16 over this grid)."""
    from asva_amd.schedulers import NoisyMultistepPlan

    worst = 0.0
    for order, typ, spacing, karras, final in itertools.product((1, 2), ("midpoint", "heun"), ("linspace", "leading", "trailing"),
                                                                (False, True), ("zero", "sigma_min")):
        s = _sde(solver_order=order, solver_type=typ, timestep_spacing=spacing, use_karras_sigmas=karras, final_sigmas_type=final)
        for n in STEPS_SDE:
            s.set_timesteps(n)
            for i in range(s.num_forwards()):
                p = s.plan_step(i)
                assert type(p) is NoisyMultistepPlan and p.noise_step == i and p.c_noise >= 0.0
                a_t, s_t = K.alpha_sigma(float(s.sigmas[i + 1]))
                mean, var = K.multistep_moments(s, i, p)
                # relative to sigma_t^2 itself; onto a final sigma of zero the variance must vanish exactly
                worst = max(worst, abs(mean - a_t) / a_t, abs(var - s_t * s_t) / (s_t * s_t) if s_t else (1.0 if var else 0.0))
    print(f"SDE-DPM-Solver++ point-mass identities: worst relative residual {worst:.2e}")
    assert worst < 1e-12


def test_ddim_eta_plans_carry_the_marginals_of_point_mass_data():
    """ca sqrt(a) = sqrt(a') and (ca sqrt(1 - a) + cb)^2 + c_noise^2 = 1 - a'.  Relative residual < 1e-12 (at most 3.3e-15 here)."""
    from asva_amd.schedulers import NoisyStepPlan

    worst = 0.0
    for eta in (0.25, 0.5, 1.0):
        s = _ddim(eta)
        for n in STEPS_DDIM:
            s.set_timesteps(n)
            ratio = s.num_train_timesteps // n
            for i in range(s.num_forwards()):
                p = s.plan_step(i)
                assert type(p) is NoisyStepPlan and p.noise_step == i and p.c_noise > 0.0
                a, ap = s._acp(s._ts[i]), s._acp(s._ts[i] - ratio)
                mean = p.ca * a ** 0.5
                var = (p.ca * (1.0 - a) ** 0.5 + p.cb) ** 2 + p.c_noise ** 2
                worst = max(worst, abs(mean - ap ** 0.5) / ap ** 0.5, abs(var - (1.0 - ap)) / (1.0 - ap))
    print(f"DDIM eta > 0 point-mass identities: worst relative residual {worst:.2e}")
    assert worst < 1e-12


# ---- order of convergence on Gaussian data ----------------------------------------------------------------------------------
@pytest.mark.parametrize("order,typ", [(1, "midpoint"), (2, "midpoint"), (2, "heun")])
def test_sde_order_of_convergence_on_gaussian_data(order, typ):
    """Unit-variance Gaussian data with the exact linear eps; the sampler's covariance propagated in closed form through the plans
    (tests/sde_contract.py), Karras sigmas, final_sigmas_type="sigma_min".  Relative error of the final variance at n = 40, 80, 160:
    order 1 falls by a factor in [1.7, 2.3] per doubling (the formulas give 1.91 / 1.95), order 2 by more than 3.5 (midpoint
    4.24 / 4.12, heun 4.38 / 4.17).  A wrong D1 coefficient drops order 2 to order 1."""
    s = _sde(solver_order=order, solver_type=typ, use_karras_sigmas=True, final_sigmas_type="sigma_min")
    errs = []
    for n in (40, 80, 160):
        got, want = K.gaussian_final_variance(s, n)
        errs.append(abs(got - want) / want)
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print(f"SDE-DPM-Solver++ order {order} {typ}: errors {errs}, ratios {ratios}")
    for r in ratios:
        assert (1.7 <= r <= 2.3) if order == 1 else r > 3.5, (errs, ratios)


# ---- the object protocol equals the plan-driven contract ----------------------------------------------------------------------
def _eps_model(x, i):
    return torch.tanh(0.7 * x + 0.05 * i) - 0.1 * x                      # any smooth function of (x, step) serves


@pytest.mark.parametrize("kind", ["ddim", "sde1", "sde2m", "sde2h"])
def test_object_protocol_equals_plan_driven_contract(emu_rng, kind):  # noqa: F811
    """step() is diffusers' formula on tensors, driven as the reference loop drives it: on the (B, C, F - 1, H, W) slice with a
    DeviceGenerator.  The contract is the float64 emulation of the kernels with tests/philox_ref.py's normals under the key the
    same generator hands the engine.  7 steps, agreement to 1e-12 in float64."""
    from asva_amd.rng import DeviceGenerator

    make = {"ddim": lambda: _ddim(0.8), "sde1": lambda: _sde(solver_order=1), "sde2m": lambda: _sde(),
            "sde2h": lambda: _sde(solver_type="heun", final_sigmas_type="sigma_min")}[kind]
    B, C, F, H, W = 2, 3, 4, 2, 5
    x0 = torch.randn(B, C, F, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    # object protocol
    s, gen = make(), DeviceGenerator(77)
    gen.next_stream()                                                    # the key does not start at stream 0
    s.set_timesteps(7)
    x = x0.clone()
    extra = dict(eta=0.8) if kind == "ddim" else {}
    for i, t in enumerate(s.timesteps):
        eps = _eps_model(x, i)
        x[:, :, 1:] = s.step(eps[:, :, 1:], t, x[:, :, 1:], generator=gen, **extra).prev_sample
    assert gen.streams == 1 + B                                          # B streams, taken once
    # plans on the contract
    s2, gen2 = make(), DeviceGenerator(77)
    gen2.next_stream()
    s2.set_timesteps(7)
    y = x0.clone()
    bufs = K.Bufs(y, (gen2.seed, gen2.take_streams(B)))
    for i in range(s2.num_forwards()):
        s2.plan_step(i).launch(K.ContractOps, _eps_model(y, i), 1, 1.0, 0.0, y, bufs)
    assert torch.equal(y[:, :, 0], x0[:, :, 0]) and not torch.equal(y[:, :, 1:], x0[:, :, 1:])
    err = float((x - y).abs().max() / y.abs().max())
    print(f"{kind}: object protocol vs plan-driven contract, 7 steps: max relative difference {err:.2e}")
    assert err < 1e-12
    # variance_noise wins over the generator; another generator draws torch.randn of the model output's shape
    s.set_timesteps(7)
    zero = torch.zeros(B, C, F - 1, H, W, dtype=torch.float64)
    a = s.step(x0[:, :, 1:], s.timesteps[0], x0[:, :, 1:], generator=gen, variance_noise=zero, **extra).prev_sample
    s.set_timesteps(7)
    b = s.step(x0[:, :, 1:], s.timesteps[0], x0[:, :, 1:], generator=torch.Generator().manual_seed(1), **extra).prev_sample
    s.set_timesteps(7)
    c = s.step(x0[:, :, 1:], s.timesteps[0], x0[:, :, 1:], generator=torch.Generator().manual_seed(1), **extra).prev_sample
    p = s.plan_step(0)
    assert torch.equal(b, c) and not torch.equal(a, b)
    want = torch.randn(zero.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert float(((b - a) - p.c_noise * want).abs().max()) < 1e-12


# ---- what must not change, and what is refused ------------------------------------------------------------------------------
def test_deterministic_settings_return_todays_plans():
    from asva_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, MultistepPlan, StepPlan

    d = DDIMScheduler()
    before = dict(d.config)
    assert d.eta == 0.0 and not d.stochastic and "eta" not in d.config
    d.set_timesteps(9)
    plain = [d.plan_step(i) for i in range(9)]
    assert all(type(p) is StepPlan and len(p.record(1.0)) == 64 for p in plain)
    d.set_eta(0.5)
    assert d.stochastic and d.config == before                          # eta is no configuration key
    assert all(type(d.plan_step(i)).__name__ == "NoisyStepPlan" for i in range(9))
    d.set_eta(0.0)
    assert [p.record(3.0) for p in plain] == [d.plan_step(i).record(3.0) for i in range(9)]
    # the plain coefficients are those of the formula the class has always used
    a, ap = d._acp(d._ts[2]), d._acp(d._ts[2] - 1000 // 9)
    assert plain[2] == StepPlan(ca=(ap / a) ** 0.5, cb=(1.0 - ap) ** 0.5 - (ap * (1.0 - a) / a) ** 0.5)
    for order in (1, 2, 3):
        s = DPMSolverMultistepScheduler(solver_order=order)
        assert not s.stochastic
        s.set_timesteps(9)
        assert all(type(s.plan_step(i)) is MultistepPlan and len(s.plan_step(i).record(1.0)) == 60 for i in range(9))
    # the first-order SDE step with its noise switched off differs from the ODE step: it is another sampler, not a flag
    s, z = DPMSolverMultistepScheduler(solver_order=1), _sde(solver_order=1)
    s.set_timesteps(9), z.set_timesteps(9)
    assert s.plan_step(3).ca != z.plan_step(3).ca and z.config["algorithm_type"] == "sde-dpmsolver++"


def test_refused_settings():
    from asva_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, SDEDPMSolverMultistepScheduler

    for bad in (dict(solver_order=3), dict(algorithm_type="dpmsolver++"), dict(algorithm_type="sde-dpmsolver"), dict(thresholding=True)):
        with pytest.raises(NotImplementedError):
            SDEDPMSolverMultistepScheduler(**bad)
    with pytest.raises(NotImplementedError):                             # the deterministic class takes "dpmsolver++" alone, as before
        DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    # the diffusers idiom from a deterministic scheduler's configuration; positional arguments reach the parent unchanged
    s = SDEDPMSolverMultistepScheduler.from_config(DPMSolverMultistepScheduler(solver_type="heun").config)
    assert s.stochastic and s.config["algorithm_type"] == "sde-dpmsolver++" and s.solver_type == "heun" and s.solver_order == 2
    assert SDEDPMSolverMultistepScheduler(1000, 0.00085, 0.012, "scaled_linear", None, 1).solver_order == 1
    with pytest.raises(NotImplementedError):
        SDEDPMSolverMultistepScheduler(1000, 0.00085, 0.012, "scaled_linear", None, 3)
    # ... and back: the deterministic class adopts an SDE configuration, whose own class loads it unchanged
    d = DPMSolverMultistepScheduler.from_config(s.config)
    assert type(d) is DPMSolverMultistepScheduler and not d.stochastic and d.config["algorithm_type"] == "dpmsolver++"
    assert d.solver_type == "heun" and SDEDPMSolverMultistepScheduler.from_config(s.config).config == s.config
    d.set_timesteps(5)
    assert type(d.plan_step(1)).__name__ == "MultistepPlan"
    d = DDIMScheduler()
    d.set_timesteps(10)
    x = torch.zeros(1, 4, 3, 2, 2)
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError):
            d.set_eta(bad)
        with pytest.raises(ValueError):
            d.step(x, d.timesteps[0], x, eta=bad)
    d.set_eta(40.0)                                                      # sigma^2 > 1 - a': no real coefficient is left for eps
    with pytest.raises(ValueError, match="< 0"):
        d.plan_step(0)
    with pytest.raises(ValueError, match="< 0"):
        d.step(x, d.timesteps[0], x, eta=40.0)


@pytest.mark.parametrize("kind", ["ddim", "sde"])
def test_engine_with_a_noisy_plan_needs_a_device_generator(emu_rng, kind):  # noqa: F811
    """before any launch: the UNet here would fail if it were called"""
    from asva_amd.engine import DenoiseEngine
    from asva_amd.rng import DeviceGenerator

    eng = DenoiseEngine(None, _ddim(1.0) if kind == "ddim" else _sde(), use_graph=False)
    x = torch.zeros(2, 4, 3, 2, 2)
    for gen in (None, torch.Generator().manual_seed(0)):
        with pytest.raises(ValueError, match="DeviceGenerator"):
            eng.prepare(x, 5, gen)
        with pytest.raises(ValueError, match="DeviceGenerator"):
            eng.run(x, 5) if gen is None else eng.run(x, 5, gen)
    g = DeviceGenerator(9)
    g.next_stream()
    eng.prepare(x, 5, g)
    assert eng._noise_key == (9, 1) and g.streams == 3                   # one stream per batch row
    eng.prepare(x, 5, g)
    assert eng._noise_key == (9, 3)                                      # fresh ones for the next clip
    det = DenoiseEngine(None, _ddim(0.0), use_graph=False)
    det.prepare(x, 5)                                                    # deterministic: no generator asked for, none touched
    det.prepare(x, 5, g)
    assert det._noise_key is None and g.streams == 5


def test_pipeline_eta_and_generator_plumbing():
    """`eta=None` (the default) leaves the scheduler's own eta; a value overrides it and stays.  A stochastic scheduler gets a
    DeviceGenerator: the caller's, or one seeded by one draw from the torch generator"""
    from asva_amd.pipeline import AudioCondAnimationPipeline
    from asva_amd.rng import DeviceGenerator

    pipe = AudioCondAnimationPipeline(unet=None, scheduler=_ddim(0.5), vae=None)
    a = pipe._step_generator(torch.Generator().manual_seed(3), None)
    b = pipe._step_generator(torch.Generator().manual_seed(3), None)
    assert pipe.scheduler.eta == 0.5 and isinstance(a, DeviceGenerator) and a.seed == b.seed
    assert a.seed != pipe._step_generator(torch.Generator().manual_seed(4), None).seed
    own = DeviceGenerator(4)
    assert pipe._step_generator(own, 1.0) is own and pipe.scheduler.eta == 1.0
    gen = torch.Generator().manual_seed(3)
    assert pipe._step_generator(gen, 0.0) is gen and pipe.scheduler.eta == 0.0      # deterministic: the generator passes through
    pipe.scheduler = _sde()
    assert isinstance(pipe._step_generator(None, None), DeviceGenerator)


def test_take_streams():
    from asva_amd.rng import DeviceGenerator

    g = DeviceGenerator(1)
    assert g.take_streams(3) == 0 and g.take_streams(0) == 3 and g.next_stream() == 3 and g.take_streams(2) == 4 and g.streams == 6
    g.streams = (1 << 32) - 1
    with pytest.raises(RuntimeError):
        g.take_streams(2)
    assert g.take_streams(1) == (1 << 32) - 1


def test_step_tables(tmp_path):
    """72-byte and 68-byte records: the parent's line, then f32 c_noise, u32 noise_step; plan.export_steps writes them"""
    from asva_amd import plan

    for s, size, parent in ((_ddim(0.7), 72, "<4f4i4i4f"), (_sde(), 68, "<5f2i4i4f")):
        s.set_timesteps(6)
        plans = [s.plan_step(i) for i in range(6)]
        path = tmp_path / f"steps_{size}.bin"
        plan.export_steps(str(path), s.timesteps.tolist(), plans)
        raw = path.read_bytes()
        assert len(raw) == 6 * size
        for i, p in enumerate(plans):
            rec = raw[size * i:size * (i + 1)]
            assert rec == p.record(float(s.timesteps[i])) and rec[:size - 8] == type(p).__mro__[1].record(p, float(s.timesteps[i]))
            assert struct.unpack_from(parent, rec)[0] == float(s.timesteps[i])
            c_noise, noise_step = struct.unpack_from("<fI", rec, size - 8)
            assert noise_step == i and c_noise == struct.unpack("<f", struct.pack("<f", p.c_noise))[0]


def test_new_entry_points_report_argument_errors_without_a_device():
    from asva_amd import _lib, ops

    h = _lib.lib()
    idx, w = (ctypes.c_int32 * 4)(), (ctypes.c_float * 4)()
    some = ctypes.c_void_p(4096)                                         # never dereferenced: the checks come before any launch
    assert h.avsd_guided_step_sde(None, 2, 4.0, 0.0, None, -1, 1.0, idx, w, 0, None, None, 1.0, 0.5, 1, 4, 12, 1024, 0.3, 1, 0, 0,
                                  None) == -1
    assert b"guided_step_sde: null pointer" in h.avsd_last_error()
    assert h.avsd_guided_multistep_sde(None, 2, 4.0, 0.0, None, -1, idx, w, 0, None, None, 1.0, 0.5, 1.0, 0.0, 1, 4, 12, 1024, 0.3, 1,
                                       0, 0, None) == -1
    assert b"guided_multistep_sde: null pointer" in h.avsd_last_error()
    top = (1 << 32) - 2
    assert h.avsd_guided_step_sde(some, 1, 4.0, 0.0, None, -1, 1.0, idx, w, 0, some, some, 1.0, 0.5, 3, 4, 12, 1024, 0.3, 1, top, 0,
                                  None) == -1
    assert b"guided_step_sde: stream + B exceeds 2^32" in h.avsd_last_error()
    assert h.avsd_guided_multistep_sde(some, 1, 4.0, 0.0, None, -1, idx, w, 0, some, some, 1.0, 0.5, 1.0, 0.0, 3, 4, 12, 1024, 0.3,
                                       2 ** 64 - 1, top, 0, None) == -1
    assert b"guided_multistep_sde: stream + B exceeds 2^32" in h.avsd_last_error()
    # the wrappers check the ids before they reach the library
    assert ops._noise_key("guided_step_sde", 2, 0.5, 2 ** 64 - 1, top, 7) == (0.5, 2 ** 64 - 1, top, 7)
    for bad in (dict(stream=top + 1), dict(seed=-1), dict(seed=1 << 64), dict(step=1 << 32), dict(stream=-1)):
        with pytest.raises(ValueError, match="guided_step_sde"):
            ops._noise_key("guided_step_sde", 2, 0.5, **{**dict(seed=1, stream=0, step=0), **bad})
