"""DPM-Solver++ multistep sampling (asva_amd.schedulers.DPMSolverMultistepScheduler + avsd_guided_multistep) on CPU
(-m "not gpu"): the solver against the exact probability-flow solution of Gaussian data, its first-order map against DDIM's,
the timestep tables, configuration handling, the fused engine against the reference-style loop on the emulated kernel
contracts (tests/emu_ops.py, plus the new entry point's contract stated below), and the C ABI's argument check."""
import ctypes
import json
import math
import struct

import numpy as np
import pytest
import torch

from tests import emu_ops
from tests.helpers import load_golden, rel_l2
from tests.test_pipeline_cpu import _clip, _pipe, emu  # noqa: F401  (emu: fixture)


def guided_multistep(noise_pred, n_branch, g, x_in, x_out, ca, c_cur, s_x, s_e, *, hist=None, store_slot=-1, hist_idx=(), w=(),
                     g2=0.0):
    """avsd_guided_multistep's contract (include/avsd.h), computed in the dtype of its arguments"""
    B = x_in.shape[0]
    eps = noise_pred[:B]
    if n_branch >= 2:
        e1 = noise_pred[B:2 * B]
        eps = eps + g * (e1 - eps)
        if n_branch == 3:
            eps = eps + g2 * (noise_pred[2 * B:] - e1)
    d = s_x * x_in + s_e * eps
    if store_slot >= 0:
        hist[store_slot] = d
    new = ca * x_in + c_cur * d
    for i, wk in zip(hist_idx, w):
        new = new + wk * hist[i]
    new[:, :, 0] = x_in[:, :, 0]
    x_out.copy_(new)


def _sched(**kw):
    from asva_amd.schedulers import DPMSolverMultistepScheduler

    return DPMSolverMultistepScheduler(**kw)


def _alpha_sigma(sig):
    a = 1.0 / math.sqrt(1.0 + sig * sig)
    return a, sig * a


# ---- Gaussian data: the exact noise prediction and the exact probability-flow solution --------------------------------------
def _gauss(seed=0, shape=(1, 3, 4, 5, 6)):
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn(shape, generator=gen, dtype=torch.float64)
    s = 0.3 + torch.rand(shape, generator=gen, dtype=torch.float64)
    z = torch.randn(shape, generator=gen, dtype=torch.float64)
    return mu, s, z


def _eps_star(x, sig, mu, s):
    a, sg = _alpha_sigma(sig)
    return sg * (x - a * mu) / (a * a * s * s + sg * sg)


def _exact(sig, mu, s, z):
    a, sg = _alpha_sigma(sig)
    return a * mu + torch.sqrt(a * a * s * s + sg * sg) * z


def _solve(sched, steps, data, planned, warm=False):
    """x at the solver's last sigma, from the exact x at its first one; the planned form runs the kernel contract in place.
    warm: start at step solver_order - 1 from the exact state, with the exact data predictions of the steps before it in the
    history — no lower-order warm-up steps."""
    mu, s, z = data
    sched.set_timesteps(steps)
    k0 = sched.solver_order - 1 if warm else 0
    sig = [float(v) for v in sched.sigmas]
    x0s = [(_exact(sig[j], mu, s, z) - _alpha_sigma(sig[j])[1] * _eps_star(_exact(sig[j], mu, s, z), sig[j], mu, s)) / _alpha_sigma(sig[j])[0]
           for j in range(k0)]
    x = _exact(sig[k0], mu, s, z)
    if planned:
        hist = torch.zeros((4,) + tuple(x.shape), dtype=torch.float64)
        for j, x0 in enumerate(x0s):
            hist[j % sched.solver_order] = x0
        for i in range(k0, sched.num_forwards()):
            p = sched.plan_step(i)
            guided_multistep(_eps_star(x, sig[i], mu, s), 1, 1.0, x, x, p.ca, p.c_cur, p.s_x, p.s_e, hist=hist,
                             store_slot=p.store_slot, hist_idx=p.hist_idx, w=p.hist_w)
    else:
        if warm:
            sched._step_index, sched.lower_order_nums = k0, k0
            sched.model_outputs = ([None] * sched.solver_order + x0s)[-sched.solver_order:]
        for i in range(k0, sched.num_forwards()):
            x = sched.step(_eps_star(x, sig[i], mu, s), sched.timesteps[i], x).prev_sample
    return x, _exact(sig[-1], mu, s, z)


def _err(sched, steps, data, planned=False, warm=False):
    x, want = _solve(sched, steps, data, planned, warm)
    return rel_l2(x[:, :, 1:], want[:, :, 1:])


@pytest.mark.parametrize("order,solver_type,karras,spacing", [(1, "midpoint", False, "linspace"), (2, "midpoint", False, "linspace"),
                                                              (2, "heun", False, "trailing"), (3, "midpoint", False, "leading"),
                                                              (2, "midpoint", True, "linspace"), (3, "heun", True, "trailing")])
@pytest.mark.parametrize("final", ["zero", "sigma_min"])
def test_object_protocol_equals_planned_form(order, solver_type, karras, spacing, final):
    """`step()` (diffusers' update over the data predictions) and `plan_step()` through the kernel contract (the same update
    folded into per-slot weights of the device ring) are two statements of one solver"""
    data = _gauss(1)
    for steps in (6, 20):
        kw = dict(solver_order=order, solver_type=solver_type, use_karras_sigmas=karras, timestep_spacing=spacing, final_sigmas_type=final,
                  steps_offset=1 if spacing == "leading" else 0)
        a, _ = _solve(_sched(**kw), steps, data, planned=False)
        b, _ = _solve(_sched(**kw), steps, data, planned=True)
        assert float((a[:, :, 1:] - b[:, :, 1:]).abs().max()) <= 1e-6
        assert bool(torch.isfinite(a).all())


def test_plans_use_the_ring_as_documented():
    """order k stores step i's data prediction in slot i % k and reads the previous k - 1 (3M: 3 slots of the 4-slot ring);
    the last step stores nothing"""
    for order in (1, 2, 3):
        s = _sched(solver_order=order, lower_order_final=False, final_sigmas_type="sigma_min")
        s.set_timesteps(20)
        plans = [s.plan_step(i) for i in range(20)]
        for i, p in enumerate(plans):
            assert p.store_slot == (i % order if order > 1 and i < 19 else -1)
            assert p.hist_idx == tuple((i - k) % order for k in range(1, min(i, order - 1) + 1))
            assert len(p.hist_w) == len(p.hist_idx) and all(0 <= j < 3 for j in p.hist_idx)


def test_solver_converges_to_the_exact_probability_flow_solution():
    """Per-element Gaussian data N(mu, s^2): eps*(x, t) = sigma_t (x - alpha_t mu) / (alpha_t^2 s^2 + sigma_t^2) is the exact noise
    prediction and x_t = alpha_t mu + sqrt(alpha_t^2 s^2 + sigma_t^2) z the exact probability-flow solution.  The solver ends at
    sigma_min with a finite last step (final_sigmas_type="sigma_min", lower_order_final=False) on Karras sigmas, whose steps in
    lambda shrink evenly with n (the linspace table keeps a large last step in lambda at every n, which hides the order).

    3M: the update as published (D2 = (D1_0 - D1_1) / (r0 + r1) with coefficient -alpha_t phi_3) weighs the second-derivative term
    at half of what a third-order Taylor match needs, so its observed order tends to 2, with a constant about 5x below 2M's.
    Doubling that coefficient measures 3.0 - 3.1 here; the restatement keeps the published form (see the class docstring)."""
    data = _gauss(2)
    kw = dict(final_sigmas_type="sigma_min", lower_order_final=False, use_karras_sigmas=True)
    err = {(k, n): _err(_sched(solver_order=k, **kw), n, data) for k in (1, 2, 3) for n in (20, 25, 50)}
    print({f"{k}M/{n}": f"{e:.3e}" for (k, n), e in err.items()})
    for k in (1, 2, 3):                     # the planned form follows the same trajectory
        assert abs(_err(_sched(solver_order=k, **kw), 20, data, planned=True) - err[(k, 20)]) < 1e-9
    assert err[(2, 20)] < 0.25 * err[(1, 20)]         # measured: 1M 5.03e-2, 2M 8.19e-3 at 20 steps
    assert all(err[(3, n)] < 0.5 * err[(2, n)] for n in (20, 25, 50))   # measured 3M: 9.93e-4 / 7.42e-4 / 2.39e-4 (2M: 8.19e-3 / 5.03e-3 / 1.16e-3)
    p1, p2, p3 = (math.log2(err[(k, 25)] / err[(k, 50)]) for k in (1, 2, 3))
    print(f"observed order between 25 and 50 steps: 1M {p1:.2f}, 2M {p2:.2f}, 3M {p3:.2f}")
    assert 0.85 < p1 < 1.2                            # measured 1.01
    assert 1.85 < p2 < 2.4                            # measured 2.12
    assert 1.4 < p3 < 2.4                             # measured 1.63 (1.86 / 1.94 between 50-100 / 100-200 steps)


def test_heun_second_order_converges():
    data = _gauss(3)
    kw = dict(solver_order=2, solver_type="heun", final_sigmas_type="sigma_min", lower_order_final=False, use_karras_sigmas=True)
    e25, e50 = (_err(_sched(**kw), n, data) for n in (25, 50))
    assert 1.85 < math.log2(e25 / e50) < 2.4           # measured 2.16 (other data seed)


@pytest.mark.parametrize("spacing", ["linspace", "leading", "trailing"])
@pytest.mark.parametrize("final", ["zero", "sigma_min"])
def test_first_order_map_is_ddim(spacing, final):
    """x_s = (alpha_s / alpha_t) x_t + (sigma_s - alpha_s sigma_t / alpha_t) eps: the order-1 DPM-Solver++ map is DDIM's (eta = 0)
    for the same pair of noise levels — compared with DDIMScheduler.plan_step's (ca, cb) formula on alphas_cumprod"""
    s = _sched(solver_order=1, timestep_spacing=spacing, final_sigmas_type=final, steps_offset=1 if spacing == "leading" else 0)
    s.set_timesteps(20)
    x, eps = torch.randn(2, 4, 3, 8, 8, dtype=torch.float64), torch.randn(2, 4, 3, 8, 8, dtype=torch.float64)
    for i in range(20):
        p = s.plan_step(i)
        assert p.store_slot == -1 and p.hist_idx == ()
        ca, cb = p.ca + p.c_cur * p.s_x, p.c_cur * p.s_e
        a, ap = (1.0 / (1.0 + float(s.sigmas[j]) ** 2) for j in (i, i + 1))      # alphas_cumprod at t and at s
        assert abs(ca - (ap / a) ** 0.5) < 1e-12
        assert abs(cb - ((1.0 - ap) ** 0.5 - (ap * (1.0 - a) / a) ** 0.5)) < 1e-12
        got = s.step(eps, s.timesteps[i], x).prev_sample
        assert float((got - (ca * x + cb * eps)).abs().max()) < 1e-12


@pytest.mark.parametrize("n", [20, 25])
@pytest.mark.parametrize("spacing", ["linspace", "leading", "trailing"])
def test_timestep_tables(n, spacing):
    s = _sched(timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0)
    s.set_timesteps(n)
    ts = s.timesteps.tolist()
    assert len(ts) == n == s.num_forwards() and all(a > b for a, b in zip(ts, ts[1:])) and 0 <= ts[-1] and ts[0] <= 999
    want = {
        # linspace: round(linspace(0, 999, n + 1))[::-1][:-1]              -> 999 ... round(999 / n)
        ("linspace", 20): (999, 50), ("linspace", 25): (999, 40),
        # leading: (arange(n + 1) * (1000 // (n + 1)))[::-1][:-1] + steps_offset (1)  -> n r + 1 ... r + 1, r = 1000 // (n + 1)
        ("leading", 20): (941, 48), ("leading", 25): (951, 39),
        # trailing: round(arange(1000, 0, -1000 / n)) - 1                   -> 999 ... 1000 / n - 1
        ("trailing", 20): (999, 49), ("trailing", 25): (999, 39),
    }[(spacing, n)]
    assert (ts[0], ts[-1]) == want
    # the sigma table: the training schedule's sigma at each timestep, then the final sigma (0 by default)
    acp = s.acp
    np.testing.assert_allclose(s.sigmas[:-1], ((1 - acp[ts]) / acp[ts]) ** 0.5, rtol=1e-6)
    assert s.sigmas[-1] == 0.0


@pytest.mark.parametrize("n", [20, 25])
def test_karras_sigmas(n):
    s = _sched(use_karras_sigmas=True, final_sigmas_type="sigma_min")
    s.set_timesteps(n)
    sig, acp = s.sigmas[:-1], s.acp
    assert len(sig) == n and np.all(np.diff(sig) < 0)
    np.testing.assert_allclose(sig[0], ((1 - acp[-1]) / acp[-1]) ** 0.5, rtol=1e-6)      # sigma_max of the training schedule
    np.testing.assert_allclose(sig[-1], ((1 - acp[0]) / acp[0]) ** 0.5, rtol=1e-6)       # sigma_min
    assert s.sigmas[-1] == sig[-1].astype(np.float32)
    ts = s.timesteps.tolist()
    assert ts[0] == 999 and ts[-1] == 0 and all(a >= b for a, b in zip(ts, ts[1:]))


def test_config_from_pndm_config_and_from_pretrained(tmp_path):
    from asva_amd.schedulers import DPMSolverMultistepScheduler, PNDMScheduler

    # the diffusers idiom: DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    s = DPMSolverMultistepScheduler.from_config(PNDMScheduler().config)
    assert s.config["timestep_spacing"] == "leading" and s.config["steps_offset"] == 1 and s.config["solver_order"] == 2
    s.set_timesteps(20)
    assert s.timesteps[0] == 941
    assert DPMSolverMultistepScheduler.from_config(s.config, solver_order=3).config["solver_order"] == 3
    # SD1.5's scheduler_config.json (a PNDM file: its PNDM-only keys are accepted and have no effect)
    sd15 = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.6.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
            "beta_start": 0.00085, "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1,
            "trained_betas": None, "clip_sample": False}
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(sd15))
    p = DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    np.testing.assert_array_equal(p.acp, PNDMScheduler().acp)
    p.set_timesteps(20)
    assert p.timesteps[0] == 999                   # the file names no spacing: this class's default, linspace
    for bad in (dict(algorithm_type="sde-dpmsolver++"), dict(algorithm_type="dpmsolver"), dict(prediction_type="v_prediction"),
                dict(thresholding=True), dict(variance_type="learned_range"), dict(euler_at_final=True), dict(lambda_min_clipped=-5.1),
                dict(use_lu_lambdas=True), dict(solver_order=4), dict(solver_type="bh2"), dict(final_sigmas_type="denoise_to_zero"),
                dict(timestep_spacing="karras"), dict(rescale_betas_zero_snr=True), dict(trained_betas=[0.1] * 1000),
                dict(no_such_option=1)):
        with pytest.raises(NotImplementedError):
            DPMSolverMultistepScheduler(**bad)


def test_step_table_writer(tmp_path):
    """plan.export_steps: the table tools/plan_host.cpp's denoise_ms reads (60 bytes per step)"""
    from asva_amd import plan

    s = _sched(solver_order=3)
    s.set_timesteps(7)
    plans = [s.plan_step(i) for i in range(7)]
    path = tmp_path / "steps_ms.bin"
    plan.export_steps(str(path), s.timesteps.tolist(), plans)
    raw = path.read_bytes()
    assert len(raw) == 7 * 60
    for i, p in enumerate(plans):
        v = struct.unpack_from("<5f2i4i4f", raw, 60 * i)
        assert v[0] == float(s.timesteps[i]) and v[5] == p.store_slot and v[6] == len(p.hist_idx)
        np.testing.assert_array_equal(np.array(v[1:5], dtype=np.float32), np.array([p.ca, p.c_cur, p.s_x, p.s_e], dtype=np.float32))
        assert list(v[7:7 + len(p.hist_idx)]) == list(p.hist_idx)
        np.testing.assert_array_equal(np.array(v[11:11 + len(p.hist_w)], dtype=np.float32), np.array(p.hist_w, dtype=np.float32))


@pytest.mark.parametrize("tg,ag", [(1.0, 4.0), (7.5, 4.0)])
def test_engine_loop_equals_reference_style_loop_dpmsolver(emu, monkeypatch, tg, ag):   # noqa: F811
    """test_pipeline_cpu.py::test_engine_loop_equals_reference_style_loop for DPM++ 2M: the fused engine (plan_step + one
    avsd_guided_multistep per step) and the reference-style loop (`step()` on frames 1..), audio-only and dual guidance"""
    from asva_amd.schedulers import DPMSolverMultistepScheduler, MultistepPlan

    monkeypatch.setattr(emu_ops, "guided_multistep", guided_multistep, raising=False)
    g = load_golden("unet_tiny_e2e.pt")
    c = _clip(g, seed=1)
    pipe, _, _ = _pipe(g, DPMSolverMultistepScheduler())
    pipe.null_text_encoding = torch.randn(1, *c["text"].shape[1:], generator=torch.Generator().manual_seed(5))
    kw = dict(texts=[""], text_encodings=[c["text"]], video_length=c["f"], height=c["hw"][0], width=c["hw"][1], num_inference_steps=6,
              audio_guidance_scale=ag, text_guidance_scale=tg, image_latents=c["image_latents"], audio_encodings=c["audio"],
              null_audio_encodings=c["null_audio"], audio_masks=c["mask"], noise=c["noise"], output_latents=True)
    fused = pipe(**kw)
    assert len(pipe._engine._plans) == 6 and all(isinstance(p, MultistepPlan) for p in pipe._engine._plans)   # the engine ran it
    pipe.use_engine = False
    looped = pipe(**kw)
    assert torch.equal(fused[:, :, 0], looped[:, :, 0])
    err = rel_l2(fused, looped)
    print(f"DPM++ 2M, 6 steps, tg {tg} ag {ag}: engine vs reference-style loop rel-L2 {err:.3e}")
    assert err < 2e-2


def test_guided_multistep_argument_errors_without_a_device():
    from asva_amd import _lib

    h = _lib.lib()
    idx, w = (ctypes.c_int32 * 4)(), (ctypes.c_float * 4)()
    assert h.avsd_guided_multistep(None, 2, 4.0, 0.0, None, -1, idx, w, 0, None, None, 1.0, 0.5, 1.0, 0.0, 1, 4, 12, 1024, None) == -1
    assert b"guided_multistep: null pointer" in h.avsd_last_error()
