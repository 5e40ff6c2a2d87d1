"""UniPC sampling (asva_amd.schedulers.UniPCMultistepScheduler + avsd_guided_unipc) on CPU (-m "not gpu"): the object protocol and
the planned form (through the kernel's contract, stated below in the dtype of its arguments) against the float64 restatement of
the paper (tests/unipc_ref.py), the predictor alone against DPM-Solver++ 2M and DDIM, convergence on the exact probability-flow
solution of Gaussian data, the use of the history ring, configuration handling, the step table, the fused engine against the
reference-style loop on the emulated kernel contracts (tests/emu_ops.py), and the C ABI's argument check."""
import ctypes
import json
import math
import struct

import numpy as np
import pytest
import torch

from tests import emu_ops, unipc_ref
from tests.helpers import load_golden, rel_l2
from tests.test_dpmsolver_cpu import _alpha_sigma, _eps_star, _exact, _gauss
from tests.test_pipeline_cpu import _clip, _pipe, emu  # noqa: F401  (emu: fixture)


def guided_unipc(noise_pred, n_branch, g, x_in, x_out, x_last, use_corrector, s_x, s_e, cc_last, cc_cur, cp_x, cp_cur, *, hist=None,
                 store_slot=-1, hist_idx=(), wc=(), wp=(), g2=0.0):
    """avsd_guided_unipc's contract (include/avsd.h), computed in the dtype of its arguments"""
    B = x_in.shape[0]
    eps = noise_pred[:B]
    if n_branch >= 2:
        e1 = noise_pred[B:2 * B]
        eps = eps + g * (e1 - eps)
        if n_branch == 3:
            eps = eps + g2 * (noise_pred[2 * B:] - e1)
    xin = x_in.clone()
    d = s_x * xin + s_e * eps
    h = [hist[i].clone() for i in hist_idx]                 # every read happens before the store
    xc = xin
    if use_corrector:
        xc = cc_last * x_last + cc_cur * d
        for hk, w in zip(h, wc):
            xc = xc + w * hk
    if store_slot >= 0:
        hist[store_slot] = d
    new = cp_x * xc + cp_cur * d
    for hk, w in zip(h, wp):
        new = new + w * hk
    xc = xc.clone()
    xc[:, :, 0] = xin[:, :, 0]
    new[:, :, 0] = xin[:, :, 0]
    x_last.copy_(xc)
    x_out.copy_(new)


def _sched(**kw):
    from asva_amd.schedulers import UniPCMultistepScheduler

    return UniPCMultistepScheduler(**kw)


def _run_object(s, steps, eps_fn, x):
    s.set_timesteps(steps)
    outs = []
    for i in range(s.num_forwards()):
        x = s.step(eps_fn(x, i), s.timesteps[i], x).prev_sample
        outs.append(x)
    return outs


def _run_planned(s, steps, eps_fn, x):
    s.set_timesteps(steps)
    x = x.clone()
    hist = torch.full((4,) + tuple(x.shape), float("nan"), dtype=x.dtype)     # a slot read before it was stored shows as NaN
    x_last = torch.full_like(x, float("nan"))
    outs = []
    for i in range(s.num_forwards()):
        p = s.plan_step(i)
        guided_unipc(eps_fn(x, i), 1, 1.0, x, x, x_last, p.use_corrector, p.s_x, p.s_e, p.cc_last, p.cc_cur, p.cp_x, p.cp_cur, hist=hist,
                     store_slot=p.store_slot, hist_idx=p.hist_idx, wc=p.wc, wp=p.wp)
        outs.append(x.clone())
    return outs


def _model(seed):
    """a smooth nonlinear stand-in for the network: eps depends on the sample and on the step"""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(1, 3, 4, 5, 6, generator=gen, dtype=torch.float64)
    b = torch.randn(1, 3, 4, 5, 6, generator=gen, dtype=torch.float64)
    x0 = torch.randn(1, 3, 4, 5, 6, generator=gen, dtype=torch.float64)

    def eps_fn(x, i):
        return torch.tanh(0.7 * x + a) + 0.1 * math.cos(i) * b

    return eps_fn, x0


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("variant", ["bh1", "bh2"])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", ["linspace", "leading", "trailing"])
@pytest.mark.parametrize("final", ["zero", "sigma_min"])
def test_object_protocol_and_planned_form_equal_the_restated_paper(order, variant, karras, spacing, final):
    """`step()` (the update over the differences of data predictions), `plan_step()` through the kernel contract (both updates
    folded into per-slot weights of the ring) and tests/unipc_ref.py are three statements of one sampler: 8 steps, with every
    corrector on and with those after steps 0 and 3 off; every step's output within float64 rounding (1e-9 relative)"""
    eps_fn, x0 = _model(order)
    for lof in (True, False):
        for dc in ([], [0, 3]):
            kw = dict(solver_order=order, solver_type=variant, use_karras_sigmas=karras, timestep_spacing=spacing, final_sigmas_type=final,
                      steps_offset=1 if spacing == "leading" else 0, disable_corrector=dc, lower_order_final=lof)
            a = _run_object(_sched(**kw), 8, eps_fn, x0)
            b = _run_planned(_sched(**kw), 8, eps_fn, x0)
            s = _sched(**kw)
            s.set_timesteps(8)
            want, _ = unipc_ref.sample(s.sigmas, lambda x, i: eps_fn(torch.from_numpy(x), i).numpy(), x0.numpy(), order, variant,
                                       lower_order_final=lof, disable_corrector=dc)
            assert len(a) == len(b) == len(want) == 8
            for i in range(8):
                w = torch.from_numpy(want[i])
                assert bool(torch.isfinite(w).all())
                assert rel_l2(a[i][:, :, 1:], w[:, :, 1:]) < 1e-9, (i, "object protocol")
                assert rel_l2(b[i][:, :, 1:], w[:, :, 1:]) < 1e-9, (i, "planned form")
                assert torch.equal(b[i][:, :, 0], x0[:, :, 0])                 # the contract pins frame 0


def test_predictor_alone_is_dpmsolver_2m_midpoint():
    """With rho = 1/2 and B(h) = e^h - 1 the order-2 predictor is DPM-Solver++ 2M's midpoint update: every corrector off, the
    two classes agree step by step on one table"""
    from asva_amd.schedulers import DPMSolverMultistepScheduler

    eps_fn, x0 = _model(7)
    for karras, final, n in ((False, "zero", 9), (True, "sigma_min", 9), (False, "sigma_min", 20)):
        kw = dict(solver_order=2, lower_order_final=False, use_karras_sigmas=karras, final_sigmas_type=final)
        u = _sched(solver_type="bh2", disable_corrector=list(range(n)), **kw)
        d = DPMSolverMultistepScheduler(solver_type="midpoint", **kw)
        u.set_timesteps(n)
        d.set_timesteps(n)
        np.testing.assert_array_equal(u.sigmas, d.sigmas)
        assert u.timesteps.tolist() == d.timesteps.tolist()
        xu = xd = x0
        for i in range(n):
            xu = u.step(eps_fn(xu, i), u.timesteps[i], xu).prev_sample
            xd = d.step(eps_fn(xd, i), d.timesteps[i], xd).prev_sample
            assert rel_l2(xu, xd) < 1e-10, i


@pytest.mark.parametrize("spacing", ["linspace", "leading", "trailing"])
@pytest.mark.parametrize("final", ["zero", "sigma_min"])
def test_first_order_predictor_is_ddim(spacing, final):
    """test_dpmsolver_cpu.py::test_first_order_map_is_ddim for UniP-1 (corrector off): DDIMScheduler.plan_step's (ca, cb) formula"""
    s = _sched(solver_order=1, timestep_spacing=spacing, final_sigmas_type=final, steps_offset=1 if spacing == "leading" else 0,
               disable_corrector=list(range(20)))
    s.set_timesteps(20)
    x, eps = torch.randn(2, 4, 3, 8, 8, dtype=torch.float64), torch.randn(2, 4, 3, 8, 8, dtype=torch.float64)
    for i in range(20):
        p = s.plan_step(i)
        assert p.store_slot == -1 and p.hist_idx == () and not p.use_corrector
        ca, cb = p.cp_x + p.cp_cur * p.s_x, p.cp_cur * p.s_e
        a, ap = (1.0 / (1.0 + float(s.sigmas[j]) ** 2) for j in (i, i + 1))      # alphas_cumprod at t and at s
        assert abs(ca - (ap / a) ** 0.5) < 1e-12
        assert abs(cb - ((1.0 - ap) ** 0.5 - (ap * (1.0 - a) / a) ** 0.5)) < 1e-12
        s._step_index = i
        got = s.step(eps, s.timesteps[i], x).prev_sample
        assert float((got - (ca * x + cb * eps)).abs().max()) < 1e-12


# ---- convergence on Gaussian data (the problem of tests/test_dpmsolver_cpu.py) -----------------------------------------------
def _gauss_err(s, steps, data, planned=False):
    mu, sd, z = data
    s.set_timesteps(steps)
    sig = [float(v) for v in s.sigmas]
    run = _run_planned if planned else _run_object
    x = run(s, steps, lambda x, i: _eps_star(x, sig[i], mu, sd), _exact(sig[0], mu, sd, z))[-1]
    want = _exact(sig[-1], mu, sd, z)
    return rel_l2(x[:, :, 1:], want[:, :, 1:])


def test_unipc_converges_at_the_order_the_paper_states():
    """Per-element Gaussian data with the exact noise prediction (test_dpmsolver_cpu.py::
    test_solver_converges_to_the_exact_probability_flow_solution explains the problem and why Karras sigmas ending on sigma_min
    with lower_order_final=False show the order).  UniP-p converges at order p, UniPC-p at p + 1: observed between 25 and 50
    steps within 0.4 of that for p = 1, 2, 3 and both B(h).  The corrector lowers the error at every step count tried, UniPC-2
    beats DPM++ 2M, and UniPC-3 beats DPM++ 3M at 25 and 50 steps (at 20 the repo's 3M is ahead)."""
    from asva_amd.schedulers import DPMSolverMultistepScheduler

    data = _gauss(2)
    kw = dict(final_sigmas_type="sigma_min", lower_order_final=False, use_karras_sigmas=True)
    ns = (10, 20, 25, 50)
    err = {}
    for n in ns:
        for k in (1, 2, 3):
            err[(f"dpm{k}", n)] = _gauss_err(DPMSolverMultistepScheduler(solver_order=k, **kw), n, data)
            for v in ("bh1", "bh2"):
                err[(f"p{k}{v}", n)] = _gauss_err(_sched(solver_order=k, solver_type=v, disable_corrector=list(range(n)), **kw), n, data)
                err[(f"pc{k}{v}", n)] = _gauss_err(_sched(solver_order=k, solver_type=v, **kw), n, data)
    cols = ["dpm2", "dpm3", "p2bh2", "pc1bh2", "pc2bh2", "pc3bh2", "pc2bh1", "pc3bh1"]
    print("\nsteps " + " ".join(f"{c:>9}" for c in cols))
    for n in ns:
        print(f"{n:5d} " + " ".join(f"{err[(c, n)]:9.2e}" for c in cols))
    lin = dict(final_sigmas_type="sigma_min", lower_order_final=False)          # the plain table: its last lambda step dominates
    e_dpm, e_pc = _gauss_err(DPMSolverMultistepScheduler(solver_order=2, **lin), 10, data), _gauss_err(_sched(solver_order=2, **lin), 10, data)
    print(f"linspace sigmas, 10 steps: DPM++ 2M {e_dpm:.2e}, UniPC-2 bh2 {e_pc:.2e}")
    for k in (1, 2, 3):                     # the planned form follows the same trajectory
        assert abs(_gauss_err(_sched(solver_order=k, **kw), 20, data, planned=True) - err[(f"pc{k}bh2", 20)]) < 1e-9
    print("observed order between 25 and 50 steps:")
    for v in ("bh1", "bh2"):
        for k in (1, 2, 3):
            op = math.log2(err[(f"p{k}{v}", 25)] / err[(f"p{k}{v}", 50)])
            oc = math.log2(err[(f"pc{k}{v}", 25)] / err[(f"pc{k}{v}", 50)])
            print(f"  {v} order {k}: predictor only {op:.2f}, with corrector {oc:.2f}")
            assert abs(op - k) < 0.4 and abs(oc - (k + 1)) < 0.4
            for n in (20, 25, 50):
                assert err[(f"pc{k}{v}", n)] < err[(f"p{k}{v}", n)]
    for n in (20, 25, 50):
        assert err[("pc2bh2", n)] < err[("dpm2", n)]
        assert abs(err[("p2bh2", n)] - err[("dpm2", n)]) < 1e-9 * err[("dpm2", n)] + 1e-12     # the same formula
    for n in (25, 50):
        assert err[("pc3bh2", n)] < err[("dpm3", n)]


# ---- the ring ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("dc", [[], [0, 3], list(range(12))])
@pytest.mark.parametrize("lof", [True, False])
def test_plans_use_the_ring_as_documented(order, dc, lof):
    """step i stores m_i in slot i % solver_order, or nowhere when no later step reads it; a plan names at most solver_order
    slots; the corrector of step i runs at the order of step i - 1's predictor"""
    s = _sched(solver_order=order, disable_corrector=dc, lower_order_final=lof)
    s.set_timesteps(12)
    plans = [s.plan_step(i) for i in range(12)]
    holder = {}                                   # slot -> step whose data prediction it holds
    read_by_later = set()
    for i, p in enumerate(plans):
        assert len(p.hist_idx) == len(p.wc) == len(p.wp) <= order and len(set(p.hist_idx)) == len(p.hist_idx)
        assert all(0 <= j < order for j in p.hist_idx) and p.store_slot in (-1, i % order)
        assert p.order == min(order, 12 - i if lof else order, i + 1, 1 if i == 11 else order)     # final sigma 0: first order
        assert p.use_corrector == (i > 0 and (i - 1) not in dc)
        assert p.corrector_order == (plans[i - 1].order if p.use_corrector else 0)
        steps_read = [holder[j] for j in p.hist_idx]                               # KeyError: a slot nobody stored
        want = set(range(i - p.order + 1, i)) | (set(range(i - p.corrector_order, i)) if p.use_corrector else set())
        assert set(steps_read) == want
        for st, wc, wp in zip(steps_read, p.wc, p.wp):
            assert (wc != 0.0) == (p.use_corrector and st >= i - p.corrector_order)
            assert (wp != 0.0) == (st > i - p.order)
        read_by_later |= set(steps_read)
        if p.store_slot >= 0:
            holder[p.store_slot] = i
    for i, p in enumerate(plans):
        assert (p.store_slot >= 0) == (i in read_by_later), i


# ---- configuration -----------------------------------------------------------------------------------------------------------
def test_config_from_other_schedulers_from_pretrained_and_refusals(tmp_path):
    from asva_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, UniPCMultistepScheduler

    # the diffusers idiom: UniPCMultistepScheduler.from_config(pipe.scheduler.config)
    s = UniPCMultistepScheduler.from_config(PNDMScheduler().config)
    assert s.config["timestep_spacing"] == "leading" and s.config["steps_offset"] == 1
    assert s.config["solver_order"] == 2 and s.config["solver_type"] == "bh2" and s.config["disable_corrector"] == []
    s.set_timesteps(20)
    assert s.timesteps[0] == 941 and s.num_forwards() == 20
    assert UniPCMultistepScheduler.from_config(DDIMScheduler().config).config["steps_offset"] == 1
    d = UniPCMultistepScheduler.from_config(DPMSolverMultistepScheduler(solver_order=3, use_karras_sigmas=True).config)
    assert d.config["solver_order"] == 3 and d.config["solver_type"] == "bh2" and d.config["use_karras_sigmas"] is True
    assert UniPCMultistepScheduler.from_config(s.config, solver_order=3, solver_type="bh1").config["solver_type"] == "bh1"
    assert UniPCMultistepScheduler.from_config(s.config).config == s.config
    sd15 = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.6.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
            "beta_start": 0.00085, "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1,
            "trained_betas": None, "clip_sample": False}
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(sd15))
    p = UniPCMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    np.testing.assert_array_equal(p.acp, PNDMScheduler().acp)
    p.set_timesteps(20)
    assert p.timesteps[0] == 999                   # the file names no spacing: this class's default, linspace
    for bad in (dict(predict_x0=False), dict(prediction_type="v_prediction"), dict(thresholding=True), dict(solver_order=4),
                dict(solver_order=0), dict(solver_type="midpoint"), dict(solver_type="logrho"), dict(solver_p=object()),
                dict(rescale_betas_zero_snr=True), dict(trained_betas=[0.1] * 1000), dict(final_sigmas_type="denoise_to_zero"),
                dict(timestep_spacing="karras"), dict(no_such_option=1)):
        with pytest.raises(NotImplementedError):
            UniPCMultistepScheduler(**bad)


def test_tables_are_the_dpm_class_s():
    from asva_amd.schedulers import DPMSolverMultistepScheduler

    for kw in (dict(), dict(use_karras_sigmas=True, final_sigmas_type="sigma_min"), dict(timestep_spacing="leading", steps_offset=1),
               dict(timestep_spacing="trailing")):
        u, d = _sched(**kw), DPMSolverMultistepScheduler(**kw)
        u.set_timesteps(17)
        d.set_timesteps(17)
        np.testing.assert_array_equal(u.sigmas, d.sigmas)
        assert u.timesteps.tolist() == d.timesteps.tolist()


def test_step_table_writer_round_trips(tmp_path):
    """plan.export_steps: the table tools/plan_host.cpp's denoise_unipc reads (88 bytes per step)"""
    from asva_amd import plan

    s = _sched(solver_order=3, disable_corrector=[2])
    s.set_timesteps(7)
    plans = [s.plan_step(i) for i in range(7)]
    path = tmp_path / "steps_unipc.bin"
    plan.export_steps(str(path), s.timesteps.tolist(), plans)
    raw = path.read_bytes()
    assert len(raw) == 7 * 88
    f32 = lambda vs: np.array(vs, dtype=np.float32)  # noqa: E731
    for i, p in enumerate(plans):
        v = struct.unpack_from("<7f3i4i8f", raw, 88 * i)
        assert v[0] == float(s.timesteps[i])
        np.testing.assert_array_equal(f32(v[1:7]), f32([p.s_x, p.s_e, p.cc_last, p.cc_cur, p.cp_x, p.cp_cur]))
        nh = len(p.hist_idx)
        assert v[7:10] == (int(p.use_corrector), p.store_slot, nh)
        assert list(v[10:10 + nh]) == list(p.hist_idx) and all(x == 0 for x in v[10 + nh:14])
        np.testing.assert_array_equal(f32(v[14:14 + nh]), f32(p.wc))
        np.testing.assert_array_equal(f32(v[18:18 + nh]), f32(p.wp))
        assert all(x == 0.0 for x in v[14 + nh:18] + v[18 + nh:22])


@pytest.mark.parametrize("tg,ag", [(1.0, 4.0), (7.5, 4.0)])
def test_engine_loop_equals_reference_style_loop_unipc(emu, monkeypatch, tg, ag):   # noqa: F811
    """test_dpmsolver_cpu.py::test_engine_loop_equals_reference_style_loop_dpmsolver for UniPC-2: the fused engine (plan_step + one
    avsd_guided_unipc per step) and the reference-style loop (`step()` on frames 1..), audio-only and dual guidance"""
    from asva_amd.schedulers import UniPCMultistepScheduler, UniPCPlan

    monkeypatch.setattr(emu_ops, "guided_unipc", guided_unipc, raising=False)
    g = load_golden("unet_tiny_e2e.pt")
    c = _clip(g, seed=1)
    pipe, _, _ = _pipe(g, UniPCMultistepScheduler())
    pipe.null_text_encoding = torch.randn(1, *c["text"].shape[1:], generator=torch.Generator().manual_seed(5))
    kw = dict(texts=[""], text_encodings=[c["text"]], video_length=c["f"], height=c["hw"][0], width=c["hw"][1], num_inference_steps=6,
              audio_guidance_scale=ag, text_guidance_scale=tg, image_latents=c["image_latents"], audio_encodings=c["audio"],
              null_audio_encodings=c["null_audio"], audio_masks=c["mask"], noise=c["noise"], output_latents=True)
    fused = pipe(**kw)
    assert len(pipe._engine._plans) == 6 and all(isinstance(p, UniPCPlan) for p in pipe._engine._plans)   # the engine ran it
    assert sum(p.use_corrector for p in pipe._engine._plans) == 5
    pipe.use_engine = False
    looped = pipe(**kw)
    assert torch.equal(fused[:, :, 0], looped[:, :, 0])
    err = rel_l2(fused, looped)
    print(f"UniPC-2 bh2, 6 steps, tg {tg} ag {ag}: engine vs reference-style loop rel-L2 {err:.3e}")
    assert err < 2e-2


def test_guided_unipc_argument_errors_without_a_device():
    from asva_amd import _lib

    h = _lib.lib()
    idx, wc, wp = (ctypes.c_int32 * 4)(), (ctypes.c_float * 4)(), (ctypes.c_float * 4)()
    coef = (1, 1.0, -0.5, 0.9, 0.1, 0.8, 0.2, 1, 4, 12, 1024, None)
    assert h.avsd_guided_unipc(None, 2, 4.0, 0.0, None, -1, idx, wc, wp, 0, None, None, None, *coef) == -1
    assert b"guided_unipc: null pointer" in h.avsd_last_error()
    buf = (ctypes.c_float * 8)()                   # host memory: every check below fails before anything is launched
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 16
    assert h.avsd_guided_unipc(a, 2, 4.0, 0.0, None, -1, idx, wc, wp, 0, a, b, a, *coef) == -1
    assert b"x_last must not alias" in h.avsd_last_error()
    assert h.avsd_guided_unipc(a, 2, 4.0, 0.0, None, -1, idx, wc, wp, 0, a, b, b, *coef) == -1
    assert b"x_last must not alias" in h.avsd_last_error()
    assert h.avsd_guided_unipc(a, 4, 4.0, 0.0, None, -1, idx, wc, wp, 0, a, a, b, *coef) == -1
    assert b"n_branch" in h.avsd_last_error()
    assert h.avsd_guided_unipc(a, 2, 4.0, 0.0, None, -1, idx, wc, wp, 5, a, a, b, *coef) == -1
    assert b"n_hist" in h.avsd_last_error()
    assert h.avsd_guided_unipc(a, 2, 4.0, 0.0, None, 0, idx, wc, wp, 0, a, a, b, *coef) == -1
    assert b"history requested without hist" in h.avsd_last_error()
