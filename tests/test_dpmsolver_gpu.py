"""DPM-Solver++ on the MI355X (-m gpu): avsd_guided_multistep against its contract in float64, the engine with and without graph
replay, 20 steps through the engine against the fp32 oracle UNet driven by the scheduler's object protocol, an SD1.5-shaped clip
through AudioCondAnimationPipeline, and tools/plan_host.cpp running the DPM-Solver++ loop without Python."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import filled_unet, load_golden, rel_l2
from tests.test_dpmsolver_cpu import guided_multistep as contract

pytestmark = pytest.mark.gpu
TOL_NORTH_STAR = 1e-3     # BASELINE.json: "outputs within 1e-3 rel-L2 of reference"


def _f32(v):
    return float(np.float32(v))


@pytest.mark.parametrize("n_branch,store,hist_idx", [(1, -1, ()), (1, 0, (1,)), (2, 1, (0, 3)), (3, 2, (2, 0, 1)), (2, 3, (1, 2, 0, 3))])
@pytest.mark.parametrize("inplace", [False, True])
def test_guided_multistep_kernel_matches_float64(n_branch, store, hist_idx, inplace):
    """n_branch 1 / 2 / 3, a store slot outside and inside hist_idx (read back from registers), in place and out of place,
    B = 2 and HW = 35 (not a multiple of 4)"""
    from asva_amd import ops

    B, C, F, H, W = 2, 4, 5, 5, 7
    gen = torch.Generator().manual_seed(10 * n_branch + store + 3)
    npred = torch.randn(n_branch * B, C, F, H, W, generator=gen)
    x = torch.randn(B, C, F, H, W, generator=gen)
    hist = torch.randn(4, B, C, F, H, W, generator=gen)
    w = tuple(_f32(v) for v in torch.randn(len(hist_idx), generator=gen))
    coef = dict(ca=_f32(0.93), c_cur=_f32(0.41), s_x=_f32(1.07), s_e=_f32(-0.38))
    g, g2 = 4.0, 2.5
    use_hist = store >= 0 or bool(hist_idx)
    want, want_hist = torch.empty_like(x, dtype=torch.float64), hist.double()
    contract(npred.double(), n_branch, g, x.double(), want, **coef, hist=want_hist, store_slot=store, hist_idx=hist_idx, w=w, g2=g2)
    xd, hd = x.cuda(), hist.cuda()
    out = xd if inplace else torch.empty_like(xd)
    ops.guided_multistep(npred.cuda(), n_branch, g, xd, out, **coef, hist=hd if use_hist else None, store_slot=store,
                         hist_idx=hist_idx, w=w, g2=g2)
    torch.cuda.synchronize()
    err = rel_l2(out[:, :, 1:], want[:, :, 1:])
    assert err < 1e-6, err
    assert torch.equal(out[:, :, 0].cpu(), x[:, :, 0])                     # frame 0 pinned, bit-exact
    for k in range(4):
        if k == store:
            assert rel_l2(hd[k], want_hist[k]) < 1e-6
        else:
            assert torch.equal(hd[k].cpu(), hist[k])                          # other slots untouched


def _tiny(order=2, use_graph=True, unet=None):
    from asva_amd.engine import DenoiseEngine
    from asva_amd.schedulers import DPMSolverMultistepScheduler

    g = load_golden("unet_tiny_e2e.pt")
    unet = unet if unet is not None else filled_unet(g["config"]).to("cuda")
    eng = DenoiseEngine(unet, DPMSolverMultistepScheduler(solver_order=order), audio_guidance_scale=4.0, use_graph=use_graph)
    f = g["sample"].shape[2]
    eng.set_conditioning(g["text"][:1].cuda(), g["audio"][1:2].cuda(), g["audio"][:1].cuda(), g["mask"], f)
    return eng, unet


@pytest.mark.parametrize("order", [2, 3])
def test_engine_graph_replay_is_bit_identical(order):
    g = load_golden("unet_tiny_e2e.pt")
    lat = torch.randn(1, 4, *g["sample"].shape[2:], generator=torch.Generator().manual_seed(4)).cuda()
    eager, unet = _tiny(order, use_graph=False)
    a = eager.run(lat, 8)
    replay, _ = _tiny(order, use_graph=True, unet=unet)
    b = replay.run(lat, 8)
    c = replay.run(lat, 8)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(b, c)
    assert torch.equal(a[:, :, 0], lat[:, :, 0]) and not torch.equal(a, lat) and bool(torch.isfinite(a).all())


def test_dpmsolver_20_steps_through_engine_against_fp32_oracle():
    """The tiny golden UNet in split precision (and bf16) through the engine, DPM++ 2M for 20 steps, audio guidance 4.0, against
    the fp32 oracle UNet (oracle/unet_ref.py) driven by the same class's object protocol with the guidance in torch"""
    from asva_amd import precision as P
    from asva_amd.engine import DenoiseEngine
    from asva_amd.schedulers import DPMSolverMultistepScheduler
    from oracle.unet_ref import unet_forward

    g = load_golden("unet_tiny_e2e.pt")
    f, h, w = g["sample"].shape[2:]
    lat = torch.randn(1, 4, f, h, w, generator=torch.Generator().manual_seed(7))
    lat[:, :, 0] *= 0.18215
    text, audio, null_audio = g["text"][:1], g["audio"][1:2], g["audio"][:1]
    ref_unet = filled_unet(g["config"])
    sd, cfg = {k: v.clone() for k, v in ref_unet.state_dict().items()}, dict(ref_unet.config)
    sch = DPMSolverMultistepScheduler()
    sch.set_timesteps(20)
    txt = torch.cat([text, text])[:, None].expand(-1, f, -1, -1)
    aud = torch.cat([null_audio, audio])[:, None].expand(-1, f, -1, -1)
    m = g["mask"][None].expand(2, -1, -1)
    want = lat.clone()
    for t in sch.timesteps:
        n0, n1 = unet_forward(sd, cfg, torch.cat([want, want]), int(t), txt, aud, m).chunk(2)
        eps = n0 + 4.0 * (n1 - n0)
        want[:, :, 1:] = sch.step(eps[:, :, 1:], t, want[:, :, 1:]).prev_sample
    errs = {}
    for mode in ("bf16x2", "bf16"):
        P.set_split(mode == "bf16x2")
        try:
            eng = DenoiseEngine(filled_unet(g["config"]).to("cuda"), DPMSolverMultistepScheduler(), audio_guidance_scale=4.0)
            eng.set_conditioning(text.cuda(), audio.cuda(), null_audio.cuda(), g["mask"], f)
            got = eng.run(lat.cuda(), 20)
            torch.cuda.synchronize()
        finally:
            P.set_split(False)
        assert torch.equal(got[:, :, 0].cpu(), lat[:, :, 0])
        errs[mode] = rel_l2(got, want)
    print("DPM++ 2M, 20 steps, engine vs fp32 oracle loop: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["bf16x2"] < TOL_NORTH_STAR
    assert errs["bf16"] < 2.6e-2       # regression guard, 1.5 x the measured 1.76e-2 (split precision: 2.4e-5)


def test_sd15_clip_through_pipeline_dpmsolver_20_steps():
    """An SD1.5-shaped 12 x 32 x 32 clip through AudioCondAnimationPipeline with DPM++ 2M, 20 steps, audio guidance 4.0: the fused
    engine (hipGraph replay + one avsd_guided_multistep per step) and the reference-style loop"""
    from asva_amd.conditioning import audio_segment_mask
    from asva_amd.pipeline import AudioCondAnimationPipeline, synthetic_clip
    from asva_amd.schedulers import DPMSolverMultistepScheduler
    from tests.test_configs_gpu import _cfg

    dev = torch.device("cuda")
    pipe = AudioCondAnimationPipeline(unet=filled_unet(_cfg()), scheduler=DPMSolverMultistepScheduler(), vae=None).to(dev)
    pipe.set_progress_bar_config(disable=True)
    c = synthetic_clip(0, device=dev)
    kw = dict(texts=[""], text_encodings=[c["text_encodings"][None]], image_latents=c["image_latents"][None], noise=c["noise"][None],
              audio_encodings=c["audio_encodings"][None], null_audio_encodings=c["null_audio_encodings"][None],
              audio_masks=audio_segment_mask(12), num_inference_steps=20, audio_guidance_scale=4.0, output_latents=True)
    fused = pipe(**kw)
    assert fused.shape == (1, 4, 12, 32, 32) and bool(torch.isfinite(fused).all())
    assert torch.equal(fused[:, :, 0], c["image_latents"][None])
    pipe.use_engine = False
    looped = pipe(**kw)
    err = rel_l2(fused, looped)
    print(f"SD1.5-shaped clip, DPM++ 2M 20 steps: engine vs reference-style loop rel-L2 {err:.3e}")
    assert err < 2e-2                  # measured 1.73e-2: the engine's shared guidance prefix sums rows in another f32 order
                                       # (test_pipeline_gpu.py::_pipeline_vs_oracle explains it); the tile choice is deterministic


@pytest.mark.parametrize("graph", ["0", "1"])
def test_cpp_host_runs_the_dpmsolver_loop_without_python(tmp_path, graph):
    """test_plan_gpu.py::test_cpp_host_runs_the_denoising_loop_without_python for DPM++ 2M, 20 steps: the table written by
    plan.export_steps, plan_host's `denoise_ms` — latents byte-identical to the Python engine's"""
    from asva_amd import _lib, build, plan
    from asva_amd.engine import DenoiseEngine
    from asva_amd.schedulers import DPMSolverMultistepScheduler
    from tests.test_plan_gpu import _bytes, _record

    assert os.path.exists(build.PLAN_HOST), "asva_amd/plan_host not built (python -m asva_amd.build)"
    r = _record(tmp_path, "ddim", steps=2)
    g, lat0 = r["g"], r["lat0"]
    eng = DenoiseEngine(r["unet"], DPMSolverMultistepScheduler(), audio_guidance_scale=4.0, use_graph=False)
    eng.set_conditioning(g["text"][:1].cuda(), g["audio"][1:2].cuda(), g["audio"][:1].cuda(), g["mask"], lat0.shape[2])
    want = eng.run(lat0, 20)
    torch.cuda.synchronize()
    plan.export_steps(str(tmp_path / "steps_ms.bin"), eng._ts.tolist(), eng._plans)
    for name, tns in (("text", r["text"]), ("audio", r["audio"]), ("latents", lat0)):
        _bytes(tns).cpu().numpy().tofile(str(tmp_path / f"{name}.in"))
    b, c, f, h, w = r["shape"]
    prog = tmp_path / "program.txt"
    prog.write_text(
        f"load text {tmp_path}/text.in\nload audio {tmp_path}/audio.in\nload latents {tmp_path}/latents.in\n"
        "run set_conditioning\n"
        f"denoise_ms {tmp_path}/steps_ms.bin latents x t noise_pred 2 4.0 0.0 {b} {c} {f} {h * w}\n"
        f"save latents {tmp_path}/latents.out\n")
    out = subprocess.run([build.PLAN_HOST, _lib.LIB_PATHS["bf16"], r["path"], str(prog)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PLAN_HOST_GRAPH=graph))
    print(out.stdout[-600:], out.stderr[-600:])
    assert out.returncode == 0
    assert "20 denoising steps" in out.stdout
    got = torch.from_numpy(np.fromfile(str(tmp_path / "latents.out"), dtype=np.float32)).reshape(r["shape"])
    assert torch.equal(got, want.cpu()), f"max |diff| {float((got - want.cpu()).abs().max()):.3e}"
    assert torch.equal(got[:, :, 0], lat0[:, :, 0].cpu())
