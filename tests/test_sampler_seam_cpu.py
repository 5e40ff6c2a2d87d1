"""The sampler seam: what the four schedulers plan, what each plan launches and what it writes into a plan table, pinned bit for
bit against tests/golden/sampler_plans.json.  That file was recorded from the schedulers, DenoiseEngine.step and the three plan
exporters as they stood before the samplers moved onto one base and the plans learnt to launch and record themselves
(floats as float.hex(), tensors and table lines as hex bytes), so every comparison here is exact.  One configuration per class
is kept in full, to be read; every other one is kept as the SHA-256 of the same JSON text, which pins the same bits."""
import dataclasses
import hashlib
import itertools
import json
import os
import types

import pytest
import torch

from asva_amd import schedulers as S

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "sampler_plans.json")
CLASSES = {"pndm": S.PNDMScheduler, "ddim": S.DDIMScheduler, "dpm": S.DPMSolverMultistepScheduler, "unipc": S.UniPCMultistepScheduler}
SHAPE = (1, 4, 3, 5, 5)


def enc(v):
    """JSON form with nothing lost: floats as float.hex()"""
    if isinstance(v, float):
        return v.hex()
    if isinstance(v, (tuple, list)):
        return [enc(x) for x in v]
    if isinstance(v, dict):
        return {k: enc(x) for k, x in v.items()}
    assert v is None or isinstance(v, (bool, int, str)), type(v)
    return v


def _solvers():
    for order, kind in itertools.product((1, 2, 3), ("midpoint", "heun")):
        yield "dpm", dict(solver_order=order, solver_type=kind)
    for order, kind in itertools.product((1, 2, 3), ("bh1", "bh2")):
        yield "unipc", dict(solver_order=order, solver_type=kind)
        yield "unipc", dict(solver_order=order, solver_type=kind, disable_corrector=(0,))


def grid():
    """(class, options, steps).  PNDM / DDIM at 4, 7, 20 steps; every multistep solver (order x type, UniPC also with the first
    corrector off, at 7 steps) with and without Karras sigmas at 4, 7, 20 steps; and, at 7 steps, every solver with the corrector on across
    final_sigmas_type x timestep_spacing, and with Karras sigmas ending on sigma_min.  The full product of all options would not
    fit a committed file."""
    for steps in (4, 7, 20):
        yield "pndm", {}, steps
        yield "pndm", dict(cur_sample_aliases_latents=False), steps
        yield "ddim", {}, steps
        for (name, kw), karras in itertools.product(_solvers(), (False, True)):
            if "disable_corrector" not in kw or steps == 7:
                yield name, dict(kw, use_karras_sigmas=karras), steps
    for name, kw in _solvers():
        if "disable_corrector" in kw:
            continue
        for final, spacing in itertools.product(("zero", "sigma_min"), ("linspace", "leading", "trailing")):
            if (final, spacing) != ("zero", "linspace"):
                yield name, dict(kw, use_karras_sigmas=False, final_sigmas_type=final, timestep_spacing=spacing), 7
        yield name, dict(kw, use_karras_sigmas=True, final_sigmas_type="sigma_min"), 7       # Karras sigmas replace the spacing


def key(name, kw, steps):
    return f"{name} {json.dumps(kw, sort_keys=True)} {steps}"


def digest(v) -> str:
    """SHA-256 of the JSON text of `v`, key order included"""
    return hashlib.sha256(json.dumps(v, separators=(",", ":")).encode()).hexdigest()


def pinned(got, want) -> bool:
    """`want` is the recorded value itself or, where the file keeps only that, its digest"""
    return digest(got) == want if isinstance(want, str) else (got == want and digest(got) == digest(want))


def describe(s, steps, record=lambda p, t: p.record(t)):
    s.set_timesteps(steps)
    plans = [s.plan_step(i) for i in range(s.num_forwards())]
    out = dict(timesteps=s.timesteps.tolist(), config=enc(s.config), plan=type(plans[0]).__name__,
               fields=[f.name for f in dataclasses.fields(plans[0])], plans=[enc(dataclasses.astuple(p)) for p in plans],
               records=[record(p, t).hex() for t, p in zip(s.timesteps.tolist(), plans)])
    if getattr(s, "sigmas", None) is not None:
        out["sigmas"] = [float(v).hex() for v in s.sigmas]
    return out


def drive(s, steps):
    """the object protocol the way the reference-style loop uses it: the result is written back into the sample's own storage"""
    g = torch.Generator().manual_seed(steps)
    x = torch.randn(SHAPE, generator=g)
    s.set_timesteps(steps)
    shas = []
    for t in s.timesteps:
        x.copy_(s.step(torch.randn(SHAPE, generator=g), t, x).prev_sample)
        shas.append(hashlib.sha256(x.numpy().tobytes()).hexdigest())
    return dict(sha256=shas, final=x.numpy().tobytes().hex())


def drive_grid():
    for name, kw, steps in grid():
        if steps == 7 and "final_sigmas_type" not in kw:
            yield name, kw, steps
    yield "dpm", dict(solver_order=3, final_sigmas_type="sigma_min", use_karras_sigmas=True), 7
    yield "unipc", dict(solver_order=3, final_sigmas_type="sigma_min", use_karras_sigmas=True), 7


LAUNCHES = [("pndm", {}, 6), ("pndm", dict(cur_sample_aliases_latents=False), 4), ("ddim", {}, 3), ("dpm", dict(solver_order=3), 5),
            ("unipc", dict(solver_order=3), 5)]
LAUNCH_ARGS = (3, 7.5, 4.0)          # n_branch, g, g2


class Recorder:
    """stands in for the ops module: keeps (function, positional, keyword) of every call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append([name, enc(a), enc(k)])


def from_config_cases():
    for src in ("pndm", "dpm"):
        for dst in CLASSES:
            yield src, dst


def from_config(src, dst, build=lambda cls, cfg: cls.from_config(cfg)):
    try:
        s = build(CLASSES[dst], CLASSES[src]().config)
    except NotImplementedError:
        return dict(raises="NotImplementedError")
    s.set_timesteps(7)
    return dict(config=enc(s.config), timesteps=s.timesteps.tolist())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_grid_is_the_recorded_one(golden):
    assert sorted(golden["grid"]) == sorted(key(*c) for c in grid())
    assert sorted(golden["drive"]) == sorted(key(*c) for c in drive_grid())


@pytest.mark.parametrize("name", list(CLASSES))
def test_plans_tables_and_records_are_bit_identical(golden, name, tmp_path):
    from asva_amd import plan

    n = 0
    for cls, kw, steps in grid():
        if cls != name:
            continue
        s = CLASSES[cls](**kw)
        got = describe(s, steps)
        assert pinned(got, golden["grid"][key(cls, kw, steps)]), key(cls, kw, steps)          # values, and key order too
        # the file export_steps writes is those lines, whatever the plan type
        path = tmp_path / f"steps{n}.bin"
        plan.export_steps(str(path), s.timesteps.tolist(), [s.plan_step(i) for i in range(s.num_forwards())])
        assert path.read_bytes().hex() == "".join(got["records"])
        n += 1
    assert n >= 3          # DDIM: one configuration at three step counts


@pytest.mark.parametrize("name", list(CLASSES))
def test_object_protocol_is_bit_identical(golden, name):
    n = 0
    for cls, kw, steps in drive_grid():
        if cls != name:
            continue
        got, want = drive(CLASSES[cls](**kw), steps), golden["drive"][key(cls, kw, steps)]
        assert pinned(got, want), key(cls, kw, steps)
        if not isinstance(want, str):
            assert got["sha256"] == want["sha256"], key(cls, kw, steps)
            assert torch.equal(torch.frombuffer(bytearray.fromhex(got["final"]), dtype=torch.float32),
                               torch.frombuffer(bytearray.fromhex(want["final"]), dtype=torch.float32)), key(cls, kw, steps)
        n += 1
    assert n >= 1


@pytest.mark.parametrize("name,kw,steps", LAUNCHES)
def test_plan_launch_issues_the_engines_calls(golden, name, kw, steps):
    """p.launch(ops, ...) makes the calls DenoiseEngine.step made for that plan: same function, same positional and keyword values,
    the copy of save_sample and the choice of the saved sample over the latents included"""
    s = CLASSES[name](**kw)
    s.set_timesteps(steps)
    bufs = types.SimpleNamespace(_hist="@hist", _saved="@saved", _x_last="@x_last")
    got = []
    for i in range(s.num_forwards()):
        rec = Recorder()
        assert s.plan_step(i).launch(rec, "@noise", *LAUNCH_ARGS, "@latents", bufs) is None
        got.append(rec.calls)
    want = golden["launch"][key(name, kw, steps)]
    assert got == want
    if kw.get("cur_sample_aliases_latents") is False:
        assert want[0][0][:2] == ["copy", ["@latents", "@saved"]] and want[1][0][1][3] == "@saved"


def test_engine_step_is_unet_then_launch(monkeypatch):
    import asva_amd.engine as E

    rec = Recorder()
    monkeypatch.setattr(E, "ops", rec)
    s = S.UniPCMultistepScheduler(solver_order=2)
    s.set_timesteps(4)
    eng = E.DenoiseEngine.__new__(E.DenoiseEngine)
    eng.n_branch, eng.g, eng.g2 = LAUNCH_ARGS
    eng._plans = [s.plan_step(i) for i in range(4)]
    eng._ts = torch.arange(4.0)
    eng._hist, eng._saved, eng._x_last = "@hist", "@saved", "@x_last"
    seen = []
    eng.unet_step = lambda latents, t: seen.append((latents, t.tolist())) or "@noise"
    eng.step("@latents", 2)
    assert seen == [("@latents", [2.0])]
    want = Recorder()
    eng._plans[2].launch(want, "@noise", *LAUNCH_ARGS, "@latents", eng)
    assert rec.calls == want.calls and [c[0] for c in rec.calls] == ["guided_unipc"]


@pytest.mark.parametrize("src,dst", list(from_config_cases()))
def test_from_config_is_bit_identical(golden, src, dst):
    assert from_config(src, dst) == golden["from_config"][f"{src}->{dst}"]


class _Foreign:
    """a scheduler from elsewhere: the object protocol and nothing of the plan seam"""

    def __init__(self):
        self._s = S.PNDMScheduler()
        self.init_noise_sigma = self._s.init_noise_sigma

    timesteps = property(lambda self: self._s.timesteps)

    def set_timesteps(self, n, device=None):
        self._s.set_timesteps(n, device=device)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, *a, **k):
        return self._s.step(*a, **k)


def test_foreign_scheduler_takes_the_reference_style_loop(monkeypatch):
    from tests.helpers import load_golden
    from tests.test_pipeline_cpu import _clip, _pipe
    import asva_amd.engine as e
    import asva_amd.unet as u
    import asva_amd.vae as v
    from tests import emu_ops

    for m in (e, u, v):
        monkeypatch.setattr(m, "ops", emu_ops)
    g = load_golden("unet_tiny_e2e.pt")
    c = _clip(g, seed=1)
    kw = dict(texts=[""], text_encodings=[c["text"]], video_length=c["f"], height=c["hw"][0], width=c["hw"][1],
              num_inference_steps=2, audio_guidance_scale=4.0, image_latents=c["image_latents"], audio_encodings=c["audio"],
              null_audio_encodings=c["null_audio"], audio_masks=c["mask"], noise=c["noise"], output_latents=True)
    pipe, _, _ = _pipe(g, _Foreign())
    assert pipe.use_engine
    monkeypatch.setattr(pipe, "_engine_for", lambda *a: pytest.fail("a scheduler without plan_step went to the engine"))
    loops = []
    loop = pipe._reference_style_loop
    monkeypatch.setattr(pipe, "_reference_style_loop", lambda *a: loops.append(1) or loop(*a))
    foreign = pipe(**kw)
    assert loops == [1]
    with pytest.raises(ValueError, match="animate_track: runs on the DenoiseEngine, which has no plan for _Foreign"):
        pipe.animate_track(image_latents=c["image_latents"], audio_encodings=c["audio"])
    pipe.scheduler, pipe.use_engine = S.PNDMScheduler(), False         # the same loop, asked for by name
    assert torch.equal(foreign, pipe(**kw))
