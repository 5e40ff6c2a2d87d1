"""CLIP text encoder on the MI355X (asva_amd/text_encoder.py, csrc/clip_text.hip), in both builds of the library.

Truth is float64 (torch on the CPU; for whole networks the restatement tests/clip_text_ref.py, which tests/test_clip_text_cpu.py pins to
transformers).  Tolerance rule for every f32 kernel: e_ref = rel-L2 error against float64 of torch's fp32 CPU result for the same
input; the kernel's rel-L2 error against float64 must stay within 4 x e_ref (the factor covers another summation order and another
exp).  No bound comes from what the kernels give.  Each test prints `MEASURED <name> e_ref=<..> kernel=<..>`
(run with -s).
"""
import os
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import clip_text_ref as R
from tests.helpers import GOLDEN, ROOT, filled_unet, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIR = os.path.join(GOLDEN, "clip_text")


@pytest.fixture(params=["bf16", "fp16"])
def build(request):
    """the library the test runs in; a library that is not built is a build failure, not missing hardware"""
    from asva_amd import _lib, precision

    assert os.path.isfile(_lib.LIB_PATHS[request.param]), f"the {request.param} library is not built"
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


def _within(name, got, ref32, ref64, factor=4.0):
    e_ref, e_k = R.rel_l2(ref32, ref64), R.rel_l2(got, ref64)
    print(f"MEASURED {name} e_ref={e_ref:.4e} kernel={e_k:.4e}")
    assert e_k <= factor * e_ref, (name, e_k, e_ref)
    return e_ref, e_k


@pytest.fixture(scope="module")
def fixture():
    return torch.load(os.path.join(DIR, "encoder.pt"), map_location="cpu", weights_only=True)


_NETS = {}


def _net(name):
    """the seeded small nets (and "sd15": the SD1.5 shape with the vocabulary cut to 1024), built once"""
    from asva_amd.text_encoder import CLIPTextModel

    if name not in _NETS:
        cfg = R.SD15 if name == "sd15" else R.NETS[name]
        sd = R.draw_state_dict(cfg)
        m = CLIPTextModel.from_config(cfg)
        m.load_state_dict(sd)
        _NETS[name] = (cfg, sd, m.to(DEV))
    return _NETS[name]


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------
def test_embed_is_exact(build):
    from asva_amd import ops

    g = torch.Generator().manual_seed(0)
    b, L, c, v = 2, 77, 128, 128
    tok, pos = torch.randn(v, c, generator=g), torch.randn(L, c, generator=g)
    ids = torch.randint(0, v, (b, L), generator=g)
    ids[0, 0], ids[1, -1] = 0, v - 1
    out = ops.embed_tokens_f32(ids.to(torch.int32).view(-1).to(DEV), tok.to(DEV), pos.to(DEV), b, L)
    assert torch.equal(out.cpu().view(b, L, c), tok[ids] + pos)


@pytest.mark.parametrize("c", [128, 768])
def test_layernorm_rows_of_a_wider_buffer_with_a_large_mean(build, c):
    from asva_amd import ops

    g = torch.Generator().manual_seed(c)
    wide = torch.randn(5, c + 64, generator=g) + 100.0          # rows with mean 100 and standard deviation 1
    gamma, beta = 1.0 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    x = wide[:, 32:32 + c]
    ref32 = F.layer_norm(x, (c,), gamma, beta, 1e-5)
    ref64 = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), 1e-5)
    wd = wide.to(DEV)
    out = ops.layernorm_f32(wd[:, 32:32 + c], gamma.to(DEV), beta.to(DEV), 1e-5)
    _within(f"layernorm_c{c}", out, ref32, ref64)
    assert torch.equal(wd.cpu(), wide)                          # the columns around the slice are untouched
    xs = wd[:, 32:32 + c]
    assert torch.equal(ops.layernorm_f32(xs, gamma.to(DEV), beta.to(DEV), 1e-5, out=xs), out)      # in place, into the slice
    assert torch.equal(wd[:, :32].cpu(), wide[:, :32]) and torch.equal(wd[:, 32 + c:].cpu(), wide[:, 32 + c:])


def test_quick_gelu_in_place_with_extreme_values(build):
    from asva_amd import ops

    n = 77 * 256 + 3
    x = 3.0 * torch.randn(n, generator=torch.Generator().manual_seed(3))
    x[:8] = torch.tensor([100.0, -100.0, 1e4, -1e4, 0.0, -0.0, 50.0, -50.0])
    ref32 = x * torch.sigmoid(1.702 * x)
    ref64 = x.double() * torch.sigmoid(1.702 * x.double())
    xd = x.to(DEV)
    out = ops.quick_gelu_f32(xd, out=xd)
    assert out.data_ptr() == xd.data_ptr() and bool(torch.isfinite(out).all())
    _within("quick_gelu", out, ref32, ref64)
    assert out[:4].cpu().tolist() == [100.0, 0.0, 1e4, 0.0]


def _attn_inputs(b, L, seed=0):
    g = torch.Generator().manual_seed(seed + L)
    buf = torch.randn(b * L, 384, generator=g)
    buf[:, :128] *= 1.5                                          # a peaked softmax: logits of standard deviation ~ 1.5
    return buf


def _attn_ref(buf, b, L, dtype):
    q, k, v = (buf[:, i * 128:(i + 1) * 128].to(dtype).view(b, L, 2, 64).transpose(1, 2) for i in range(3))
    keep = torch.ones(L, L, dtype=torch.bool).tril()
    logits = ((q * 64 ** -0.5) @ k.transpose(-1, -2)).masked_fill(~keep, float("-inf"))
    return (torch.softmax(logits, -1) @ v).transpose(1, 2).reshape(b * L, 128)


def _attn(buf, b, L):
    from asva_amd import ops

    return ops.attention_causal_f32(buf[:, :128], buf[:, 128:256], buf[:, 256:], b, L, 2)


@pytest.mark.parametrize("L", [1, 31, 32, 33, 77])
def test_causal_attention_against_float64(build, L):
    b = 2
    buf = _attn_inputs(b, L)
    out = _attn(buf.to(DEV), b, L)
    assert out.shape == (b * L, 128)
    if L == 1:                                                   # one key: the output is V itself
        assert torch.equal(out.cpu(), buf[:, 256:])
        return
    _within(f"attention_L{L}", out, _attn_ref(buf, b, L, torch.float32), _attn_ref(buf, b, L, torch.float64))


@pytest.mark.parametrize("L,cut", [(77, 40), (33, 31)])
def test_causal_attention_never_reads_the_future(build, L, cut):
    """rows j > cut of K and V of sequence 0 replaced by values of magnitude 1e4: rows <= cut of sequence 0 and all of sequence 1 keep
    their bits"""
    b = 2
    buf = _attn_inputs(b, L).to(DEV)
    base = _attn(buf, b, L)
    poisoned = buf.clone()
    sign = torch.where(torch.arange(256, device=DEV) % 2 == 0, 1.0, -1.0)
    poisoned[cut + 1:L, 128:] = 1e4 * sign
    out = _attn(poisoned, b, L)
    assert torch.equal(out[:cut + 1], base[:cut + 1]) and torch.equal(out[L:], base[L:])
    assert not torch.equal(out[cut + 1:L], base[cut + 1:L])       # the later rows do see them


@pytest.mark.parametrize("L", [33, 77])
def test_causal_attention_is_batch_invariant_and_deterministic(build, L):
    buf = _attn_inputs(3, L).to(DEV)
    full = _attn(buf, 3, L)
    assert torch.equal(full, _attn(buf, 3, L))
    for s in range(3):
        assert torch.equal(_attn(buf[s * L:(s + 1) * L], 1, L), full[s * L:(s + 1) * L])


# ---- the whole model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["l1", "l2"])
def test_small_nets_reproduce_the_transformers_fixture(build, fixture, net):
    cfg, sd, m = _net(net)
    g = fixture["nets"][net]
    for key, ids in g["ids"].items():
        out = m(ids.to(DEV))
        assert out[0].shape == (ids.shape[0], 77, 128) and out[0].dtype == torch.float32 and out[1].shape == (ids.shape[0], 128)
        assert out[0] is out.last_hidden_state and out[1] is out.pooler_output
        ref32, ref64 = R.forward(sd, cfg, ids, torch.float32), R.forward(sd, cfg, ids, torch.float64)
        e_ref, _ = _within(f"{net}_{key}_last_hidden_state", out[0], ref32, ref64)
        _within(f"{net}_{key}_pooler_output", out[1], R.pooled(cfg, ids, ref32), R.pooled(cfg, ids, ref64))
        # the fixture is transformers' own fp32 run: the same bound around it
        d_last, d_pool = R.rel_l2(out[0], g["last"][key]), R.rel_l2(out[1], g["pooled"][key])
        print(f"{net} {key} [{build}] vs transformers: last_hidden_state {d_last:.3e}, pooler_output {d_pool:.3e}")
        assert d_last <= 4.0 * e_ref and d_pool <= 4.0 * R.rel_l2(R.pooled(cfg, ids, ref32), R.pooled(cfg, ids, ref64))
        assert torch.equal(out[1], out[0][torch.arange(ids.shape[0]), R.eos_positions(cfg, ids).to(DEV)])


def test_both_builds_and_any_batch_give_the_same_bits(fixture):
    from asva_amd import _lib

    assert all(os.path.isfile(p) for p in _lib.LIB_PATHS.values()), "needs both the bf16 and the fp16 library"
    for net in ("l1", "l2"):
        _, _, m = _net(net)
        ids = fixture["nets"][net]["ids"]
        batch = ids["batch3"].to(DEV)                              # rows: eos10, none, eos1

        def run():
            return [t.clone() for t in m(batch)]

        a, b = _in_build("bf16", run), _in_build("fp16", run)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for row, key in enumerate(("eos10", "none", "eos1")):
            alone = m(ids[key].to(DEV))
            assert torch.equal(alone[0][0], a[0][row]) and torch.equal(alone[1][0], a[1][row])


def test_sd15_shape_against_float64_restatement(build):
    """12 layers, C = 768, 12 heads, intermediate 3072 (vocabulary cut to 1024): the launch shapes of the real encoder, M = 77,
    N = 2304 / 768 / 3072"""
    cfg, sd, m = _net("sd15")
    ids = R.make_ids(cfg)["eos10"]
    out = m(ids.to(DEV))[0]
    assert out.shape == (1, 77, 768)
    _within("sd15_last_hidden_state", out, R.forward(sd, cfg, ids, torch.float32), R.forward(sd, cfg, ids, torch.float64))


def test_recorded_forward_replays_bit_identically(tmp_path):
    from asva_amd import plan

    cfg, _, m = _net("l2")
    ids = R.make_ids(cfg)["batch3"]
    pk = m.pack(DEV)
    dev_ids = ids.to(torch.int32).contiguous().view(-1).to(DEV)
    want = m.encode_ids(dev_ids, 3, 77).clone()
    rec = plan.Recorder()
    rec.region("weights", pk.blob, plan.CONST)
    rec.region("ids", dev_ids, plan.INPUT)
    with rec.record("encode_text"):
        out = m.encode_ids(dev_ids, 3, 77)
    rec.region("hidden", out, plan.OUTPUT)
    assert torch.equal(out, want)
    b = rec.save(str(tmp_path / "text.plan"))
    assert b.n_calls["encode_text"] == 1 + 2 * 8 + 1               # embed, 8 launches per layer, final LayerNorm
    b.bind_fresh(torch.device(DEV))                                # new zero-filled buffers; only the weights are loaded
    b.view("ids").copy_(dev_ids.view(torch.uint8))
    b.run("encode_text")
    torch.cuda.synchronize()
    assert torch.equal(b.view("hidden"), want.reshape(-1).view(torch.uint8))
    b.close()


# ---- pipeline and tool ---------------------------------------------------------------------------------------------------------------------
def _tiny_text_stack():
    from asva_amd.text_encoder import CLIPTextModel, CLIPTokenizer

    tok = CLIPTokenizer.from_pretrained(DIR, subfolder="tokenizer")
    tok.model_max_length = 7                                       # the tiny UNet's golden text has 7 tokens of width 64
    cfg = dict(R.SMALL, vocab_size=len(tok), hidden_size=64, intermediate_size=128, num_attention_heads=1, num_hidden_layers=1,
               eos_token_id=tok.eos_token_id, bos_token_id=tok.bos_token_id, pad_token_id=tok.pad_token_id)
    enc = CLIPTextModel.from_config(cfg)
    enc.load_state_dict(R.draw_state_dict(cfg))
    return tok, enc


@pytest.mark.parametrize("text_scale", [1.0, 2.0])
def test_pipeline_with_native_tokenizer_and_encoder(text_scale):
    from asva_amd.pipeline import AudioCondAnimationPipeline
    from asva_amd.schedulers import PNDMScheduler
    from tests.test_host_cpu import TINY_VAE, _filled_vae

    g = load_golden("unet_tiny_e2e.pt")
    f, h, w = g["sample"].shape[2:]
    gen = torch.Generator().manual_seed(0)
    il, noise = torch.randn(1, 4, h, w, generator=gen) * 0.18215, torch.randn(1, 4, f - 1, h, w, generator=gen)
    tok, enc = _tiny_text_stack()
    pipe = AudioCondAnimationPipeline(text_encoder=enc, tokenizer=tok, unet=filled_unet(g["config"]), scheduler=PNDMScheduler(),
                                      vae=_filled_vae(TINY_VAE))
    pipe.to(torch_device="cuda", dtype=torch.float16)             # what generate_videos_for_dataset does; the encoder stays f32
    assert enc.device.type == "cuda" and all(p.dtype == torch.float32 for p in enc.parameters())
    pipe.set_progress_bar_config(disable=True)
    kw = dict(video_length=f, height=h * 8, width=w * 8, num_inference_steps=3, audio_guidance_scale=4.0, text_guidance_scale=text_scale,
              image_latents=il, audio_encodings=g["audio"][1:2], null_audio_encodings=g["audio"][:1], audio_masks=g["mask"], noise=noise,
              output_latents=True)
    prompt = "the dog is barking"
    ids = tok([prompt], padding="max_length", max_length=7, truncation=True, return_tensors="pt").input_ids
    encodings = enc(ids)[0]
    assert encodings.shape == (1, 7, 64) and encodings.dtype == torch.float32
    a = pipe(texts=[prompt], **kw)
    b = pipe(texts=[prompt], text_encodings=encodings, **kw)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    c = pipe(texts=["hammering"], **kw)
    assert not torch.equal(a, c)                                   # the prompt reaches the latents


def test_encode_text_tool_writes_the_dataset_files(tmp_path):
    from asva_amd.text_encoder import CLIPTextModel, CLIPTokenizer

    cfg = R.NETS["l1"]
    sd15 = tmp_path / "sd15"
    shutil.copytree(os.path.join(DIR, "tokenizer"), sd15 / "tokenizer")
    tok = CLIPTokenizer.from_pretrained(str(sd15))
    cfg = dict(cfg, vocab_size=len(tok), eos_token_id=tok.eos_token_id, bos_token_id=tok.bos_token_id, pad_token_id=tok.pad_token_id)
    enc = CLIPTextModel.from_config(cfg)
    enc.load_state_dict(R.draw_state_dict(cfg))
    enc.save_pretrained(str(sd15 / "text_encoder"))
    prompts = ["dog barking", "hammering"]
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tools", "encode_text.py"), "--sd15", str(sd15), "--out",
                        str(tmp_path / "classes.pt"), "--null-out", str(tmp_path / "null.pt"), *prompts], capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    classes = torch.load(tmp_path / "classes.pt", map_location="cpu", weights_only=True)
    null = torch.load(tmp_path / "null.pt", map_location="cpu", weights_only=True)
    enc = enc.to(DEV)
    want = enc(tok(prompts + [""], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids)[0].cpu()
    assert list(classes) == prompts and all(v.shape == (77, 128) and v.dtype == torch.float32 for v in classes.values())
    assert torch.equal(classes["dog barking"], want[0]) and torch.equal(classes["hammering"], want[1]) and torch.equal(null, want[2])
