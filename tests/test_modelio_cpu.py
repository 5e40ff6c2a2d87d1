"""What the model holders share on the host, without a GPU (-m "not gpu"): the model folders of asva_amd/modelio.py as the five classes
read and write them, the rule that a change of the parameters drops what was packed, the text encoder's pack as a weights.Blob, and
the launch sequence of f32net.run_blocks driven by a torch backend.

Bound of the launch-sequence check, the project's rule: the rel-L2 error against the float64 restatement is at most 4 x the error of
the restatement's own float32 run against float64 - stored for the text nets (tests/golden/clip_text/ meta: bound_rel_l2), computed
here from the restatement at the two dtypes for the towers.  No bound comes from the code under test."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import clip_text_ref as T
from tests import imagebind_ref as I
from tests.helpers import GOLDEN, filled_unet, load_golden
from tests.test_host_cpu import TINY_VAE, _filled_vae

DIFFUSERS = ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin")
TRANSFORMERS = ("model.safetensors", "pytorch_model.bin")

# ---- what each class writes into config.json for the tiny model of this file, written out ------------------------------------------------
UNET_JSON = {
    "_class_name": "AudioUNet3DConditionModel", "_diffusers_version": "0.29.2", "sample_size": 8, "in_channels": 4, "out_channels": 4,
    "center_input_sample": False, "flip_sin_to_cos": True, "freq_shift": 0,
    "down_block_types": ["FFSpatioAudioTempCrossAttnDownBlock3D", "FFSpatioAudioTempCrossAttnDownBlock3D",
                         "FFSpatioAudioTempCrossAttnDownBlock3D", "FFSpatioTempResDownBlock3D"],
    "mid_block_type": "FFSpatioAudioTempCrossAttnUNetMidBlock3D",
    "up_block_types": ["FFSpatioTempResUpBlock3D", "FFSpatioAudioTempCrossAttnUpBlock3D", "FFSpatioAudioTempCrossAttnUpBlock3D",
                       "FFSpatioAudioTempCrossAttnUpBlock3D"],
    "only_cross_attention": False, "block_out_channels": [80, 160, 160, 160], "layers_per_block": 2, "downsample_padding": 1,
    "mid_block_scale_factor": 1, "act_fn": "silu", "norm_num_groups": 16, "norm_eps": 1e-05, "cross_attention_dim": 64,
    "encoder_hid_dim": None, "attention_head_dim": 2, "dual_cross_attention": False, "use_linear_projection": False,
    "class_embed_type": None, "addition_embed_type": None, "num_class_embeds": None, "upcast_attention": False,
    "resnet_time_scale_shift": "default", "resnet_skip_time_act": False, "resnet_out_scale_factor": 1.0,
    "time_embedding_type": "positional", "time_embedding_dim": None, "time_embedding_act_fn": None, "timestep_post_act": None,
    "time_cond_proj_dim": None, "conv_in_kernel": 3, "conv_out_kernel": 3, "projection_class_embeddings_input_dim": None,
    "class_embeddings_concat": False, "mid_block_only_cross_attention": None, "cross_attention_norm": None,
    "addition_embed_type_num_heads": 64, "audio_cross_attention_dim": 64}
VAE_JSON = {
    "_class_name": "AutoencoderKL", "_diffusers_version": "0.29.2", "in_channels": 3, "out_channels": 3,
    "down_block_types": ["DownEncoderBlock2D"] * 4, "up_block_types": ["UpDecoderBlock2D"] * 4, "block_out_channels": [32, 64, 128, 128],
    "layers_per_block": 2, "act_fn": "silu", "latent_channels": 4, "norm_num_groups": 32, "sample_size": 512, "scaling_factor": 0.18215,
    "force_upcast": True}
AUDIO_JSON = {"_class_name": "ImageBindSegmaskAudioEncoder", "_diffusers_version": "0.29.2", "n_segment": 12,
              "pretrained_model_name": "imagebind-huge"}
TEXT_JSON = {
    "architectures": ["CLIPTextModel"], "model_type": "clip_text_model", "vocab_size": 128, "hidden_size": 128, "intermediate_size": 256,
    "projection_dim": 512, "num_hidden_layers": 2, "num_attention_heads": 2, "max_position_embeddings": 77, "hidden_act": "quick_gelu",
    "layer_norm_eps": 1e-05, "attention_dropout": 0.0, "pad_token_id": 127, "bos_token_id": 126, "eos_token_id": 2}
HEAD_JSON = {"_class_name": "FCHead", "dim": 16, "out_dim": 1, "dropout": 0.0}


class _Case:
    """one class with a tiny model of it: `names` = (safetensors, torch.save) file names, `safe_default` what save_pretrained() writes
    when it is not told, `stamps` the keys of config.json that are no setting of the model"""

    def __init__(self, cls, model, want_json, names=DIFFUSERS, safe_default=True, stamps=("_class_name", "_diffusers_version"), **load_kw):
        self.cls, self.model, self.want_json, self.names, self.safe_default, self.stamps, self.load_kw = \
            cls, model, want_json, names, safe_default, stamps, load_kw

    def load(self, folder, **kw):
        return self.cls.from_pretrained(str(folder), **dict(self.load_kw, **kw))


def _seeded(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    model.load_state_dict({k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v) for k, v in model.state_dict().items()})
    return model


@pytest.fixture(scope="module")
def cases():
    import asva_amd.audio_encoder as AE
    from asva_amd import avsync as A
    from asva_amd.text_encoder import CLIPTextModel
    from asva_amd.unet import AudioUNet3DConditionModel
    from asva_amd.vae import AutoencoderKL

    depth, AE.DEPTH = AE.DEPTH, 1                                   # the audio trunk's geometry is fixed: ONE of its twelve blocks
    try:
        audio = AE.ImageBindSegmaskAudioEncoder(n_segment=12).eval()
    finally:
        AE.DEPTH = depth
    text = CLIPTextModel.from_config(T.NETS["l2"])
    text.load_state_dict(T.draw_state_dict(T.NETS["l2"]))
    return {"unet": _Case(AudioUNet3DConditionModel, filled_unet(load_golden("unet_tiny_e2e.pt")["config"]), UNET_JSON),
            "vae": _Case(AutoencoderKL, _filled_vae(TINY_VAE), VAE_JSON),
            "audio": _Case(AE.ImageBindSegmaskAudioEncoder, audio, AUDIO_JSON),
            "text": _Case(CLIPTextModel, text, TEXT_JSON, names=TRANSFORMERS, stamps=("architectures", "model_type"), subfolder=None),
            "head": _Case(A.FCHead, _seeded(A.FCHead(dim=16)).eval(), HEAD_JSON, safe_default=False, stamps=("_class_name",))}


@pytest.fixture()
def one_audio_block(monkeypatch):
    import asva_amd.audio_encoder as AE

    monkeypatch.setattr(AE, "DEPTH", 1)                           # from_pretrained builds the class again


def _same_tensors(a, b):
    a, b = a.state_dict(), b.state_dict()
    return list(a) == list(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)


NAMES = ["unet", "vae", "audio", "text", "head"]


# ---- 1. folder round trips -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("safe", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_folder_round_trip(cases, one_audio_block, tmp_path, name, safe):
    c = cases[name]
    c.model.save_pretrained(str(tmp_path), safe_serialization=safe)
    assert sorted(os.listdir(tmp_path)) == sorted(["config.json", c.names[0 if safe else 1]])
    with open(tmp_path / "config.json") as f:
        text = f.read()
    got = json.loads(text)
    assert got == c.want_json and list(got) == list(c.want_json) and text == json.dumps(c.want_json, indent=2)
    back = c.load(tmp_path)
    settings = {k: (tuple(v) if isinstance(v, list) else v) for k, v in c.want_json.items() if k not in c.stamps}
    assert dict(back.config) == dict(c.model.config) == settings
    assert _same_tensors(back, c.model) and not back.training


@pytest.mark.parametrize("name", NAMES)
def test_default_format_and_subfolder(cases, one_audio_block, tmp_path, name):
    c = cases[name]
    sub = "text_encoder" if name == "text" else "modules"
    c.model.save_pretrained(str(tmp_path / sub))
    assert sorted(os.listdir(tmp_path / sub)) == sorted(["config.json", c.names[0 if c.safe_default else 1]])
    back = c.cls.from_pretrained(str(tmp_path)) if name == "text" else c.cls.from_pretrained(str(tmp_path), subfolder=sub)
    assert _same_tensors(back, c.model)                            # (the text encoder's default subfolder is text_encoder)


def _shifted(model, by):
    return {k: (v + by if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("name", NAMES)
def test_safetensors_wins_over_the_bin_file(cases, one_audio_block, tmp_path, name):
    c = cases[name]
    c.model.save_pretrained(str(tmp_path), safe_serialization=True)
    other = _shifted(c.model, 1.0)
    torch.save(other, tmp_path / c.names[1])
    assert _same_tensors(c.load(tmp_path), c.model)
    if name == "head":                                             # the switch of the AVSync sub-networks
        back = c.load(tmp_path, use_safetensors=False).state_dict()
        assert all(torch.equal(back[k], v) for k, v in other.items())
        assert _same_tensors(c.load(tmp_path, use_safetensors=True), c.model)


def test_text_encoder_finds_each_of_its_four_names_in_order(cases, tmp_path):
    from safetensors.torch import save_file

    c = cases["text"]
    c.model.save_pretrained(str(tmp_path))
    os.remove(tmp_path / TRANSFORMERS[0])
    order = TRANSFORMERS + DIFFUSERS
    for i, file in enumerate(order):                               # file i holds the weights + i
        (save_file if file.endswith(".safetensors") else torch.save)(_shifted(c.model, float(i)), str(tmp_path / file))
    for i, file in enumerate(order):
        back, want = c.load(tmp_path).state_dict(), _shifted(c.model, float(i))
        assert all(torch.equal(back[k], want[k]) for k in want), file
        os.remove(tmp_path / file)
    with pytest.raises(FileNotFoundError) as e:
        c.load(tmp_path)
    assert str(tmp_path) in str(e.value) and all(file in str(e.value) for file in order)


@pytest.mark.parametrize("name", NAMES)
def test_folder_without_weights_raises_file_not_found_naming_it(cases, one_audio_block, tmp_path, name):
    c = cases[name]
    with open(tmp_path / "config.json", "w") as f:
        json.dump(c.want_json, f)
    with pytest.raises(FileNotFoundError) as e:
        c.load(tmp_path)
    assert str(tmp_path) in str(e.value) and all(n in str(e.value) for n in c.names)
    if name == "head":
        open(tmp_path / DIFFUSERS[0], "w").close()                 # only the .safetensors name is there, and that one is barred
        with pytest.raises(FileNotFoundError) as e:
            c.load(tmp_path, use_safetensors=False)
        assert str(tmp_path) in str(e.value) and DIFFUSERS[1] in str(e.value) and DIFFUSERS[0] not in str(e.value)


def test_names_and_scheduler_config(tmp_path):
    from asva_amd import modelio, unet
    from asva_amd.schedulers import _read_config
    from asva_amd.unet import AudioUNet3DConditionModel

    assert (unet.CONFIG_NAME, unet.SAFETENSORS_NAME, unet.BIN_NAME) == ("config.json",) + DIFFUSERS
    assert (modelio.CONFIG_NAME, modelio.SAFETENSORS_NAME, modelio.BIN_NAME) == ("config.json",) + DIFFUSERS
    os.makedirs(tmp_path / "scheduler")
    with open(tmp_path / "scheduler" / "scheduler_config.json", "w") as f:
        json.dump({"_class_name": "PNDMScheduler", "beta_start": 0.00085, "skip_prk_steps": True}, f)
    assert _read_config(str(tmp_path), "scheduler") == {"beta_start": 0.00085, "skip_prk_steps": True}
    assert _read_config(str(tmp_path / "scheduler"), None) == {"beta_start": 0.00085, "skip_prk_steps": True}
    with open(tmp_path / "config.json", "w") as f:
        json.dump(UNET_JSON, f)
    assert AudioUNet3DConditionModel.load_config(str(tmp_path)) == UNET_JSON            # public, and the stamps stay in


# ---- 2. invalidation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", ["load_state_dict", "to", "_invalidate"])
def test_unet_drops_pack_and_conditioning(cases, change):
    m = cases["unet"].model
    m._packed, m._cond, m._cond_key, m._cond_refs = object(), object(), ("key",), (1, 2, 3)
    if change == "load_state_dict":
        m.load_state_dict(m.state_dict())
    elif change == "to":
        assert m.to("cpu") is m
    else:
        m._invalidate()
    assert m._packed is None and m._cond is None and m._cond_key is None and m._cond_refs is None


@pytest.mark.parametrize("name", ["vae", "audio"])
def test_vae_and_audio_encoder_drop_their_pack(cases, name):
    m = cases[name].model
    for change in (lambda: m.load_state_dict(m.state_dict()), lambda: m.to("cpu")):
        m._packed = {"key": "stale"}
        change()
        assert m._packed is None


def test_epoch_grows_on_the_f32_family(cases):
    from asva_amd import avsync as A, f32net, modelio
    from asva_amd.imagebind_eval import CLIPModel

    assert f32net.F32Net._epoch == 0 and A.FCHead._epoch == 0 and "_epoch" not in vars(A.FCHead(dim=16))      # a class-level default
    clip = CLIPModel(I.CONFIGS["t64"])
    clip.load_state_dict(I.draw_state_dict(I.CONFIGS["t64"]))
    for m in (cases["text"].model, cases["head"].model, clip):
        assert isinstance(m, modelio.EpochCounted)
        e0 = m._epoch
        m.load_state_dict(m.state_dict())
        e1 = m._epoch
        assert m.to("cpu") is m
        assert e0 < e1 < m._epoch
    net = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()
    e0 = net._pack_epoch()
    net.head.load_state_dict(net.head.state_dict())                # a sub-network on its own
    e1 = net._pack_epoch()
    net.load_state_dict(net.state_dict())
    e2 = net._pack_epoch()
    net.to("cpu")
    assert e0 < e1 < e2 < net._pack_epoch()


# ---- 3. the text encoder's pack --------------------------------------------------------------------------------------------------------------
def _cpu_pack(model):
    """pack() on the CPU (the kernels cannot read it; the layouts can be checked)"""
    from asva_amd import ops

    ops.EMULATED = True
    try:
        return model.pack("cpu")
    finally:
        del ops.EMULATED


BLOCK_ITEMS = ("n1_g", "n1_b", "in_w", "in_b", "out_w", "out_b", "n2_g", "n2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


def test_text_encoder_pack_is_one_blob_in_the_stated_order(cases):
    m = cases["text"].model
    sd = {k[len("text_model."):]: v for k, v in m.state_dict().items()}
    pk = _cpu_pack(m)
    want = [("tok", sd["embeddings.token_embedding.weight"]), ("pos", sd["embeddings.position_embedding.weight"]),
            ("lnf_g", sd["final_layer_norm.weight"]), ("lnf_b", sd["final_layer_norm.bias"])]
    views = [pk.tok, pk.pos, pk.lnf_g, pk.lnf_b]
    assert len(pk.blocks) == 2
    for i, blk in enumerate(pk.blocks):
        p = f"encoder.layers.{i}."
        src = {"n1_g": sd[p + "layer_norm1.weight"], "n1_b": sd[p + "layer_norm1.bias"],
               "in_w": torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in ("q", "k", "v")]),
               "in_b": torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in ("q", "k", "v")]),
               "out_w": sd[p + "self_attn.out_proj.weight"], "out_b": sd[p + "self_attn.out_proj.bias"],
               "n2_g": sd[p + "layer_norm2.weight"], "n2_b": sd[p + "layer_norm2.bias"], "fc1_w": sd[p + "mlp.fc1.weight"],
               "fc1_b": sd[p + "mlp.fc1.bias"], "fc2_w": sd[p + "mlp.fc2.weight"], "fc2_b": sd[p + "mlp.fc2.bias"]}
        assert tuple(k for k in vars(blk)) == BLOCK_ITEMS
        assert blk.in_w.shape == (384, 128) and blk.in_b.shape == (384,)
        want += [(f"blocks.{i}.{k}", src[k]) for k in BLOCK_ITEMS]
        views += [getattr(blk, k) for k in BLOCK_ITEMS]
    at = 0
    for (name, src), v in zip(want, views):
        assert v.dtype == torch.float32 and v.is_contiguous() and torch.equal(v, src), name
        assert v.untyped_storage().data_ptr() == pk.blob.untyped_storage().data_ptr(), name
        assert v.storage_offset() * 4 == at and at % 256 == 0, name                  # one after the other, 256-byte-aligned items
        at += (v.numel() * 4 + 255) // 256 * 256
    assert pk.blob.numel() * pk.blob.element_size() == at
    assert _cpu_pack(m) is pk
    from asva_amd import precision

    precision.set_precision("fp16")                                # the pack does not follow the storage mode
    try:
        assert _cpu_pack(m) is pk
    finally:
        precision.set_precision("bf16")
    m.load_state_dict(m.state_dict())
    again = _cpu_pack(m)
    assert again is not pk and torch.equal(again.blob, pk.blob)


# ---- 4. the launch sequence under torch ------------------------------------------------------------------------------------------------------
class _Torch:
    """the launches of f32net._HipBase with plain torch ops in the dtype of the operands, each call recorded by name"""

    def __init__(self):
        self.calls = []

    def linear(self, x, w, b=None, res=None):
        self.calls.append("linear")
        y = F.linear(x, w, b)
        return y if res is None else res + y

    def layernorm(self, x, g, b, eps, out=None):
        self.calls.append("layernorm")
        return F.layer_norm(x, (x.shape[1],), g, b, eps)

    def _attend(self, q, k, v, b, seq, heads, causal):
        d = q.shape[1] // heads
        q, k, v = (t.reshape(b, seq, heads, d).transpose(1, 2) for t in (q, k, v))
        logits = (q * d ** -0.5) @ k.transpose(-1, -2)
        if causal:
            logits = logits.masked_fill(~torch.ones(seq, seq, dtype=torch.bool).tril(), float("-inf"))
        return (torch.softmax(logits, dim=-1) @ v).transpose(1, 2).reshape(b * seq, heads * d)

    def attention(self, q, k, v, b, seq, heads):
        self.calls.append("attention")
        return self._attend(q, k, v, b, seq, heads, False)

    def attention_causal(self, q, k, v, b, seq, heads):
        self.calls.append("attention_causal")
        return self._attend(q, k, v, b, seq, heads, True)

    def _pointwise(self, name, fn, x, out):
        self.calls.append(name)
        assert out is x                                            # the activation writes into its input
        return out.copy_(fn(x))

    def gelu(self, x, out=None):
        return self._pointwise("gelu", F.gelu, x, out)

    def quick_gelu(self, x, out=None):
        return self._pointwise("quick_gelu", lambda t: t * torch.sigmoid(1.702 * t), x, out)


def _block_calls(layers, causal, act):
    return ["layernorm", "linear", "attention_causal" if causal else "attention", "linear", "layernorm", "linear", act, "linear"] * layers


@pytest.fixture(scope="module")
def text_meta():
    return torch.load(os.path.join(GOLDEN, "clip_text", "encoder.pt"), map_location="cpu", weights_only=True)["meta"]


@pytest.mark.parametrize("net", ["l1", "l2"])
def test_text_encoder_launch_sequence_under_torch(text_meta, net):
    from asva_amd import f32net
    from asva_amd.text_encoder import CLIPTextModel

    cfg = T.NETS[net]
    sd = T.draw_state_dict(cfg)
    m = CLIPTextModel.from_config(cfg)
    m.load_state_dict(sd)
    pk = _cpu_pack(m)
    bound = text_meta["nets"][net]["bound_rel_l2"]
    assert bound == 4.0 * text_meta["nets"][net]["restatement_fp32_vs_float64_rel_l2"]
    for key, ids in T.make_ids(cfg).items():
        b, seq = ids.shape
        be = _Torch()
        x = (pk.tok[ids] + pk.pos[:seq]).view(b * seq, -1)
        x = f32net.run_blocks(x, pk.blocks, b, seq, cfg["num_attention_heads"], cfg["layer_norm_eps"], causal=True, act="quick_gelu", be=be)
        out = F.layer_norm(x, (x.shape[1],), pk.lnf_g, pk.lnf_b, cfg["layer_norm_eps"]).view(b, seq, -1)
        assert be.calls == _block_calls(cfg["num_hidden_layers"], True, "quick_gelu")
        err = T.rel_l2(out, T.forward(sd, cfg, ids, torch.float64))
        print(f"MEASURED text_{net}_{key} runner-under-torch={err:.4e} bound={bound:.4e}")
        assert out.dtype == torch.float32 and err <= bound, (net, key, err, bound)


def _tower_under_torch(tower, cfg, t, x, be):
    """the encode_* of CLIPModel around the runner, in torch: stem and tokens, blocks, head"""
    from asva_amd import f32net
    from asva_amd.imagebind_eval import EPS, STEM_EPS, n_tokens

    c, causal = cfg["width"], tower == "text"
    if tower == "text":
        n, seq = x.shape
        h = (t.tok[x] + t.pos[:seq]).view(n * seq, c)
        rows = x.argmax(dim=-1)
    else:
        n, seq, p = x.shape[0], n_tokens(tower, cfg), cfg["patch"]
        w = t.stem_w.view(c, p, p, -1).permute(0, 3, 1, 2)         # tap-major, channels-last -> conv2d's layout
        emb = F.conv2d(x, w, stride=p if tower == "vision" else cfg["stride"]).flatten(2).transpose(1, 2)
        if tower == "audio":
            emb = F.layer_norm(emb, (c,), t.stem_g, t.stem_b, STEM_EPS)
        h = torch.cat([t.cls.expand(n, 1, c), emb], dim=1) + t.pos
        if tower == "vision":
            h = F.layer_norm(h, (c,), t.pre_g, t.pre_b, EPS)
        else:
            h, seq = torch.cat([h, torch.zeros(n, 1, c)], dim=1), seq + 1          # the spare row of the bias_kv slot
        h, rows = h.reshape(n * seq, c), torch.zeros(n, dtype=torch.long)
    h = f32net.run_blocks(h, t.blocks, n, seq, cfg["heads"], EPS, causal=causal, be=be)
    assert be.calls == _block_calls(cfg["layers"], causal, "gelu")
    e = F.linear(F.layer_norm(h.view(n, seq, c)[torch.arange(n), rows], (c,), t.head_g, t.head_b, EPS), t.head_w)
    return F.normalize(e, dim=-1)


@pytest.mark.parametrize("name", ["t64", "v64", "a1"])
def test_tower_launch_sequence_under_torch(name):
    from asva_amd.imagebind_eval import CLIPModel

    config = I.CONFIGS[name]
    (tower, cfg), = config.items()
    sd, x = I.draw_state_dict(config), I.make_inputs(name)
    x = x["ids"] if tower == "text" else x["images"] if tower == "vision" else x["audios"]
    restated = {"text": I.encode_text, "vision": I.encode_image, "audio": I.encode_audio}[tower]
    ref32, ref64 = restated(sd, cfg, x, torch.float32), restated(sd, cfg, x, torch.float64)
    m = CLIPModel(config)
    m.load_state_dict(sd)
    t = getattr(_cpu_pack(m), tower)
    assert (tower == "audio") == hasattr(t.blocks[0], "bias_kv")
    with torch.no_grad():
        out = _tower_under_torch(tower, cfg, t, x, _Torch())
    e_ref, err = I.rel_l2(ref32, ref64), I.rel_l2(out, ref64)
    print(f"MEASURED tower_{name} e_ref={e_ref:.4e} runner-under-torch={err:.4e}")
    assert out.dtype == torch.float32 and out.shape == ref64.shape and err <= 4.0 * e_ref, (name, err, e_ref)
    if tower == "audio":                                           # the appended pair is seen: without it the bound is missed
        assert I.rel_l2(I.encode_audio(sd, cfg, x, torch.float64, bias_kv=False), ref64) > 4.0 * e_ref
