"""CLIP text encoder and tokenizer without a GPU (-m "not gpu"): the tokenizer against transformers' ids, the torch restatement
(tests/clip_text_ref.py) against transformers' outputs, the model's state-dict surface and guards, and the argument checks of the
attention entry point.  Fixtures: tests/golden/clip_text/ (tools/gen_clip_text_golden.py).

Bound of the restatement check: the rel-L2 distance of the restatement's fp32 run to its own float64 run, times 4, as the generator
measured and stored it (meta.json, bound_rel_l2)."""
import json
import os

import pytest
import torch

from tests import clip_text_ref as R
from tests.helpers import GOLDEN

DIR = os.path.join(GOLDEN, "clip_text")


@pytest.fixture(scope="module")
def fixture():
    return torch.load(os.path.join(DIR, "encoder.pt"), map_location="cpu", weights_only=True)


# ---- tokenizer ---------------------------------------------------------------------------------------------------------------------
def test_tokenizer_matches_transformers_ids():
    from asva_amd.text_encoder import CLIPTokenizer

    with open(os.path.join(DIR, "tokenizer_cases.json"), encoding="utf-8") as f:
        cases = json.load(f)
    tok = CLIPTokenizer.from_pretrained(DIR, subfolder="tokenizer")
    assert tok.model_max_length == 77 and tok.pad_token_id == tok.eos_token_id == cases["eos_token_id"] and tok.bos_token_id == cases["bos_token_id"]
    out = tok(cases["strings"], padding="max_length", max_length=77, truncation=True, return_tensors="pt")
    assert out.input_ids.shape == (len(cases["strings"]), 77) and out.input_ids.dtype == torch.long
    for text, got, want, mask, want_mask in zip(cases["strings"], out.input_ids.tolist(), cases["input_ids"], out.attention_mask.tolist(),
                                                cases["attention_mask"]):
        assert got == want, text
        assert mask == want_mask, text
    long_row = out.input_ids[-1].tolist()
    assert len(tok.tokenize_ids(cases["strings"][-1])) > 75 and long_row[-1] == tok.eos_token_id and long_row[-2] != tok.eos_token_id
    one = tok("", padding="max_length", max_length=77, truncation=True, return_tensors="pt")        # the pipeline's null prompt
    assert one.input_ids.shape == (1, 77) and one.input_ids[0].tolist() == [tok.bos_token_id] + [tok.eos_token_id] * 76


def test_tokenizer_without_regex_gives_the_same_ids(monkeypatch):
    """the module's own fallback: with `regex` made unimportable, _compile_split() takes its ImportError branch and builds the `re`
    pattern"""
    import re
    import sys

    from asva_amd import text_encoder as T

    with open(os.path.join(DIR, "tokenizer_cases.json"), encoding="utf-8") as f:
        cases = json.load(f)
    monkeypatch.setitem(sys.modules, "regex", None)              # `import regex` now raises ImportError
    split, space = T._compile_split()
    assert isinstance(split, re.Pattern) and split.pattern == T._SPLIT_RE
    monkeypatch.setattr(T, "_SPLIT", split)
    monkeypatch.setattr(T, "_SPACE", space)
    tok = T.CLIPTokenizer.from_pretrained(DIR, subfolder="tokenizer")
    out = tok(cases["strings"], padding="max_length", max_length=77, truncation=True, return_tensors="pt")
    assert out.input_ids.tolist() == cases["input_ids"]


# ---- the restatement against transformers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", sorted(R.NETS))
def test_restatement_reproduces_the_transformers_fixture(fixture, net):
    cfg, g = R.NETS[net], fixture["nets"][net]
    meta = fixture["meta"]["nets"][net]
    assert meta["logit_std_min"] >= 1.0                      # the softmax of the fixture is peaked: a masking error is visible
    bound = meta["bound_rel_l2"]
    assert bound == 4.0 * meta["restatement_fp32_vs_float64_rel_l2"]
    sd = R.draw_state_dict(cfg, fixture["seed"])
    for k, (total, head) in g["probe"].items():              # the recipe still draws what the generator drew
        assert abs(sd[k].double().sum().item() - total) <= 1e-9 * max(1.0, abs(total)) and sd[k].double().reshape(-1)[:4].tolist() == head, k
    for key, ids in R.make_ids(cfg, fixture["seed"]).items():
        assert torch.equal(ids, g["ids"][key])
        last = R.forward(sd, cfg, ids, torch.float32)
        err = R.rel_l2(last, g["last"][key])
        print(f"restatement fp32 vs transformers [{net} {key}]: rel-L2 {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (net, key, err, bound)
        assert R.rel_l2(R.pooled(cfg, ids, last), g["pooled"][key]) <= bound
        assert torch.equal(R.pooled(cfg, ids, g["last"][key]), g["pooled"][key])


# ---- model surface -----------------------------------------------------------------------------------------------------------------------
def _small(net="l1"):
    from asva_amd.text_encoder import CLIPTextModel

    m = CLIPTextModel.from_config(R.NETS[net])
    m.load_state_dict(R.draw_state_dict(R.NETS[net]))
    return m


def test_state_dict_surface_matches_transformers():
    from asva_amd.text_encoder import CLIPTextModel

    with open(os.path.join(DIR, "state_dict_shapes.json")) as f:
        shapes = json.load(f)
    shapes = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in shapes.items() if not k.endswith("position_ids")}
    m = CLIPTextModel()                                       # transformers' default CLIPTextConfig
    own = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert own == {"text_model." + k: v for k, v in shapes.items()}      # SD1.5's names
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(v, generator=g) for k, v in shapes.items()}
    for prefix in ("", "text_model."):
        m.load_state_dict({prefix + k: v for k, v in sd.items()})
        assert all(torch.equal(m.state_dict()["text_model." + k], v) for k, v in sd.items())
    m.load_state_dict(dict(sd, **{"embeddings.position_ids": torch.arange(77)[None]}))       # ignored
    m.load_state_dict(dict(sd, **{"text_model.embeddings.position_ids": torch.arange(77)[None]}))
    dropped = "encoder.layers.3.mlp.fc2.bias"
    with pytest.raises(KeyError, match=dropped.replace(".", r"\.")):
        m.load_state_dict({k: v for k, v in sd.items() if k != dropped})
    with pytest.raises(KeyError, match="bogus"):
        m.load_state_dict(dict(sd, bogus=torch.zeros(1)))


@pytest.mark.parametrize("safe", [True, False])
def test_save_and_from_pretrained_round_trip(tmp_path, safe):
    from asva_amd.text_encoder import CLIPTextModel

    m = _small("l2")
    m.save_pretrained(str(tmp_path / "text_encoder"), safe_serialization=safe)
    assert os.path.isfile(tmp_path / "text_encoder" / ("model.safetensors" if safe else "pytorch_model.bin"))
    back = CLIPTextModel.from_pretrained(str(tmp_path), subfolder="text_encoder")
    assert dict(back.config) == dict(m.config) and back.config.eos_token_id == 2 and back.dtype == torch.float32
    a, b = m.state_dict(), back.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(FileNotFoundError):
        os.remove(tmp_path / "text_encoder" / ("model.safetensors" if safe else "pytorch_model.bin"))
        CLIPTextModel.from_pretrained(str(tmp_path), subfolder="text_encoder")


def test_what_is_not_implemented_says_so():
    from asva_amd.text_encoder import CLIPTextModel

    with pytest.raises(NotImplementedError, match="gelu"):
        CLIPTextModel.from_config(dict(R.NETS["l1"], hidden_act="gelu"))
    with pytest.raises(NotImplementedError, match="head dim"):
        CLIPTextModel.from_config(dict(R.NETS["l1"], num_attention_heads=4))          # 128 / 4 = heads of 32
    with pytest.raises(NotImplementedError, match="projection"):
        CLIPTextModel.from_config(dict(R.NETS["l1"], architectures=["CLIPTextModelWithProjection"]))
    m = _small()
    ids = R.make_ids(R.NETS["l1"])["eos10"]
    mask = torch.ones_like(ids)
    mask[0, 11:] = 0
    with pytest.raises(NotImplementedError, match="padding mask"):
        m(ids, attention_mask=mask)
    with pytest.raises(NotImplementedError, match="output_hidden_states"):
        m(ids, output_hidden_states=True)
    with pytest.raises(NotImplementedError, match="max_position_embeddings"):
        m(torch.cat([ids, ids], 1))
    with pytest.raises(ValueError, match="must lie in"):
        m(ids + 1)                                            # 127 + 1 = the table size
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        m(ids)                                                # all ones / no mask passes the guards and reaches pack()


def test_pooled_row_follows_the_eos_rule():
    ids = R.make_ids(R.NETS["l1"])
    want = {"eos1": [1], "eos10": [10], "eos76": [76], "none": [0], "batch3": [10, 0, 1]}
    for net in ("l1", "l2"):
        m = _small(net)
        for key, w in want.items():
            assert m.eos_positions(ids[key]).tolist() == R.eos_positions(R.NETS[net], ids[key]).tolist()
            if net == "l1":
                assert m.eos_positions(ids[key]).tolist() == w


def test_to_keeps_f32_and_module_switch_defaults_off():
    import asva_amd.pipeline as PL
    from avgen.pipelines import pipeline_audio_cond_animation as shim
    from asva_amd import text_encoder as T

    assert PL.native_text_encoder is False
    assert shim.CLIPTextModel is T.CLIPTextModel and shim.CLIPTokenizer is T.CLIPTokenizer
    m = _small()
    assert m.to(torch.float16) is m and m.to(device="cpu", dtype=torch.float16) is m and m.half() is m
    assert all(p.dtype == torch.float32 for p in m.parameters()) and m.dtype == torch.float32 and m.device.type == "cpu"
    pipe = PL.AudioCondAnimationPipeline(text_encoder=m, tokenizer=None)
    pipe.to(torch_device="cpu", dtype=torch.float16)
    assert all(p.dtype == torch.float32 for p in m.parameters())


# ---- argument errors without a device -------------------------------------------------------------------------------------------------
def test_attention_argument_errors_are_reported_without_a_device():
    from asva_amd import _lib

    h = _lib.lib()
    p = 4096                                                  # never dereferenced: every call below is refused before a launch
    assert h.avsd_attention_causal_f32(p, 192, p, 192, p, 192, p, 64, 1, 77, 1, 40, 0.125, None) == -1
    assert b"head dim 64" in h.avsd_last_error()
    assert h.avsd_attention_causal_f32(p, 192, p, 192, p, 192, p, 64, 1, 129, 1, 64, 0.125, None) == -1
    assert b"L <= 128" in h.avsd_last_error()
    assert h.avsd_attention_causal_f32(p, 192, None, 192, p, 192, p, 64, 1, 77, 1, 64, 0.125, None) == -1
    assert b"null pointer" in h.avsd_last_error()
    assert h.avsd_layernorm_f32(p, 64, p, 64, 5, 128, p, p, 1e-5, None) == -1 and b"row strides" in h.avsd_last_error()
    assert h.avsd_quick_gelu_f32(p, p, 0, None) == -1
    assert h.avsd_embed_tokens_f32(None, p, p, p, 1, 77, 128, 128, None) == -1
