"""CLIPSim / AlignSync without a device (asva_amd/imagebind_eval.py): the restatement tests/imagebind_ref.py pinned to transformers in
float64, the stem fold, the metric arithmetic on hand-computed values, the checkpoint loader and the argument contract."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import imagebind_ref as R
from tests.helpers import GOLDEN


# ---- the written key mapping: ImageBind checkpoint names -> transformers' CLIP*ModelWithProjection ------------------------------------
def _hf_blocks(sd, src, dst, layers, c):
    out = {}
    for i in range(layers):
        s, d = f"{src}.blocks.{i}.", f"{dst}.encoder.layers.{i}."
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):              # in_proj = q | k | v rows
            out[d + f"self_attn.{n}.weight"] = sd[s + "attn.in_proj_weight"][j * c:(j + 1) * c]
            out[d + f"self_attn.{n}.bias"] = sd[s + "attn.in_proj_bias"][j * c:(j + 1) * c]
        for a, b in (("attn.out_proj", "self_attn.out_proj"), ("norm_1", "layer_norm1"), ("norm_2", "layer_norm2"), ("mlp.fc1", "mlp.fc1"),
                     ("mlp.fc2", "mlp.fc2")):
            out[d + b + ".weight"], out[d + b + ".bias"] = sd[s + a + ".weight"], sd[s + a + ".bias"]
    return out


def _hf_vision(sd, cfg):
    c = cfg["width"]
    w3 = sd["modality_preprocessors.vision.rgbt_stem.proj.1.weight"].double()      # (the fold summed in float64, as the Conv3d sums)
    out = {"vision_model.embeddings.class_embedding": sd["modality_preprocessors.vision.cls_token"].reshape(c),
           "vision_model.embeddings.patch_embedding.weight": w3[:, :, 0] + w3[:, :, 1],          # the Conv3d stem folded into a Conv2d
           "vision_model.embeddings.position_embedding.weight": sd["modality_preprocessors.vision.pos_embedding_helper.pos_embed"][0],
           "vision_model.pre_layrnorm.weight": sd["modality_trunks.vision.pre_transformer_layer.0.weight"],
           "vision_model.pre_layrnorm.bias": sd["modality_trunks.vision.pre_transformer_layer.0.bias"],
           "vision_model.post_layernorm.weight": sd["modality_heads.vision.0.weight"],
           "vision_model.post_layernorm.bias": sd["modality_heads.vision.0.bias"],
           "visual_projection.weight": sd["modality_heads.vision.2.weight"]}
    out.update(_hf_blocks(sd, "modality_trunks.vision", "vision_model", cfg["layers"], c))
    return out


def _hf_text(sd, cfg):
    out = {"text_model.embeddings.token_embedding.weight": sd["modality_preprocessors.text.token_embedding.weight"],
           "text_model.embeddings.position_embedding.weight": sd["modality_preprocessors.text.pos_embed"][0],
           "text_model.final_layer_norm.weight": sd["modality_heads.text.proj.0.weight"],
           "text_model.final_layer_norm.bias": sd["modality_heads.text.proj.0.bias"],
           "text_projection.weight": sd["modality_heads.text.proj.1.weight"]}
    out.update(_hf_blocks(sd, "modality_trunks.text", "text_model", cfg["layers"], cfg["width"]))
    return out


def _load_hf(model, mapped):
    own = model.state_dict()
    extra = {k: v for k, v in own.items() if k.endswith("position_ids")}
    assert set(own) - set(extra) == set(mapped), (set(own) - set(extra)) ^ set(mapped)
    model = model.double().eval()          # (sdpa attention: transformers' eager path forms its softmax in float32 whatever the dtype)
    model.load_state_dict({**{k: v.double() for k, v in mapped.items()}, **extra})
    return model


@pytest.mark.parametrize("name", ["v80", "v64"])
def test_vision_restatement_equals_transformers_in_float64(name):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    cfg = R.CONFIGS[name]["vision"]
    sd = R.draw_state_dict(R.CONFIGS[name])
    hf = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=cfg["width"], intermediate_size=cfg["mlp"], projection_dim=cfg["out"],
                                                        num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                                                        image_size=cfg["image"], patch_size=cfg["patch"], hidden_act="gelu",
                                                        layer_norm_eps=1e-6, attn_implementation="sdpa"))
    hf = _load_hf(hf, _hf_vision(sd, cfg))
    images = torch.randn(3, 3, cfg["image"], cfg["image"], generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with torch.no_grad():
        want = F.normalize(hf(pixel_values=images).image_embeds, dim=-1)
    got = R.encode_image(sd, cfg, images, torch.float64)
    assert got.shape == (3, cfg["out"]) and R.rel_l2(got, want) < 1e-10


def test_text_restatement_equals_transformers_in_float64():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection

    cfg = R.CONFIGS["t64"]["text"]
    sd = R.draw_state_dict(R.CONFIGS["t64"])
    top = cfg["vocab"] - 1                                   # eos_token_id = the largest id: transformers' pooling = the argmax rule
    hf = CLIPTextModelWithProjection(CLIPTextConfig(vocab_size=cfg["vocab"], hidden_size=cfg["width"], intermediate_size=cfg["mlp"],
                                                    projection_dim=cfg["out"], num_hidden_layers=cfg["layers"],
                                                    num_attention_heads=cfg["heads"], max_position_embeddings=cfg["positions"],
                                                    hidden_act="gelu", layer_norm_eps=1e-6, eos_token_id=top, bos_token_id=top - 1,
                                                    pad_token_id=top, attn_implementation="sdpa"))
    hf = _load_hf(hf, _hf_text(sd, cfg))
    ids = R.make_ids(cfg)
    with torch.no_grad():
        want = F.normalize(hf(input_ids=ids).text_embeds, dim=-1)
    got = R.encode_text(sd, cfg, ids, torch.float64)
    assert got.shape == (4, cfg["out"]) and R.rel_l2(got, want) < 1e-10


def test_text_restatement_on_tokenised_strings():
    """strings through the project's tokenizer and the synthetic vocabulary: the largest id is <|endoftext|>, so the argmax rule picks the
    first end-of-text, as transformers' pooling does"""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection

    from asva_amd.text_encoder import CLIPTokenizer

    tok = CLIPTokenizer.from_pretrained(os.path.join(GOLDEN, "clip_text"), subfolder="tokenizer")
    assert tok.eos_token_id == len(tok) - 1
    cfg = dict(R.CONFIGS["t64"]["text"], vocab=len(tok))
    sd = R.draw_state_dict({"text": cfg})
    ids = tok(["the dog is barking", "hammering", ""], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    hf = CLIPTextModelWithProjection(CLIPTextConfig(vocab_size=cfg["vocab"], hidden_size=cfg["width"], intermediate_size=cfg["mlp"],
                                                    projection_dim=cfg["out"], num_hidden_layers=cfg["layers"],
                                                    num_attention_heads=cfg["heads"], max_position_embeddings=77, hidden_act="gelu",
                                                    layer_norm_eps=1e-6, eos_token_id=tok.eos_token_id, bos_token_id=tok.bos_token_id,
                                                    pad_token_id=tok.pad_token_id, attn_implementation="sdpa"))
    hf = _load_hf(hf, _hf_text(sd, cfg))
    with torch.no_grad():
        want = F.normalize(hf(input_ids=ids).text_embeds, dim=-1)
    assert R.rel_l2(R.encode_text(sd, cfg, ids, torch.float64), want) < 1e-10


def _cpu_pack(model):
    """CLIPModel.pack() on the CPU (the kernels cannot read it; the layouts can be checked)"""
    from asva_amd import ops

    ops.EMULATED = True
    try:
        return model.pack("cpu")
    finally:
        del ops.EMULATED


def test_packed_stem_fold_is_exact_against_the_conv3d_on_the_repeated_image():
    from asva_amd.imagebind_eval import CLIPModel

    cfg = R.CONFIGS["v80"]["vision"]
    sd = R.draw_state_dict(R.CONFIGS["v80"])
    m = CLIPModel(R.CONFIGS["v80"])
    m.load_state_dict(sd)
    w = _cpu_pack(m).vision.stem_w                                               # [C, 14 * 14 * 3], tap-major and channels-last
    assert w.shape == (cfg["width"], 14 * 14 * 3) and w.dtype == torch.float32
    images = torch.randn(2, 3, 56, 56, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want = R.vision_stem({"stem_w": sd["modality_preprocessors.vision.rgbt_stem.proj.1.weight"].double()}, cfg, images)     # (2, 16, C)
    patches = images.permute(0, 2, 3, 1).unfold(1, 14, 14).unfold(2, 14, 14)     # (n, 4, 4, 3, 14, 14)
    rows = patches.permute(0, 1, 2, 4, 5, 3).reshape(2, 16, 14 * 14 * 3)
    got = rows @ w.double().t()
    # the fold itself rounds w0 + w1 to f32 once (2^-24 relative per weight); everything else is float64
    assert R.rel_l2(got, want) < 2.0 ** -23
    w3 = sd["modality_preprocessors.vision.rgbt_stem.proj.1.weight"]
    assert torch.equal(w.view(cfg["width"], 14, 14, 3).permute(0, 3, 1, 2), w3[:, :, 0] + w3[:, :, 1])


def test_metric_arithmetic_on_hand_computed_values():
    e = 2.718281828459045
    ia = torch.tensor([[0.0, 0.0, 0.0], [0.2, 0.2, 1.2], [0.5, -0.5, 0.5]], dtype=torch.float64)
    rel = torch.tensor([1.0, 0.5, 0.8], dtype=torch.float64)
    want = torch.tensor([0.5, 0.5 * 0.5 * (0.5 + 1.0 / (1.0 + 1.0 / e)), 0.8 * 0.5 * (1.0 / (1.0 + e) + 0.5)], dtype=torch.float64)
    assert torch.allclose(R.alignsync_from_sims(ia, rel), want, atol=1e-15)
    from asva_amd.imagebind_eval import alignsync_from_sims

    assert torch.allclose(alignsync_from_sims(ia, rel), want, atol=1e-15)
    x = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]], dtype=torch.float64)
    y = torch.tensor([[4.0, 3.0], [1.0, 1.0], [-2.0, 0.0]], dtype=torch.float64)
    assert torch.allclose(R.cosine(x, y), torch.tensor([0.96, 0.0, -1.0], dtype=torch.float64), atol=1e-15)


def test_restated_clip_consistency_broadcasts_each_clips_audio_and_text():
    """(b, f) similarities: frame j of clip i against clip i's audio and text, by hand from the encoders"""
    config = R.CONFIGS["tiny"]
    sd = R.draw_state_dict(config)
    g = torch.Generator().manual_seed(3)
    videos = torch.rand(2, 3, 3, 40, 56, generator=g, dtype=torch.float64)
    audios = torch.randn(2, 1, 128, 204, generator=g, dtype=torch.float64)
    ids = R.make_ids(config["text"])[:2]
    out = R.compute_clip_consistency(sd, config, videos, audios, ids, torch.float64)
    img = R.encode_image(sd, config["vision"], R.preprocess(videos, 56), torch.float64).view(2, 3, -1)
    aud, txt = R.encode_audio(sd, config["audio"], audios, torch.float64), R.encode_text(sd, config["text"], ids, torch.float64)
    assert out["ia_sim"].shape == (2, 3) and out["it_sim"].shape == (2, 3)
    for i in range(2):
        for j in range(3):
            assert abs(out["ia_sim"][i, j] - img[i, j] @ aud[i]) < 1e-12 and abs(out["it_sim"][i, j] - img[i, j] @ txt[i]) < 1e-12
    # AlignSync: ground-truth frame 0, predicted frames 1..
    ref = torch.rand(2, 3, 3, 40, 56, generator=g, dtype=torch.float64)
    rel = torch.tensor([0.25, 0.75], dtype=torch.float64)
    got = R.compute_alignsync(sd, config, audios, videos.transpose(1, 2), ref.transpose(1, 2), rel, torch.float64)
    mixed = torch.cat([ref[:, :1], videos[:, 1:]], dim=1)
    ia = R.compute_clip_consistency(sd, config, mixed, audios, dtype=torch.float64)["ia_sim"]
    want = torch.stack([torch.sigmoid(ia[:, k] - ia[:, 0]) for k in (1, 2)], dim=1).mean(1) * rel
    assert torch.allclose(got, want, atol=1e-14)


def test_loader_builds_the_towers_the_checkpoint_holds():
    from asva_amd.imagebind_eval import CLIPModel, load_clip_model, state_dict_shapes

    config = R.CONFIGS["tiny"]
    sd = R.draw_state_dict(config)
    assert {k: list(v.shape) for k, v in sd.items()} == state_dict_shapes(config)
    full = dict(sd, **{"modality_trunks.depth.blocks.0.norm_1.weight": torch.zeros(4)})          # other modalities are ignored
    m = load_clip_model(full, config=config)
    assert sorted(m.config) == ["audio", "text", "vision"] and set(m.state_dict()) == set(sd)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert m.to(dtype=torch.float32) is m and m.to("cpu", torch.float32) is m
    with pytest.raises(ValueError, match="float32 only"):
        m.to(dtype=torch.float16)
    gone = "modality_trunks.vision.blocks.1.mlp.fc2.bias"
    with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
        load_clip_model({k: v for k, v in sd.items() if k != gone}, config=config)
    two = load_clip_model({k: v for k, v in sd.items() if ".text." not in k}, config=config)
    assert sorted(two.config) == ["audio", "vision"]
    with pytest.raises(RuntimeError, match="text tower is not built"):
        two.encode_text(torch.zeros(1, 77, dtype=torch.long))
    with pytest.raises(KeyError, match="vision"):
        load_clip_model({k: v for k, v in sd.items() if ".vision." not in k}, config=config)
    with pytest.raises(ValueError, match="expected"):
        CLIPModel(config).load_state_dict(dict(sd, **{gone: torch.zeros(3)}))
    pk = _cpu_pack(m)
    assert pk.audio.blocks[0].bias_kv.shape == (128,) and pk.text.pos.shape == (77, 128) and pk.vision.cls.shape == (160,)
    assert _cpu_pack(m) is pk
    m.load_state_dict(sd)
    assert _cpu_pack(m) is not pk                                                # repacked after a load


def test_contract_of_the_entry_points():
    from asva_amd import avsync as A
    from asva_amd.imagebind_eval import CLIPModel

    wave, clip = torch.zeros(1, 32000), torch.zeros(3, 12, 8, 8)
    with pytest.raises(NotImplementedError, match="ImageBind.*clip_net=load_clip_model"):
        A.compute_sync_metrics_on_av(wave, 16000, clip, ref_video=clip, metric="alignsync")
    with pytest.raises(ValueError, match="ref_video is needed"):
        A.compute_sync_metrics_on_av(wave, 16000, clip, metric="alignsync", clip_net=object())
    m = CLIPModel(R.CONFIGS["t64"])
    with pytest.raises(ValueError, match="tokenizer"):
        m.encode_text(["a dog"])
    with pytest.raises(RuntimeError, match="vision tower is not built"):
        m.encode_image(torch.zeros(1, 3, 56, 56))
    with pytest.raises(NotImplementedError, match="head dims"):
        CLIPModel({"vision": dict(R.CONFIGS["v80"]["vision"], width=96)})


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    from asva_amd import _lib

    h = _lib.lib()
    p = 4096                                             # never dereferenced: every call below is refused before any launch
    att = lambda q, ld, d, **k: h.avsd_attention_f32(q, ld, p, ld, p, ld, p, k.get("ldo", ld), 2, 33, 2, d, 0.125, None)  # noqa: E731
    assert att(None, 384, 64) == -1 and b"null" in h.avsd_last_error()
    assert att(p, 384, 48) == -1 and b"head dims 64 and 80" in h.avsd_last_error()
    assert att(p, 124, 64) == -1 and b"at least heads * d = 128" in h.avsd_last_error()
    assert att(p, 480, 80, ldo=156) == -1 and b"at least heads * d = 160" in h.avsd_last_error()
    assert att(p, 130, 64) == -1 and b"multiple of 4" in h.avsd_last_error()
    assert h.avsd_attention_f32(p, 384, p, 384, p, 384, p, 384, 2, 0, 2, 64, 0.125, None) == -1 and b"L >= 1" in h.avsd_last_error()
    assert h.avsd_gelu_f32(p, None, 8, None) == -1 and b"null" in h.avsd_last_error()
    assert h.avsd_gelu_f32(p, p, 0, None) == -1 and b"positive" in h.avsd_last_error()
    assert h.avsd_vit_tokens_f32(p, None, p, p, 1, 4, 8, 0, None) == -1 and b"null" in h.avsd_last_error()
    assert h.avsd_vit_tokens_f32(p, p, p, p, 1, 4, 8, -1, None) == -1 and b"bad sizes" in h.avsd_last_error()
    assert h.avsd_cosine_rows_f32(p, p, None, 12, 8, 3, None) == -1 and b"null" in h.avsd_last_error()
    assert h.avsd_cosine_rows_f32(p, p, p, 12, 8, 5, None) == -1 and b"must divide" in h.avsd_last_error()
    assert h.avsd_normalize_rows_f32(None, p, 2, 8, None) == -1 and b"null" in h.avsd_last_error()
    assert h.avsd_normalize_rows_f32(p, p, 0, 8, None) == -1 and b"positive" in h.avsd_last_error()


def test_shim_paths_import_the_same_objects():
    import avgen.evaluations.avsync.compute_avsync as S
    import avgen.evaluations.clip as C
    import avgen.evaluations.clip.compute_clip as CC
    import avgen.evaluations.models.clip as M
    from asva_amd import imagebind_eval as E

    assert M.CLIPModel is E.CLIPModel and M.load_clip_model is E.load_clip_model
    assert C.compute_clip_consistency is E.compute_clip_consistency and C.preprocess_videos is E.preprocess_videos
    assert CC.compute_clip_consistency is E.compute_clip_consistency and CC.preprocess_videos is E.preprocess_videos
    assert S.compute_alignsync is E.compute_alignsync and S.load_clip_model is E.load_clip_model
