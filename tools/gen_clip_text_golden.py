"""Writes the fixtures of the CLIP text encoder and tokenizer (asva_amd/text_encoder.py) by running transformers' own CLIPTextModel and
CLIPTokenizer in fp32 on the CPU:

    python tools/gen_clip_text_golden.py

CPU only, needs transformers, never run on the GPU machine.  The files under tests/golden/clip_text/ hold tensors, names, shapes and
numbers only:

    encoder.pt                  ids (EOS at position 1, 10, 76, nowhere; a batch of 3) and transformers' last_hidden_state and
                                pooler_output for the two small seeded nets of tests/clip_text_ref.py (weights are re-drawn from the
                                recipe in the tests, a probe of every tensor is stored), and the meta figures
    meta.json                   the same meta figures, readable: logit spread, fp32-vs-float64 distance of the restatement, bounds
    state_dict_shapes.json      names and shapes of a default-config CLIPTextModel (for the surface test)
    tokenizer/                  a synthetic vocab.json / merges.txt / tokenizer_config.json
    tokenizer_cases.json        strings and the ids transformers returns for them (padding="max_length", max_length=77, truncation)

The generator refuses to write a fixture that could not see a wrong kernel (see the assertions in main()).
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import clip_text_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "clip_text")

MERGES = [("t", "h"), ("th", "e</w>"), ("i", "n"), ("in", "g</w>"), ("a", "n"), ("an", "d</w>"), ("o", "g</w>"), ("d", "og</w>"),
          ("e", "r"), ("b", "a"), ("r", "k"), ("ba", "rk"), ("'", "s</w>"), ("Ã", "±")]
STRINGS = ["a dog barking", "The  Dog   is BARKING and\tthe baby  laughing", "hello, world!!! (really?) -- yes.", "it's the dog's bark; they'll say I'm done, he'd've",
           "the 3rd of 12 hammers, 1000x", "un café crème and a naïve piñata", "", "   ", "underscore_and__more ~^ $5",
           "hammering " * 60 + "the end"]


def tokenizer_fixture():
    from transformers import CLIPTokenizer

    sys.path.insert(0, ROOT)
    from asva_amd.text_encoder import bytes_to_unicode

    sym = list(bytes_to_unicode().values())
    tokens = sym + [s + "</w>" for s in sym] + [a + b for a, b in MERGES] + ["<|startoftext|>", "<|endoftext|>"]
    assert len(set(tokens)) == len(tokens)
    vocab = {t: i for i, t in enumerate(tokens)}
    tdir = os.path.join(OUT, "tokenizer")
    os.makedirs(tdir, exist_ok=True)
    with open(os.path.join(tdir, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    with open(os.path.join(tdir, "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in MERGES))
    with open(os.path.join(tdir, "tokenizer_config.json"), "w") as f:
        json.dump(dict(model_max_length=77, bos_token="<|startoftext|>", eos_token="<|endoftext|>", pad_token="<|endoftext|>",
                       unk_token="<|endoftext|>"), f, indent=1)
    tok = CLIPTokenizer(vocab=vocab, merges=[tuple(m) for m in MERGES], model_max_length=77)
    assert tok.pad_token_id == tok.eos_token_id == vocab["<|endoftext|>"]
    enc = tok(STRINGS, padding="max_length", max_length=77, truncation=True, return_tensors="pt")
    ids, mask = enc.input_ids.tolist(), enc.attention_mask.tolist()
    assert all(len(r) == 77 for r in ids) and ids[-1][-1] == tok.eos_token_id and sum(mask[-1]) == 77
    merged = {vocab[a + b] for a, b in MERGES}
    assert any(i in merged for r in ids for i in r), "no merge fired: the BPE loop is not exercised"
    with open(os.path.join(OUT, "tokenizer_cases.json"), "w", encoding="utf-8") as f:
        json.dump(dict(strings=STRINGS, input_ids=ids, attention_mask=mask, eos_token_id=tok.eos_token_id, bos_token_id=tok.bos_token_id,
                       pad_token_id=tok.pad_token_id), f, ensure_ascii=True)


def hf_model(cfg, sd):
    from transformers import CLIPTextConfig, CLIPTextModel

    m = CLIPTextModel(CLIPTextConfig(**cfg)).eval()
    own = m.state_dict()
    pre = "text_model." if any(k.startswith("text_model.") for k in own) else ""
    missing, unexpected = m.load_state_dict({pre + k: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return m


def main():
    import transformers
    from transformers import CLIPTextConfig, CLIPTextModel

    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    default = CLIPTextModel(CLIPTextConfig())
    with open(os.path.join(OUT, "state_dict_shapes.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in default.state_dict().items()}, f, indent=0)

    fixture, meta = dict(seed=R.SEED, nets={}), dict(transformers=transformers.__version__, torch=str(torch.__version__), nets={})
    for name, cfg in R.NETS.items():
        sd = R.draw_state_dict(cfg)
        m = hf_model(cfg, sd)
        rows = R.make_ids(cfg)
        net = dict(ids=rows, last={}, pooled={}, probe={k: (v.double().sum().item(), v.double().reshape(-1)[:4].tolist()) for k, v in sd.items()})
        spread, d32, dhf = [], 0.0, 0.0
        for key, ids in rows.items():
            with torch.no_grad():
                out = m(input_ids=ids)
            net["last"][key], net["pooled"][key] = out.last_hidden_state.contiguous(), out.pooler_output.contiguous()
            logits = []
            r64 = R.forward(sd, cfg, ids, torch.float64, logits_out=logits)
            r32 = R.forward(sd, cfg, ids, torch.float32)
            spread += [lg.std().item() for lg in logits]
            d32 = max(d32, R.rel_l2(r32, r64))
            dhf = max(dhf, R.rel_l2(r32, out.last_hidden_state))
            assert torch.equal(R.pooled(cfg, ids, out.last_hidden_state), out.pooler_output), (name, key)
        # the fixture must be able to see a wrong kernel: peaked softmax, rows that differ, a pooled row that depends on the EOS rule
        assert min(spread) >= 1.0, (name, spread)
        assert R.rel_l2(net["last"]["eos1"][0, 5], net["last"]["eos10"][0, 5]) > 0.05
        assert not torch.equal(net["pooled"]["eos10"], net["last"]["eos10"][:, 0])
        bound = 4.0 * d32
        assert dhf <= bound, (name, dhf, bound)
        meta["nets"][name] = dict(config=cfg, logit_std_min=min(spread), logit_std_max=max(spread), restatement_fp32_vs_float64_rel_l2=d32,
                                  restatement_fp32_vs_transformers_rel_l2=dhf, bound_rel_l2=bound)
        print(name, meta["nets"][name])
        fixture["nets"][name] = net
    fixture["meta"] = meta
    torch.save(fixture, os.path.join(OUT, "encoder.pt"))
    with open(os.path.join(OUT, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    tokenizer_fixture()
    for root, _, files in os.walk(OUT):
        for n in files:
            size = os.path.getsize(os.path.join(root, n))
            assert size < (1 << 20), (n, size)
            print(os.path.relpath(os.path.join(root, n), OUT), size, "bytes")


if __name__ == "__main__":
    main()
