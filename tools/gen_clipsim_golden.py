"""Writes the CLIPSim fixtures tests/golden/clipsim/<name>.pt: for every small tower of tests/imagebind_ref.py the restatement's float64
and fp32 outputs on the seeded inputs (R.make_inputs) and seeded weights (R.draw_state_dict).  Weights and inputs are not stored: the
seed regenerates them.  torch on the CPU only (tests/test_clipsim_cpu.py pins the restatement to transformers).

    python tools/gen_clipsim_golden.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests import imagebind_ref as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "clipsim")


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    meta = {"seed": R.SEED, "configs": R.CONFIGS, "files": {}}
    for name, config in R.CONFIGS.items():
        sd, x = R.draw_state_dict(config), R.make_inputs(name)
        out = {}
        for dt, tag in ((torch.float64, "ref64"), (torch.float32, "ref32")):
            with torch.no_grad():
                if name == "tiny":
                    r = R.compute_clip_consistency(sd, config, x["videos"], x["audios"], x["ids"], dt)
                    out[tag] = {k: v.contiguous() for k, v in r.items()}
                elif "vision" in config:
                    out[tag] = R.encode_image(sd, config["vision"], x["images"], dt)
                elif "text" in config:
                    out[tag] = R.encode_text(sd, config["text"], x["ids"], dt)
                else:
                    out[tag] = R.encode_audio(sd, config["audio"], x["audios"], dt)
        if name == "a1":
            # the appended bias_kv pair must matter: without the 230th key the embedding misses the tests' bound (4 x e_ref) by far
            with torch.no_grad():
                dropped = R.encode_audio(sd, config["audio"], x["audios"], torch.float64, bias_kv=False)
            e_ref, e_drop = R.rel_l2(out["ref32"], out["ref64"]), R.rel_l2(dropped, out["ref64"])
            assert e_drop > 100.0 * 4.0 * e_ref, (e_drop, e_ref)
            out["e_dropped_bias_kv"] = e_drop
            print(f"a1: e_ref {e_ref:.3e}, without bias_kv {e_drop:.3e}")
        # a probe of the draw, so that a changed recipe or generator is noticed before the outputs disagree
        out["probe"] = {k: sd[k].flatten()[:4].clone() for k in list(sd)[:3]}
        torch.save(out, os.path.join(OUT, name + ".pt"))
        meta["files"][name + ".pt"] = os.path.getsize(os.path.join(OUT, name + ".pt"))
        e = R.rel_l2(*(torch.cat([v.flatten() for v in o.values()]) if isinstance(o, dict) else o for o in (out["ref32"], out["ref64"])))
        print(f"{name}: wrote {meta['files'][name + '.pt']} bytes, fp32 vs float64 {e:.3e}")
    with open(os.path.join(OUT, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
