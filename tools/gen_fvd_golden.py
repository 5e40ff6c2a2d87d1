"""Writes the FVD fixtures under tests/golden/fvd/ by running the REFERENCE's own InceptionI3d module on the CPU:

    python tools/gen_fvd_golden.py --reference <checkout of lzhangbj/ASVA>

CPU only, never on the GPU machine (the reference does not exist there); no checkpoint, nothing fetched.  The reference's
pytorch_i3d.py is loaded by path with `torchvision` stubbed in sys.modules (only its classifier's T.Resize needs it).  The files hold
tensors, names, shapes and numbers only:

  state_dict_shapes.json   the state-dict layout of InceptionI3d(400, in_channels=3) (names and shapes), read from the module
  fvd_tiny.pt              seed + probe of the seeded weights (tests/i3d_ref.py re-draws them), two uint8 clips of 40 x 56 pixels
                           (A: 12 frames, the workload; B: 17 frames: odd temporal sizes 9, 5, 3 through the net and two average-pool
                           windows), the module's float64 features (400,) on the float32-preprocessed clips, and the per-endpoint
                           channel means of both
  measured.json            "cpu": rel-L2 of the module's own float32 forward against its float64 forward (the bound of the device tests
                           is 4 x this, capped at 1e-4), rel-L2 of the restatement tests/i3d_ref.py against the module (float64), the
                           share of non-zero activations at every endpoint.  An existing "gpu" section (figures measured on the
                           MI355X, entered by hand) is kept.

The generator refuses to write a fixture through which the signal dies: at every endpoint at least 25 % of the activations must be
non-zero, and the features of the two clips must differ by rel-L2 >= 0.1.  A draw that fails is changed, not the thresholds.
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import i3d_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fvd")
SEED = 20170522
CLIPS = [dict(frames=12, height=40, width=56, angle=0.5, wavelength=11.0, speed=0.9, seed=1),
         dict(frames=17, height=40, width=56, angle=2.1, wavelength=5.0, speed=-0.5, mean=0.42, contrast=0.22, seed=2)]
PROBE_KEYS = ["Conv3d_1a_7x7.conv3d.weight", "Conv3d_2c_3x3.bn.running_var", "Mixed_4c.b2a.conv3d.weight", "Mixed_4e.b3b.bn.bias",
              "Mixed_5c.b1b.conv3d.weight", "logits.conv3d.weight", "logits.conv3d.bias"]


def reference_module(checkout):
    for name in ("torchvision", "torchvision.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    path = os.path.join(os.path.abspath(checkout), "avgen", "evaluations", "models", "pytorch_i3d.py")
    spec = importlib.util.spec_from_file_location("reference_pytorch_i3d", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stages_of(net, x):
    """the reference module's forward with a hook on every endpoint"""
    st, hooks = {}, []
    for name in R.ENDPOINTS:
        hooks.append(net._modules[name].register_forward_hook(lambda m, i, o, name=name: st.__setitem__(name, o)))
    with torch.no_grad():
        y = net(x)
    for h in hooks:
        h.remove()
    return y, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    ref = reference_module(args.reference)
    os.makedirs(OUT, exist_ok=True)
    net32 = ref.InceptionI3d(400, in_channels=3).eval()
    shapes = {k: list(v.shape) for k, v in net32.state_dict().items()}
    assert shapes == R.state_dict_shapes(), "tests/i3d_ref.py states another layout than the reference module"
    assert list(ref.InceptionI3d.VALID_ENDPOINTS[:-2]) == R.ENDPOINTS
    with open(os.path.join(OUT, "state_dict_shapes.json"), "w") as f:
        json.dump(shapes, f, indent=0, sort_keys=True)
    sd = R.draw_state_dict(shapes, SEED)
    probe = {k: (sd[k].double().sum().item(), sd[k].double().reshape(-1)[:8].tolist()) for k in PROBE_KEYS}
    net32.load_state_dict(sd)
    net64 = ref.InceptionI3d(400, in_channels=3).eval()
    net64.load_state_dict(sd)
    net64 = net64.double()
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}

    clips = [R.clip_u8(**kw) for kw in CLIPS]
    feats, stage_means, alive = [], {n: [] for n in R.ENDPOINTS}, {n: 1.0 for n in R.ENDPOINTS}
    e_f32, e_restated = 0.0, 0.0
    for clip in clips:
        x = R.preprocess(R.clip_to_bcthw(clip))                        # float32, as the reference computes it
        y64, st64 = stages_of(net64, x.double())
        y32, st32 = stages_of(net32, x)
        st_r = {}
        with torch.no_grad():
            y_r = R.forward(sd64, x.double(), st_r)
        assert y64.shape == (1, 400)
        feats.append(y64[0])
        e_f32 = max(e_f32, R.rel_l2(y32, y64))
        e_restated = max(e_restated, R.rel_l2(y_r, y64))
        for n in R.ENDPOINTS:
            m64 = st64[n][0].mean(dim=(1, 2, 3))
            stage_means[n].append(m64)
            alive[n] = min(alive[n], (st64[n] != 0).double().mean().item())
            e_f32 = max(e_f32, R.rel_l2(st32[n][0].double().mean(dim=(1, 2, 3)), m64))
            e_restated = max(e_restated, R.rel_l2(st_r[n], st64[n]))
    feats = torch.stack(feats)
    dist = R.rel_l2(feats[0], feats[1])
    print("non-zero share per endpoint:", json.dumps(alive, indent=1))
    print(f"features of the two clips differ by rel-L2 {dist:.4f}; restatement vs module {e_restated:.3e}; float32 vs float64 {e_f32:.3e}")
    assert min(alive.values()) >= 0.25, "the draw lets the network die"
    assert dist >= 0.1, "the two clips give nearly the same features"
    assert e_restated <= 1e-12, "tests/i3d_ref.py does not restate the reference module"
    torch.save({"seed": SEED, "probe": probe, "clips_u8": clips, "features": feats, "stage_means": stage_means},
               os.path.join(OUT, "fvd_tiny.pt"))
    path = os.path.join(OUT, "measured.json")
    measured = {}
    if os.path.isfile(path):
        with open(path) as f:
            measured = json.load(f)
    measured["cpu"] = {"f32_vs_f64_rel_l2": e_f32, "restatement_vs_module_rel_l2": e_restated, "nonzero_share_per_endpoint": alive,
                       "feature_distance_rel_l2": dist}
    with open(path, "w") as f:
        json.dump(measured, f, indent=1, sort_keys=True)
    print("fvd_tiny.pt:", os.path.getsize(os.path.join(OUT, "fvd_tiny.pt")) >> 10, "KiB")


if __name__ == "__main__":
    main()
