"""Writes the FID fixtures under tests/golden/fid/ on the CPU (no device, no checkpoint, nothing fetched):

    python tools/gen_fid_golden.py

  state_dict_shapes.json   torchvision's Inception3 state-dict layout (names and shapes) as tests/inception_ref.py states it
  fid_tiny.pt              seed + probe of the seeded weights, three uint8 images of different sizes (256 x 256; 128 x 200, which is
                           upscaled; 75 x 91), their float64 features and logits from tests/inception_ref.py on the float32-preprocessed
                           input, and the per-stage position means of every image
  measured.json            "cpu": rel-L2 of torch's own float32 CPU forward against that float64 forward (the reference's arithmetic:
                           the bound of the device tests is 4 x this, capped at 1e-4); "frechet": our Fréchet distance against the
                           reference's formula (numpy + scipy.linalg.sqrtm) on the sizes of tests/test_fid_cpu.py.  An existing "gpu"
                           section (figures measured on the MI355X, entered by hand) is kept.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import inception_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fid")
SEED = 20151205
IMAGES = [dict(height=256, width=256, angle=0.5, wavelength=37.0, phase=0.3, seed=1),
          dict(height=128, width=200, angle=1.9, wavelength=13.0, phase=1.1, mean=0.45, contrast=0.3, seed=2),
          dict(height=75, width=91, angle=2.6, wavelength=7.0, phase=2.0, mean=0.55, contrast=0.35, seed=3)]
PROBE_KEYS = ["Conv2d_1a_3x3.conv.weight", "Mixed_5b.branch5x5_2.bn.running_var", "Mixed_6c.branch7x7dbl_3.conv.weight",
              "Mixed_7c.branch_pool.bn.bias", "fc.weight"]
FD_SIZES = [(200, 160, 32), (64, 48, 32), (500, 400, 128), (20, 24, 32), (96, 96, 128)]


def fd_features(n, d, seed, shift=0.0):
    """clipped-Gaussian float32 features with an uneven spectrum (shared with tests/test_fid_cpu.py)"""
    g = torch.Generator().manual_seed(seed)
    mix = torch.randn(d, d, generator=g) / d ** 0.5
    scale = torch.linspace(0.2, 2.0, d)
    return ((torch.randn(n, d, generator=g) * scale) @ mix + 0.3 + shift).clamp_min(0.0).float()


def fd_reference(x1, x2):
    """dists.py:78-119 of the reference, literally (numpy + scipy); also says which of its branches ran"""
    import numpy as np
    from scipy import linalg

    x1, x2 = x1.numpy(), x2.numpy()
    mu1, sigma1 = np.mean(x1, axis=0), np.cov(x1, rowvar=False)
    mu2, sigma2 = np.mean(x2, axis=0), np.cov(x2, rowvar=False)
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    fallback = not np.isfinite(covmean).all()
    if fallback:
        offset = np.eye(sigma1.shape[0]) * 1e-6
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    imag = 0.0
    if np.iscomplexobj(covmean):
        imag = float(np.max(np.abs(covmean.imag)))
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(imag))
        covmean = covmean.real
    fd = diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)
    return float(fd), float(np.trace(sigma1) + np.trace(sigma2) + diff.dot(diff)), fallback, imag


def main():
    from asva_amd.fid import frechet_distance

    os.makedirs(OUT, exist_ok=True)
    shapes = R.state_dict_shapes()
    with open(os.path.join(OUT, "state_dict_shapes.json"), "w") as f:
        json.dump(shapes, f, indent=0, sort_keys=True)
    sd = R.draw_state_dict(shapes, SEED)
    probe = {k: (sd[k].double().sum().item(), sd[k].double().reshape(-1)[:8].tolist()) for k in PROBE_KEYS}
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    images = [R.image_u8(**kw) for kw in IMAGES]
    feats, logits, stage_means, e_stage = [], [], {n: [] for n in R.STAGES}, 0.0
    f32_feats, f32_logits = [], []
    with torch.no_grad():
        for img in images:
            x = R.preprocess(R.u8_to_unit(img)[None])                  # float32, as the reference computes it
            st64, st32 = {}, {}
            f64, l64 = R.forward(sd64, x.double(), st64)
            f32, l32 = R.forward(sd, x, st32)
            feats.append(f64[0]), logits.append(l64[0]), f32_feats.append(f32[0]), f32_logits.append(l32[0])
            for n in R.STAGES:
                m64 = st64[n][0].mean(dim=(1, 2))
                stage_means[n].append(m64)
                e_stage = max(e_stage, R.rel_l2(st32[n][0].double().mean(dim=(1, 2)), m64))
    feats, logits = torch.stack(feats), torch.stack(logits)
    nonzero = [(f != 0).sum().item() for f in feats]
    assert min(nonzero) >= 1024, f"the draw lets the network die: non-zero features per image {nonzero}"
    for i in range(len(images)):
        for j in range(i):
            assert not torch.equal(feats[i], feats[j]) and R.rel_l2(feats[i], feats[j]) > 1e-2, "two images give the same features"
    e_feat, e_logit = R.rel_l2(torch.stack(f32_feats), feats), R.rel_l2(torch.stack(f32_logits), logits)
    torch.save({"seed": SEED, "probe": probe, "images_u8": images, "features": feats, "logits": logits,
                "stage_means": {n: torch.stack(v) for n, v in stage_means.items()}}, os.path.join(OUT, "fid_tiny.pt"))
    path = os.path.join(OUT, "measured.json")
    measured = {}
    if os.path.isfile(path):
        with open(path) as f:
            measured = json.load(f)
    measured["cpu"] = {"f32_vs_f64_features_rel_l2": e_feat, "f32_vs_f64_logits_rel_l2": e_logit, "f32_vs_f64_stage_means_max_rel_l2": e_stage,
                       "f32_vs_f64_rel_l2": max(e_feat, e_logit, e_stage), "nonzero_features_per_image": nonzero,
                       "feature_distance_rel_l2_min": min(R.rel_l2(feats[i], feats[j]) for i in range(3) for j in range(i))}
    fr = {}
    for n1, n2, d in FD_SIZES:
        x1, x2 = fd_features(n1, d, 11 * d + n1), fd_features(n2, d, 13 * d + n2, shift=0.05)
        ours, (ref, scale, fallback, imag) = frechet_distance(x1, x2).item(), fd_reference(x1, x2)
        same_ours, same_ref = frechet_distance(x1, x1.clone()).item(), fd_reference(x1, x1.clone())[0]
        fr[f"{n1}x{n2}x{d}"] = {"ours": ours, "reference": ref, "rel_difference": abs(ours - ref) / scale, "reference_took_fallback": fallback,
                               "reference_max_imag": imag, "identical_sets_ours": same_ours, "identical_sets_reference": same_ref}
    measured["frechet"] = fr
    with open(path, "w") as f:
        json.dump(measured, f, indent=1, sort_keys=True)
    print(json.dumps(measured, indent=1, sort_keys=True))
    print("fid_tiny.pt:", os.path.getsize(os.path.join(OUT, "fid_tiny.pt")) >> 10, "KiB")


if __name__ == "__main__":
    main()
