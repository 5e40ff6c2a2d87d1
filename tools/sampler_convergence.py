"""How fast do the multistep samplers approach the probability-flow solution of the network itself?  On the SD1.5-shaped UNet with
seeded random weights (tools/clip_bench.py's), the n-step latents of DPM-Solver++ 2M, UniPC-2 and UniPC-3 (bh2) are compared with a
400-step first-order run from the same noise: rel-L2 over frames 1.. per n.  All runs use one table family (linspace, or Karras
sigmas with --karras) ending on sigma_min (final_sigmas_type="sigma_min"), so they start and end at the same noise levels; the first-order DPM-Solver++ map is DDIM's
(tests/test_dpmsolver_cpu.py::test_first_order_map_is_ddim), which is what the 400-step reference is.

    python tools/sampler_convergence.py [--steps 5 8 10 15 20] [--ref-steps 400] [--karras] [--out table.md]

Seeded weights are not a trained model: the table shows how the solvers' discretisation error falls on THIS network's ODE, not the
sample quality of any step count."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from asva_amd.conditioning import audio_segment_mask  # noqa: E402
from asva_amd.pipeline import AudioCondAnimationPipeline, synthetic_clip  # noqa: E402
from asva_amd.schedulers import DPMSolverMultistepScheduler, UniPCMultistepScheduler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, nargs="+", default=[5, 8, 10, 15, 20])
    ap.add_argument("--ref-steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--karras", action="store_true", help="Karras sigmas (ending on sigma_min) instead of the linspace table")
    ap.add_argument("--out", default=None, help="also write the markdown table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    unet = bench.build_unet(dev, 0, 1)
    c = synthetic_clip(a.seed, device=dev)
    kw = dict(texts=[""], text_encodings=[c["text_encodings"][None]], image_latents=c["image_latents"][None], noise=c["noise"][None],
              audio_encodings=c["audio_encodings"][None], null_audio_encodings=c["null_audio_encodings"][None],
              audio_masks=audio_segment_mask(12), audio_guidance_scale=4.0, output_latents=True)
    tail = dict(final_sigmas_type="sigma_min", lower_order_final=True, use_karras_sigmas=a.karras)

    def run(sched, n):
        pipe = AudioCondAnimationPipeline(unet=unet, scheduler=sched, vae=None).to(dev)
        pipe.set_progress_bar_config(disable=True)
        return pipe(num_inference_steps=n, **kw).double().cpu()

    ref = run(DPMSolverMultistepScheduler(solver_order=1, **tail), a.ref_steps)
    samplers = [("DPM++ 2M", lambda: DPMSolverMultistepScheduler(solver_order=2, **tail)),
                ("UniPC-2 bh2", lambda: UniPCMultistepScheduler(solver_order=2, **tail)),
                ("UniPC-3 bh2", lambda: UniPCMultistepScheduler(solver_order=3, **tail))]
    lines = ["| steps | " + " | ".join(name for name, _ in samplers) + " |", "|---|" + "---|" * len(samplers)]
    for n in a.steps:
        errs = []
        for _, make in samplers:
            got = run(make(), n)
            errs.append(float((got[:, :, 1:] - ref[:, :, 1:]).norm() / ref[:, :, 1:].norm()))
        lines.append(f"| {n} | " + " | ".join(f"{e:.3e}" for e in errs) + " |")
    table = "\n".join(lines)
    print(f"rel-L2 of the n-step latents against {a.ref_steps} first-order (DDIM) steps, seed {a.seed}, "
          f"{'Karras' if a.karras else 'linspace'} sigmas:\n{table}")
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
