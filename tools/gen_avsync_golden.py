"""Writes the fixtures of the AVSync scorer by running the REFERENCE's own classifier modules in fp32 on the CPU:

    python tools/gen_avsync_golden.py --reference <checkout of lzhangbj/ASVA>

CPU only, never on the GPU machine (the reference does not exist there).  The reference's modules subclass diffusers mixins;
oracle/diffusers_restated supplies those.  The files hold tensors, names, shapes and numbers only:

    tests/golden/avsync_state_dict_shapes.json     names and shapes of the classifier's state dict
    tests/golden/avsync_tiny.pt                    seed of the weights (tests/avsync_ref.py re-draws them) with a probe of every tensor,
                                                   inputs audio (2, 1, 128, 204) and video (2, 3, 12, 64, 64) (uint8 gratings, normalised by
                                                   the test), both embeddings, the output of conv1 and of the four stages of both networks
                                                   for sample 0 mean-reduced over positions, the 2 x 2 score matrix of every (audio, video)
                                                   pairing, RelSync both ways
    tests/golden/avsync_preprocess.pt              one 256 x 256 frame (uint8) and its preprocessed f32 output
    tests/golden/avsync_preprocess_128x256.pt      the same for a 128 x 256 frame (two files: one would pass the 1 MiB limit of a
                                                   committed file, and the outputs are kept whole)

The generator refuses to write a fixture that could not see a wrong kernel (see the assertions in main()).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reference", required=True, help="checkout of the reference project")
ap.add_argument("--seed", type=int, default=20240607)
args = ap.parse_args()

# the repository's own avsync/ and avgen/ shims would shadow the reference's packages: import the reference first, with the
# repository root not on the path yet
sys.path[:] = [p for p in sys.path if os.path.abspath(p or os.getcwd()) != ROOT]
sys.path[:0] = [os.path.join(ROOT, "oracle", "diffusers_restated"), os.path.abspath(args.reference)]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from avsync.models.audio import AudioConv2DNet  # noqa: E402  (the reference)
from avsync.models.avsync_classifier import AVSyncClassifier  # noqa: E402
from avsync.models.head import FCHead  # noqa: E402
from avsync.models.video import VideoR2Plus1DNet  # noqa: E402

sys.path.append(ROOT)
from tests import avsync_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def synthetic_audio(seed):
    """(2, 1, 128, 204): two different smooth ridge patterns plus a little noise, of the scale of a normalised log-mel"""
    g = torch.Generator().manual_seed(seed)
    m = torch.arange(128.0).view(128, 1)
    t = torch.arange(204.0).view(1, 204)
    a0 = 0.8 * torch.sin(2 * torch.pi * (m / 37.0 + t / 51.0)) + 0.4 * torch.cos(2 * torch.pi * t / 17.0) - 0.3
    a1 = 0.8 * torch.sin(2 * torch.pi * (m / 19.0 - t / 29.0)) * torch.exp(-((t - 120.0) / 60.0) ** 2) + 0.2
    return (torch.stack([a0, a1])[:, None] + 0.1 * torch.randn(2, 1, 128, 204, generator=g)).contiguous()


def main():
    torch.manual_seed(0)
    net = AVSyncClassifier(AudioConv2DNet(), VideoR2Plus1DNet(), FCHead()).eval()
    shapes = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert len(shapes) == 261, len(shapes)
    sd = R.draw_state_dict(shapes, args.seed)
    net.load_state_dict(sd)

    audio = synthetic_audio(args.seed)
    video_u8 = torch.stack([R.grating_video_u8(12, 64, 64, 0.3, 0.11, 9.0), R.grating_video_u8(12, 64, 64, 1.9, -0.23, 29.0, 1.0, mean=0.3, contrast=0.25, colour=2.1)])
    video = R.normalize_clip(R.u8_to_unit(video_u8))

    taps = {}

    def hook(name):
        def fn(_m, _i, out):
            taps.setdefault(name, out.detach())
        return fn

    a_names = ["conv1", "block1", "block2", "block3", "block4"]
    v_names = ["conv1", "conv2x", "conv3x", "conv4x", "conv5x"]
    handles = [getattr(net.audio_encoder, n).register_forward_hook(hook("a." + n)) for n in a_names]
    handles += [getattr(net.video_encoder, n).register_forward_hook(hook("v." + n)) for n in v_names]
    with torch.no_grad():
        a_emb, v_emb = net.audio_encoder(audio), net.video_encoder(video)
        for h in handles:
            h.remove()
        scores = torch.stack([torch.stack([net(audio[i:i + 1], video[j:j + 1])[0] for j in range(2)]) for i in range(2)])   # [audio i][video j]
        own = torch.stack([scores[0, 0], scores[1, 1]])
        relsync_ref_audio = R.relsync(torch.stack([scores[1, 0], scores[0, 1]]), own)       # reference = the other clip's audio
        relsync_ref_video = R.relsync(torch.stack([scores[0, 1], scores[1, 0]]), own)       # reference = the other clip's video
        # float64 run of the same modules: the reference's own fp32 error, the basis of the tests' bounds
        net64 = AVSyncClassifier(AudioConv2DNet(), VideoR2Plus1DNet(), FCHead()).eval()
        net64.load_state_dict(sd)
        net64 = net64.double()
        a64, v64 = net64.audio_encoder(audio.double()), net64.video_encoder(video.double())
        s64 = net64(audio.double(), video.double())

    # ---- the fixture must be able to see a wrong kernel
    rms = lambda x: x.pow(2).mean().sqrt().item()  # noqa: E731
    for name, e in (("audio", a_emb), ("video", v_emb)):
        assert 0.05 <= rms(e) <= 5.0, (name, rms(e))
        assert R.rel_l2(e[0], e[1]) >= 0.05, (name, R.rel_l2(e[0], e[1]))
    flat = scores.reshape(-1)
    for i in range(4):
        for j in range(i + 1, 4):
            assert abs(flat[i] - flat[j]).item() >= 1e-3, scores
    stage_means = {}
    for k, v in taps.items():
        zeros = (v == 0).float().mean().item()
        assert 0.10 < zeros < 0.90, (k, zeros)
        stage_means[k] = v[0].reshape(v.shape[1], -1).mean(1).contiguous()
    ref_err = dict(audio_emb=R.rel_l2(a_emb, a64), video_emb=R.rel_l2(v_emb, v64),
                   score=(torch.stack([scores[0, 0], scores[1, 1]]).double() - s64).abs().max().item())
    print("embedding rms", rms(a_emb), rms(v_emb), "scores", scores.tolist(), "relsync", relsync_ref_audio.tolist(), relsync_ref_video.tolist())
    print("fp32 vs float64 of the reference modules:", ref_err)

    with open(os.path.join(GOLDEN, "avsync_state_dict_shapes.json"), "w") as f:
        json.dump(shapes, f, indent=0)
    probe = {k: (v.double().sum().item(), v.double().reshape(-1)[:8].tolist()) for k, v in sd.items()}
    torch.save(dict(seed=args.seed, probe=probe, audio=audio, video_u8=video_u8, audio_emb=a_emb, video_emb=v_emb, stage_means=stage_means,
                    scores=scores, relsync_ref_audio=relsync_ref_audio, relsync_ref_video=relsync_ref_video,
                    reference_fp32_error=ref_err, torch_version=str(torch.__version__)), os.path.join(GOLDEN, "avsync_tiny.pt"))

    # ---- preprocessing: F.interpolate(bicubic, antialias) is what torchvision's Resize calls for tensors
    g = torch.Generator().manual_seed(args.seed + 1)
    for (h, w), name in (((256, 256), "avsync_preprocess.pt"), ((128, 256), "avsync_preprocess_128x256.pt")):
        yy, xx = torch.arange(h).view(1, h, 1), torch.arange(w).view(1, 1, w)
        base = 127.0 + 90.0 * torch.sin(xx / 5.0 + yy / 9.0 + torch.arange(3).view(3, 1, 1)) + 25.0 * torch.randn(3, h, w, generator=g)
        base[:, h // 3:h // 3 + 20, w // 4:w // 4 + 40] = 255.0       # hard edges: the cubic's overshoot is part of the contract
        frames = base.clamp(0, 255).round().to(torch.uint8)[None]
        out = F.interpolate(frames.float() / 255.0, size=(224, 224), mode="bicubic", antialias=True, align_corners=False)
        out = (out - torch.tensor(R.CLIP_MEAN).view(1, 3, 1, 1)) / torch.tensor(R.CLIP_STD).view(1, 3, 1, 1)
        torch.save(dict(frames_u8=frames, out=out.contiguous()), os.path.join(GOLDEN, name))
    for n in ("avsync_tiny.pt", "avsync_preprocess.pt", "avsync_preprocess_128x256.pt", "avsync_state_dict_shapes.json"):
        size = os.path.getsize(os.path.join(GOLDEN, n))
        assert size < (1 << 20), (n, size)
        print(n, size, "bytes")


if __name__ == "__main__":
    main()
