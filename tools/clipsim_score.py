"""IA, IT and AlignSync of one clip with the ImageBind towers (asva_amd/imagebind_eval.py) — the counterpart of tools/avsync_score.py.

    python tools/clipsim_score.py --clip clip.pt --audio audio.pt --checkpoint .checkpoints/imagebind_huge.pth \\
        [--ref-clip ref.pt --avsync-model checkpoints/avsync/.../modules] [--text "a dog barking" --tokenizer sd15/tokenizer]

--clip / --ref-clip: torch files holding a (3, 12, H, W) tensor in [0, 1]; --audio: a (channels, samples) waveform at 16 kHz.  IA and IT
are the means over the frames of the image-audio and image-text cosines; AlignSync needs the reference clip and a trained AVSync
classifier.  The script needs a real ImageBind checkpoint: none was available when this was written, so no value it prints has been
compared with the reference's."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from asva_amd import avsync, imagebind_eval  # noqa: E402
from asva_amd.audio_features import waveform_to_melspectrogram  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip", required=True)
    ap.add_argument("--audio", required=True)
    ap.add_argument("--checkpoint", default=imagebind_eval.DEFAULT_CHECKPOINT)
    ap.add_argument("--ref-clip", default=None)
    ap.add_argument("--avsync-model", default=avsync.DEFAULT_MODEL_PATH)
    ap.add_argument("--text", default=None)
    ap.add_argument("--tokenizer", default=None, help="folder with vocab.json and merges.txt (SD1.5's tokenizer/)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    clip = torch.load(args.clip, map_location="cpu", weights_only=True).float()
    wave = torch.load(args.audio, map_location="cpu", weights_only=True).float()
    if clip.dim() != 4 or clip.shape[0] != 3:
        raise SystemExit(f"--clip must hold a (3, f, H, W) tensor, got {tuple(clip.shape)}")
    if args.text is not None and args.tokenizer is None:
        raise SystemExit("--text needs --tokenizer")
    net = imagebind_eval.load_clip_model(args.checkpoint, tokenizer=args.tokenizer).to(dev)
    mel = waveform_to_melspectrogram(wave, device=dev).unsqueeze(0).contiguous()
    frames = clip.permute(1, 0, 2, 3)[None].to(dev)                               # (1, f, 3, H, W)
    sims = imagebind_eval.compute_clip_consistency(frames, mel, None if args.text is None else [args.text], net=net)
    out = {"IA": float(sims["ia_sim"].mean())}
    if "it_sim" in sims:
        out["IT"] = float(sims["it_sim"].mean())
    if args.ref_clip is not None:
        ref = torch.load(args.ref_clip, map_location="cpu", weights_only=True).float()
        sync = avsync.load_avsync_model(args.avsync_model).to(dev)
        out["AlignSync"] = float(avsync.compute_sync_metrics_on_av(wave, 16000, clip, ref_video=ref, metric="alignsync", device=dev, net=sync,
                                                                   clip_net=net))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
