"""The reference's evaluation driver (avgen/evaluations/eval.py:28-281) over the device metrics of this package: FID
(asva_amd.fid), FVD (asva_amd.fvd), IA / IT (asva_amd.imagebind_eval), RelSync (asva_amd.avsync) and AlignSync.

`evaluate_generation_results` follows the reference step by step: the file-count assertion, groundtruth clips in sorted order, the
generated clips of each in sorted order, the first frame excluded from FID, the same `result_dict` keys and JSON file.  Steps 4 and 5
(features and scores -> metrics, per-instance record) are one pure host function, `reduce_metrics`.

Two deviations, both noted in INTEGRATION.md: the per-instance "IT" holds the IT value (the reference writes the IA value there,
eval.py:269), and generated files are looked up with the groundtruth file's own extension (for `.mp4` names that is the reference's
pattern), so that pre-decoded `.npz` clip containers work too; when no such file exists, the `.avi` files the generation drivers
write without torchvision are taken.
"""
from __future__ import annotations

import json
import os
from glob import glob
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

FVD_MESSAGE = ("FVD needs the I3D detector, which is never downloaded: pass models={'fvd': asva_amd.fvd.load_i3d_pretrained(weights=...)} "
               "or set the environment variable AVSD_FVD_I3D to the path of i3d_torchscript.pt (or of a state dict), or pass eval_fvd=False "
               "(FID, IA / IT, RelSync and AlignSync do not need it)")


def _generated_paths(generated_video_root: str, groundtruth_video_name: str) -> List[str]:
    stem, ext = os.path.splitext(groundtruth_video_name)
    found = sorted(glob(f"{generated_video_root}/{stem}*{ext}"))
    # without torchvision the generation drivers write Motion-JPEG .avi files (asva_amd.video_io), whatever the groundtruth is
    return found or sorted(glob(f"{generated_video_root}/{stem}*.avi"))


def reduce_metrics(groundtruth_fid_features: Optional[Sequence[torch.Tensor]] = None,
                   generated_fid_features: Optional[Sequence[torch.Tensor]] = None,
                   generated_ias: Optional[Sequence[torch.Tensor]] = None, generated_its: Optional[Sequence[torch.Tensor]] = None,
                   groundtruth_avsync_scores: Optional[Sequence[torch.Tensor]] = None,
                   generated_avsync_scores: Optional[Sequence[torch.Tensor]] = None,
                   groundtruth_first_frame_ia_sims: Optional[Sequence[torch.Tensor]] = None,
                   generated_pred_frame_ia_sims: Optional[Sequence[torch.Tensor]] = None,
                   generated_video_names: Optional[Sequence[str]] = None, *,
                   groundtruth_fvd_features: Optional[Sequence[torch.Tensor]] = None,
                   generated_fvd_features: Optional[Sequence[torch.Tensor]] = None) -> Dict:
    """eval.py:203-275 as a pure host function: lists of per-video / per-clip CPU tensors in, the metric entries of `result_dict` out.
    A metric is computed when its inputs are given: FID from (b, f, c) feature lists (first frame dropped), IA / IT from per-clip
    means (b,), FVD from (b, c) feature lists (one row per clip, all frames), RelSync from raw classifier scores (b,), AlignSync from the (b, 1) first-frame and (b, f - 1) predicted-frame
    image-audio similarities together with RelSync.  `generated_video_names`, if given, adds "instance_metrics": one record per
    generated clip, in the order the lists were filled."""
    from .fid import frechet_distance

    out: Dict = {}
    if groundtruth_fid_features is not None:
        gt = torch.cat(list(groundtruth_fid_features))[:, 1:].flatten(end_dim=1)          # exclude the first frame: (B * (f - 1), c)
        gen = torch.cat(list(generated_fid_features))[:, 1:].flatten(end_dim=1)
        out["FID"] = frechet_distance(gt, gen).item()
    if groundtruth_fvd_features is not None:
        out["FVD"] = frechet_distance(torch.cat(list(groundtruth_fvd_features)), torch.cat(list(generated_fvd_features))).item()
    ias = its = relsync = alignsync = None
    if generated_ias is not None:
        ias, its = torch.cat(list(generated_ias)), torch.cat(list(generated_its))
        out.update({"IA_mean": ias.mean().item(), "IA_std": ias.std().item(), "IT_mean": its.mean().item(), "IT_std": its.std().item()})
    if groundtruth_avsync_scores is not None:
        gt_s, gen_s = torch.cat(list(groundtruth_avsync_scores)), torch.cat(list(generated_avsync_scores))
        relsync = torch.exp(gen_s) / (torch.exp(gt_s) + torch.exp(gen_s))
        out.update({"RelSync_mean": relsync.mean().item(), "RelSync_std": relsync.std().item()})
    if groundtruth_first_frame_ia_sims is not None:
        if relsync is None:
            raise ValueError("AlignSync needs the RelSync scores")
        first, pred = torch.cat(list(groundtruth_first_frame_ia_sims)), torch.cat(list(generated_pred_frame_ia_sims))
        probs = (torch.exp(pred) / (torch.exp(first) + torch.exp(pred))).mean(dim=1)
        alignsync = probs * relsync
        out.update({"AlignSync_mean": alignsync.mean().item(), "AlignSync_std": alignsync.std().item()})
    if generated_video_names is not None:
        inst: Dict[str, Dict[str, float]] = {}
        for i, name in enumerate(generated_video_names):
            rec = inst[name] = {}
            if ias is not None:
                rec["IA"] = ias[i].item()
                rec["IT"] = its[i].item()            # the reference stores the IA value here (eval.py:269)
            if relsync is not None:
                rec["RelSync"] = relsync[i].item()
            if alignsync is not None:
                rec["AlignSync"] = alignsync[i].item()
        out["instance_metrics"] = inst
    return out


@torch.no_grad()
def evaluate_generation_results(groundtruth_video_root: str, groundtruth_video_names: List[str], groundtruth_categories: List[str],
                                num_clips_per_video: int, generated_video_root: str, result_save_path: str,
                                image_size: Union[int, Tuple[int, int]], video_fps: int = 6, video_num_frame: int = 12,
                                eval_fid: bool = True, eval_fvd: bool = True, eval_clipsim: bool = True, eval_relsync: bool = True,
                                eval_alignsync: bool = True, record_instance_metrics: bool = False, dtype: torch.dtype = torch.float32,
                                models: Optional[Dict[str, torch.nn.Module]] = None) -> Dict:
    """eval.py:28-281.  `models` (not in the reference): preloaded nets under the keys "fid" (asva_amd.fid.InceptionV3 returning block
    3 first), "fvd" (asva_amd.fvd.InceptionI3d), "avsync" (AVSyncClassifier) and "clip" (imagebind_eval.CLIPModel); a net that is needed
    and not given comes from its default loader (load_inceptionv3_pretrained, load_i3d_pretrained, load_avsync_model, load_clip_model),
    none of which downloads anything.  eval_fvd=True (the default, as in the reference) without models["fvd"] and without
    $AVSD_FVD_I3D is refused before any file is read and before any other network is loaded."""
    if eval_fvd and not (models or {}).get("fvd") and not os.environ.get("AVSD_FVD_I3D"):
        raise NotImplementedError(FVD_MESSAGE)
    if dtype != torch.float32:
        raise ValueError("the evaluation networks compute in float32 only")
    from .avsync import compute_avsync_scores, load_avsync_model
    from .data_utils import load_av_clips_uniformly
    from .fid import compute_fid_image_features, load_inceptionv3_pretrained
    from .fvd import compute_fvd_video_features, load_i3d_pretrained
    from .imagebind_eval import compute_clip_consistency, load_clip_model

    device = torch.device("cuda")
    models = dict(models or {})
    # For each xxxx.mp4 in groundtruth_video_root there are num_clips_per_video generated clips xxxx_clip-{i}.mp4 in
    # generated_video_root, whose audio is that of the i-th uniformly sampled clip of the groundtruth video
    for name in groundtruth_video_names:
        n = len(_generated_paths(generated_video_root, name))
        assert n == num_clips_per_video, \
            f'number of generated videos({n}) does not equal to num_clips_per_video({num_clips_per_video}) for {name}'
    result_dict = {"groundtruth_video_root": groundtruth_video_root, "generated_video_root": generated_video_root,
                   "num_clips_per_video": num_clips_per_video}
    if eval_alignsync:
        assert eval_clipsim and eval_relsync

    # 1. models and feature lists
    iv3_fid = i3d_fvd = clip_model = avsync_net = None
    if eval_fid:
        iv3_fid = (models.get("fid") or load_inceptionv3_pretrained(block_ids=[3], use_fid_inception=True)).to(device=device, dtype=dtype)
    if eval_fvd:
        i3d_fvd = (models.get("fvd") or load_i3d_pretrained()).to(device=device, dtype=dtype)
    if eval_clipsim:
        clip_model = (models.get("clip") or load_clip_model()).to(device=device, dtype=dtype)
    if eval_relsync:
        avsync_net = (models.get("avsync") or load_avsync_model()).to(device=device, dtype=dtype)
    gt_fvd, gen_fvd = [], []
    gt_fid, gen_fid, gen_ias, gen_its, gt_scores, gen_scores, gt_first_ia, gen_pred_ia, gen_names = [], [], [], [], [], [], [], [], []

    def load(path, num_clips):
        v, a = load_av_clips_uniformly(video_path=path, video_fps=video_fps, video_num_frame=video_num_frame, image_size=image_size,
                                       num_clips=num_clips, load_audio_as_melspectrogram=True)
        return v.to(device=device, dtype=dtype), a.to(device=device, dtype=dtype)      # (b f c h w) in [0, 1], (b 1 n t)

    def fid_features(videos):
        b, f = videos.shape[:2]
        return compute_fid_image_features(videos.flatten(end_dim=1), iv3_fid).detach().cpu().view(b, f, -1)

    def fvd_features(videos):                                                   # all frames: the first one is not dropped (eval.py:118-123)
        return compute_fvd_video_features(videos.permute(0, 2, 1, 3, 4), i3d_fvd).detach().cpu()      # b f c h w -> b c f h w; (b, c)

    # 2. groundtruth clips, in sorted order
    groundtruth_video_names.sort()
    for name, _category in zip(groundtruth_video_names, groundtruth_categories):
        videos, audios = load(os.path.join(groundtruth_video_root, name), num_clips_per_video)
        if eval_fid:
            gt_fid.append(fid_features(videos))
        if eval_fvd:
            gt_fvd.append(fvd_features(videos))
        if eval_alignsync:
            gt_first_ia.append(compute_clip_consistency(videos[:, 0:1], audios, net=clip_model)["ia_sim"].detach().cpu())      # (b, 1)
        if eval_relsync:
            gt_scores.append(compute_avsync_scores(audios, videos.permute(0, 2, 1, 3, 4), avsync_net).detach().cpu())         # (b,)

    # 3. generated clips, in the order of the groundtruth clips they belong to
    for name, category in zip(groundtruth_video_names, groundtruth_categories):
        for path in _generated_paths(generated_video_root, name):
            gen_names.append(path.replace(f"{generated_video_root}/", ""))
            videos, audios = load(path, 1)
            if eval_fid:
                gen_fid.append(fid_features(videos))
            if eval_fvd:
                gen_fvd.append(fvd_features(videos))
            if eval_clipsim:
                sims = compute_clip_consistency(videos, audios, [category], net=clip_model)
                ia, it = sims["ia_sim"].detach().cpu()[:, 1:], sims["it_sim"].detach().cpu()[:, 1:]                            # (b, f - 1)
                gen_ias.append(ia.mean(dim=1))
                gen_its.append(it.mean(dim=1))
                if eval_alignsync:
                    gen_pred_ia.append(ia)
            if eval_relsync:
                gen_scores.append(compute_avsync_scores(audios, videos.permute(0, 2, 1, 3, 4), avsync_net).detach().cpu())

    # 4. + 5. metrics and the per-clip record
    result_dict.update(reduce_metrics(
        groundtruth_fid_features=gt_fid if eval_fid else None, generated_fid_features=gen_fid if eval_fid else None,
        generated_ias=gen_ias if eval_clipsim else None, generated_its=gen_its if eval_clipsim else None,
        groundtruth_avsync_scores=gt_scores if eval_relsync else None, generated_avsync_scores=gen_scores if eval_relsync else None,
        groundtruth_first_frame_ia_sims=gt_first_ia if eval_alignsync else None,
        generated_pred_frame_ia_sims=gen_pred_ia if eval_alignsync else None,
        generated_video_names=gen_names if record_instance_metrics else None,
        groundtruth_fvd_features=gt_fvd if eval_fvd else None, generated_fvd_features=gen_fvd if eval_fvd else None))

    os.makedirs(os.path.dirname(result_save_path) or ".", exist_ok=True)
    with open(result_save_path, "w") as f:
        json.dump(result_dict, f, indent=4)
    return result_dict
