"""Records the layout of the packed weight blobs (tests/golden/pack_layout.json) — what the multi-GPU start-up broadcasts and the
launch-plan export ships as CONST regions — for the tiny UNet and a small VAE in the four storage modes, and for the four f32 metric
networks (FID's Inception-v3, FVD's I3D, the AVSync classifier, a small three-tower CLIPSim model) in the bf16 and split modes (they
are f32 throughout: only the twin allocation of split precision changes their blob), on CPU through the tests/emu_ops.py seam.  tests/test_host_cpu.py::test_packed_blob_layout_is_pinned compares against the recorded file with the
functions below; the file is regenerated only by a change that MEANS to move the layout.

    python oracle/gen_pack_layout.py             # print the records
    python oracle/gen_pack_layout.py --write     # ... and store them as the fixture
    python oracle/gen_pack_layout.py --bytes     # ... and the SHA-256 of each blob's bytes (equal between two commits on ONE machine:
                                                 # weight values go through host matrix products whose last bit depends on the CPU)
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "pack_layout.json")
MODES = ("bf16", "fp16", "split", "plan")
MODELS = ("unet", "vae")
F32_MODELS = ("fid", "fvd", "avsync", "clipsim")        # f32 in every storage mode
F32_MODES = ("bf16", "split")
SEED = 0
_NOT_LAYOUT = ("blob", "key", "split", "act_dtype", "plan", "subpixel", "epoch", "versions")      # the blob itself and what pack() keys its cache on
_NOT_IN_BLOB = ("bias_kv",)     # CLIPModel joins bias_k | bias_v (two 256-byte-aligned items) into one row AFTER the blob is laid out


def modes_of(which):
    return F32_MODES if which in F32_MODELS else MODES


def set_mode(mode):
    """one of MODES, or None: back to the default (bf16, no split, no plan)"""
    from asva_amd import precision as P

    P.set_plan(False)
    P.set_split(mode == "split")
    P.set_precision("fp16" if mode == "fp16" else "bf16")
    if mode == "plan":
        P.set_plan(True)


def build_model(which):
    from tests.helpers import filled_unet, load_golden

    torch.manual_seed(0)
    if which in F32_MODELS:
        return build_f32_model(which)
    if which == "unet":         # its upsamplers keep the padded 3x3 form
        return filled_unet(load_golden("unet_tiny_e2e.pt")["config"])
    from asva_amd.vae import AutoencoderKL

    return AutoencoderKL(block_out_channels=(64, 128), layers_per_block=1, norm_num_groups=32)      # its upsampler takes the sub-pixel form


def build_f32_model(which):
    """the metric networks with seeded state dicts (the draws of the tests' restatements)"""
    if which == "fid":
        from asva_amd import fid
        from tests import inception_ref as R

        net = fid.InceptionV3()
        net.load_state_dict(R.draw_state_dict(fid.state_dict_shapes(), SEED))
    elif which == "fvd":
        from asva_amd import fvd
        from tests import i3d_ref as R

        net = fvd.InceptionI3d()
        net.load_state_dict(R.draw_state_dict(fvd.state_dict_shapes(), SEED))
    elif which == "avsync":
        from asva_amd import avsync as A
        from tests import avsync_ref as R
        from tests.helpers import load_shapes

        net = A.AVSyncClassifier(A.AudioConv2DNet(), A.VideoR2Plus1DNet(), A.FCHead()).eval()
        net.load_state_dict(R.draw_state_dict(load_shapes("avsync_state_dict_shapes.json"), SEED))
    else:
        from asva_amd.imagebind_eval import CLIPModel
        from tests import imagebind_ref as R

        net = CLIPModel(R.CONFIGS["tiny"])
        net.load_state_dict(R.draw_state_dict(R.CONFIGS["tiny"]))
    return net


def pack_cpu(model):
    """model.pack("cpu") with the kernels' module replaced by its CPU emulation (no kernel runs while packing)"""
    from asva_amd import unet as U
    from asva_amd import vae as V
    from asva_amd import ops
    from tests import emu_ops

    old = U.ops, V.ops, getattr(ops, "EMULATED", False)
    U.ops = V.ops = emu_ops
    ops.EMULATED = True         # the f32 networks call the kernels' module itself: this lets their pack() target the CPU
    try:
        return model.pack("cpu")
    finally:
        U.ops, V.ops, ops.EMULATED = old


def views_of(pk):
    """sorted (attribute path, dtype, shape, byte offset inside pk.blob) of every tensor in the tree of attribute bags and lists
    under `pk`, walked by attribute NAME (so the classes may move)"""
    base = pk.blob.untyped_storage().data_ptr()
    start = pk.blob.storage_offset() * pk.blob.element_size()
    out = []

    def walk(obj, path):
        if isinstance(obj, torch.Tensor):
            assert obj.untyped_storage().data_ptr() == base, f"{path} is not a view of the blob"
            out.append((path, str(obj.dtype), list(obj.shape), obj.storage_offset() * obj.element_size() - start))
        elif isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                walk(v, f"{path}[{i}]")
        elif hasattr(obj, "__dict__"):
            for k, v in vars(obj).items():
                if k not in _NOT_IN_BLOB and (path or k not in _NOT_LAYOUT):
                    walk(v, f"{path}.{k}" if path else k)

    walk(pk, "")
    return sorted(out)


def layout_record(pk):
    views = views_of(pk)
    return {"nbytes": pk.blob.numel() * pk.blob.element_size(), "views": len(views),
            "layout_sha256": hashlib.sha256(json.dumps(views).encode()).hexdigest()}


def bytes_sha256(pk):
    return hashlib.sha256(pk.blob.contiguous().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help=f"store the records as {os.path.relpath(FIXTURE, ROOT)}")
    ap.add_argument("--bytes", action="store_true", help="also print the SHA-256 of each blob's bytes")
    a = ap.parse_args()
    rec = {which: {} for which in MODELS + F32_MODELS}
    try:
        for mode in MODES:
            set_mode(mode)
            for which in MODELS + F32_MODELS:
                if mode not in modes_of(which):
                    continue
                pk = pack_cpu(build_model(which))
                rec[which][mode] = layout_record(pk)
                print(which, mode, json.dumps(rec[which][mode]), *(["bytes_sha256", bytes_sha256(pk)] if a.bytes else []), flush=True)
    finally:
        set_mode(None)
    if a.write:
        with open(FIXTURE, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
