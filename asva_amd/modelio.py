"""What every model holder here shares on the host: the diffusers-style model folder (a JSON config next to one weight file) read and
written in one place, and the rule that a change of the parameters drops what was packed from them.  No kernel, no device code.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Sequence

import torch

CONFIG_NAME = "config.json"
SAFETENSORS_NAME = "diffusion_pytorch_model.safetensors"
BIN_NAME = "diffusion_pytorch_model.bin"
WEIGHT_NAMES = (SAFETENSORS_NAME, BIN_NAME)      # read in this order; written as (safetensors, torch.save)


def folder(path: str, subfolder: Optional[str] = None) -> str:
    return os.path.join(path, subfolder) if subfolder else path


def read_config(path: str, subfolder: Optional[str] = None, name: str = CONFIG_NAME, drop_private: bool = False) -> Dict:
    """the JSON config of a model folder; `drop_private` leaves out the `_`-prefixed keys (the stamps of `diffusers_config`)"""
    with open(os.path.join(folder(path, subfolder), name)) as f:
        cfg = json.load(f)
    return {k: v for k, v in cfg.items() if not k.startswith("_")} if drop_private else cfg


def read_state_dict(path: str, subfolder: Optional[str] = None, names: Sequence[str] = WEIGHT_NAMES,
                    use_safetensors: Optional[bool] = None) -> Dict[str, torch.Tensor]:
    """the first of `names` that exists in the folder, on the CPU; use_safetensors=False passes over the .safetensors names"""
    path = folder(path, subfolder)
    names = [n for n in names if not (use_safetensors is False and n.endswith(".safetensors"))]
    for name in names:
        file = os.path.join(path, name)
        if os.path.isfile(file):
            if name.endswith(".safetensors"):
                from safetensors.torch import load_file

                return load_file(file)
            return torch.load(file, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"none of {', '.join(names)} under {path}")


def diffusers_config(model, config: Dict) -> Dict:
    """`config` under the stamps diffusers' ModelMixin writes, tuples as lists"""
    return {"_class_name": type(model).__name__, "_diffusers_version": "0.29.2",
            **{k: (list(v) if isinstance(v, tuple) else v) for k, v in config.items()}}


def write_folder(directory: str, config: Dict, state_dict: Dict[str, torch.Tensor], safe_serialization: bool,
                 names: Sequence[str] = WEIGHT_NAMES) -> None:
    """config.json and ONE weight file: names[0] through safetensors, or names[1] through torch.save"""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, CONFIG_NAME), "w") as f:
        json.dump(config, f, indent=2)
    sd = {k: v.detach().cpu().contiguous() for k, v in state_dict.items()}
    if safe_serialization:
        from safetensors.torch import save_file

        save_file(sd, os.path.join(directory, names[0]))
    else:
        torch.save(sd, os.path.join(directory, names[1]))


class Invalidating:
    """Mixin in front of nn.Module: load_state_dict and _apply (.to(), .half(), ...) change the parameters, so both end in
    `_invalidate()`, where the class says what it had derived from them and now drops."""

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        r = super().load_state_dict(state_dict, strict=strict, **kw)
        self._invalidate()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._invalidate()
        return r

    def _invalidate(self) -> None:
        raise NotImplementedError


class EpochCounted(Invalidating):
    """... for a model whose pack is kept by something that compares `_epoch`, the count of the changes of the parameters"""

    _epoch = 0

    def _invalidate(self) -> None:
        self._epoch += 1
