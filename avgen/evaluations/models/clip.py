"""Reference import path avgen/evaluations/models/clip.py (:23-80): the ImageBind CLIPModel and its loader, implemented in
asva_amd.imagebind_eval."""
from asva_amd.imagebind_eval import CLIPModel, load_clip_model  # noqa: F401
