"""Reference import path avgen/evaluations/clip/compute_clip.py: preprocessing (:8-38) and the per-frame similarities (:41-54),
implemented in asva_amd.imagebind_eval."""
from asva_amd.imagebind_eval import compute_clip_consistency, preprocess_videos  # noqa: F401
