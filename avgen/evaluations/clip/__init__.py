"""Reference import path avgen/evaluations/clip: CLIPSim (the IA and IT rows of the evaluation), implemented in asva_amd.imagebind_eval."""
from asva_amd.imagebind_eval import compute_clip_consistency, preprocess_videos  # noqa: F401
