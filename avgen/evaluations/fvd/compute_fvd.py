"""Reference import path avgen/evaluations/fvd/compute_fvd.py: video preprocessing and I3D features, implemented in asva_amd.fvd."""
from asva_amd.fvd import compute_fvd_video_features, preprocess_videos  # noqa: F401
