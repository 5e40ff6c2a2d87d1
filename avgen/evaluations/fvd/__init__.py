"""Reference import path avgen/evaluations/fvd: FVD feature extraction, implemented in asva_amd.fvd."""
from .compute_fvd import compute_fvd_video_features, preprocess_videos  # noqa: F401
