"""Reference import path avgen/evaluations/fid: FID feature extraction, implemented in asva_amd.fid."""
from .compute_fid import compute_fid_image_features, preprocess_images  # noqa: F401
