"""Reference import path avgen/evaluations/fid/compute_fid.py: preprocessing (:5-18) and Inception features (:21-31), implemented in
asva_amd.fid."""
from asva_amd.fid import compute_fid_image_features, preprocess_images  # noqa: F401
