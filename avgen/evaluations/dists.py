"""Reference import path avgen/evaluations/dists.py: the Fréchet distance (:56-119), implemented in asva_amd.fid (float64 torch on the
host, symmetric eigenvalue form; no scipy or sklearn)."""
from asva_amd.fid import frechet_distance  # noqa: F401
