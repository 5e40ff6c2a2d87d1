"""Reference import path avgen/evaluations/models/download.py: the I3D loader (:47-55), implemented in asva_amd.fvd.  It takes the
detector from a path or $AVSD_FVD_I3D: nothing is downloaded."""
from asva_amd.fvd import load_i3d_pretrained  # noqa: F401
