"""Reference import path avgen/evaluations/models/pytorch_i3d.py: the Inception-v1 I3D (:137-326), implemented in asva_amd.fvd as a
parameter holder over device kernels.  Unit3D, MaxPool3dSamePadding and InceptionModule exist there only as launches, not as classes."""
from asva_amd.fvd import InceptionI3d  # noqa: F401
