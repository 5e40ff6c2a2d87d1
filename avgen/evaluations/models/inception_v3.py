"""Reference import path avgen/evaluations/models/inception_v3.py: the pytorch-fid Inception-v3 (:16-150) and its loader (:331-332),
implemented in asva_amd.fid.  The loader takes the checkpoint from a path or $AVSD_FID_INCEPTION: nothing is downloaded."""
from asva_amd.fid import InceptionV3, load_inceptionv3_pretrained  # noqa: F401
