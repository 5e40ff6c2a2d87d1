"""Reference import path avsync/models/video.py, implemented in asva_amd."""
from asva_amd.avsync import VideoR2Plus1DNet  # noqa: F401
