"""Reference import path avsync/models/audio.py, implemented in asva_amd."""
from asva_amd.avsync import AudioConv2DNet  # noqa: F401
