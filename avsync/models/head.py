"""Reference import path avsync/models/head.py, implemented in asva_amd."""
from asva_amd.avsync import FCHead  # noqa: F401
