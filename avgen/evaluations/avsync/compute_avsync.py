"""Reference import path avgen/evaluations/avsync/compute_avsync.py: preprocessing (:14-34), raw score (:37-46), RelSync (:49-68)
and the one-clip front end (:105-end), implemented in asva_amd.  AlignSync (:71-102) needs the ImageBind vision trunk and is not
implemented: compute_sync_metrics_on_av(metric="alignsync") raises NotImplementedError."""
from asva_amd.avsync import (compute_avsync_scores, compute_relsync, compute_sync_metrics_on_av,  # noqa: F401
                             load_avsync_model, preprocess_videos)
