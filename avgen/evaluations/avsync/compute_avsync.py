"""Reference import path avgen/evaluations/avsync/compute_avsync.py: preprocessing (:14-34), raw score (:37-46), RelSync (:49-68),
AlignSync (:71-102, on the ImageBind towers of asva_amd.imagebind_eval) and the one-clip front end (:105-end), implemented in asva_amd.
compute_sync_metrics_on_av(metric="alignsync") needs clip_net=load_clip_model(path): no ImageBind checkpoint is fetched."""
from asva_amd.avsync import (compute_avsync_scores, compute_relsync, compute_sync_metrics_on_av,  # noqa: F401
                             load_avsync_model, preprocess_videos)
from asva_amd.imagebind_eval import compute_alignsync, load_clip_model  # noqa: F401
