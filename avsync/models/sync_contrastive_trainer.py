"""Reference import path avsync/models/sync_contrastive_trainer.py: the classifier's contrastive objective (:9-60), implemented in
asva_amd (forward values only, no gradients)."""
from asva_amd.avsync import AVSyncContrastiveTrainer  # noqa: F401
