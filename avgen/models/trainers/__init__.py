from asva_amd.trainer import AudioCondAnimationTrainer  # noqa: F401  (reference: avgen/models/trainers/__init__.py:1)
