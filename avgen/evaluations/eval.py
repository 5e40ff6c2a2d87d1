"""Reference import path avgen/evaluations/eval.py: the evaluation driver (:28-281), implemented in asva_amd.evaluation (FVD excepted)."""
from asva_amd.evaluation import evaluate_generation_results, reduce_metrics  # noqa: F401
