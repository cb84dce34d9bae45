"""The probe of the reference's ``SSLOnlineEval`` callback (``pl_bolts.models.self_supervised.evaluator.SSLEvaluator``,
imported at src/callbacks/callbacks.py:163), served by the MI355X build."""
from dvt_amd.models.evaluator import SSLEvaluator  # noqa: F401

__all__ = ['SSLEvaluator']
