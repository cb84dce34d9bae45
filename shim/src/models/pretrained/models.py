"""``src/models/pretrained/models.py`` of the reference, served by the MI355X build."""
from dvt_amd.models.pretrained.models import EmbeddingExtractor, Identity  # noqa: F401

__all__ = ['EmbeddingExtractor', 'Identity']
