"""The reference's ``src/models/pretrained`` package (``EmbeddingExtractor``, src/models/pretrained/models.py) and the audio
network it names at ``:13``, served by the MI355X build."""
from dvt_amd.models.pretrained import EmbeddingExtractor, Identity, VGGish, vggish  # noqa: F401

__all__ = ['EmbeddingExtractor', 'Identity', 'VGGish', 'vggish']
