"""Mirror of the reference's ``src/models/pretrained`` package: the expert-embedding extractor and the audio network it names."""
from .models import EmbeddingExtractor, Identity  # noqa: F401
from .vggish import VGGish, vggish  # noqa: F401
