"""Mirror of the reference's ``src/models/pretrained`` package: the expert-embedding extractor."""
from .models import EmbeddingExtractor, Identity  # noqa: F401
