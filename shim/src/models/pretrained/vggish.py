"""VGGish, the audio network the reference names at src/models/pretrained/models.py:13, served by the MI355X build."""
from dvt_amd.models.pretrained.vggish import VGGish, vggish  # noqa: F401

__all__ = ['VGGish', 'vggish']
