"""Mirror of the reference's ``src/models`` package (module names kept so that
``from models.vit import ViViT`` style imports resolve to the build)."""
from . import vit  # noqa: F401
from .vit import ViViT  # noqa: F401
from . import frame_transformer, transformer  # noqa: F401,E402
from .frame_transformer import FrameTransformer, TransformerBase, PositionalEncoding  # noqa: F401,E402
from .transformer import SimpleTransformer  # noqa: F401,E402
from . import custom_resnet, TPN  # noqa: F401,E402
from . import LSTM  # noqa: F401,E402
from .LSTM import LSTMRegressor  # noqa: F401,E402
from . import contrastivemodel, basicmlp  # noqa: F401,E402
from .contrastivemodel import SpatioTemporalContrastiveModel  # noqa: F401,E402
from .basicmlp import BasicMLP  # noqa: F401,E402
from . import evaluator  # noqa: F401,E402
from .evaluator import SSLEvaluator  # noqa: F401,E402
from . import mae  # noqa: F401,E402
from .mae import MaskedClipAutoencoder  # noqa: F401,E402
from . import joint_vivit  # noqa: F401,E402
from .joint_vivit import JointViViT  # noqa: F401,E402
