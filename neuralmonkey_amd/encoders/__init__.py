from .recurrent import FactoredEncoder, RecurrentEncoder, SentenceEncoder   # noqa: F401
from .numpy_stateful_filler import SpatialFiller, StatefulFiller          # noqa: F401
from .sentence_cnn_encoder import SentenceCNNEncoder    # noqa: F401
from .transformer import TransformerEncoder             # noqa: F401
from .pooling import SequenceAveragePooling, SequenceMaxPooling, SequencePooling    # noqa: F401
from .attentive import AttentiveEncoder                 # noqa: F401
from .cnn_encoder import CNNEncoder, CNNTemporalView     # noqa: F401
