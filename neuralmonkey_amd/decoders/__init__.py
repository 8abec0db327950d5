from .decoder import Decoder                             # noqa: F401
from .beam_search_decoder import BeamSearchDecoder       # noqa: F401
from .sampling_decoder import SamplingDecoder         # noqa: F401
from .transformer import TransformerDecoder             # noqa: F401
from .ctc_decoder import CTCDecoder                       # noqa: F401
from .sequence_labeler import EmbeddingsLabeler, SequenceLabeler  # noqa: F401
from .classifier import Classifier                       # noqa: F401
from .sequence_regressor import SequenceRegressor        # noqa: F401
from .word_alignment_decoder import WordAlignmentDecoder  # noqa: F401
from .mbr_decoder import MBRDecoder                      # noqa: F401  (last: it imports the utilities of trainers/)
