from .runner import GreedyRunner                                                # noqa: F401
from .beamsearch_runner import BeamSearchRunner, beam_search_runner_range       # noqa: F401
from .sampling_runner import SamplingRunner, sampling_runner_range           # noqa: F401
from .mbr_runner import MBRRunner                                               # noqa: F401
from .plain_runner import PlainRunner                                           # noqa: F401
from .xent_runner import XentRunner                                             # noqa: F401
from .tensor_runner import RepresentationRunner, TensorRunner                   # noqa: F401
from .label_runner import LabelRunner                                           # noqa: F401
from .logits_runner import LogitsRunner                                         # noqa: F401
from .regression_runner import RegressionRunner                                 # noqa: F401
from .word_alignment_runner import WordAlignmentRunner                         # noqa: F401
