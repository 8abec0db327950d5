"""Minimum Bayes risk decoding over the samples of a ``SamplingDecoder``: of the ``n`` samples of a sentence, output the
one that agrees most, on average, with all of them under a sentence-level utility.

The reference has no such decoder.  Candidates and evidence are the same samples ``s_0 .. s_{n-1}``:

    U[b, i, j]     = utility(reference = s_j, hypothesis = s_i)
    expected[b, i] = mean over j of U[b, i, j]            (summed in double in j order, i == j included)
    best[b]        = argmax_i expected[b, i]              (on the double sums; ties to the lowest i, NaN last)

``sentence_gleu`` (the default) and ``sentence_bleu`` of trainers/self_critical_objective.py are recognised by identity
and scored on the device, one wavefront per unordered pair (nm_mbr_pairwise, csrc/nm_mbr.hip).  Any other callable gets
the convention of ``SelfCriticalObjective.reward_function``: it is called ONCE on the host with the ``B * n * n`` pairs
tiled side by side, time-major, and its result travels back.  Either way the sums, the choice and the gather of the
chosen column are one launch (nm_mbr_select): no torch kernel runs on this path.
"""
from typing import Any, Callable, List, NamedTuple

import numpy as np
import torch

from .. import ops
from ..model.model_part import ModelPart
from ..runtime import tensor
from ..trainers.self_critical_objective import DEVICE_REWARDS, sentence_gleu
from ..vocabulary import END_TOKEN_INDEX, Vocabulary
from .sampling_decoder import SamplingDecoder, SamplingOutput

# pylint: disable=invalid-name
UtilityFunction = Callable[[np.ndarray, np.ndarray], np.ndarray]
# pylint: enable=invalid-name


class MBROutput(NamedTuple):
    token_ids: torch.Tensor          # [steps, B] int32: the chosen sample of every sentence
    best: torch.Tensor               # [B] int32: its index among the samples
    expected_utility: torch.Tensor   # [B, n] the mean utility of every sample against all samples
    utilities: torch.Tensor          # [B, n, n]: [b, i, j] scores sample i against sample j as the reference
    samples: SamplingOutput


def tile_pairs(token_ids: np.ndarray):
    """(references, hypotheses), both [T, B * n * n]: column ``(b * n + i) * n + j`` pairs hypothesis ``s_i`` with
    reference ``s_j`` of sentence ``b`` -- the layout of ``MBROutput.utilities``, flattened."""
    steps, bsz, n = token_ids.shape
    hypotheses = np.repeat(token_ids[:, :, :, None], n, axis=3)
    references = np.repeat(token_ids[:, :, None, :], n, axis=2)
    return references.reshape(steps, bsz * n * n), hypotheses.reshape(steps, bsz * n * n)


class MBRDecoder(ModelPart):
    def __init__(self, name: str, sampling_decoder: SamplingDecoder, utility: UtilityFunction = sentence_gleu) -> None:
        ModelPart.__init__(self, name)
        self.sampling_decoder = sampling_decoder
        self.utility = utility

    @property
    def dependencies(self) -> List[str]:
        return ["sampling_decoder"]

    @property
    def vocabulary(self) -> Vocabulary:
        return self.sampling_decoder.vocabulary

    @property
    def num_samples(self) -> int:
        return self.sampling_decoder.num_samples

    @tensor
    def outputs(self, ctx) -> MBROutput:
        samples = self.sampling_decoder.outputs(ctx)
        tok = samples.token_ids
        steps, bsz, n = tok.shape
        if steps == 0:                                    # nothing was drawn: nothing to score, nothing is launched
            return MBROutput(tok[:, :, 0], torch.zeros(bsz, dtype=torch.int32), torch.zeros((bsz, n)),
                             torch.zeros((bsz, n, n)), samples)
        key = (id(self), "mbr", bsz, n)
        utilities = ctx.buffer(key + ("U",), (bsz, n, n))
        kind = DEVICE_REWARDS.get(self.utility)
        if kind is not None and tok.is_cuda:
            ops.mbr_pairwise(kind, tok, END_TOKEN_INDEX, out=utilities)
        else:
            references, hypotheses = tile_pairs(tok.cpu().numpy())
            host = self.utility(references, hypotheses.astype(np.int64))
            host = np.ascontiguousarray(np.asarray(host, dtype=np.float32).reshape(bsz, n, n))
            utilities.copy_(torch.from_numpy(host))
        max_steps = max(int(ctx.fed(self.sampling_decoder.max_steps)), steps)
        expected = ctx.buffer(key + ("expected",), (bsz, n))
        best = ctx.buffer(key + ("best",), (bsz,), torch.int32)
        chosen = ctx.buffer(key + ("chosen",), (max_steps * bsz,), torch.int32)[:steps * bsz].view(steps, bsz)
        ops.mbr_select(utilities, tok, expected, best, chosen)
        return MBROutput(chosen, best, expected, utilities, samples)

    def ensemble_outputs(self, ctxs: List[Any]) -> MBROutput:
        if len(ctxs) > 1:
            self.sampling_decoder.ensemble_outputs(ctxs)  # raises: sampling from an ensemble is not implemented
        return self.outputs(ctxs[0])
