"""``RegressionRunner``: the predictions of a SequenceRegressor as nested lists of floats (interface of
neuralmonkey/runners/regression_runner.py:16-56).

With several sessions (an ensemble) the predictions are the mean over the sessions and the reported ``mse`` is the SUM
of the sessions' losses, as in the reference (:24-33); a session that was run without losses contributes nothing to
it.  ``postprocess`` maps the list of predictions before it is handed out."""
from typing import Any, Callable, Dict, List

import numpy as np

from ..checking import check_argument_types
from ..decoders.sequence_regressor import SequenceRegressor
from .base_runner import BaseRunner

Postprocessor = Callable[[List[float]], List[float]]


class RegressionRunner(BaseRunner):
    class Executable(BaseRunner.Executable):
        def collect_results(self, results: List[Dict]) -> None:
            runner = self.executor
            stacked = np.stack([np.asarray(session["prediction"]) for session in results])      # [sessions, B, dim]
            mse = float(sum(float(session["mse"]) for session in results if "mse" in session))
            predictions = stacked.mean(axis=0).tolist()
            if runner.postprocess is not None:
                predictions = runner.postprocess(predictions)
            self.set_runner_result(outputs=predictions, losses=[mse])

    def __init__(self, output_series: str, decoder: SequenceRegressor, postprocess: Postprocessor = None) -> None:
        check_argument_types()
        BaseRunner.__init__(self, output_series, decoder)
        self.postprocess = postprocess

    @property
    def fetches(self) -> Dict[str, Any]:
        return {"prediction": self.decoder.predictions, "mse": self.decoder.cost}

    @property
    def loss_names(self) -> List[str]:
        return ["mse"]
