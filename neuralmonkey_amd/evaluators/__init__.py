"""Evaluators that serve as sentence-level rewards of ``trainers.rl_trainer.ReinforceObjective``: ``bleu.BLEUEvaluator``
and ``gleu.GLEUEvaluator`` by their module paths.  The package itself exports nothing: the names INI files list under
``evaluation=`` (``evaluators.BLEU``, ``evaluators.TER``, ...) belong to the reference's host control plane and stay
placeholders (config/builder.py)."""
