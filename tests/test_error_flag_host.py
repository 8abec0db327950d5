"""The error word of a training step on the host (no GPU needed).

A step's losses travel to the host as float32 values with the session's int32 error word behind them, its raw bits in the
last slot (trainers/generic_trainer.py::objective_values).  A set word is the denormal 1.4e-45 there: a host that
flushes denormals (torch.set_flush_denormal(True), or any loaded library built with -ffast-math that sets FTZ / DAZ)
reads it as 0.0, so the flag is read through an integer view (runtime.error_flag_set) wherever the host looks at it:
Session.begin_guarded_step / settle_training / recover_training and runners/base_runner.py::LazyLosses."""
import numpy as np
import pytest
import torch

NAMES = ["decoder - cost", "train_l1", "train_l2"]
GARBAGE = [7.0e8, 3.0, 4.0]           # what a given-up step leaves in its loss slots
CLEAN = [2.5, 3.0, 4.0]               # the losses of the step that was run again


def _values(losses, word):
    out = np.zeros(len(losses) + 1, np.float32)
    out[:-1] = losses
    out[-1:].view(np.int32)[0] = word
    return out


class _Session:
    """What LazyLosses needs of a session: ``recover_training`` runs the step again and points the caller's pending
    losses at the new values."""

    def __init__(self):
        self.recovered = []

    def recover_training(self, index=0, pending=None):
        self.recovered.append(pending)
        pending.values = _values(CLEAN, 0)

    def raise_device_error(self):
        raise RuntimeError("the step that was run again gave up too")


class _Pending:
    def __init__(self, word):
        self.session = _Session()
        self.values = _values(GARBAGE if word else CLEAN, word)

    def get(self):
        return self.values


def _both_checks():
    from neuralmonkey_amd.runners.base_runner import LazyLosses
    # a set word: ONE call of recover_training, the clean losses handed out
    failed = _Pending(1)
    losses = LazyLosses(NAMES, failed)
    assert losses["decoder - cost"] == CLEAN[0]
    assert dict(losses) == dict(zip(NAMES, CLEAN))
    assert failed.session.recovered == [failed]
    # a clear word: no recovery
    fine = _Pending(0)
    losses = LazyLosses(NAMES, fine)
    assert dict(losses) == dict(zip(NAMES, CLEAN)) and fine.session.recovered == []


def test_a_set_error_word_is_seen_with_flush_to_zero_on():
    if not torch.set_flush_denormal(True):
        torch.set_flush_denormal(False)
        pytest.skip("this host cannot flush denormals")
    try:
        # the premise: as a float the flag is gone
        assert not float(_values(CLEAN, 1)[-1]) != 0.0
        _both_checks()
    finally:
        torch.set_flush_denormal(False)


def test_a_set_error_word_is_seen_without_flush_to_zero():
    _both_checks()


def test_the_helper_reads_the_bits_of_the_last_slot():
    from neuralmonkey_amd.runtime import error_flag_set
    for flush in (False, True):
        if flush and not torch.set_flush_denormal(True):
            torch.set_flush_denormal(False)
            continue
        try:
            assert error_flag_set(_values(CLEAN, 1)) and not error_flag_set(_values(CLEAN, 0))
            assert error_flag_set(_values(CLEAN, 1).reshape(1, -1))
            assert error_flag_set(_values(CLEAN, -2 ** 31))                  # -0.0 as a float
            assert not error_flag_set(_values([1.0e-45, 1.0, 1.0], 0)), "only the last slot is the flag"
        finally:
            torch.set_flush_denormal(False)
    with pytest.raises(TypeError):
        error_flag_set(np.zeros(4, np.float64))


def test_the_guarded_steps_of_a_session_read_the_flag_as_an_integer():
    """Session.settle_training on records whose flags are set: recovery starts at the first of them -- with
    flush-to-zero on as well."""
    from neuralmonkey_amd.runtime import Session

    class Stub(Session):
        def __init__(self):                                # pylint: disable=super-init-not-called
            self.device = torch.device("cuda")             # (settle_training returns at once on a CPU session)
            self.hits = []

        def recover_training(self, index=0, pending=None):
            self.hits.append(index)
            del self._train_guard[index:]

        def cluster_failure(self):
            return False

    for flush in (False, True):
        if flush and not torch.set_flush_denormal(True):
            torch.set_flush_denormal(False)
            continue
        try:
            sess = Stub()
            sess._train_guard = [{"pending": _Pending(0)}, {"pending": _Pending(1)}, {"pending": _Pending(1)}]
            sess.settle_training()
            assert sess.hits == [1] and sess._train_guard == []
        finally:
            torch.set_flush_denormal(False)
