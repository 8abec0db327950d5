"""Optimizer descriptions (stand-ins for the tf.train.* objects INI files name).

The update itself is one fused clip + update HIP kernel over the flat parameter buffer
(csrc/nm_optim.hip, one instantiation per ``kind``); these classes only carry what the trainer
reads: ``kind`` (0..5), ``params(step, applied)`` -- the four scalars of the update --
``slot_initial`` and the names of the slot variables -- none, one or two -- a TensorFlow
checkpoint holds per variable (``slot_suffixes``, ``<var>/<name>`` and ``<var>/<name>_1`` as
TensorFlow's slot creator makes them)."""
import math
from typing import Callable, Union

from .checking import check_argument_types


class Optimizer:
    kind = -1
    slot_suffixes = ("/Adam", "/Adam_1")
    slot_initial = (0.0, 0.0)          # the value each slot starts at

    def learning_rate(self, step: int) -> float:
        """Learning rate of update number ``step`` (1-based).  A schedule is evaluated at the
        global step before the update, as the TF graph does (functions.py)."""
        return float(self._lr(step - 1)) if callable(self._lr) else float(self._lr)

    def params(self, step: int, applied: int = None):
        """(p0, p1, p2, p3) of update number ``step``; ``applied``: see ``AdamOptimizer.lr_t``."""
        raise NotImplementedError


class AdamOptimizer(Optimizer):
    """tf.train.AdamOptimizer: lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v EMA; theta -= lr_t*m/(sqrt(v)+eps)."""
    kind = 0

    def __init__(self, learning_rate: Union[float, Callable[[int], float]] = 0.001, beta1: float = 0.9,
                 beta2: float = 0.999, epsilon: float = 1e-8, use_locking: bool = False,
                 name: str = "Adam") -> None:
        self._lr = learning_rate
        self.beta1, self.beta2, self.epsilon = beta1, beta2, epsilon

    def lr_t(self, step: int, applied: int = None) -> float:
        """``step`` counts from 1 (the value of global_step after this update) and drives the learning
        rate schedule; ``applied`` is the number of updates this optimizer has applied including this
        one (TF keeps beta1_power / beta2_power per optimizer) -- equal to ``step`` with one trainer."""
        t = step if applied is None else applied
        return self.learning_rate(step) * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t)

    def params(self, step: int, applied: int = None):
        return (self.lr_t(step, applied), self.beta1, self.beta2, self.epsilon)


class LazyAdamOptimizer(AdamOptimizer):
    """tf.contrib.opt.LazyAdamOptimizer.  In Neural Monkey the L1/L2 terms make
    every embedding gradient dense (SURVEY section 9 "Gradient density"), so it
    behaves exactly like Adam."""


class AdadeltaOptimizer(Optimizer):
    """tf.train.AdadeltaOptimizer (tests/bpe.ini:102-108, tests/str.ini:100-106).  TF 1.12's ApplyAdadelta:
    accum = rho*accum + (1-rho)*g^2;  update = sqrt(accum_update + eps) * rsqrt(accum + eps) * g;
    var -= lr*update;  accum_update = rho*accum_update + (1-rho)*update^2.  The slots are created under the
    optimizer's ``name``: ``<var>/<name>`` (accum) and ``<var>/<name>_1`` (accum_update)."""
    kind = 1

    def __init__(self, learning_rate: Union[float, Callable[[int], float]] = 0.001, rho: float = 0.95,
                 epsilon: float = 1e-8, use_locking: bool = False, name: str = "Adadelta") -> None:
        self._lr = learning_rate
        self.rho, self.epsilon = rho, epsilon
        self.slot_suffixes = ("/" + name, "/" + name + "_1")

    def params(self, step: int, applied: int = None):
        return (self.learning_rate(step), self.rho, self.epsilon, 0.0)


class _FamilyOptimizer(Optimizer):
    """The optimizers of kinds 2..5 (include/nmhip_optim.h): no slot unless the class names one, and no beta powers
    in a checkpoint, so ``params`` ignores ``applied``."""
    slot_suffixes = ()
    slot_initial = ()


class GradientDescentOptimizer(_FamilyOptimizer):
    """tf.train.GradientDescentOptimizer, TF 1.12's ApplyGradientDescent: var -= lr*g.  No slots."""
    kind = 2

    def __init__(self, learning_rate: Union[float, Callable[[int], float]], use_locking: bool = False,
                 name: str = "GradientDescent") -> None:
        check_argument_types()
        self._lr = learning_rate

    def params(self, step: int, applied: int = None):
        return (self.learning_rate(step), 0.0, 0.0, 0.0)


class MomentumOptimizer(_FamilyOptimizer):
    """tf.train.MomentumOptimizer, TF 1.12's ApplyMomentum: accum = accum*momentum + g; var -= lr*accum, or with
    ``use_nesterov`` var -= g*lr + accum*momentum*lr (the new accum).  One slot, ``<var>/<name>``, starting at 0."""
    kind = 3

    def __init__(self, learning_rate: Union[float, Callable[[int], float]], momentum: float,
                 use_locking: bool = False, name: str = "Momentum", use_nesterov: bool = False) -> None:
        check_argument_types()
        self._lr = learning_rate
        self.momentum, self.use_nesterov = float(momentum), use_nesterov
        self.slot_suffixes = ("/" + name,)
        self.slot_initial = (0.0,)

    def params(self, step: int, applied: int = None):
        return (self.learning_rate(step), self.momentum, 1.0 if self.use_nesterov else 0.0, 0.0)


class AdagradOptimizer(_FamilyOptimizer):
    """tf.train.AdagradOptimizer, TF 1.12's ApplyAdagrad: accum += g*g; var -= g*lr*rsqrt(accum) -- no epsilon.  One
    slot, ``<var>/<name>``, starting at ``initial_accumulator_value``."""
    kind = 4

    def __init__(self, learning_rate: Union[float, Callable[[int], float]], initial_accumulator_value: float = 0.1,
                 use_locking: bool = False, name: str = "Adagrad") -> None:
        check_argument_types()
        if initial_accumulator_value <= 0.0:
            raise ValueError("initial_accumulator_value must be positive: {}".format(initial_accumulator_value))
        self._lr = learning_rate
        self.initial_accumulator_value = float(initial_accumulator_value)
        self.slot_suffixes = ("/" + name,)
        self.slot_initial = (self.initial_accumulator_value,)

    def params(self, step: int, applied: int = None):
        return (self.learning_rate(step), 0.0, 0.0, 0.0)


class RMSPropOptimizer(_FamilyOptimizer):
    """tf.train.RMSPropOptimizer, TF 1.12's ApplyRMSProp: ms += (g*g - ms)*(1-decay); mom = mom*momentum +
    (g*lr)/sqrt(ms + epsilon); var -= mom.  Two slots: ``<var>/<name>`` (rms, starting at ONE) and ``<var>/<name>_1``
    (momentum, starting at 0).  ``centered=True`` (a third slot, the mean gradient) constructs and is refused by the
    trainer that takes it."""
    kind = 5

    def __init__(self, learning_rate: Union[float, Callable[[int], float]], decay: float = 0.9, momentum: float = 0.0,
                 epsilon: float = 1e-10, use_locking: bool = False, centered: bool = False,
                 name: str = "RMSProp") -> None:
        check_argument_types()
        self._lr = learning_rate
        self.decay, self.momentum, self.epsilon, self.centered = float(decay), float(momentum), float(epsilon), centered
        self.slot_suffixes = ("/" + name, "/" + name + "_1")
        self.slot_initial = (1.0, 0.0)

    def params(self, step: int, applied: int = None):
        return (self.learning_rate(step), self.decay, self.momentum, self.epsilon)
