"""Stacks of dense layers (mirror of neuralmonkey/nn/projection.py:38-57 ``multilayer_projection`` and nn/mlp.py):
per layer tf.layers.dense (glorot_uniform kernel, zero bias) + activation + dropout, variables
``<prefix>/mlp_layer_{i}/{kernel,bias}``.  The products are the fp32 MFMA GEMM, relu in its epilogue."""
from typing import List, Optional

from .. import autodiff as F
from ..variables import glorot_uniform_initializer, zeros_initializer

ACTIVATIONS = ("relu", "tanh", "identity")


def activation_name(fn) -> Optional[str]:
    return getattr(fn, "nm_name", None)


def declare_dense(part, store, name: str, d_in: int, d_out: int) -> None:
    part.declare(store, name + "/kernel", (d_in, d_out), glorot_uniform_initializer())
    part.declare(store, name + "/bias", (d_out,), zeros_initializer())


def declare_multilayer_projection(part, store, prefix: str, d_in: int, layer_sizes: List[int]) -> int:
    """-> the width of the last layer (``d_in`` without layers)."""
    for i, size in enumerate(layer_sizes):
        declare_dense(part, store, "{}/mlp_layer_{}".format(prefix, i), d_in, size)
        d_in = size
    return d_in


def dense(tape: F.Tape, part, name: str, x: F.Var, activation: Optional[str] = None) -> F.Var:
    out = F.linear(tape, x, tape.param(part, name + "/kernel"), tape.param(part, name + "/bias"),
                   act="relu" if activation == "relu" else None)
    return F.tanh(tape, out) if activation == "tanh" else out


def multilayer_projection(tape: F.Tape, ctx, part, prefix: str, x: F.Var, layer_sizes: List[int], activation: str,
                          keep_prob: float, train: bool) -> F.Var:
    for i, _ in enumerate(layer_sizes):
        name = "{}/mlp_layer_{}".format(prefix, i)
        x = dense(tape, part, name, x, activation)
        x = F.dropout(tape, x, keep_prob, train, ctx.salt(part.name, name))
    return x
