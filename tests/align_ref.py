"""Supervised attention restated (decoders/word_alignment_decoder.py:87-110), NumPy for the kernel tests and torch for
whole training steps, in any float type.

With H [T, B, S] the recorded attention WEIGHTS, ``target`` the fed alignment [B, T', S'] (T' >= T, S' >= S) and
``pad`` [T, B] the decoder's train_padding, row (t, b) uses label = target[b, t, :S]:

    loss_rows[t, b] = pad * sum_s label_s * (lse(H[t, b, :]) - H[t, b, s])       softmax_cross_entropy_with_logits
    loss            = sum(loss_rows)
    dH[t, b, s]     = scale * pad * (softmax(H[t, b, :])_s - label_s)

-- the gradient TensorFlow 1.12 REGISTERS for the op (_SoftmaxCrossEntropyWithLogitsGrad: the incoming gradient times the
op's second output), which is the derivative of the value only where the labels of a row sum to 1.  The softmax runs
over all S entries, padded source positions (weight 0) included.  ``decoded`` [B, T, S] = transpose(softmax(H), [1, 0, 2])."""
import numpy as np
import torch


def check_shapes(weights_shape, target_shape):
    """The shape rule: ValueError unless target is [B, T' >= T, S' >= S]."""
    steps, bsz, slen = weights_shape
    if len(target_shape) != 3 or target_shape[0] != bsz or target_shape[1] < steps or target_shape[2] < slen:
        raise ValueError("weights {} against a fed alignment {}".format(tuple(weights_shape), tuple(target_shape)))


def labels_of(weights_shape, target):
    """[T, B, S]: the part of the fed array the rows read."""
    check_shapes(weights_shape, np.shape(target))
    steps, _, slen = weights_shape
    return np.transpose(np.asarray(target)[:, :steps, :slen], (1, 0, 2))


def rows(weights, target, pad, scale=1.0, dtype=np.float64):
    """dict(loss_rows [T, B], loss, grad [T, B, S], softmax [T, B, S], decoded [B, T, S]) evaluated in ``dtype``."""
    h = np.asarray(weights, dtype)
    label = labels_of(h.shape, target).astype(dtype)
    pad = np.asarray(pad, dtype)
    m = h.max(axis=2, keepdims=True)
    ex = np.exp(h - m)
    z = ex.sum(axis=2, keepdims=True, dtype=dtype)
    lse = m + np.log(z)
    soft = ex / z
    loss_rows = pad * (label * (lse - h)).sum(axis=2, dtype=dtype)
    grad = dtype(scale) * pad[:, :, None] * (soft - label)
    return {"loss_rows": loss_rows, "loss": loss_rows.sum(dtype=dtype), "grad": grad.astype(dtype), "softmax": soft,
            "decoded": np.ascontiguousarray(np.transpose(soft, (1, 0, 2)))}


def value(weights: torch.Tensor, label: torch.Tensor, pad: torch.Tensor) -> torch.Tensor:
    """The loss as a differentiable torch expression (autograd gives the derivative of the VALUE)."""
    lse = torch.logsumexp(weights, dim=2, keepdim=True)
    return (pad * (label * (lse - weights)).sum(dim=2)).sum()


class _TensorFlowXent(torch.autograd.Function):
    """The value above with TensorFlow's registered gradient."""

    @staticmethod
    def forward(ctx, weights, label, pad):           # pylint: disable=arguments-differ
        ctx.save_for_backward(weights, label, pad)
        return value(weights, label, pad)

    @staticmethod
    def backward(ctx, grad_out):                     # pylint: disable=arguments-differ
        weights, label, pad = ctx.saved_tensors
        return grad_out * pad.unsqueeze(2) * (torch.softmax(weights, dim=2) - label), None, None


def train_loss(weights: torch.Tensor, target, pad) -> torch.Tensor:
    """``WordAlignmentDecoder.train_loss`` of weights [T, B, S] that are part of a torch graph."""
    label = torch.as_tensor(labels_of(tuple(weights.shape), target), dtype=weights.dtype)
    return _TensorFlowXent.apply(weights, label, torch.as_tensor(np.asarray(pad), dtype=weights.dtype))


def random_case(rng, steps, bsz, slen, extra_t=2, extra_s=3):
    """(weights [T, B, S] float32 in [0, 1] with row sums <= 1, target [B, T + extra_t, S + extra_s] float32 whose
    unread tail is NaN, pad [T, B] float32).  Rows cycle through: a normalised label row, an all-zero one (an
    unaligned target word), one that does not sum to 1 (normalize=False), a padded position (pad 0)."""
    w = rng.random((steps, bsz, slen))
    w[rng.random(w.shape) < 0.3] = 0.0                              # padded source positions carry weight 0
    w = w / np.maximum(w.sum(axis=2, keepdims=True), 1e-3) * rng.random((steps, bsz, 1))
    target = np.full((bsz, steps + extra_t, slen + extra_s), np.nan, np.float32)
    pad = np.ones((steps, bsz), np.float32)
    for t in range(steps):
        for b in range(bsz):
            kind = (t * bsz + b) % 4 if steps * bsz > 1 else 0
            lab = rng.random(slen) * (rng.random(slen) < 0.4)
            if kind == 0:
                lab[rng.integers(slen)] += 0.5
                lab = lab / lab.sum()
            elif kind == 1:
                lab[:] = 0.0
            elif kind == 2:
                lab = 2.0 * lab + (np.arange(slen) == 0)
            else:
                pad[t, b] = 0.0
            target[b, t, :slen] = lab
    return w.astype(np.float32), target, pad
