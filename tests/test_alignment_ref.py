"""tests/align_ref.py pinned to itself: the explicit gradient is TensorFlow's registered one -- the derivative of the
value where a row's labels sum to 1, ``pad * softmax(H)`` (not autograd's 0) where the label row is all zero -- and the
shape rule refuses what the kernels must never be given."""
import numpy as np
import pytest
import torch

from . import align_ref as R


def test_explicit_gradient_against_autograd_of_the_value():
    rng = np.random.default_rng(11)
    steps, bsz, slen = 5, 4, 7
    w, target, pad = R.random_case(rng, steps, bsz, slen)
    label = R.labels_of(w.shape, target).astype(np.float64)
    assert not np.isnan(label).any()                                  # the NaN tail is outside what the rows read
    sums = label.sum(axis=2)
    ones, zeros = np.abs(sums - 1.0) < 1e-6, sums == 0.0              # float32 rows normalised to 1, unaligned rows
    assert ones.sum() >= 5 and zeros.sum() >= 5 and (~ones & ~zeros).sum() >= 5 and (pad == 0).sum() >= 5
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    loss = R.value(wt, torch.tensor(label), torch.tensor(pad, dtype=torch.float64))
    loss.backward()
    auto = wt.grad.numpy()
    mine = R.rows(w, target, pad)
    assert abs(float(mine["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(mine["loss"]))
    # (the float32 label rows sum to 1 within a few float32 epsilons: so does the agreement)
    assert np.abs(mine["grad"][ones] - auto[ones]).max() <= 1e-6
    soft = torch.softmax(wt.detach(), dim=2).numpy()
    assert np.abs(mine["grad"][zeros] - pad[zeros][:, None] * soft[zeros]).max() <= 1e-15
    assert not auto[zeros].any() and np.abs(mine["grad"][zeros & (pad == 1)]).min() > 0
    assert not mine["grad"][pad == 0].any() and not mine["loss_rows"][pad == 0].any()
    other = ~ones & ~zeros & (pad == 1)                               # labels summing to something else: they differ
    assert np.abs(mine["grad"][other] - auto[other]).max() > 1e-3
    # the torch function hands autograd the same explicit gradient, scaled by what arrives
    wt2 = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    (0.5 * R.train_loss(wt2, target, pad)).backward()
    assert np.abs(wt2.grad.numpy() - R.rows(w, target, pad, scale=0.5)["grad"]).max() <= 1e-15
    assert np.abs(mine["decoded"] - np.transpose(soft, (1, 0, 2))).max() <= 1e-15
    assert np.abs(mine["decoded"].sum(axis=2) - 1.0).max() <= 1e-12


def test_shape_rule():
    R.check_shapes((3, 2, 5), (2, 3, 5))
    R.check_shapes((3, 2, 5), (2, 8, 12))
    for bad in ((3, 3, 5), (2, 2, 5), (2, 3, 4), (2, 3), (3, 2, 5, 1)):
        with pytest.raises(ValueError):
            R.check_shapes((3, 2, 5), bad)
