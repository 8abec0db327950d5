"""Inputs, expected values and the bound of the direct tests of nm_optim_update / nm_optim_update_list
(tests/test_optim_family_gpu.py), shared with the CPU headroom check (tests/test_optim_family_host.py).

The flat buffers are those of tests/test_pointwise_kernels_gpu.py::_optimizer_setup: four variables of 70001, 37, 500
and 1031 elements (one longer than a 65536-element chunk, one frozen, padded offsets).  A case is two consecutive
updates -- the second reads the accumulators the first wrote -- with a gradient of its own each, behind the
regulariser terms and a per-tensor clip of 1.0 that bites on w_a (norm ~13) and w_c (~1.6) and spares bias_b (~0.3)."""
import numpy as np

from tests import optim_ref as R

REGULARIZABLE = ("w_a", "frozen", "w_c")
TRAINABLE = ("w_a", "bias_b", "w_c")
L1W, L2W, CLIP = 1e-3, 1e-2, 1.0
TOL = 2e-5                      # x the tensor's largest entry: the bound of test_optimizer_kernels_direct

# variant -> (kind, (p0, p1, p2, p3))
VARIANTS = {
    "sgd": (2, (0.1, 0.0, 0.0, 0.0)),
    "momentum": (3, (0.05, 0.9, 0.0, 0.0)),
    "nesterov": (3, (0.05, 0.9, 1.0, 0.0)),
    "adagrad": (4, (0.1, 0.0, 0.0, 0.0)),
    "rmsprop": (5, (1e-2, 0.9, 0.5, 1e-10)),
}
PATHS = ("whole", "ranges", "lists")


def seed_of(variant):
    return 31 + sorted(VARIANTS).index(variant)


def prepare(host, variant):
    """``host``: the dict of _optimizer_setup (theta, grad, s0, s1), adjusted for the variant (the accumulators of
    Adagrad and RMSProp are sums of squares: positive), plus ``grad2``, the gradient of the second update."""
    kind = VARIANTS[variant][0]
    host = dict(host)
    if kind in (4, 5):
        host["s0"] = np.abs(host["s0"])
    rng = np.random.default_rng(1000 + seed_of(variant))
    host["grad2"] = (rng.standard_normal(host["grad"].size) * 0.05).astype(np.float32)
    return host


def expected(specs, host, variant, dtype=np.float64):
    """The state after each of the two updates, evaluated in ``dtype``: a list of two dicts theta / grad (with the
    regulariser terms) / s0 / s1 of flat arrays; frozen variables and padding are as they were."""
    kind, params = VARIANTS[variant]
    dt = np.dtype(dtype).type
    theta, s0, s1 = (host[k].astype(dtype) for k in ("theta", "s0", "s1"))
    states = []
    for key in ("grad", "grad2"):
        grad = host[key].astype(dtype)
        theta, s0, s1 = theta.copy(), s0.copy(), s1.copy()
        for name, sp in specs.items():
            sl = slice(sp.offset, sp.offset + sp.size)
            if name in REGULARIZABLE:
                grad[sl] = grad[sl] + (dt(L1W) * np.sign(theta[sl]) + dt(2.0) * dt(L2W) * theta[sl])
            if name in TRAINABLE:
                g = grad[sl] * R.clip_scale(grad[sl], CLIP)
                theta[sl], a, b = R.update(kind, theta[sl], g, s0[sl], s1[sl], params)
                if R.SLOTS[kind] >= 1:
                    s0[sl] = a
                if R.SLOTS[kind] == 2:
                    s1[sl] = b
        states.append(dict(theta=theta, grad=grad, s0=s0, s1=s1))
    return states


def compare(specs, got, want, what):
    """Every variable's theta, grad and slots within TOL x the expected tensor's largest entry."""
    for name, sp in specs.items():
        sl = slice(sp.offset, sp.offset + sp.size)
        for key in ("theta", "grad", "s0", "s1"):
            ref = want[key][sl].astype(np.float64)
            err = np.abs(got[key][sl].astype(np.float64) - ref).max()
            assert err <= TOL * np.abs(ref).max(), "{} {} {}: {:.3g} > {:.3g}".format(
                what, name, key, err, TOL * np.abs(ref).max())
