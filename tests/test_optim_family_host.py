"""GradientDescent, Momentum, Adagrad and RMSProp without a GPU: the tf.train.* names through the config loader,
constructor signatures and refusals, ``kind`` / ``params`` of Adam and Adadelta beside them, the NumPy restatement (tests/optim_ref.py) against the formulas written out and
against torch.optim, the float32 headroom of the direct GPU test's bound on its exact inputs, the binding table of
include/nmhip_optim.h with its refusals, and checkpoints with none, one or two slot variables per variable."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import optim_family_cases as OC
from tests import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INI_SECTIONS = {
    "GradientDescentOptimizer": 'class=tf.train.GradientDescentOptimizer\nlearning_rate=0.1',
    "MomentumOptimizer": 'class=tf.train.MomentumOptimizer\nname="momentum"\nlearning_rate=1e-2\nmomentum=0.9\n'
                         'use_nesterov=True',
    "AdagradOptimizer": 'class=tf.train.AdagradOptimizer\nname="adagrad"\nlearning_rate=1e-2\n'
                        'initial_accumulator_value=0.5',
    "RMSPropOptimizer": 'class=tf.train.RMSPropOptimizer\nname="rmsprop"\nlearning_rate=1e-3\ndecay=0.95\n'
                        'momentum=0.5\nepsilon=1.0e-6',
}


def _ini_model(tmp_path, section):
    from neuralmonkey_amd.config.configuration import load_experiment
    from .test_host import write_ini
    path = write_ini(tmp_path)
    with open(path) as fh:
        text = fh.read()
    old = "class=tf.contrib.opt.LazyAdamOptimizer\nlearning_rate=0.001"
    assert old in text
    with open(path, "w") as fh:
        fh.write(text.replace(old, section))
    return load_experiment(path)


# ---- INI and construction ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", sorted(INI_SECTIONS))
def test_ini_with_each_new_optimizer_builds_a_trainer(tmp_path, cls):
    """``class=tf.train.<cls>`` in the optimizer section of tests/test_host.py's INI builds through the tf.* shim into
    the experiment's trainer.  Without the feature: SymbolNotShipped."""
    from neuralmonkey_amd import optimizers
    model = _ini_model(tmp_path, INI_SECTIONS[cls])
    opt = model.trainer.optimizer
    assert type(opt) is getattr(optimizers, cls)                                  # pylint: disable=unidiomatic-typecheck
    assert type(model.trainer).__name__ == "CrossEntropyTrainer"
    want = {"GradientDescentOptimizer": (2, (), (), (0.1, 0.0, 0.0, 0.0)),
            "MomentumOptimizer": (3, ("/momentum",), (0.0,), (1e-2, 0.9, 1.0, 0.0)),
            "AdagradOptimizer": (4, ("/adagrad",), (0.5,), (1e-2, 0.0, 0.0, 0.0)),
            "RMSPropOptimizer": (5, ("/rmsprop", "/rmsprop_1"), (1.0, 0.0), (1e-3, 0.95, 0.5, 1e-6))}[cls]
    assert (opt.kind, opt.slot_suffixes, opt.slot_initial, opt.params(1)) == want


def test_constructors_defaults_and_refusals():
    from neuralmonkey_amd import tf_shim
    from neuralmonkey_amd.optimizers import (AdagradOptimizer, GradientDescentOptimizer, MomentumOptimizer,
                                             RMSPropOptimizer)
    assert tf_shim.train.MomentumOptimizer is MomentumOptimizer and tf_shim.train.RMSPropOptimizer is RMSPropOptimizer
    assert tf_shim.train.AdagradOptimizer is AdagradOptimizer
    assert tf_shim.train.GradientDescentOptimizer is GradientDescentOptimizer
    sgd = GradientDescentOptimizer(0.5)
    assert (sgd.kind, sgd.slot_suffixes, sgd.slot_initial, sgd.params(7)) == (2, (), (), (0.5, 0.0, 0.0, 0.0))
    mom = MomentumOptimizer(0.1, 0.8)
    assert (mom.kind, mom.slot_suffixes, mom.slot_initial) == (3, ("/Momentum",), (0.0,))
    assert mom.use_nesterov is False and mom.params(1) == (0.1, 0.8, 0.0, 0.0)
    assert MomentumOptimizer(0.1, 0.8, use_nesterov=True, name="m").params(1) == (0.1, 0.8, 1.0, 0.0)
    assert MomentumOptimizer(0.1, 0.8, name="m").slot_suffixes == ("/m",)
    ada = AdagradOptimizer(0.1)
    assert (ada.kind, ada.slot_suffixes, ada.slot_initial, ada.params(1)) == (4, ("/Adagrad",), (0.1,), (0.1, 0.0, 0.0, 0.0))
    assert AdagradOptimizer(0.1, 0.25, name="a").slot_initial == (0.25,)
    rms = RMSPropOptimizer(0.01)
    assert (rms.kind, rms.slot_suffixes, rms.slot_initial) == (5, ("/RMSProp", "/RMSProp_1"), (1.0, 0.0))
    assert rms.params(1) == (0.01, 0.9, 0.0, 1e-10) and rms.centered is False
    assert RMSPropOptimizer(0.01, name="r").slot_suffixes == ("/r", "/r_1")
    # a schedule is evaluated at the global step BEFORE the update, as AdamOptimizer.learning_rate does
    for opt in (GradientDescentOptimizer(lambda s: 1.0 / (s + 1)), MomentumOptimizer(lambda s: 1.0 / (s + 1), 0.9),
                AdagradOptimizer(lambda s: 1.0 / (s + 1)), RMSPropOptimizer(lambda s: 1.0 / (s + 1))):
        assert opt.params(1)[0] == 1.0 and opt.params(4)[0] == 0.25
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="initial_accumulator_value"):
            AdagradOptimizer(0.1, initial_accumulator_value=bad)
    with pytest.raises(TypeError, match='"learning_rate"'):
        GradientDescentOptimizer("0.1")
    with pytest.raises(TypeError, match='"momentum"'):
        MomentumOptimizer(0.1, "0.9")
    with pytest.raises(TypeError, match='"use_nesterov"'):
        MomentumOptimizer(0.1, 0.9, use_nesterov="yes")
    with pytest.raises(TypeError, match='"name"'):
        AdagradOptimizer(0.1, name=3)
    with pytest.raises(TypeError, match='"decay"'):
        RMSPropOptimizer(0.1, decay=None)
    with pytest.raises(TypeError):
        MomentumOptimizer(0.1)                                   # momentum has no default, as in TensorFlow


def test_adam_and_adadelta_describe_themselves_as_the_family_does():
    """``kind`` and ``params(step, applied)`` of the two optimizers of nm_optim_apply against their formulas written
    out, for a constant and a callable learning rate: Adam's bias correction counts the updates THIS optimizer applied,
    its schedule (evaluated at the global step before the update) follows ``step``."""
    import math
    from neuralmonkey_amd.optimizers import AdadeltaOptimizer, AdamOptimizer, LazyAdamOptimizer
    b1, b2, eps = 0.8, 0.99, 1e-7
    for lr, at in ((0.25, lambda step: 0.25), (lambda s: 1.0 / (s + 1), lambda step: 1.0 / step)):
        adam = AdamOptimizer(lr, beta1=b1, beta2=b2, epsilon=eps)
        assert adam.kind == 0 and LazyAdamOptimizer(lr).kind == 0
        for step, applied, t in ((1, None, 1), (6, None, 6), (6, 6, 6), (6, 3, 3)):
            want = (at(step) * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t), b1, b2, eps)
            assert adam.params(step, applied) == want, (step, applied)
        assert adam.params(6, 3) != adam.params(6) and adam.params(6, 3)[0] == adam.lr_t(6, 3)
        delta = AdadeltaOptimizer(lr, rho=0.9, epsilon=1e-6, name="delta")
        assert delta.kind == 1 and delta.slot_suffixes == ("/delta", "/delta_1")
        for step in (1, 6):
            assert delta.params(step) == delta.params(step, 2) == (at(step), 0.9, 1e-6, 0.0)
    # the family takes the same call and ignores the count
    from neuralmonkey_amd.optimizers import MomentumOptimizer
    assert MomentumOptimizer(0.1, 0.8).params(4, 2) == MomentumOptimizer(0.1, 0.8).params(4) == (0.1, 0.8, 0.0, 0.0)


def test_centered_rmsprop_constructs_and_is_refused_by_the_trainer(tmp_path):
    from neuralmonkey_amd.optimizers import RMSPropOptimizer
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    opt = RMSPropOptimizer(0.01, centered=True)                 # signature parity
    assert opt.centered is True
    model = _ini_model(tmp_path, INI_SECTIONS["GradientDescentOptimizer"])
    with pytest.raises(NotImplementedError, match="centered"):
        CrossEntropyTrainer(decoders=[model.runners[0].decoder], optimizer=opt)
    from neuralmonkey_amd.optimizers import Optimizer

    class Ftrl(Optimizer):
        pass
    with pytest.raises(NotImplementedError, match="GradientDescent / Momentum / Adagrad / RMSProp; got Ftrl"):
        CrossEntropyTrainer(decoders=[model.runners[0].decoder], optimizer=Ftrl())


# ---- the restatement -------------------------------------------------------------------------------------------------
def _two_tensors(seed=5):
    """'big' (norm ~ 3: a clip of 1 bites) and 'small' (norm ~ 0.1: spared), with two gradients each."""
    rng = np.random.default_rng(seed)
    p = {"big": rng.standard_normal((30, 7)), "small": rng.standard_normal(11)}
    grads = [{"big": rng.standard_normal((30, 7)) * 0.2, "small": rng.standard_normal(11) * 0.03} for _ in range(2)]
    return p, grads


def test_restatements_equal_the_formulas_written_out():
    """Two updates of every kind in float64 against TF 1.12's lines written out here, the clip biting on one tensor
    and sparing the other."""
    clip, lr = 1.0, 0.3
    p0, grads = _two_tensors()

    def close(got, want):
        """float64 on both sides; the operations associate differently (g * (clip / norm) here, (g * clip) / norm
        there): a few units in the last place of values of order one."""
        return np.allclose(got, want, rtol=1e-13, atol=1e-15)

    def clipped(g):
        return g * clip / max(np.sqrt((g ** 2).sum()), clip)
    assert np.sqrt((grads[0]["big"] ** 2).sum()) > clip > np.sqrt((grads[0]["small"] ** 2).sum())

    def run(kind, params, init):
        p = {k: v.copy() for k, v in p0.items()}
        slots = [{k: np.full(v.shape, i) for k, v in p.items()} for i in init] + [None, None]
        counts = [R.clip_and_update(kind, p, g, slots[0], slots[1], clip, params) for g in grads]
        assert counts == [1, 1]
        return p, slots[0], slots[1]

    for k in p0:
        g1, g2 = clipped(grads[0][k]), clipped(grads[1][k])
        # GradientDescent
        got, _, _ = run(2, (lr, 0, 0, 0), ())
        assert close(got[k], p0[k] - lr * g1 - lr * g2)
        # Momentum, plain and Nesterov
        mu = 0.9
        a1 = 0.0 * mu + g1
        a2 = a1 * mu + g2
        got, acc, _ = run(3, (lr, mu, 0, 0), (0.0,))
        assert close(acc[k], a2) and close(got[k], p0[k] - lr * a1 - lr * a2)
        got, acc, _ = run(3, (lr, mu, 1, 0), (0.0,))
        assert close(acc[k], a2)
        assert close(got[k], p0[k] - (g1 * lr + a1 * mu * lr) - (g2 * lr + a2 * mu * lr))
        # Adagrad, accumulator from 0.1, no epsilon
        a1 = 0.1 + g1 * g1
        a2 = a1 + g2 * g2
        got, acc, _ = run(4, (lr, 0, 0, 0), (0.1,))
        assert close(acc[k], a2)
        assert close(got[k], p0[k] - g1 * lr / np.sqrt(a1) - g2 * lr / np.sqrt(a2))
        # RMSProp, rms from ONE, momentum from 0
        decay, mom, eps = 0.9, 0.5, 1e-10
        ms1 = 1.0 + (g1 * g1 - 1.0) * (1 - decay)
        m1 = 0.0 * mom + (g1 * lr) / np.sqrt(ms1 + eps)
        ms2 = ms1 + (g2 * g2 - ms1) * (1 - decay)
        m2 = m1 * mom + (g2 * lr) / np.sqrt(ms2 + eps)
        got, ms, mm = run(5, (lr, decay, mom, eps), (1.0, 0.0))
        assert close(ms[k], ms2) and close(mm[k], m2) and close(got[k], p0[k] - m1 - m2)


def test_restatements_agree_with_torch_optim_where_the_formulas_coincide():
    """float64, two updates behind the same clip, against torch.optim on the CPU.  What makes them coincide:
      * SGD(lr): the same line.
      * SGD(lr, momentum, dampening=0): buf = mu*buf + g; p -= lr*buf is ApplyMomentum with a constant lr (TensorFlow
        keeps lr out of the accumulator too); nesterov=True: p -= lr*(g + mu*buf), TensorFlow's g*lr + accum*mu*lr.
      * Adagrad(lr, lr_decay=0, initial_accumulator_value, eps=0): state_sum += g^2; p -= lr*g/(sqrt(state_sum) + 0).
      * RMSprop(lr, alpha=decay, momentum, eps=0, centered=False): torch's buf = mu*buf + g/sqrt(sq) is TensorFlow's
        mom/lr while lr is constant (TensorFlow folds lr into the accumulator, torch multiplies at the end).  torch
        starts its squared average at ZERO, so this comparison starts the restatement's rms at zero as well (that
        the trainer starts it at one is test_ini_... / the checkpoint tests' business), and it needs epsilon = 0 on
        both sides: TensorFlow adds epsilon INSIDE the square root, torch outside, so no common non-zero value
        exists and RMSProp's epsilon cannot be cross-checked this way."""
    clip, lr = 1.0, 0.3
    p0, grads = _two_tensors(seed=9)

    def torch_run(make):
        params = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p0.items()}
        opt = make(list(params.values()))
        for g in grads:
            for k, v in params.items():
                gk = torch.tensor(g[k], dtype=torch.float64)
                v.grad = gk * (clip / max(float(gk.norm()), clip))
            opt.step()
        return {k: v.detach().numpy() for k, v in params.items()}

    def ref_run(kind, params, init):
        p = {k: v.copy() for k, v in p0.items()}
        slots = [{k: np.full(v.shape, i) for k, v in p.items()} for i in init] + [None, None]
        for g in grads:
            R.clip_and_update(kind, p, g, slots[0], slots[1], clip, params)
        return p

    cases = [
        (lambda ps: torch.optim.SGD(ps, lr=lr), (2, (lr, 0, 0, 0), ())),
        (lambda ps: torch.optim.SGD(ps, lr=lr, momentum=0.9, dampening=0), (3, (lr, 0.9, 0, 0), (0.0,))),
        (lambda ps: torch.optim.SGD(ps, lr=lr, momentum=0.9, dampening=0, nesterov=True), (3, (lr, 0.9, 1, 0), (0.0,))),
        (lambda ps: torch.optim.Adagrad(ps, lr=lr, lr_decay=0, initial_accumulator_value=0.1, eps=0),
         (4, (lr, 0, 0, 0), (0.1,))),
        (lambda ps: torch.optim.RMSprop(ps, lr=lr, alpha=0.9, momentum=0.5, eps=0, centered=False),
         (5, (lr, 0.9, 0.5, 0.0), (0.0, 0.0))),
    ]
    for make, ref in cases:
        want, got = torch_run(make), ref_run(*ref)
        for k in p0:
            assert np.abs(p0[k] - want[k]).max() > 1e-3
            assert np.allclose(got[k], want[k], rtol=1e-12, atol=1e-13), (ref[0], k, np.abs(got[k] - want[k]).max())


# ---- headroom of the direct GPU test's bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(OC.VARIANTS))
def test_float32_restatement_meets_the_gpu_bound_on_the_gpu_inputs(variant):
    """On the exact inputs of tests/test_optim_family_gpu.py::test_family_kernels_direct, the float32 NumPy evaluation
    of the restatement stays within that test's bound (2e-5 x the tensor's largest entry) of the float64 one, after
    each of the two updates: the bound leaves a float32 kernel room."""
    from .test_pointwise_kernels_gpu import _optimizer_setup
    specs, _, host = _optimizer_setup("cpu", OC.seed_of(variant))
    host = OC.prepare(host, variant)
    want = OC.expected(specs, host, variant, np.float64)
    got = OC.expected(specs, host, variant, np.float32)
    for step in range(2):
        assert got[step]["theta"].dtype == np.float32
        OC.compare(specs, got[step], want[step], "{} update {}".format(variant, step + 1))
    # the case means something: the clip bites on two variables and spares one; the frozen variable stays
    norms = {n: float(np.sqrt((want[0]["grad"][sp.offset:sp.offset + sp.size] ** 2).sum())) for n, sp in specs.items()}
    assert norms["w_a"] > OC.CLIP and norms["w_c"] > OC.CLIP > norms["bias_b"]
    sp = specs["frozen"]
    assert np.array_equal(want[1]["theta"][sp.offset:sp.offset + sp.size],
                          host["theta"][sp.offset:sp.offset + sp.size].astype(np.float64))
    assert not np.array_equal(want[1]["theta"], want[0]["theta"])


# ---- the binding table ---------------------------------------------------------------------------------------------
def optim_header_symbols():
    text = open(os.path.join(ROOT, "include", "nmhip_optim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def test_optim_header_matches_its_binding_table(lib):
    from neuralmonkey_amd import _lib
    from .test_abi import header_symbols
    mine = optim_header_symbols()
    assert mine == set(_lib.OPTIM_SIGNATURES) == {"nm_optim_update", "nm_optim_update_list"}
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SIGNATURES") and name != "OPTIM_SIGNATURES"]
    assert len(others) >= 11
    for other in others:
        assert not mine & set(other)
    assert not mine & header_symbols()
    for name, (res, args) in _lib.OPTIM_SIGNATURES.items():
        fn = getattr(lib, name)                                          # exported, and bound by load()
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # the argument lists are those of nm_optim_apply / nm_optim_apply_list
    assert _lib.OPTIM_SIGNATURES["nm_optim_update"] == _lib.SIGNATURES["nm_optim_apply"]
    assert _lib.OPTIM_SIGNATURES["nm_optim_update_list"] == _lib.SIGNATURES["nm_optim_apply_list"]


def test_optim_entry_points_refuse_before_any_launch(lib):
    """Host buffers and a null stream: a call that got as far as a launch would fault or fail differently."""
    buf = (ctypes.c_float * 64)()
    i64 = (ctypes.c_int64 * 8)()
    i32 = (ctypes.c_int32 * 8)()
    need = lib.nm_optim_workspace_bytes(2, 1)
    assert need == 28

    def call(name, kind=3, theta=buf, grad=buf, slot0=buf, slot1=buf, tab=i32, nchunk=2, nseg=1, select=None,
             workspace=buf, nbytes=need):
        if select is None:
            select = (0, 2) if name == "nm_optim_update" else (i32, 2)
        return getattr(lib, name)(None, kind, theta, grad, slot0, slot1, i64, tab, tab, tab, tab, tab, nchunk, nseg,
                                  1.0, 0.1, 0.9, 0.0, 0.0, select[0], select[1], None, workspace, nbytes)

    for name in ("nm_optim_update", "nm_optim_update_list"):
        who = name.encode()
        cases = [(dict(kind=1), who + b": kind 1 (2 GradientDescent, 3 Momentum, 4 Adagrad, 5 RMSProp)"),
                 (dict(kind=6), who + b": kind 6 (2 GradientDescent, 3 Momentum, 4 Adagrad, 5 RMSProp)"),
                 (dict(kind=0), who + b": kind 0 ("),
                 (dict(theta=None), who + b": null theta, grad or workspace"),
                 (dict(grad=None), who + b": null theta, grad or workspace"),
                 (dict(workspace=None), who + b": null theta, grad or workspace"),
                 (dict(tab=None), who + b": null table"),
                 (dict(kind=3, slot0=None), who + b": kind 3 needs slot0"),
                 (dict(kind=4, slot0=None), who + b": kind 4 needs slot0"),
                 (dict(kind=5, slot0=None), who + b": kind 5 needs slot0"),
                 (dict(kind=5, slot1=None), who + b": kind 5 needs slot1"),
                 (dict(nchunk=0), who + b": bad sizes nchunk 0, nseg 1"),
                 (dict(nbytes=need - 1), who + b": workspace of 27 bytes, 28 needed")]
        if name == "nm_optim_update":
            cases += [(dict(select=(-1, 2)), b"nm_optim_update: bad chunk range [-1, 2) of 2"),
                      (dict(select=(2, 1)), b"nm_optim_update: bad chunk range [2, 1) of 2"),
                      (dict(select=(0, 3)), b"nm_optim_update: bad chunk range [0, 3) of 2")]
        else:
            cases += [(dict(select=(i32, -1)), b"nm_optim_update_list: bad chunk list (-1 of 2)"),
                      (dict(select=(i32, 3)), b"nm_optim_update_list: bad chunk list (3 of 2)"),
                      (dict(select=(None, 1)), b"nm_optim_update_list: bad chunk list (1 of 2)")]
        for kwargs, text in cases:
            assert call(name, **kwargs) < 0, (name, kwargs)
            assert lib.nm_last_error().startswith(text), (kwargs, lib.nm_last_error())
        # an empty range / list is a no-op -- nothing is launched (these are host buffers) -- also with the slots a
        # kind does not have missing
        empty = (1, 1) if name == "nm_optim_update" else (None, 0)
        assert call(name, select=empty) == 0
        assert call(name, kind=2, slot0=None, slot1=None, select=empty) == 0
        assert call(name, kind=3, slot1=None, select=empty) == 0
        assert call(name, kind=4, slot1=None, select=empty) == 0
        assert call(name, kind=5, select=empty) == 0
    # kinds 2..5 stay refused where they always were
    assert lib.nm_optim_apply(None, 3, buf, buf, buf, buf, i64, i32, i32, i32, i32, i32, 2, 1, 1.0, 0.1, 0.9, 0.0, 0.0,
                              0, 2, None, buf, need) < 0
    assert b"nm_optim_apply: kind 3" in lib.nm_last_error()


# ---- checkpoints on a CPU store ------------------------------------------------------------------------------------
SHAPES = {"enc/embedding": (7, 5), "enc/bias": (5,), "dec/W": (5, 9), "dec/moving_mean": (9,)}


def _store(seed=3):
    from neuralmonkey_amd.variables import VariableStore, random_normal_initializer
    st = VariableStore("cpu", seed=seed)
    for name, shape in SHAPES.items():
        st.declare(name, shape, random_normal_initializer(stddev=0.3), trainable=name != "dec/moving_mean")
    st.finalize()
    return st


def _optimizers():
    from neuralmonkey_amd.optimizers import (AdagradOptimizer, GradientDescentOptimizer, MomentumOptimizer,
                                             RMSPropOptimizer)
    return {2: GradientDescentOptimizer(0.1), 3: MomentumOptimizer(0.1, 0.9), 4: AdagradOptimizer(0.1, name="ada"),
            5: RMSPropOptimizer(0.1)}


def _read_keys(path, fmt):
    if fmt == "tf":
        from neuralmonkey_amd import tf_bundle
        return set(tf_bundle.read_bundle(path))
    with np.load(path + ".npz") as data:
        return {k.replace("|", "/") for k in data.files}


@pytest.mark.parametrize("fmt", ["npz", "tf"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_checkpoints_carry_exactly_the_slots_the_optimizer_has(tmp_path, kind, fmt):
    opt = _optimizers()[kind]
    st = _store()
    # what the trainer's first step does to the store: the optimizer's slots, under its names, at their initial values
    slots = st.ensure_slots(opt.slot_initial)
    st.slot_suffixes = tuple(opt.slot_suffixes)
    assert [s is not None for s in slots] == [R.SLOTS[kind] >= 1, R.SLOTS[kind] >= 2]
    assert (st.adam_m is None) == (R.SLOTS[kind] == 0) and (st.adam_v is None) == (R.SLOTS[kind] < 2)
    for s, value in zip(st.slots(), opt.slot_initial):
        assert s.shape == (st.total,) and bool((s == value).all())
    rng = np.random.default_rng(kind)
    for s in st.slots():
        s.copy_(torch.from_numpy(rng.standard_normal(st.total).astype(np.float32)))
    path = str(tmp_path / "variables.data")
    st.save(path, fmt=fmt, global_step=4)
    keys = _read_keys(path, fmt)
    trainable = [n for n in SHAPES if n != "dec/moving_mean"]
    want = set(SHAPES) | {"global_step"} | {n + s for n in trainable for s in opt.slot_suffixes}
    assert keys == want
    assert "beta1_power" not in keys and not any(k.endswith("/Adam") or k.endswith("/Adam_1") for k in keys)
    if kind == 3:
        assert "dec/W/Momentum" in keys and "dec/W/Momentum_1" not in keys
    # into a fresh store, which has not named its slots yet
    fresh = _store(seed=8)
    assert fresh.slot_suffixes == ("/Adam", "/Adam_1") and fresh.adam_m is None
    info = fresh.load(path)
    assert info["global_step"] == 4 and torch.equal(fresh.theta, st.theta)
    assert len(fresh.slots()) == R.SLOTS[kind]
    if R.SLOTS[kind]:
        assert fresh.slot_suffixes == tuple(opt.slot_suffixes)
    for got, saved in zip(fresh.slots(), st.slots()):
        for n in trainable:
            sp = st.specs[n]
            assert torch.equal(got[sp.offset:sp.offset + sp.size], saved[sp.offset:sp.offset + sp.size])
    # ... and written again: the same keys
    again = str(tmp_path / "again.data")
    fresh.save(again, fmt=fmt, global_step=4)
    assert _read_keys(again, fmt) == keys


@pytest.mark.parametrize("fmt", ["npz", "tf"])
def test_two_slot_checkpoints_are_written_as_before(tmp_path, fmt):
    """Adam's checkpoint: both slots of every trainable variable and, in the TF format, the beta powers."""
    st = _store()
    m, v = st.ensure_adam()
    m.fill_(0.25)
    v.fill_(0.5)
    path = str(tmp_path / "variables.data")
    st.save(path, fmt=fmt, global_step=2)
    keys = _read_keys(path, fmt)
    trainable = [n for n in SHAPES if n != "dec/moving_mean"]
    want = set(SHAPES) | {"global_step"} | {n + s for n in trainable for s in ("/Adam", "/Adam_1")}
    assert keys == want | ({"beta1_power", "beta2_power"} if fmt == "tf" else set())
    if fmt == "npz":                            # slot keys follow their variable, first slot first
        with np.load(path + ".npz") as data:
            files = list(data.files)
        i = files.index("enc|embedding|Adam")
        assert files[i + 1] == "enc|embedding|Adam_1" and files[i + 2] == "enc|bias|Adam"


@pytest.mark.parametrize("fmt", ["npz", "tf"])
def test_adam_checkpoint_under_a_momentum_trainer_warns_and_starts_the_slot_afresh(tmp_path, fmt):
    from types import SimpleNamespace
    from neuralmonkey_amd.optimizers import AdagradOptimizer
    st = _store()
    m, v = st.ensure_adam()
    m.fill_(-0.25)
    v.fill_(0.5)
    path = str(tmp_path / "variables.data")
    st.save(path, fmt=fmt, global_step=2)
    model = _ini_model(tmp_path, INI_SECTIONS["MomentumOptimizer"])
    trainer = model.trainer
    fresh = _store(seed=8)
    fresh.load(path)
    assert fresh.slot_suffixes == ("/Adam", "/Adam_1") and bool((fresh.adam_v[:35] == 0.5).all())
    sess = SimpleNamespace(global_step=2)
    with pytest.warns(UserWarning, match="do not belong to MomentumOptimizer"):
        state = trainer._adam_state(sess, fresh)                                   # pylint: disable=protected-access
    assert state["v"] is None and fresh.adam_v is None and state["m"] is fresh.adam_m and state["applied"] == 2
    assert bool((state["m"] == 0.0).all()) and fresh.slot_suffixes == ("/momentum",)
    # Adagrad: the accumulator goes back to its initial value, not to zero (rsqrt(0) would be infinite)
    other = _ini_model(tmp_path, INI_SECTIONS["AdagradOptimizer"]).trainer
    fresh = _store(seed=8)
    fresh.load(path)
    with pytest.warns(UserWarning, match="reset to their initial values"):
        state = other._adam_state(SimpleNamespace(global_step=2), fresh)          # pylint: disable=protected-access
    assert isinstance(other.optimizer, AdagradOptimizer) and state["v"] is None and bool((state["m"] == 0.5).all())
    # a GradientDescent trainer allocates no slot buffer at all; a second trainer on the store gets private slots at
    # ITS optimizer's initial values
    sgd = _ini_model(tmp_path, INI_SECTIONS["GradientDescentOptimizer"]).trainer
    clean = _store()
    shared = SimpleNamespace(global_step=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        state = sgd._adam_state(shared, clean)                                     # pylint: disable=protected-access
        second = other._adam_state(shared, clean)                                  # pylint: disable=protected-access
    assert state["m"] is None and state["v"] is None and clean.adam_m is None and clean.slot_suffixes == ()
    assert second["v"] is None and bool((second["m"] == 0.5).all()) and second["applied"] == 0 and clean.adam_m is None
