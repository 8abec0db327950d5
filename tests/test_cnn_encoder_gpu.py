"""encoders.cnn_encoder.CNNEncoder and CNNTemporalView on the MI355X.

  * every fixture of tests/golden/cnn2d (numbers of the REFERENCE'S OWN Python, see make_cnn2d_golden.py): the fixture's
    variables loaded by name, its images fed; every recorded tensor within 1e-4 of the tensor's largest magnitude, masks
    and shapes exact, in inference mode and -- where recorded -- in training mode with the batch statistics;
  * the engine's gradient against central differences of the reference's cost (6e-3 + 2e-2 |fd|);
  * the moving statistics after one trainer step, and untouched by a runner;
  * the reference's tests/str.ini with NumPy images in place of its image reader: Adadelta steps, greedy decoding, a
    save / load round trip."""
import numpy as np
import pytest
import torch

from . import cnn2d_models as M
from .test_cnn2d_host import str_root, with_numpy_images  # noqa: F401  pylint: disable=unused-import
from .test_reference_exec_gpu import close

pytestmark = pytest.mark.gpu


def fetches_of(m, train):
    cnn = m["cnn"]
    fetches = {"image_mask": cnn.image_mask, "layers": cnn.image_processing_layers, "spatial_states": cnn.spatial_states,
               "spatial_mask": cnn.spatial_mask, "output": cnn.output}
    if train and cnn.batch_normalize:
        fetches["stats"] = cnn.batch_statistics
    if m["view"] is not None:
        fetches.update(temporal_states=m["view"].temporal_states, temporal_mask=m["view"].temporal_mask,
                       enc_states=m["enc"].temporal_states, enc_output=m["enc"].output, pool_output=m["pool"].output)
    if m["dec"] is not None:
        fetches.update(decoded_logits=m["dec"].decoded_logits, cost=m["dec"].cost)
    return fetches


def flatten(out):
    """The run's results under the names the fixtures record them by."""
    flat = {}
    for key, val in out.items():
        if key == "layers":
            for i, (states, mask) in enumerate(val):
                flat["layer_{}_states".format(i)], flat["layer_{}_mask".format(i)] = states, mask
        elif key == "stats":
            for name, arr in val.items():
                flat["stats/cnn/" + name] = arr
        else:
            flat[key] = val
    return flat


@pytest.mark.parametrize("case", M.ALL_CASES)
def test_engine_equals_the_reference(dev, case):
    z, cfg, params, m, ds = M.loaded(dev, case)
    frozen_before = {n: m["store"][n].clone() for n in m["store"].names() if n not in m["store"].trainable_names()}
    for prefix, train in M.passes(case, cfg):
        want = M.recorded(z, prefix)
        out = flatten(m["tfm"].sessions[0].run(fetches_of(m, train), M.feed(m, ds, train)))
        if not any(k.startswith("layer_") for k in want):                  # a pass recorded without its per-layer maps
            out = {k: v for k, v in out.items() if not k.startswith("layer_")}
        assert sorted(out) == sorted(want), (prefix, sorted(set(out) ^ set(want)))      # every recorded tensor is compared
        for key in sorted(want):
            got = np.asarray(out[key].cpu() if isinstance(out[key], torch.Tensor) else out[key])
            assert got.shape == want[key].shape, (key, got.shape, want[key].shape)
            if key.endswith("mask"):
                assert np.array_equal(got, want[key]), key
            else:
                print("{} {}{}: max |diff| {:.3e}".format(case, prefix, key, float(np.abs(got - want[key]).max())))
                close(got, want[key], case + " " + prefix + key, 1e-4)
    # runners never move the moving statistics, whatever train_mode they feed
    for name, before in frozen_before.items():
        assert torch.equal(m["store"][name], before), name


@pytest.mark.parametrize("case", M.FD_CASES)
def test_engine_gradients_against_the_reference_finite_differences(dev, case):
    z, cfg, params, m, ds = M.loaded(dev, case)
    store = m["store"]
    frozen = {str(n) for n in z["out/non_trainable"]}
    assert frozen == set(store.names()) - set(store.trainable_names()) and frozen
    res = m["tfm"].execute(ds, m["trainer"].feedables, [m["trainer"]], train=True)[0]
    close(res.losses["classifier - cost"], z["out/cost"], "cost", 1e-4)
    seen = set()
    for name, i, fd in zip([str(n) for n in z["fd/names"]], z["fd/index"], z["fd/value"]):
        got = float(store.g(name).reshape(-1)[int(i)])
        print("{}[{}]: engine {:.6f} finite difference {:.6f}".format(name, i, got, fd))
        assert abs(got - fd) <= 6e-3 + 2e-2 * abs(fd), "{}[{}]: engine {:.6f} vs finite difference {:.6f}".format(
            name, i, got, fd)
        seen.add(name)
    assert seen == set(store.trainable_names())                        # every variable that has a gradient is seen
    for name in frozen:
        assert not bool(store.g(name).any()), name                      # ... and the moving statistics have none


def test_moving_statistics_after_a_trainer_step_and_a_runner(dev):
    """cnn_str_stack under a trainer: moving = 0.99 init + 0.01 recorded batch statistics, the variance times
    n / (n - 1); updated once per step; a runner's execution leaves them alone."""
    from neuralmonkey_amd.decoders import Classifier
    from neuralmonkey_amd.runners import GreedyRunner
    from neuralmonkey_amd.tf_manager import TensorFlowManager
    from neuralmonkey_amd.trainers import CrossEntropyTrainer
    z, cfg, params = M.load_fixture("cnn_str_stack")
    m = M.build_parts(cfg)
    dec = Classifier(name="classifier", encoders=[m["cnn"]], vocabulary=M.words(5), data_id="target", layers=[],
                     dropout_keep_prob=1.0)
    trainer = CrossEntropyTrainer(decoders=[dec], l2_weight=0.0, clip_norm=None)
    runner = GreedyRunner(output_series="cls", decoder=dec)
    tfm = TensorFlowManager(num_sessions=1, num_threads=1, device=str(dev), seed=1)
    tfm.initialize_sessions()
    store = tfm.sessions[0].store
    store.load_state_dict(params, strict=False)
    from neuralmonkey_amd.dataset import BatchingScheme, Dataset
    images = [np.asarray(im) for im in z["in/images"]]
    ds = Dataset("fixture", {"images": images, "target": [["w1"], ["w2"], ["w0"]]}, BatchingScheme(batch_size=3))
    stats = {k[len("out/train/stats/"):]: z[k] for k in z.files if k.startswith("out/train/stats/")}
    assert len(stats) == 8
    maps = M.restate(cfg, params, z["in/images"], True)
    sizes = {"layer_0_convolution": maps["layer_0_states"], "project_input": maps["layer_2_states"],
             "conv_a": maps["layer_1_states"], "conv_b": maps["layer_2_states"]}

    def expected():
        want = {}
        for key, batch in stats.items():
            scope, leaf = key.rsplit("/", 1)
            n = [v for k, v in sizes.items() if k in scope][0][..., 0].size
            if leaf == "batch_mean":
                want[scope + "/moving_mean"] = 0.99 * params[scope + "/moving_mean"] + 0.01 * batch
            else:
                want[scope + "/moving_variance"] = 0.99 * params[scope + "/moving_variance"] + 0.01 * batch * n / (n - 1)
        return want
    tfm.execute(ds, runner.feedables, [runner], compute_losses=True)
    for name in expected():
        assert np.array_equal(store[name].cpu().numpy(), params[name].astype(np.float32)), name      # a runner: unchanged
    tfm.execute(ds, trainer.feedables, [trainer], train=True)
    for name, want in expected().items():
        got = store[name].cpu().numpy().astype(np.float64)
        print("{}: max |diff| {:.3e}".format(name, float(np.abs(got - want).max())))
        assert np.abs(got - want).max() <= 1e-5 * max(1.0, float(np.abs(want).max())), name
        assert np.abs(got - params[name]).max() > 1e-4                   # they did move, once
    after = {name: store[name].clone() for name in expected()}
    tfm.execute(ds, runner.feedables, [runner], compute_losses=True)
    assert all(torch.equal(store[name], val) for name, val in after.items())


def _batches(dataset, n, size):
    from neuralmonkey_amd.dataset import BatchingScheme
    out = []
    for b in dataset.batches(BatchingScheme(batch_size=size)):
        out.append(b)
        if len(out) == n:
            break
    return out


def test_str_ini_trains_decodes_and_round_trips(dev, str_root, tmp_path):  # noqa: F811
    """tests/str.ini over 3 batches of 4 synthetic images: Adadelta steps with finite losses, a loss that has gone down
    after eight steps on one repeated batch, greedy decoding, checkpoint save -> restore -> identical outputs (the moving
    statistics travel along)."""
    from .test_reference_inis import load_verbatim
    ini = with_numpy_images(str_root, n_train=12, n_val=4)
    model = load_verbatim(str_root, ini, device=str(dev), seed=1234)
    tfm = model.tf_manager
    store = tfm.sessions[0].store
    mine = [n for n in store.names() if n.startswith("cnn/")]
    assert len(mine) == 24 and all(bool(torch.isfinite(store[n]).all()) for n in mine)
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    batches = _batches(model.train_dataset, 3, model.batch_size)
    assert [len(b) for b in batches] == [4, 4, 4]
    step0 = tfm.sessions[0].global_step
    moving = "cnn/convolutions/layer_0_convolution/batch_normalization/moving_mean"
    before = store[moving].clone()
    losses = []
    for batch in batches:
        res = tfm.execute(batch, feedables, model.trainers, train=True)
        assert res[0].losses and all(np.isfinite(v) for v in res[0].losses.values()), res[0].losses
        losses.append(float(sum(res[0].losses.values())))
    assert tfm.sessions[0].global_step == step0 + 3 and len(set(losses)) == 3
    assert not torch.equal(store[moving], before) and all(bool(torch.isfinite(store[n]).all()) for n in mine)
    # "Decreasing" needs a loss that can show it: str.ini's learning rate of 1e-4 moves a weight by about 5e-7 in
    # Adadelta's first steps, far below what the decoder's dropout of 0.5 does to the loss from step to step.  The INI
    # is as the reference has it; on the BUILT objects the test now takes the dropout out and gives Adadelta its
    # customary learning rate of 1, then repeats one batch (training mode: the batch's own statistics, no noise left).
    dec = model.runners[0].decoder
    assert dec.dropout_keep_prob == 0.5 and model.trainers[0].optimizer.learning_rate(1) == 1.0e-4
    dec.dropout_keep_prob = 1.0
    model.trainers[0].optimizer._lr = 1.0                                # pylint: disable=protected-access
    objective = model.trainers[0].objectives[0].name                    # (the losses also list the raw L1 / L2 norms)
    repeated = []
    for _ in range(8):
        res = tfm.execute(batches[0], feedables, model.trainers, train=True)
        repeated.append(float(res[0].losses[objective]))
    print("str.ini, one batch repeated:", repeated)
    # (Adadelta promises no descent step by step -- its first updates have the same size for every weight --, so what
    # is asked is progress over the run: the last loss below the first)
    assert all(np.isfinite(v) for v in repeated) and repeated[-1] < repeated[0], repeated
    val = _batches(model.val_dataset, 1, model.batch_size)[0]
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)
    decoded = out[0].outputs["target_chars"] if isinstance(out[0].outputs, dict) else out[0].outputs
    assert len(decoded) == len(val) == 4
    path = str(tmp_path / "variables.data")
    tfm.save(path)
    again = load_verbatim(str_root, ini, device=str(dev), seed=99)
    again.tf_manager.restore(path)
    store2 = again.tf_manager.sessions[0].store
    assert torch.equal(store2[moving], store[moving])
    out2 = again.tf_manager.execute(val, set.union(*[r.feedables for r in again.runners]), again.runners,
                                    compute_losses=False)
    decoded2 = out2[0].outputs["target_chars"] if isinstance(out2[0].outputs, dict) else out2[0].outputs
    assert decoded2 == decoded
