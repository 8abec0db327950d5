"""encoders.facebook_conv.SentenceEncoder on the MI355X.

  * every fixture of tests/golden/convs2s (numbers of the REFERENCE'S OWN Python, see make_convs2s_golden.py): the
    fixture's variables loaded by name, its strings fed (uncut: the sequence's max_length cuts them); every recorded
    tensor within 1e-4 of the tensor's largest magnitude, the cost within 1e-4 relative, the decoded classes equal;
  * the engine's gradient against central differences of the reference's cost (6e-3 + 2e-2 |fd|), the order embeddings
    beyond the batch's length with an exactly zero gradient;
  * the reference's tests/bpe.ini, byte for byte from its bundle: variables initialise, three optimizer steps, greedy
    decoding, a save / load round trip."""
import numpy as np
import pytest
import torch

from . import convs2s_models as M
from .test_convs2s_host import bpe_root  # noqa: F401  pylint: disable=unused-import
from .test_reference_exec_gpu import close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", M.FORWARD_CASES)
def test_engine_equals_the_reference(dev, case):
    z, cfg, _, m, _, fd = M.loaded(dev, case)
    enc, dec = m["enc"], m["dec"]
    assert np.array_equal(fd[m["seq"].input_factors[0]], z["in/src_ids"])          # max_length cut the same words
    fetches = {"ordered_embedded_inputs": enc.ordered_embedded_inputs, "temporal_states": enc.temporal_states,
               "temporal_mask": enc.temporal_mask, "output": enc.output}
    if dec is not None:
        assert np.array_equal(fd[dec.targets_placeholder], z["in/tgt_ids"])
        fetches.update(avg_output=m["avg"].output, decoded_seq=dec.decoded_seq, decoded_logits=dec.decoded_logits,
                       cost=dec.cost)
    out = m["tfm"].sessions[0].run(fetches, fd)
    recorded = sorted(k[4:] for k in z.files if k.startswith("out/") and not k.startswith("out/variable_"))
    assert recorded == sorted(fetches)                                     # every out/* tensor is compared
    for key in fetches:
        if key in ("decoded_seq", "temporal_mask"):
            assert np.array_equal(out[key], z["out/" + key]), key
        else:
            print("{} {}: max |diff| {:.3e}".format(case, key, float(np.abs(
                np.asarray(out[key], np.float64) - z["out/" + key]).max())))
            close(out[key], z["out/" + key], case + " " + key, 1e-4)
    assert np.array_equal(out["output"], out["temporal_states"].max(axis=1))       # over padded positions too


@pytest.mark.parametrize("case", M.FD_CASES)
def test_engine_gradients_against_the_reference_finite_differences(dev, case):
    z, cfg, _, m, ds, _ = M.loaded(dev, case)
    res = m["tfm"].execute(ds, m["trainer"].feedables, [m["trainer"]], train=True)[0]
    close(res.losses["classifier - cost"], z["out/cost"], "cost", 1e-4)
    store = m["store"]
    seen = set()
    for name, i, fd in zip([str(n) for n in z["fd/names"]], z["fd/index"], z["fd/value"]):
        got = float(store.g(name).reshape(-1)[int(i)])
        print("{}[{}]: engine {:.6f} finite difference {:.6f}".format(name, i, got, fd))
        assert abs(got - fd) <= 6e-3 + 2e-2 * abs(fd), "{}[{}]: engine {:.6f} vs finite difference {:.6f}".format(
            name, i, got, fd)
        seen.add(name)
    assert seen == set(store.names())
    steps = z["out/temporal_states"].shape[1]
    table = store.g("encoder/input_projection/order_embeddings").cpu().numpy()
    assert table.shape[0] == cfg["max_length"] > steps
    assert not table[steps:].any() and table[:steps].any(axis=1).all()


def _batches(dataset, n, size):
    from neuralmonkey_amd.dataset import BatchingScheme
    out = []
    for b in dataset.batches(BatchingScheme(batch_size=size)):
        out.append(b)
        if len(out) == n:
            break
    return out


def test_bpe_ini_trains_decodes_and_round_trips(dev, bpe_root, tmp_path):  # noqa: F811
    from .test_reference_inis import load_verbatim
    model = load_verbatim(bpe_root, "bpe", device=str(dev), seed=1234)
    tfm = model.tf_manager
    store = tfm.sessions[0].store
    mine = [n for n in store.names() if n.startswith("sentence_encoder/")]
    assert len(mine) == 9 and all(bool(torch.isfinite(store[n]).all()) for n in mine)
    assert float(store["sentence_encoder/encoder_conv_0/convolution_filters"].abs().max()) > 0
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    step0 = tfm.sessions[0].global_step
    losses = []
    for batch in _batches(model.train_dataset, 3, model.batch_size):
        res = tfm.execute(batch, feedables, model.trainers, train=True)
        assert res[0].losses and all(np.isfinite(v) for v in res[0].losses.values()), res[0].losses
        losses.append(float(sum(res[0].losses.values())))
    assert tfm.sessions[0].global_step == step0 + 3 and len(set(losses)) == 3
    assert all(bool(torch.isfinite(store[n]).all()) for n in mine)
    val = _batches(model.val_dataset, 1, model.batch_size)[0]
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)
    decoded = out[0].outputs["target_greedy"] if isinstance(out[0].outputs, dict) else out[0].outputs
    assert len(decoded) == len(val)
    path = str(tmp_path / "variables.data")
    tfm.save(path)
    again = load_verbatim(bpe_root, "bpe", device=str(dev), seed=99)
    again.tf_manager.restore(path)
    out2 = again.tf_manager.execute(val, set.union(*[r.feedables for r in again.runners]), again.runners,
                                    compute_losses=False)
    decoded2 = out2[0].outputs["target_greedy"] if isinstance(out2[0].outputs, dict) else out2[0].outputs
    assert decoded2 == decoded
