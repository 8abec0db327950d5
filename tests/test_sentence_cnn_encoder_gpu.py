"""The assembled SentenceCNNEncoder on the MI355X against the float64 restatement of tests/sent_cnn_ref.py: one
training-mode run of the encoder (input dropout at keep 0.5 included, its mask regenerated from the same salt and step)
gives temporal_states, output and temporal_mask, and its backward pass -- a loss sum(states . dS) + sum(output . dF) --
the gradient of every variable of the encoder, each against float64 autograd.  Two configurations: tests/small_sent_cnn.ini
verbatim (E = 11, GRU 7: the step-by-step GRU tape) and the same file at sizes where the GRU layer runs as cluster
loops (E = 16, 64 filters, GRU 256)."""
import pytest
import torch

from . import sent_cnn_ref as R
from .test_sentence_cnn import cnn_root  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu

VARIANTS = {
    "ini": {},
    "cluster": {"embedding_size=11": "embedding_size=16", "max_length=10\n": "max_length=40\n", "rnn_size=7": "rnn_size=256",
                "filters=[(1,13), (2,13), (3,13)]": "filters=[(1,16), (2,16), (3,32)]", "highway_depth=3": "highway_depth=2"},
}


def _load(root, variant, dev):
    import os
    from .test_reference_inis import load_verbatim
    name = "small_sent_cnn"
    if VARIANTS[variant]:
        with open(os.path.join(root, "tests", name + ".ini")) as fh:
            text = fh.read()
        for old, new in VARIANTS[variant].items():
            assert old in text, old
            text = text.replace(old, new)
        name = "small_sent_cnn_" + variant
        with open(os.path.join(root, "tests", name + ".ini"), "w") as fh:
            fh.write(text)
    return load_verbatim(root, name, device=str(dev), seed=1234)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_whole_encoder_and_every_variable_gradient_match_float64(dev, cnn_root, variant, monkeypatch):  # noqa: F811
    from neuralmonkey_amd import ops
    from neuralmonkey_amd.dataset import BatchingScheme
    from neuralmonkey_amd.encoders import SentenceCNNEncoder
    from neuralmonkey_amd.runtime import RunContext
    taken = []
    real = SentenceCNNEncoder._gru_cluster_layer

    def spy(self, *a, **kw):
        out = real(self, *a, **kw)
        taken.append(out is not None)
        return out
    monkeypatch.setattr(SentenceCNNEncoder, "_gru_cluster_layer", spy)

    model = _load(cnn_root, variant, dev)
    enc = model.runners[0].decoder.encoders[0]
    seq = enc.input_sequence
    assert isinstance(enc, SentenceCNNEncoder) and enc.dropout_keep_prob == 0.5
    sess = model.tf_manager.sessions[0]
    store = sess.store
    batch = next(model.train_dataset.batches(BatchingScheme(batch_size=16)))
    fd = {}
    for part in (enc, seq):
        fd.update(part.feed_dict(batch, train=True))
    ctx = RunContext(sess, fd)
    # variables moved off their initial values a little, so that no gate sits at its initial bias
    g = torch.Generator(device=dev).manual_seed(5)
    names = [n for n in store.names() if n.startswith(enc.name + "/")]
    for n in names:
        store[n].add_(torch.randn(store[n].shape, device=dev, generator=g) * 0.05)
    ops.zero(store.ensure_grad())

    states, final, pmask = enc.temporal_states(ctx), enc.output(ctx), enc.temporal_mask(ctx)
    x, mask, lengths = seq.temporal_states(ctx), seq.temporal_mask(ctx), seq.lengths(ctx)
    bsz, slen, e = x.shape
    ones = torch.ones(bsz * slen, e, device=dev)
    drop = torch.empty_like(ones)
    ops.dropout(ones, drop, enc.dropout_keep_prob, ctx.salt(enc.name, "cnn_input"), step=sess.step_tensor())
    d_states = torch.randn(states.shape, device=dev, generator=g)
    d_final = torch.randn(final.shape, device=dev, generator=g)
    got_states, got_final, got_mask = states.clone(), final.clone(), pmask.clone()
    enc.backward(ctx, d_states, d_final)
    torch.cuda.synchronize()
    assert taken and all(t == (variant == "cluster") for t in taken), taken

    cpu = lambda t: t.detach().double().cpu()
    params = {n[len(enc.name) + 1:]: cpu(store[n]).requires_grad_(True) for n in names}
    lens = lengths.long().cpu()
    ref_states, ref_final, ref_mask = R.encoder(cpu(x), cpu(mask), lens, params, enc.filters, enc.segment_size,
                                                enc.highway_depth, drop=cpu(drop).view(bsz, slen, e))
    # the mask: SAME max-pool of the token mask, one position longer than ceil(len / s) where the windows shift
    assert torch.equal(cpu(got_mask), ref_mask)
    scale = max(float(ref_states.abs().max()), 1e-3)
    assert float((cpu(got_states) - ref_states).abs().max()) < 2e-5 * scale
    assert float((cpu(got_final) - ref_final).abs().max()) < 2e-5 * max(float(ref_final.abs().max()), 1e-3)
    loss = (ref_states * cpu(d_states)).sum() + (ref_final * cpu(d_final)).sum()
    loss.backward()
    for local, p in params.items():
        want = p.grad
        have = cpu(store.g(enc.name + "/" + local))
        err = float((have - want).abs().max()) / max(float(want.abs().max()), 1e-6)
        assert err < 1e-4, (local, err)
    assert len(params) == 2 * len(enc.filters) + 4 * enc.highway_depth + 8      # every variable of the encoder
