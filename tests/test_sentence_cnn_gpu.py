"""SentenceCNNEncoder on the MI355X: the fused conv + bias + relu + segment-max kernels (MFMA and scalar) and the
highway kernels against float64 restatements, and tests/small_sent_cnn.ini -- loaded byte for byte from its bundle --
training, decoding and surviving a save / load round trip."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from .test_sentence_cnn import cnn_root  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu


def _ref_conv(x, weights, biases):
    """[B, n_i, S] relu(conv1d SAME + b) per width, float64."""
    outs = []
    for w, b in zip(weights, biases):
        width = w.shape[0]
        pad = (width - 1) // 2
        xp = TF.pad(x.transpose(1, 2), (pad, width - 1 - pad))
        outs.append(TF.conv1d(xp, w.permute(2, 1, 0)) + b[None, :, None])
    return outs


def _ref_pool(r, s):
    """SAME max-pool of [B, n, S] over windows of s, stride s: [B, n, S']."""
    slen = r.shape[2]
    sp = (slen + s - 1) // s
    pb = (sp * s - slen) // 2
    rp = TF.pad(r, (pb, sp * s - slen - pb), value=-math.inf)
    return rp.view(r.shape[0], r.shape[1], sp, s).max(-1).values


CASES = [  # (B, S, E, [(w, n)], s, algo)
    (3, 10, 11, [(1, 13), (2, 13), (3, 13)], 5, 0),       # tests/small_sent_cnn.ini's encoder, S a multiple of s
    (3, 12, 11, [(1, 13), (2, 13), (3, 13)], 5, 0),       # S = 12, s = 5: the windows shift
    (2, 13, 11, [(2, 300), (5, 13)], 5, 0),
    (2, 53, 128, [(4, 200), (8, 300)], 5, 0),
    (2, 50, 128, [(1, 13), (3, 200), (5, 300)], 5, 0),
    (3, 7, 11, [(2, 13), (4, 200)], 3, 0),
    (2, 131, 128, [(3, 200)], 128, 0),                   # the widest window of the MFMA path
    (2, 29, 128, [(2, 13), (8, 200)], 4, 2),             # the scalar kernels on the same ground
    (2, 23, 11, [(9, 13), (1, 13)], 6, 0),               # a width the MFMA path does not take: scalar kernels
    (3, 12, 11, [(1, 13), (2, 13), (3, 13)], 5, 2),
    # more than one forward time tile (25 windows of 5) and more than one 128-row data-gradient tile, S mod 5 = 1 / 4 / 0
    (2, 126, 128, [(2, 200), (3, 13), (8, 300)], 5, 0),
    (2, 131, 11, [(1, 13), (4, 200), (5, 300)], 5, 0),
    (2, 250, 128, [(2, 13), (7, 300)], 5, 0),
    (2, 129, 128, [(6, 200), (1, 300)], 5, 0),
    (2, 126, 11, [(2, 13), (3, 200)], 5, 2),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-S{}-E{}-{}-s{}-algo{}".format(
    c[0], c[1], c[2], "_".join("{}x{}".format(w, n) for w, n in c[3]), c[4], c[5]))
def test_conv_pool_forward_and_gradients_match_float64(dev, case):
    from neuralmonkey_amd import ops
    bsz, slen, e, filters, s, algo = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(bsz, slen, e, generator=g, dtype=torch.float64)
    ws = [torch.randn(w, e, n, generator=g, dtype=torch.float64) / math.sqrt(w * e) for w, n in filters]
    bs = [torch.randn(n, generator=g, dtype=torch.float64) * 0.1 for _, n in filters]
    width = sum(n for _, n in filters)
    sp, pb = ops.conv1d_pool_shape(slen, s)
    lengths = torch.randint(1, slen + 1, (bsz,), generator=g, dtype=torch.int32)
    lengths[0] = min(slen, s)                          # a sentence of one segment
    mask = (torch.arange(slen)[None, :] < lengths[:, None].long()).double()

    f32 = lambda t: t.float().contiguous().to(dev)
    xd, wd, bd = f32(x), [f32(w) for w in ws], [f32(b) for b in bs]
    pooled = torch.empty(bsz, sp, width, device=dev)
    arg = torch.empty(bsz, sp, width, dtype=torch.int32, device=dev)
    mask_out = torch.empty(bsz, sp, device=dev)
    lens_out = torch.empty(bsz, dtype=torch.int32, device=dev)
    ops.conv1d_pool_fwd(xd, wd, bd, s, pooled, arg, mask=f32(mask), lengths=lengths.to(dev), mask_out=mask_out,
                        seq_lens=lens_out, algo=algo)
    torch.cuda.synchronize()

    # forward: values within the fp32 error scale of the products, every argmax a (near-)maximum of its window
    convs = _ref_conv(x, ws, bs)
    scales = _ref_conv(x.abs(), [w.abs() for w in ws], [b.abs() for b in bs])
    ref = torch.cat([_ref_pool(torch.relu(c), s) for c in convs], 1).transpose(1, 2)           # [B, S', F]
    scale = torch.cat([_ref_pool(c, s) for c in scales], 1).transpose(1, 2)
    tol = 1e-6 * scale + 1e-7
    got = pooled.double().cpu()
    assert bool(((got - ref).abs() <= 10 * tol).all()), float((got - ref).abs().max())
    relu_all = torch.relu(torch.cat(convs, 1))                                                    # [B, F, S]
    a = arg.long().cpu()
    j = torch.arange(sp)[None, :, None]
    assert bool(((a >= j * s - pb) & (a < j * s - pb + s) & (a >= 0) & (a < slen)).all())
    at_arg = relu_all.gather(2, a.transpose(1, 2)).transpose(1, 2)
    assert bool(((at_arg - ref).abs() <= 10 * tol).all())
    # the pooled mask and lengths (mask can be one segment longer than ceil(len / s))
    assert torch.equal(mask_out.cpu().double(), _ref_pool(mask[:, None, :], s)[:, 0])
    assert torch.equal(lens_out.cpu(), (lengths + s - 1) // s)

    # backward: the gradient routed through the kernel's argmax (where pooled > 0), then float64 autograd
    dpooled = torch.randn(bsz, sp, width, generator=g, dtype=torch.float64)
    gate = got > 0
    dz = torch.zeros(bsz, slen, width, dtype=torch.float64)
    dz.scatter_add_(1, a, torch.where(gate, dpooled, torch.zeros_like(dpooled)))
    x64 = x.clone().requires_grad_(True)
    w64 = [w.clone().requires_grad_(True) for w in ws]
    b64 = [b.clone().requires_grad_(True) for b in bs]
    outs = _ref_conv(x64, w64, b64)
    col = 0
    for o, (_, n) in zip(outs, filters):
        o.backward(dz[:, :, col:col + n].transpose(1, 2))
        col += n
    dzd = torch.empty(bsz, slen, width, device=dev)
    dx = torch.full((bsz, slen, e), 0.5, device=dev)                 # accumulate onto 0.5
    dws = [torch.zeros_like(w) for w in wd]
    dbs = [torch.full_like(b, 0.25) for b in bd]                      # accumulate onto 0.25
    wsp = torch.empty(max(1, ops.conv1d_wgrad_workspace_floats(bsz, slen, e, wd)), device=dev)
    ops.conv1d_pool_bwd(xd, wd, s, pooled, arg, f32(dpooled), dzd, dx=dx, accumulate_dx=True, dweights=dws,
                        dbiases=dbs, accumulate_params=True, workspace=wsp, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(dzd.cpu().double(), dz.float().double())
    # error scales ~1e-6 sum |a b| of each product
    adz = dz.abs()
    sx = _ref_conv_t(adz, [w.abs() for w in ws], filters)
    assert bool(((dx.cpu().double() - 0.5 - x64.grad).abs() <= 1e-5 * sx + 1e-6).all())
    for i, (w, (width_i, n)) in enumerate(zip(w64, filters)):
        sw = _ref_wgrad(x.abs(), adz[:, :, sum(m for _, m in filters[:i]):][:, :, :n], width_i)
        assert bool(((dws[i].cpu().double() - w.grad).abs() <= 1e-5 * sw + 1e-6).all()), i
        assert bool(((dbs[i].cpu().double() - 0.25 - b64[i].grad).abs() <= 1e-5 * adz.sum((0, 1))[
            sum(m for _, m in filters[:i]):][:n] + 1e-6).all()), i
    # deterministic: a second run is bit-identical
    dws2 = [torch.zeros_like(w) for w in wd]
    dbs2 = [torch.full_like(b, 0.25) for b in bd]
    dx2 = torch.full((bsz, slen, e), 0.5, device=dev)
    ops.conv1d_pool_bwd(xd, wd, s, pooled, arg, f32(dpooled), dzd, dx=dx2, accumulate_dx=True, dweights=dws2,
                        dbiases=dbs2, accumulate_params=True, workspace=wsp, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2) and all(torch.equal(p, q) for p, q in zip(dws + dbs, dws2 + dbs2))


def _ref_conv_t(dz, ws, filters):
    """sum over widths of the transposed convolution of dz [B, S, F]: [B, S, E]."""
    out, col = 0, 0
    for w, (width, n) in zip(ws, filters):
        pad = (width - 1) // 2
        z = dz[:, :, col:col + n].transpose(1, 2)                              # [B, n, S]
        zp = TF.pad(z, (width - 1 - pad, pad))
        out = out + TF.conv1d(zp, w.flip(0).permute(1, 2, 0)).transpose(1, 2)  # weight [E, n, w]
        col += n
    return out


def _ref_wgrad(x, dz, width):
    pad = (width - 1) // 2
    xp = TF.pad(x.transpose(1, 2), (pad, width - 1 - pad))                     # [B, E, S + w - 1]
    slen = x.shape[1]
    return torch.stack([torch.einsum("bes,bsn->en", xp[:, :, k:k + slen], dz) for k in range(width)])


@pytest.mark.parametrize("rows,d", [(40, 39), (6400, 128), (130, 2100)])
def test_highway_layer_matches_float64(dev, rows, d):
    from neuralmonkey_amd import autodiff as F
    from neuralmonkey_amd import ops

    class _Ctx:                       # the tape needs buffers only
        device = dev
        session = type("Session", (), {})()

        def buffer(self, key, shape, dtype=torch.float32, zero=False):
            return torch.zeros(shape, dtype=dtype, device=dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, d, generator=g, dtype=torch.float64)
    wt, wh = [torch.randn(d, d, generator=g, dtype=torch.float64) / math.sqrt(d) for _ in range(2)]
    bt, bh = [torch.randn(d, generator=g, dtype=torch.float64) * 0.5 - 1.0 for _ in range(2)]
    dy = torch.randn(rows, d, generator=g, dtype=torch.float64)
    tape = F.Tape(_Ctx(), "hw", recording=True)
    f32 = lambda t: t.float().contiguous().to(dev)
    v = lambda t: F.Var(f32(t), torch.zeros_like(f32(t)), True)
    xv = F.Var(f32(x), None, True)
    wtv, btv, whv, bhv = v(wt), v(bt), v(wh), v(bh)
    y = F.highway(tape, xv, wtv, btv, whv, bhv)
    y.grad = f32(dy)
    tape.backward()
    torch.cuda.synchronize()

    p = [t.clone().requires_grad_(True) for t in (x, wt, bt, wh, bh)]
    t_ = torch.sigmoid(p[0] @ p[1] + p[2])
    h_ = torch.relu(p[0] @ p[3] + p[4])
    ref = h_ * t_ + p[0] * (1 - t_)
    ref.backward(dy)
    scale = x.abs() @ wt.abs() + 1.0
    assert float(((y.data.double().cpu() - ref.detach()).abs() / scale).max()) < 1e-5
    for got, want in ((xv.grad, p[0].grad), (wtv.grad, p[1].grad), (btv.grad, p[2].grad), (whv.grad, p[3].grad),
                      (bhv.grad, p[4].grad)):
        err = (got.double().cpu() - want).abs().max() / (want.abs().max() + 1e-12)
        assert float(err) < 1e-5
    del ops


def _batches(dataset, n, size):
    from neuralmonkey_amd.dataset import BatchingScheme
    out = []
    for b in dataset.batches(BatchingScheme(batch_size=size)):
        out.append(b)
        if len(out) == n:
            break
    return out


def test_small_sent_cnn_ini_trains_decodes_and_round_trips(dev, cnn_root, tmp_path):  # noqa: F811
    from .test_reference_inis import load_verbatim
    model = load_verbatim(cnn_root, "small_sent_cnn", device=str(dev), seed=1234)
    tfm = model.tf_manager
    feedables = set.union(*[r.feedables for r in model.runners + model.trainers])
    step0 = tfm.sessions[0].global_step
    for batch in _batches(model.train_dataset, 3, model.batch_size):
        res = tfm.execute(batch, feedables, model.trainers, train=True)
        assert res[0].losses and all(np.isfinite(v) for v in res[0].losses.values()), res[0].losses
    assert tfm.sessions[0].global_step == step0 + 3
    val = _batches(model.val_dataset, 1, model.batch_size)[0]
    out = tfm.execute(val, feedables, model.runners, compute_losses=True)
    decoded = out[0].outputs["target"] if isinstance(out[0].outputs, dict) else out[0].outputs
    assert len(decoded) == len(val)
    for name in model.tf_manager.sessions[0].store.names():
        if name.startswith("sentence_encoder/"):
            assert bool(torch.isfinite(model.tf_manager.sessions[0].store[name]).all()), name
    path = str(tmp_path / "variables.data")
    tfm.save(path)
    again = load_verbatim(cnn_root, "small_sent_cnn", device=str(dev), seed=99)
    again.tf_manager.restore(path)
    out2 = again.tf_manager.execute(val, set.union(*[r.feedables for r in again.runners]), again.runners,
                                    compute_losses=False)
    decoded2 = out2[0].outputs["target"] if isinstance(out2[0].outputs, dict) else out2[0].outputs
    assert decoded2 == decoded


def test_a_sent_cnn_training_step_launches_no_torch_kernels(dev, cnn_root):  # noqa: F811
    from .test_no_foreign_kernels_gpu import _foreign_kernels
    from .test_reference_inis import load_verbatim
    model = load_verbatim(cnn_root, "small_sent_cnn", device=str(dev), seed=1234)
    tfm = model.tf_manager
    batch = _batches(model.train_dataset, 1, model.batch_size)[0]
    foreign = _foreign_kernels(lambda: tfm.execute(batch, model.trainers[0].feedables, model.trainers, train=True))
    assert not foreign, foreign
