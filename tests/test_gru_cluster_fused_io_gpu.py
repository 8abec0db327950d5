"""The inputs and outputs the GRU cluster loops take over from the passes around them (nm_gru_seq_fwd_ex /
nm_gru_seq_bwd_ex, csrc/nm_gru_cluster.hip): a zero initial state without a buffer, zeros at padded positions, the final
state in the caller's layout, h_{t-1} and r * h_{t-1} of every position, a copy of the initial state; on the way back
the initial dh read from the caller's layout and zeros at the padded positions of dxp.

Checker: the plain launches (nm_gru_seq_fwd / nm_gru_seq_bwd) followed by the separate passes they needed -- ops.zero,
ops.copy_cols, ops.gru_seq_shift, ops.gru_rh_seq -- BIT FOR BIT (torch.equal): copies, zeros and one fp32 multiply
have one possible result.  Every buffer the extended launch has to fill starts as NaN, so a position it forgets shows.
(h_{t-1} of a row's first step is the initial state; ops.gru_seq_shift knows only a zero one, so that comparison runs
from h_0 = 0 -- what the encoder uses -- and a second launch from a random h_0 checks states, final state and the copy
of h_0.)  One case per direction count also goes against the oracle's float64 GRU recurrence with the tolerance of
tests/test_gru_cluster_gpu.py::test_cluster_loops_against_the_oracle (2e-5 of the largest state), and a whole model
trains one step on the cluster path and one on the per-step path with the gradient tolerance of
tests/test_training_gpu.py::test_cluster_time_loops_train_like_the_stepwise_launches (2e-5 of each largest gradient)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, STEPS = (1, 5, 33), (1, 2, 7)      # one partial row tile, an odd count, just over a 32-row tile


@pytest.fixture(scope="module")
def shapes(dev):
    """(h, ndir) -> the (rows, steps, rev0, ragged) cases the device takes; every (h, ndir) must keep at least one."""
    from neuralmonkey_amd import ops
    table = {}
    for h, ndir in itertools.product((256, 512), (1, 2)):
        table[(h, ndir)] = [(rows, steps, rev0, ragged)
                            for rows, steps, rev0, ragged in itertools.product(ROWS, STEPS, (False, True), (False, True))
                            if ops.gru_seq_supported(rows, h, ndir)]
        assert table[(h, ndir)], "no supported case at H={} ndir={}".format(h, ndir)
    return table


def _lengths(dev, rows, steps, ragged, seed):
    lens = np.full(rows, steps, np.int32)
    if ragged:
        lens = np.random.default_rng(seed).integers(1, steps + 1, size=rows).astype(np.int32)
        lens[-1] = 1                     # one row of length 1 ...
        if rows > 1:
            lens[0] = steps              # ... and one of full length
    return torch.tensor(lens, device=dev)


def _inputs(dev, rows, steps, h, ndir, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, device=dev, generator=g)
    return (rn(rows * steps, ndir * 3 * h) * 0.5, rn(ndir, h, 2 * h) * (1.5 / h ** 0.5), rn(ndir, h, h) * (1.5 / h ** 0.5),
            rn(ndir, rows, h) * 0.3)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _forward_pair(dev, rows, steps, h, ndir, rev0, lengths, xp, wgh, wch, h0):
    """(separate passes, one extended launch): out, final, hprev_seq, rh_seq, ru_all, c_all each; h0 None: zero."""
    from neuralmonkey_amd import ops
    c_out = ndir * h
    xs, os_ = (3 * h, steps * ndir * 3 * h, ndir * 3 * h), (h, steps * c_out, c_out)
    ws = ops.gru_seq_workspace(rows, h, ndir, dev)
    # -- the plain launch and the passes around it, on zero-filled buffers
    hcur = torch.zeros(ndir, rows, h, device=dev) if h0 is None else h0.clone()
    out = _nan(dev, rows, steps, c_out)
    ops.zero(out)
    ru, cs = torch.empty(steps, ndir, rows, 2 * h, device=dev), torch.empty(steps, ndir, rows, h, device=dev)
    ops.gru_seq_fwd(steps, ndir, rows, h, xp, xs, hcur, hcur, 0, ru[0], ndir * rows * 2 * h, None, 0, cs[0], ndir * rows * h,
                    wgh, wch, ws, lengths=lengths, reverse_dir0=rev0, out=out, out_strides=os_)
    final = torch.zeros(rows, c_out, device=dev)
    for d in range(ndir):
        ops.copy_cols(hcur[d], final[:, d * h:(d + 1) * h])
    hprev, rh = torch.zeros(rows, steps, ndir, h, device=dev), torch.zeros(rows, steps, ndir, h, device=dev)
    ops.gru_seq_shift(out, hprev, lengths, ndir, h, reverse_dir0=rev0)
    ops.gru_rh_seq(ru, hprev, rh, lengths, ndir, h, reverse_dir0=rev0)
    torch.cuda.synchronize()
    assert not ops.gru_seq_failed(ws)
    want = {"out": out, "final": final, "hprev_seq": hprev, "rh_seq": rh, "gates": ru, "candidates": cs}
    # -- ONE extended launch, on NaN-filled buffers; the final state as columns of a wider matrix (row stride free)
    out2, wide = _nan(dev, rows, steps, c_out), _nan(dev, rows, c_out + 8)
    hprev2, rh2 = _nan(dev, rows, steps, ndir, h), _nan(dev, rows, steps, ndir, h)
    ru2, cs2 = _nan(dev, steps, ndir, rows, 2 * h), _nan(dev, steps, ndir, rows, h)
    scratch, h0_out = _nan(dev, ndir, rows, h), _nan(dev, ndir, rows, h)
    ops.gru_seq_fwd(steps, ndir, rows, h, xp, xs, h0, scratch, 0, ru2[0], ndir * rows * 2 * h, None, 0, cs2[0],
                    ndir * rows * h, wgh, wch, ws, lengths=lengths, reverse_dir0=rev0, out=out2, out_strides=os_,
                    zero_padded=True, final=wide[:, :c_out], hprev_seq=hprev2, rh_seq=rh2, seq_strides=os_, h0_out=h0_out)
    torch.cuda.synchronize()
    assert not ops.gru_seq_failed(ws)
    assert bool(torch.isnan(wide[:, c_out:]).all()), "the final state left its columns"
    got = {"out": out2, "final": wide[:, :c_out], "hprev_seq": hprev2, "rh_seq": rh2, "gates": ru2, "candidates": cs2,
           "h0_out": h0_out}
    return want, got


@pytest.mark.parametrize("h,ndir", [(256, 1), (256, 2), (512, 1), (512, 2)])
def test_extended_forward_launch_equals_the_launch_and_its_passes(dev, shapes, h, ndir):
    for rows, steps, rev0, ragged in shapes[(h, ndir)]:
        case = (rows, steps, rev0, ragged)
        lengths = _lengths(dev, rows, steps, ragged, seed=rows + steps)
        xp, wgh, wch, h0 = _inputs(dev, rows, steps, h, ndir, seed=rows * 31 + steps + h + ndir)
        # zero initial state, given as NO buffer: everything, bit for bit
        want, got = _forward_pair(dev, rows, steps, h, ndir, rev0, lengths, xp, wgh, wch, None)
        for name, w in want.items():
            assert torch.equal(got[name], w), (case, name)
        assert torch.equal(got["h0_out"], torch.zeros_like(got["h0_out"])), case
        # a random initial state: states, final state, saved gates and the copy of h_0
        want, got = _forward_pair(dev, rows, steps, h, ndir, rev0, lengths, xp, wgh, wch, h0)
        for name in ("out", "final", "gates", "candidates"):
            assert torch.equal(got[name], want[name]), (case, name, "h0")
        assert torch.equal(got["h0_out"], h0), case
        assert not bool(torch.isnan(got["hprev_seq"]).any() | torch.isnan(got["rh_seq"]).any()), case


@pytest.mark.parametrize("h,ndir", [(256, 1), (256, 2), (512, 1), (512, 2)])
def test_extended_backward_launch_equals_the_launch_and_its_passes(dev, shapes, h, ndir):
    from neuralmonkey_amd import ops
    c_out = ndir * h
    for rows, steps, rev0, ragged in shapes[(h, ndir)]:
        case = (rows, steps, rev0, ragged)
        lengths = _lengths(dev, rows, steps, ragged, seed=rows + steps)
        xp, wgh, wch, _ = _inputs(dev, rows, steps, h, ndir, seed=rows * 17 + steps + h + ndir)
        fwd, _ = _forward_pair(dev, rows, steps, h, ndir, rev0, lengths, xp, wgh, wch, None)
        out, ru, cs = fwd["out"], fwd["gates"], fwd["candidates"]
        g = torch.Generator(device=dev).manual_seed(5 + rows)
        wide = torch.randn(rows, c_out + 12, device=dev, generator=g)
        d_final = wide[:, 4:4 + c_out]                      # the caller's layout: columns of a wider matrix
        d_out = torch.randn(rows, steps, c_out, device=dev, generator=g)
        d_out *= (torch.arange(steps, device=dev)[None, :] < lengths[:, None]).float()[:, :, None]
        seq, xs = (h, steps * c_out, c_out), (3 * h, steps * ndir * 3 * h, ndir * 3 * h)
        ws = ops.gru_seq_workspace(rows, h, ndir, dev)
        for given in (True, False):                         # dL/dh after the last step: d_final, or zero (null)
            dh = torch.zeros(ndir, rows, h, device=dev)
            if given:
                for d in range(ndir):
                    ops.copy_cols(d_final[:, d * h:(d + 1) * h], dh[d])
            dxp = _nan(dev, rows * steps, ndir * 3 * h)
            ops.zero(dxp)
            ops.gru_seq_bwd(steps, ndir, rows, h, dh, d_out, seq, ru[0], ndir * rows * 2 * h, cs[0], ndir * rows * h, None,
                            out, seq, dxp, xs, wgh, wch, ws, lengths=lengths, reverse_dir0=rev0)
            dh2, dxp2 = _nan(dev, ndir, rows, h), _nan(dev, rows * steps, ndir * 3 * h)
            ops.gru_seq_bwd(steps, ndir, rows, h, dh2, d_out, seq, ru[0], ndir * rows * 2 * h, cs[0], ndir * rows * h, None,
                            out, seq, dxp2, xs, wgh, wch, ws, lengths=lengths, reverse_dir0=rev0, fused_io=True,
                            d_final=d_final if given else None, zero_padded=True)
            torch.cuda.synchronize()
            assert not ops.gru_seq_failed(ws)
            assert torch.equal(dxp2, dxp), (case, given, "dxp")
            assert torch.equal(dh2, dh), (case, given, "dh")


@pytest.mark.parametrize("rows,steps,h,ndir", [(33, 7, 256, 2), (5, 7, 512, 1)])
def test_extended_forward_launch_against_the_oracle(dev, rows, steps, h, ndir):
    """``out`` and the final state of one extended launch (NaN-filled buffers, no initial-state buffer) against
    oracle.nm_oracle's (bidirectional_)dynamic_rnn over TF GRUCells on a ragged batch."""
    from neuralmonkey_amd import ops
    from oracle import nm_oracle as O
    assert ops.gru_seq_supported(rows, h, ndir)
    e = 48
    rng = np.random.default_rng(rows + 3 * steps + h)
    x = (rng.standard_normal((rows, steps, e)) * 0.7).astype(np.float32)
    lens = rng.integers(1, steps + 1, size=rows).astype(np.int32)
    lens[0], lens[-1] = steps, 1
    cells = [{"gates_kernel": (rng.standard_normal((e + h, 2 * h)) * (1.2 / (e + h) ** 0.5)).astype(np.float32),
              "gates_bias": np.ones(2 * h, np.float32),
              "cand_kernel": (rng.standard_normal((e + h, h)) * (1.2 / (e + h) ** 0.5)).astype(np.float32),
              "cand_bias": (rng.standard_normal(h) * 0.1).astype(np.float32)} for _ in range(ndir)]
    if ndir == 2:
        want_out, want_fin = O.bidirectional_rnn(O.gru_cell, x, lens, cells[0], cells[1])
    else:
        want_out, want_fin = O.dynamic_rnn(O.gru_cell, x, lens, cells[0])
    xp = np.concatenate([np.concatenate([x.reshape(-1, e) @ c["gates_kernel"][:e] + c["gates_bias"],
                                         x.reshape(-1, e) @ c["cand_kernel"][:e] + c["cand_bias"]], 1) for c in cells], 1)
    T = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    c_out = ndir * h
    out, final = _nan(dev, rows, steps, c_out), _nan(dev, rows, c_out)
    ru, cs = torch.empty(steps, ndir, rows, 2 * h, device=dev), torch.empty(steps, ndir, rows, h, device=dev)
    ws = ops.gru_seq_workspace(rows, h, ndir, dev)
    ops.gru_seq_fwd(steps, ndir, rows, h, T(xp.astype(np.float32)), (3 * h, steps * ndir * 3 * h, ndir * 3 * h), None,
                    _nan(dev, ndir, rows, h), 0, ru[0], ndir * rows * 2 * h, None, 0, cs[0], ndir * rows * h,
                    T(np.stack([c["gates_kernel"][e:] for c in cells])), T(np.stack([c["cand_kernel"][e:] for c in cells])),
                    ws, lengths=T(lens, torch.int32), out=out, out_strides=(h, steps * c_out, c_out), zero_padded=True,
                    final=final)
    torch.cuda.synchronize()
    assert not ops.gru_seq_failed(ws)
    scale = max(1.0, float(np.abs(want_out).max()))
    assert np.abs(out.cpu().numpy() - want_out).max() <= 2e-5 * scale
    assert np.abs(final.cpu().numpy() - want_fin).max() <= 2e-5 * scale


def test_a_model_trains_alike_on_the_cluster_path_and_the_stepwise_path(dev):
    """One training step of the small translation model (ragged batch) with the loops as cluster launches -- which
    now also produce what the passes around them produced -- and one with two launches per recurrent step
    (NM_CLUSTER_LOOPS=0: the fallback and the recovery path, which keep those passes), from the same weights: every
    gradient within 2e-5 of its largest entry, the bound of
    tests/test_training_gpu.py::test_cluster_time_loops_train_like_the_stepwise_launches."""
    from neuralmonkey_amd import ops, synthetic
    from oracle import nm_oracle as O
    rnn, batch, slen, tlen, vocab = 256, 37, 14, 12, 200
    assert ops.gru_seq_supported(batch, rnn, 2) and ops.gru_seq_supported(batch, rnn, 1), "must take the cluster kernels"
    params = O.init_params(seed=11, vocab_src=vocab, vocab_tgt=vocab, emb=rnn, rnn=rnn, std=0.1)
    ds = synthetic.synthetic_dataset(seed=12, batch=batch, src_len=slen, tgt_len=tlen, vocab=vocab, ragged=True)
    results = []
    for cluster in (False, True):
        model = synthetic.build_translation_model(vocab_src=vocab, vocab_tgt=vocab, emb=rnn, rnn=rnn, max_len=slen,
                                                  beam_size=0, device=str(dev), l2_weight=1e-6, clip_norm=1.0)
        sess = model.tf_manager.sessions[0]
        sess.store.load_state_dict(params)
        sess.use_cluster_loops = cluster
        res = model.tf_manager.execute(ds, model.trainer.feedables, [model.trainer], train=True)[0]
        assert sess.use_cluster_loops == cluster and not sess.cluster_failure()
        results.append((res.losses["decoder - cost"], {n: sess.store.g(n).cpu().numpy().copy() for n in sess.store.names()}))
    (l0, g0), (l1, g1) = results
    assert np.isfinite(l0) and np.isfinite(l1)
    for n in g0:
        if n.endswith("attn_bias"):          # identically zero: rounding noise on both sides
            continue
        assert np.abs(g0[n] - g1[n]).max() <= 2e-5 * max(np.abs(g0[n]).max(), 1e-8), n
