"""ops.gru_seq_* / nematus_seq_* / lstm_seq_*: what the six wrappers hand to the library, checked without a device.
The library is replaced by a recorder; every field of the epilogue and of the fused-io descriptor and every argument
behind them must be what this file works out from the tensors itself, and each call sits once inside the bracket that
keeps two cluster loops from being launched side by side."""
import ctypes
import itertools

import pytest
import torch

from neuralmonkey_amd import _lib, ops

R, H, STEPS, STREAM = 4, 8, 3, 0x5EED


class Recorder:
    def __init__(self):
        self.events = []

    def __getattr__(self, name):
        def entry(*args):
            snap = []
            for a in args:
                obj = getattr(a, "_obj", None)             # ctypes.byref(struct): keep a copy of the struct's fields
                snap.append({f: getattr(obj, f) for f, _ in obj._fields_} if obj is not None else a)
            self.events.append((name, snap))
            return 0
        return entry


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops._lib, "load", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    token = object()
    monkeypatch.setattr(ops, "_cluster_serialize_before", lambda: r.events.append(("before", None)) or token)
    monkeypatch.setattr(ops, "_cluster_serialize_after", lambda s: r.events.append(("after", s is token)))
    return r


def _the_call(rec):
    """the one library call of a wrapper, bracketed once"""
    assert [n for n, _ in rec.events[::2]] == ["before", "after"] and len(rec.events) == 3, rec.events
    assert rec.events[2] == ("after", True)
    name, args = rec.events[1]
    rec.events.clear()
    return name, args


def _t(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def _weights(ndir, width, three_d):
    """[ndir, H, width] (or 2-D for one direction) as a view into wider rows: the leading dimension is not the width"""
    w = _t(ndir, H, width + 4)[:, :, :width]
    return w if three_d else w[0]


def _w_args(w):
    return [w.data_ptr(), w.stride(-2), w.stride(0) if w.dim() == 3 else 0]


def _epi(**kw):
    want = {f: (None if t is ctypes.c_void_p else 0) for f, t in _lib.GruEpilogue._fields_}
    want.update(kw)
    return want


def _io(**kw):
    want = {f: (None if t is ctypes.c_void_p else 0) for f, t in _lib.GruSeqIo._fields_}
    want.update(kw)
    return want


def _head(mode, ndir, reverse_dir0, lengths):
    return dict(mode=mode, t=0, rev_mask=1 if reverse_dir0 else (2 if ndir == 2 else 0), ndir=ndir, R=R, H=H,
                lengths=None if lengths is None else lengths.data_ptr())


def _variants():
    for ndir, three_d, rev, opt in itertools.product((1, 2), (False, True), (False, True), (False, True)):
        if ndir == 2 and not three_d:
            continue
        yield ndir, three_d, rev, opt


def _ws():
    ws = _t(100)
    return ws, [ws.data_ptr(), 400]


@pytest.mark.parametrize("ndir,three_d,rev,opt", list(_variants()))
def test_forward_wrappers(rec, ndir, three_d, rev, opt):
    xp, h_in, h_out, ru, rh, c = _t(ndir, R, STEPS, 3 * H), _t(ndir, R, H), _t(STEPS, ndir, R, H), _t(6), _t(7), _t(9)
    lengths = torch.ones(R, dtype=torch.int32) if opt else None
    out = _t(R, STEPS, ndir * H) if opt else None
    sticky = torch.zeros(1, dtype=torch.int32) if opt else None
    x_s, o_s = (11, 12, 13), ((H, STEPS * ndir * H, ndir * H) if opt else (0, 0, 0))
    wg, wc, (ws, ws_args) = _weights(ndir, 2 * H, three_d), _weights(ndir, H, three_d), _ws()
    opts = dict(lengths=lengths, reverse_dir0=rev, sticky=sticky)
    if opt:
        opts.update(out=out, out_strides=o_s)
    fwd = dict(_head(1, ndir, rev, lengths), xp=xp.data_ptr(), x_dir=11, x_row=12, x_time=13, h_in=h_in.data_ptr(),
               h_out=h_out.data_ptr(), out=None if out is None else out.data_ptr(), o_dir=o_s[0], o_row=o_s[1],
               o_time=o_s[2])
    tail = ws_args + [None if sticky is None else sticky.data_ptr()]

    ops.gru_seq_fwd(STEPS, ndir, R, H, xp, x_s, h_in, h_out, 21, ru, 22, rh if opt else None, 23, c if opt else None, 24,
                    wg, wc, ws, **opts)
    name, args = _the_call(rec)
    assert name == "nm_gru_seq_fwd" and args[0] == STREAM
    assert args[1] == _epi(ru=ru.data_ptr(), rh=rh.data_ptr() if opt else None, c_save=c.data_ptr() if opt else None, **fwd)
    assert args[2:] == [STEPS, 21, 22, 23, 24] + _w_args(wg) + _w_args(wc) + tail

    ops.nematus_seq_fwd(STEPS, ndir, R, H, xp, x_s, h_in, h_out, 21, ru, 22, rh, 23, c, 24, wg, wc, ws,
                        bgs=ru if opt else None, bcs=rh if opt else None, **opts)
    name, args = _the_call(rec)
    assert name == "nm_nematus_seq_fwd" and args[0] == STREAM
    assert args[1] == _epi(ru=ru.data_ptr(), rh=rh.data_ptr(), c_save=c.data_ptr(), **fwd)
    assert args[2:] == ([STEPS, 21, 22, 23, 24] + _w_args(wg) + _w_args(wc) +
                        [ru.data_ptr() if opt else None, rh.data_ptr() if opt else None] + tail)

    wh = _weights(ndir, 4 * H, three_d)
    ops.lstm_seq_fwd(STEPS, ndir, R, H, xp, x_s, h_in, h_out, 21, ru, 22, c, 24, wh, ws,
                     **(dict(opts, forget_bias=0.5) if opt else opts))
    name, args = _the_call(rec)
    assert name == "nm_lstm_seq_fwd" and args[0] == STREAM
    assert args[1] == _epi(ru=ru.data_ptr(), c_save=c.data_ptr(), **fwd)
    assert args[2:] == [STEPS, 21, 22, 24] + _w_args(wh) + [0.5 if opt else 1.0] + tail


@pytest.mark.parametrize("ndir,three_d,rev,opt", list(_variants()))
def test_backward_wrappers(rec, ndir, three_d, rev, opt):
    dh, ru, sc, c, hseq, dxp = _t(ndir, R, H), _t(6), _t(7), _t(9), _t(ndir, R, STEPS, H), _t(ndir, R, STEPS, 4 * H)
    lengths = torch.ones(R, dtype=torch.int32) if opt else None
    dout = _t(R, STEPS, ndir * H) if opt else None
    h0 = _t(ndir, R, H) if opt else None
    sticky = torch.zeros(1, dtype=torch.int32) if opt else None
    do_s, hs_s, dx_s = ((H, STEPS * ndir * H, ndir * H) if opt else None), (31, 32, 33), (41, 42, 43)
    wg, wc, (ws, ws_args) = _weights(ndir, 2 * H, three_d), _weights(ndir, H, three_d), _ws()
    opts = dict(lengths=lengths, reverse_dir0=rev, sticky=sticky)
    do_w = do_s or (0, 0, 0)
    bwd = dict(_head(4, ndir, rev, lengths), dh=dh.data_ptr(), dout=None if dout is None else dout.data_ptr(),
               do_dir=do_w[0], do_row=do_w[1], do_time=do_w[2], dxp=dxp.data_ptr(), dx_dir=41, dx_row=42, dx_time=43,
               ru=ru.data_ptr(), c=c.data_ptr())
    seq = dict(h0=None if h0 is None else h0.data_ptr(), hseq=hseq.data_ptr(), hs_dir=31, hs_row=32, hs_time=33)
    tail = ws_args + [None if sticky is None else sticky.data_ptr()]

    ops.gru_seq_bwd(STEPS, ndir, R, H, dh, dout, do_s, ru, 22, c, 24, h0, hseq, hs_s, dxp, dx_s, wg, wc, ws, **opts)
    name, args = _the_call(rec)
    assert name == "nm_gru_seq_bwd" and args[0] == STREAM
    assert args[1] == _epi(**bwd, **seq)
    assert args[2:] == [STEPS, 22, 24] + _w_args(wg) + _w_args(wc) + tail

    ops.nematus_seq_bwd(STEPS, ndir, R, H, dh, dout, do_s, ru, 22, sc, 23, c, 24, h0, hseq, hs_s, dxp, dx_s, wg, wc, ws,
                        **opts)
    name, args = _the_call(rec)
    assert name == "nm_nematus_seq_bwd" and args[0] == STREAM
    assert args[1] == _epi(rh=sc.data_ptr(), **bwd, **seq)
    assert args[2:] == [STEPS, 22, 23, 24] + _w_args(wg) + _w_args(wc) + tail

    wh = _weights(ndir, 4 * H, three_d)
    ops.lstm_seq_bwd(STEPS, ndir, R, H, dh, dout, do_s, ru, 22, c, 24, dxp, dx_s, wh, ws, **opts)
    name, args = _the_call(rec)
    assert name == "nm_lstm_seq_bwd" and args[0] == STREAM
    assert args[1] == _epi(**bwd)
    assert args[2:] == [STEPS, 22, 24] + _w_args(wh) + tail


FWD_IO = ("no_h_in", "zero_padded", "final", "seq", "h0_out")


@pytest.mark.parametrize("which", FWD_IO + ("all",))
def test_gru_forward_fused_io(rec, which):
    ndir = 2
    on = lambda name: which in (name, "all")
    xp, h_in, h_out, ru, out = _t(ndir, R, STEPS, 3 * H), _t(ndir, R, H), _t(STEPS, ndir, R, H), _t(6), _t(R, STEPS, ndir * H)
    final = _t(R, ndir * H + 4)[:, :ndir * H]              # (row stride free)
    hprev, rhs, h0_out = _t(ndir, R, STEPS, H), _t(ndir, R, STEPS, H), _t(ndir, R, H)
    wg, wc, (ws, ws_args) = _weights(ndir, 2 * H, True), _weights(ndir, H, True), _ws()
    ops.gru_seq_fwd(STEPS, ndir, R, H, xp, (11, 12, 13), None if on("no_h_in") else h_in, h_out, 21, ru, 22, None, 23,
                    None, 24, wg, wc, ws, out=out, out_strides=(1, 2, 3), zero_padded=on("zero_padded"),
                    final=final if on("final") else None, hprev_seq=hprev if on("seq") else None,
                    rh_seq=rhs if on("seq") else None, seq_strides=(51, 52, 53) if on("seq") else None,
                    h0_out=h0_out if on("h0_out") else None)
    name, args = _the_call(rec)
    assert name == "nm_gru_seq_fwd_ex" and args[0] == STREAM
    assert args[1] == _epi(**_head(1, ndir, False, None), xp=xp.data_ptr(), x_dir=11, x_row=12, x_time=13,
                           h_in=None if on("no_h_in") else h_in.data_ptr(), h_out=h_out.data_ptr(), ru=ru.data_ptr(),
                           out=out.data_ptr(), o_dir=1, o_row=2, o_time=3)
    want = _io(zero_padded=int(on("zero_padded")), h0_out=h0_out.data_ptr() if on("h0_out") else None)
    if on("final"):
        want.update(final_state=final.data_ptr(), final_row=ndir * H + 4, final_dir=H)
    if on("seq"):
        want.update(hprev_seq=hprev.data_ptr(), rh_seq=rhs.data_ptr(), seq_dir=51, seq_row=52, seq_time=53)
    assert args[2] == want
    assert args[3:] == [STEPS, 21, 22, 23, 24] + _w_args(wg) + _w_args(wc) + ws_args + [None]


@pytest.mark.parametrize("d_final,d_final_dir,zero_padded", [(False, None, False), (True, None, False), (True, 24, True),
                                                             (False, None, True)])
def test_gru_backward_fused_io(rec, d_final, d_final_dir, zero_padded):
    ndir = 2
    dh, ru, c, hseq, dxp = _t(ndir, R, H), _t(6), _t(9), _t(ndir, R, STEPS, H), _t(ndir, R, STEPS, 3 * H)
    dfin = _t(R, ndir * H + 4)[:, :ndir * H] if d_final else None
    wg, wc, (ws, ws_args) = _weights(ndir, 2 * H, True), _weights(ndir, H, True), _ws()
    ops.gru_seq_bwd(STEPS, ndir, R, H, dh, None, None, ru, 22, c, 24, None, hseq, (31, 32, 33), dxp, (41, 42, 43), wg, wc,
                    ws, fused_io=True, d_final=dfin, d_final_dir=d_final_dir, zero_padded=zero_padded)
    name, args = _the_call(rec)
    assert name == "nm_gru_seq_bwd_ex" and args[0] == STREAM
    assert args[1] == _epi(**_head(4, ndir, False, None), dh=dh.data_ptr(), ru=ru.data_ptr(), c=c.data_ptr(),
                           hseq=hseq.data_ptr(), hs_dir=31, hs_row=32, hs_time=33, dxp=dxp.data_ptr(), dx_dir=41,
                           dx_row=42, dx_time=43)
    want = _io(zero_padded=int(zero_padded))
    if d_final:
        want.update(d_final=dfin.data_ptr(), dfinal_row=ndir * H + 4, dfinal_dir=H if d_final_dir is None else d_final_dir)
    assert args[2] == want
    assert args[3:] == [STEPS, 22, 24] + _w_args(wg) + _w_args(wc) + ws_args + [None]
    # without fused_io the fused options are refused
    with pytest.raises(AssertionError):
        ops.gru_seq_bwd(STEPS, ndir, R, H, dh, None, None, ru, 22, c, 24, None, hseq, (31, 32, 33), dxp, (41, 42, 43), wg,
                        wc, ws, zero_padded=True)
    assert rec.events == []


def test_kernels_with_strided_columns_are_refused(rec):
    xp, h_in, h_out, ru, c, dxp = _t(1, R, STEPS, 4 * H), _t(1, R, H), _t(STEPS, 1, R, H), _t(6), _t(9), _t(1, R, STEPS, 4 * H)
    good, bad, ws = _t(H, 4 * H), _t(4 * H, H).t(), _t(100)
    calls = [lambda a, b: ops.gru_seq_fwd(STEPS, 1, R, H, xp, (1, 2, 3), h_in, h_out, 0, ru, 0, None, 0, None, 0, a, b, ws),
             lambda a, b: ops.gru_seq_bwd(STEPS, 1, R, H, h_in, None, None, ru, 0, c, 0, None, xp, (1, 2, 3), dxp, (1, 2, 3),
                                          a, b, ws),
             lambda a, b: ops.nematus_seq_fwd(STEPS, 1, R, H, xp, (1, 2, 3), h_in, h_out, 0, ru, 0, ru, 0, c, 0, a, b, ws),
             lambda a, b: ops.nematus_seq_bwd(STEPS, 1, R, H, h_in, None, None, ru, 0, ru, 0, c, 0, None, xp, (1, 2, 3),
                                              dxp, (1, 2, 3), a, b, ws)]
    for call in calls:
        for a, b in ((bad, good), (good, bad)):
            with pytest.raises(AssertionError):
                call(a, b)
    with pytest.raises(AssertionError):
        ops.lstm_seq_fwd(STEPS, 1, R, H, xp, (1, 2, 3), h_in, h_out, 0, ru, 0, c, 0, bad, ws)
    with pytest.raises(AssertionError):
        ops.lstm_seq_bwd(STEPS, 1, R, H, h_in, None, None, ru, 0, c, 0, dxp, (1, 2, 3), bad, ws)
    assert all(name in ("before", "after") for name, _ in rec.events)       # nothing reached the library
