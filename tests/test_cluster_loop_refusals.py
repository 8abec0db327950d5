"""The eight entry points of the recurrent cluster loops (csrc/nm_gru_cluster.hip) refuse bad arguments in a fixed
order and with fixed texts, before anything is launched (no GPU needed: every call here fails in the checks).  Each
loop walks the same ladder -- null descriptor, bad shape, its alignment rule, its required operands, a shape no device
takes -- and the rungs that differ between the loops (which comes first, alignment or operands; what has to be aligned)
are pinned with calls that break two rules at once."""
import ctypes

import pytest

NM_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ptr():
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    p += (-p) % 16                                         # 16-byte aligned; p + 4 is not
    yield p
    del buf


def _epilogue(ptr, H=256):
    from neuralmonkey_amd import _lib
    e = _lib.GruEpilogue()
    e.R, e.H, e.ndir = 16, H, 1
    e.xp = e.h_out = e.ru = e.rh = e.c_save = e.out = ptr
    e.h_in = ptr + 4096                                    # (another buffer than h_out, aligned)
    e.dh = e.c = e.hseq = e.dxp = ptr
    return e


# name -> (call(lib, e, io, wa, wb, ws), takes io, the field whose absence is "missing operand")
def _gru_fwd(name):
    def call(lib, e, io, wa, wb, ws):
        args = (3, 0, 0, 0, 0, wa, 512, 0, wb, 256, 0, ws, 1 << 20, None)
        return getattr(lib, name)(None, e, *((io,) if name.endswith("_ex") else ()), *args)
    return call


def _gru_bwd(name):
    def call(lib, e, io, wa, wb, ws):
        args = (3, 0, 0, wa, 512, 0, wb, 256, 0, ws, 1 << 20, None)
        return getattr(lib, name)(None, e, *((io,) if name.endswith("_ex") else ()), *args)
    return call


def _nem_fwd(lib, e, io, wa, wb, ws):
    return lib.nm_nematus_seq_fwd(None, e, 3, 0, 0, 0, 0, wa, 512, 0, wb, 256, 0, None, None, ws, 1 << 20, None)


def _nem_bwd(lib, e, io, wa, wb, ws):
    return lib.nm_nematus_seq_bwd(None, e, 3, 0, 0, 0, wa, 512, 0, wb, 256, 0, ws, 1 << 20, None)


def _lstm_fwd(lib, e, io, wa, wb, ws):
    return lib.nm_lstm_seq_fwd(None, e, 3, 0, 0, 0, wa, 1024, 0, 1.0, ws, 1 << 20, None)


def _lstm_bwd(lib, e, io, wa, wb, ws):
    return lib.nm_lstm_seq_bwd(None, e, 3, 0, 0, wa, 1024, 0, ws, 1 << 20, None)


GRU_BWD_ALIGN = "{}: kernels must be 16-byte aligned with leading dimensions % 4 == 0"
NEM_ALIGN = "{}: kernels / workspace must be 16-byte aligned"
LSTM_ALIGN = "{}: kernel / workspace must be 16-byte aligned"
# name: (call, required field, text of the alignment refusal, what is misaligned to get it, alignment before operands?)
LOOPS = {
    "nm_gru_seq_fwd": (_gru_fwd("nm_gru_seq_fwd"), "ru", "{}: operands must be 16-byte aligned", "workspace", False),
    "nm_gru_seq_fwd_ex": (_gru_fwd("nm_gru_seq_fwd_ex"), "ru", "{}: operands must be 16-byte aligned", "workspace", False),
    "nm_gru_seq_bwd": (_gru_bwd("nm_gru_seq_bwd"), "dxp", GRU_BWD_ALIGN, "weights", False),
    "nm_gru_seq_bwd_ex": (_gru_bwd("nm_gru_seq_bwd_ex"), "dxp", GRU_BWD_ALIGN, "weights", False),
    "nm_nematus_seq_fwd": (_nem_fwd, "rh", NEM_ALIGN, "weights", True),
    "nm_nematus_seq_bwd": (_nem_bwd, "rh", NEM_ALIGN, "weights", True),
    "nm_lstm_seq_fwd": (_lstm_fwd, "c_save", LSTM_ALIGN, "weights", True),
    "nm_lstm_seq_bwd": (_lstm_bwd, "c", LSTM_ALIGN, "weights", True),
}


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_the_ladder_of_refusals(lib, ptr, name):
    from neuralmonkey_amd import _lib
    call, field, align_text, misaligned, align_first = LOOPS[name]
    io = ctypes.byref(_lib.GruSeqIo())
    forward = "_fwd" in name
    missing = "{}: missing / unaligned operand" if forward and "gru" not in name else "{}: missing operand"

    def refused(rc, text):
        assert rc == NM_ERR_ARG and lib.nm_last_error().decode() == text.format(name), (rc, lib.nm_last_error())

    def run(e, wa=ptr, wb=ptr, ws=ptr):
        return call(lib, None if e is None else ctypes.byref(e), io, wa, wb, ws)

    # 1. no descriptor, no weights, no workspace: one text
    refused(run(None), "{}: null pointer / workspace")
    refused(run(_epilogue(ptr), wa=None), "{}: null pointer / workspace")
    refused(run(_epilogue(ptr), ws=None), "{}: null pointer / workspace")
    # 2. the shape, before any operand is looked at
    e = _epilogue(ptr)
    e.R = 0
    setattr(e, field, None)
    refused(run(e), "{}: bad shape R=0 H=256")
    e = _epilogue(ptr)
    e.ndir = 3
    refused(run(e, wa=ptr + 4, ws=ptr + 4), "{}: bad shape R=16 H=256")
    # 3. the loop's alignment rule
    bad = {"ws": ptr + 4} if misaligned == "workspace" else {"wa": ptr + 4}
    refused(run(_epilogue(ptr), **bad), align_text)
    if misaligned == "weights":
        refused(run(_epilogue(ptr), ws=ptr + 4), align_text)
    # 4. a required operand
    e = _epilogue(ptr)
    setattr(e, field, None)
    refused(run(e), missing)
    # ... and which of the two is reported when both are wrong
    refused(run(e, **bad), align_text if align_first else missing)
    # 5. a shape no device takes (H is not a multiple of 128), with everything else in order
    refused(run(_epilogue(ptr, H=100)), "{}: shape R=16 H=100 ndir=1 not supported (nm_gru_seq_supported)")
    # ... which comes after the operands: "missing operand" wins over "not supported"
    e = _epilogue(ptr, H=100)
    setattr(e, field, None)
    refused(run(e), missing)


def test_what_only_some_loops_require(lib, ptr):
    """nm_gru_seq_fwd looks at the alignment of h_in and the workspace only, not of the kernels; the forward loops of
    the other two cells want h_in aligned and apart from h_out; the plain GRU entry points want an initial state."""
    def text():
        return lib.nm_last_error().decode()

    e = _epilogue(ptr, H=100)
    rc = LOOPS["nm_gru_seq_fwd"][0](lib, ctypes.byref(e), None, ptr + 4, ptr + 4, ptr)
    assert rc == NM_ERR_ARG and text() == "nm_gru_seq_fwd: shape R=16 H=100 ndir=1 not supported (nm_gru_seq_supported)"
    e.h_in = ptr + 4
    rc = LOOPS["nm_gru_seq_fwd"][0](lib, ctypes.byref(e), None, ptr, ptr, ptr)
    assert rc == NM_ERR_ARG and text() == "nm_gru_seq_fwd: operands must be 16-byte aligned"
    e.h_in = None
    rc = LOOPS["nm_gru_seq_fwd"][0](lib, ctypes.byref(e), None, ptr, ptr, ptr)
    assert rc == NM_ERR_ARG and text() == "nm_gru_seq_fwd: missing operand"
    for name in ("nm_nematus_seq_fwd", "nm_lstm_seq_fwd"):
        e = _epilogue(ptr)
        e.h_in = ptr + 4
        rc = LOOPS[name][0](lib, ctypes.byref(e), None, ptr, ptr, ptr)
        assert rc == NM_ERR_ARG and text() == name + ": missing / unaligned operand"
        e.h_in = e.h_out
        rc = LOOPS[name][0](lib, ctypes.byref(e), None, ptr, ptr, ptr)
        assert rc == NM_ERR_ARG and text() == name + ": h_in and h_out must be different buffers"
    # steps < 0 is a bad shape for every loop
    e = _epilogue(ptr)
    assert lib.nm_lstm_seq_bwd(None, ctypes.byref(e), -1, 0, 0, ptr, 1024, 0, ptr, 1 << 20, None) == NM_ERR_ARG
    assert text() == "nm_lstm_seq_bwd: bad shape R=16 H=256"
