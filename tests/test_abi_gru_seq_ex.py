"""nm_gru_seq_fwd_ex / nm_gru_seq_bwd_ex (the cluster loops with the passes around them folded in): declared in
include/nmhip_gru_seq.h (a companion header of nmhip.h, like every later group of entry points), listed in the ctypes
table, exported by the library, their descriptor mirrored field for field -- and arguments are checked before anything
is launched (no GPU needed: every call here must fail in the checks)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nm_gru_seq_fwd_ex", "nm_gru_seq_bwd_ex")
NM_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import build
    build.build(verbose=False)
    from neuralmonkey_amd import _lib
    return _lib.load()


def _header():
    text = open(os.path.join(ROOT, "include", "nmhip_gru_seq.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_new_exports_are_declared_bound_and_exported(lib):
    from neuralmonkey_amd import _lib
    declared = set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(NEW) == set(_lib.GRU_SEQ_SIGNATURES)
    for name in NEW:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.GRU_SEQ_SIGNATURES[name][1], name
    # the plain entry points keep their signatures; the extended ones take the descriptor right after the epilogue
    for old, new in (("nm_gru_seq_fwd", "nm_gru_seq_fwd_ex"), ("nm_gru_seq_bwd", "nm_gru_seq_bwd_ex")):
        res_o, args_o = _lib.SIGNATURES[old]
        res_n, args_n = _lib.GRU_SEQ_SIGNATURES[new]
        assert res_o is res_n and args_n == args_o[:2] + [ctypes.c_void_p] + args_o[2:]
    assert len(_lib.SIGNATURES["nm_gru_seq_fwd"][1]) == 16 and len(_lib.SIGNATURES["nm_gru_seq_bwd"][1]) == 14


def test_descriptor_matches_the_header_and_the_kernel_side():
    from neuralmonkey_amd import _lib
    def fields(text, pattern):
        body = re.search(pattern, text, flags=re.S).group(1)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            ctype, names = re.match(r"((?:const\s+)?\w+\s*\*?)\s*(.*)", decl, flags=re.S).groups()
            for item in names.split(","):
                item = item.strip()
                out.append((ctype.replace(" ", "") + ("*" if item.startswith("*") else ""), item.lstrip("* ")))
        return out
    want = fields(_header(), r"typedef struct nm_gru_seq_io \{(.*?)\} nm_gru_seq_io;")
    # the kernel side keeps no copy: the source that defines the entry points includes the header, nothing under csrc/
    # defines the descriptor again
    csrc = os.path.join(ROOT, "neuralmonkey_amd", "csrc")
    src = open(os.path.join(csrc, "nm_gru_cluster.hip")).read()
    assert re.search(r'^#include "\.\./\.\./include/nmhip_gru_seq\.h"', src, flags=re.M)
    for f in sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f), errors="replace").read())
        assert not re.search(r"struct\s+nm_gru_seq_io\s*\{", text), f
    got = _lib.GruSeqIo._fields_
    assert [n for _, n in want] == [n for n, _ in got]
    for (ctype, field), (_, pytype) in zip(want, got):
        if "*" in ctype:
            assert pytype is ctypes.c_void_p, field
        else:
            assert ctypes.sizeof(pytype) == {"int64_t": 8, "int32_t": 4}[ctype], field


def test_arguments_are_checked_before_any_launch(lib):
    from neuralmonkey_amd import _lib
    buf = (ctypes.c_float * 4096)()
    ptr = ctypes.addressof(buf)
    ptr += (-ptr) % 16                                      # (16-byte aligned operands)
    epi, io = _lib.GruEpilogue(), _lib.GruSeqIo()
    epi.R, epi.H, epi.ndir = 16, 256, 2
    epi.xp = epi.h_out = epi.ru = epi.out = ptr
    epi.dh = epi.c = epi.hseq = epi.dxp = ptr

    def fwd(e, i, steps=3):
        return lib.nm_gru_seq_fwd_ex(None, e, i, steps, 0, 0, 0, 0, ptr, 512, 0, ptr, 256, 0, ptr, 1 << 20, None)

    def bwd(e, i, steps=3):
        return lib.nm_gru_seq_bwd_ex(None, e, i, steps, 0, 0, ptr, 512, 0, ptr, 256, 0, ptr, 1 << 20, None)

    def refused(rc, text):
        assert rc == NM_ERR_ARG and text in lib.nm_last_error(), (rc, lib.nm_last_error())

    E, IO = ctypes.byref(epi), ctypes.byref(io)
    refused(fwd(None, IO), b"nm_gru_seq_fwd_ex: null pointer")
    refused(bwd(None, IO), b"nm_gru_seq_bwd_ex: null pointer")
    refused(fwd(E, None), b"nm_gru_seq_fwd_ex: null io")
    refused(bwd(E, None), b"nm_gru_seq_bwd_ex: null io")
    refused(fwd(E, IO, steps=0), b"at least one step")
    refused(bwd(E, IO, steps=0), b"at least one step")
    # the plain call still insists on an initial state; the extended one takes none (and gets as far as the shape,
    # which no device here can take)
    rc = lib.nm_gru_seq_fwd(None, E, 3, 0, 0, 0, 0, ptr, 512, 0, ptr, 256, 0, ptr, 1 << 20, None)
    refused(rc, b"nm_gru_seq_fwd: missing operand")
    import torch
    if not torch.cuda.is_available():
        refused(fwd(E, IO), b"not supported")
    # a required operand of the loop itself
    epi.ru = None
    refused(fwd(E, IO), b"nm_gru_seq_fwd_ex: missing operand")
    epi.ru = ptr
    epi.dxp = None
    refused(bwd(E, IO), b"nm_gru_seq_bwd_ex: missing operand")
    epi.dxp = ptr
    # the final state: rows narrower than a direction's block, two directions on top of each other
    io.final_state, io.final_row, io.final_dir = ptr, 128, 256
    refused(fwd(E, IO), b"inconsistent strides of final_state")
    io.final_row, io.final_dir = 512, 100
    refused(fwd(E, IO), b"inconsistent strides of final_state")
    io.final_state = None
    # h_{t-1} and r * h_{t-1} come together, positions at least H apart
    io.hprev_seq = ptr
    refused(fwd(E, IO), b"hprev_seq and rh_seq come together")
    io.rh_seq, io.seq_dir, io.seq_row, io.seq_time = ptr, 256, 3 * 512, 100
    refused(fwd(E, IO), b"inconsistent strides of hprev_seq")
    io.hprev_seq = io.rh_seq = None
    # zeros for the padded positions of an output that is not there
    epi.out, io.zero_padded = None, 1
    refused(fwd(E, IO), b"zero_padded without out")
    epi.out, io.zero_padded = ptr, 0
    io.h0_out = ptr                                         # the copy of h_0 on top of the states
    refused(fwd(E, IO), b"h0_out may not alias")
    io.h0_out = None
    io.d_final, io.dfinal_row, io.dfinal_dir = ptr, 512, 8
    refused(bwd(E, IO), b"inconsistent strides of d_final")
    io.dfinal_row, io.dfinal_dir = 64, 256
    refused(bwd(E, IO), b"inconsistent strides of d_final")
