"""The streaming attention entry points without a GPU (include/nmhip_sdp_stream.h): where they are wanted, the
workspace size, the header against the binding table, and the arguments they refuse before a launch."""
import ctypes
import os
import re

import pytest

from . import sdp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from neuralmonkey_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_header_table_and_wrappers_agree():
    from neuralmonkey_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nmhip_sdp_stream.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(nm_[a-z0-9_]+)\s*\((.*?)\)\s*;", text, flags=re.S)}
    assert set(decl) == set(_lib.SDP_STREAM_SIGNATURES) == {
        "nm_sdp_stream_wanted", "nm_sdp_stream_workspace_bytes", "nm_sdp_stream_fwd", "nm_sdp_stream_bwd"}
    for name, (res, args) in _lib.SDP_STREAM_SIGNATURES.items():
        want = [_lib.P if "*" in p else _lib.L if "int64_t" in p else ctypes.c_uint32 if "uint32_t" in p
                else _lib.F if "float" in p else _lib.I for p in decl[name].split(",")]
        assert list(args) == want and res is (_lib.L if name.endswith("_bytes") else _lib.I), name
    assert all(callable(getattr(ops, n)) for n in ("sdp_stream_fwd", "sdp_stream_bwd", "sdp_stream_workspace",
                                                   "sdp_stream_wanted"))


@pytest.mark.parametrize("kind,tq,tk,dh", [
    ("fwd", 1, 302, 64), ("fwd", 1, 301, 64), ("fwd", 1, 154, 128), ("fwd", 1, 153, 128),
    ("bwd", 155, 155, 64), ("bwd", 154, 154, 64), ("bwd", 79, 79, 128), ("bwd", 78, 78, 128), ("bwd", 200, 128, 64),
    ("bwd", 8, 302, 64)])
def test_wanted_exactly_where_the_resident_kernels_refuse(lib, kind, tq, tk, dh):
    refused = R.variant("fwd", tq, tk, 2, dh) == ("refused",)
    assert lib.nm_sdp_stream_wanted(tq, tk, dh, 0) == int(refused)
    if kind == "bwd":
        assert lib.nm_sdp_stream_wanted(tq, tk, dh, 1) == int(refused or R.variant("bwd", tq, tk, 2, dh) == ("refused",))


def test_workspace_bytes(lib):
    assert lib.nm_sdp_stream_workspace_bytes(3, 2, 70) == 4 * 3 * 2 * 70
    assert lib.nm_sdp_stream_workspace_bytes(32, 8, 4096) == 4 * 32 * 8 * 4096
    assert lib.nm_sdp_stream_workspace_bytes(0, 8, 4) == 0


A, OFF = 64, 68                       # "pointers" that are never dereferenced: on and off 16-byte alignment
FWD = dict(q=A, q_bs=6400, k=A, k_bs=6400, v=A, v_bs=6400, mask=None, mask_bs=0, Bq=6, rpk=3, Tq=50, Tk=50, H=2, dh=64,
           causal=0, keep=1.0, salt=0, step=None, ctx=A, ctx_bs=6400, w=None, row_max=None, row_sum=None)
BWD = dict(q=A, q_bs=6400, k=A, k_bs=6400, v=A, v_bs=6400, mask=None, mask_bs=0, ctx=A, ctx_bs=6400, row_max=A,
           row_sum=A, dctx=A, dctx_bs=6400, B=6, rpk=1, Tq=50, Tk=50, H=2, dh=64, causal=0, keep=1.0, salt=0, step=None,
           dq=A, dq_bs=6400, dk=A, dk_bs=6400, dv=A, dv_bs=6400, ws=A, accumulate=0)


@pytest.mark.parametrize("name,base,kw,text", [
    ("nm_sdp_stream_fwd", FWD, dict(v=None), "null pointer"),
    ("nm_sdp_stream_fwd", FWD, dict(row_max=A), "null pointer"),                 # both or neither
    ("nm_sdp_stream_fwd", FWD, dict(Tk=0), "bad shape"),
    ("nm_sdp_stream_fwd", FWD, dict(Bq=7), "Bq=7 is no multiple of rows_per_key=3"),
    ("nm_sdp_stream_fwd", FWD, dict(dh=12), "dh=12 must be 16, 32, 64 or 128"),
    ("nm_sdp_stream_fwd", FWD, dict(k=OFF), "must start on 16 bytes"),
    ("nm_sdp_stream_fwd", FWD, dict(ctx_bs=6402), "multiples of 4 floats"),
    ("nm_sdp_stream_fwd", FWD, dict(keep=0.0), "keep_prob 0 outside (0,1]"),
    ("nm_sdp_stream_fwd", FWD, dict(keep=0.5, Tq=1 << 15, Tk=1 << 15), "dropout mask index overflow"),
    ("nm_sdp_stream_fwd", FWD, dict(Bq=3 << 29, H=2), "grid too large"),
    ("nm_sdp_stream_fwd", FWD, dict(Tq=65535 * 64 + 1), "grid too large"),
    ("nm_sdp_stream_bwd", BWD, dict(row_sum=None), "null pointer"),
    ("nm_sdp_stream_bwd", BWD, dict(ws=None), "null pointer"),
    ("nm_sdp_stream_bwd", BWD, dict(H=-1), "bad shape"),
    ("nm_sdp_stream_bwd", BWD, dict(dh=256), "dh=256 must be 16, 32, 64 or 128"),
    ("nm_sdp_stream_bwd", BWD, dict(rpk=2), "rows_per_key=2 must be 1"),
    ("nm_sdp_stream_bwd", BWD, dict(dk=OFF), "must start on 16 bytes"),
    ("nm_sdp_stream_bwd", BWD, dict(dctx_bs=6401), "multiples of 4 floats"),
    ("nm_sdp_stream_bwd", BWD, dict(keep=1.5), "keep_prob 1.5 outside (0,1]"),
    ("nm_sdp_stream_bwd", BWD, dict(keep=0.5, B=1 << 10, Tq=1 << 11, Tk=1 << 11), "dropout mask index overflow"),
])
def test_refused_before_any_launch(lib, name, base, kw, text):
    assert getattr(lib, name)(None, *dict(base, **kw).values()) == -1
    assert lib.nm_last_error().decode().startswith(name + ": ") and text in lib.nm_last_error().decode()
