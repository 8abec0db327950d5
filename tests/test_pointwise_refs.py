"""CPU checks behind tests/test_pointwise_kernels_gpu.py:
  * every hand-written forward restatement of oracle/pointwise_ref.py agrees with an independent formulation
    (torch.nn.functional pieces, np.flip per sentence, np.add.at, plain loops);
  * headroom: on the exact inputs of the GPU tests, the float32 evaluation of each reference stays inside the bound
    the GPU test applies to the kernel -- the bound can be met by plain fp32 arithmetic;
  * the coverage ledger names every entry point of include/nmhip.h exactly once, every named test exists and calls
    the entry point, and only entry points that launch no arithmetic kernel are excused."""
import ast
import functools
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nm_oracle as O
from oracle import pointwise_ref as P
from oracle.general_ref import dropout_mask
from tests import pointwise_cases as C
from tests import test_pointwise_kernels_gpu as K
from tests.test_abi import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- forward restatements against independent formulations -----------------------------------------------------------
def test_ew_restatement_against_torch():
    a, b, _ = C.ew_inputs("add", C.MID)
    ta, tb = torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    pairs = {
        "sigmoid": (P.ew("sigmoid", a64, None, 0.75), torch.sigmoid(ta + 0.75)),
        "tanh": (P.ew("tanh", a64), torch.tanh(ta)),
        "relu": (P.ew("relu", a64), F.relu(ta)),
        "logaddexp": (P.ew("logaddexp", a64, b64), torch.logaddexp(ta, tb)),
        "scale": (P.ew("scale", a64, None, 0.37), 0.37 * ta),
        "add_scalar": (P.ew("add_scalar", a64, None, -1.25), ta - 1.25),
        "div": (P.ew("div", a64, b64), ta / tb),
        "rowscale": (P.ew("rowscale", a64, b64[:, :1]), ta * tb[:, :1]),
    }
    for name, (got, want) in pairs.items():
        assert np.abs(got - want.numpy()).max() < 1e-12, name
    # the three backward op codes are the derivatives of the three activations at their outputs
    for fwd, bwd in (("sigmoid", "sigmoid_bwd"), ("tanh", "tanh_bwd"), ("relu", "relu_bwd")):
        x = ta.clone().requires_grad_(True)
        y = {"sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": F.relu}[fwd](x)
        (y * tb).sum().backward()
        assert np.abs(P.ew(bwd, y.detach().numpy(), b64) - x.grad.numpy()).max() < 1e-12, bwd
    ninf = np.full(3, -np.inf)
    assert np.array_equal(P.ew("logaddexp", ninf, ninf), ninf)
    assert set(P.EW_OPS) == set(P.EW_BINARY) | {"copy", "scale", "sigmoid", "tanh", "relu", "add_scalar"}


def test_ew_op_codes_are_the_wrappers():
    from neuralmonkey_amd import ops
    assert tuple(sorted(ops.EW, key=ops.EW.get)) == P.EW_OPS


def test_lstm_restatement_against_torch_lstm_cell():
    """torch's LSTMCell orders its gates i, f, g, o and has no forget bias: permute and fold the bias in."""
    rows, h = 37, 13
    inp = C.lstm_inputs(rows, h)
    z, c_prev = torch.tensor(inp["z"], dtype=torch.float64), torch.tensor(inp["c_prev"], dtype=torch.float64)
    for fb in (0.0, 1.0):
        c_new, h_new, gates = P.lstm_cell(z, c_prev, fb)
        i, j, f, o = torch.chunk(z, 4, dim=1)
        cell = torch.nn.LSTMCell(4 * h, h, bias=False, dtype=torch.float64)
        with torch.no_grad():
            cell.weight_ih.copy_(torch.eye(4 * h, dtype=torch.float64))
            cell.weight_hh.zero_()
            h_t, c_t = cell(torch.cat([i, f + fb, j, o], dim=1), (torch.zeros_like(c_prev), c_prev))
        assert float((c_new - c_t).abs().max()) < 1e-12 and float((h_new - h_t).abs().max()) < 1e-12
        assert float((gates[:, 2 * h:3 * h] - torch.sigmoid(f + fb)).abs().max()) < 1e-12


def test_nematus_restatement_against_the_model_oracle_cell():
    """The same cell as oracle/general_ref.py writes it inside its NematusGRU layer, piece by piece."""
    inp = C.nematus_inputs(37, 13)
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in inp.items()}
    h_new, ru, c = P.nematus_cell(t["g_pre"], t["sc"], t["ci"], t["h_prev"], t["g2"])
    r, u = torch.sigmoid(t["g_pre"] + t["g2"]).chunk(2, dim=1)
    cand = torch.tanh(t["ci"] + r * t["sc"])
    assert float((h_new - torch.lerp(cand, t["h_prev"], u)).abs().max()) < 1e-12
    assert float((ru - torch.cat([r, u], 1)).abs().max()) < 1e-12 and float((c - cand).abs().max()) < 1e-12
    assert float((P.blend(u, t["h_prev"], cand) - h_new).abs().max()) < 1e-12


def test_select_reverse_maxout_scatter_restatements():
    inp = C.select_inputs(9, 4)
    h_out, y_out = P.rnn_select(torch.tensor(inp["h_new"]), torch.tensor(inp["h_prev"]), inp["lengths"], C.SELECT_T)
    for r in range(9):
        live = C.SELECT_T < inp["lengths"][r]
        assert np.array_equal(h_out[r].numpy(), inp["h_new"][r] if live else inp["h_prev"][r])
        assert np.array_equal(y_out[r].numpy(), inp["h_new"][r] if live else np.zeros(4, np.float32))
    assert sorted(set(inp["lengths"])) == [0, C.SELECT_T, C.SELECT_T + 1, 1000]
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 6, 3)).astype(np.float32)
    lengths = np.array([0, 1, 6, 9, 4])
    rev = P.reverse_sequence(x, lengths)
    for b in range(5):
        n = min(lengths[b], 6)
        assert np.array_equal(rev[b, :n], np.flip(x[b, :n], 0)) and np.array_equal(rev[b, n:], x[b, n:])
    assert np.array_equal(P.reverse_sequence(rev, lengths), x)
    xm = np.round(rng.standard_normal((7, 12)) * 2).astype(np.float32)
    out, arg = P.maxout(torch.tensor(xm), 3)
    x3 = xm.reshape(7, 3, 4)
    assert np.array_equal(out.numpy(), F.max_pool1d(torch.tensor(x3).permute(0, 2, 1), 3).squeeze(-1).numpy())
    assert np.array_equal(arg.numpy(), x3.argmax(1))                   # NumPy's argmax takes the first maximum too
    ids = np.array([0, 3, 3, -1, 7, 2, 0, 3])
    d = rng.standard_normal((8, 5))
    for skip in (False, True):
        want = np.zeros((7, 5))
        ok = (ids >= 0) & (ids < 7) & ((ids != 0) | (not skip))
        np.add.at(want, ids[ok], d[ok])
        assert np.abs(P.embedding_grads(7, ids, torch.tensor(d), skip).numpy() - want).max() < 1e-12


def test_softmax_layer_norm_dropout_and_greedy_restatements():
    inp = C.softmax_inputs(50, 5)
    rows = inp["e"].shape[0]
    e64 = inp["e"].astype(np.float64)
    m = P.mask_rows(torch.tensor(inp["mask"], dtype=torch.float64), rows, C.SOFTMAX_B, 5)
    w = P.attn_softmax(torch.tensor(e64), m).numpy()
    # oracle/nm_oracle.py::attention_step's arithmetic on the same energies: v = 1, one feature, zero query
    for r in range(rows):
        hf = np.arctanh(np.clip(e64[r] / 50.0, -0.99, 0.99))[None, :, None]
        ap = dict(query_w=np.zeros((1, 1)), query_b=np.zeros(1), v=np.full(1, 50.0), bias=0.0)
        _, w_o = O.attention_step(np.zeros((1, 1)), hf, np.zeros((1, 50, 1)), m[r:r + 1].numpy(), ap)
        assert np.abs(w[r] - w_o[0]).max() < 1e-9
    assert len({tuple(row) for row in inp["mask"]}) == C.SOFTMAX_B and inp["mask"][1].sum() == 0
    li = C.ln_inputs(37, 512)
    y, _, _, _ = P.layer_norm(*(torch.tensor(li[k], dtype=torch.float64) for k in ("x", "gamma", "beta")))
    want = F.layer_norm(torch.tensor(li["x"], dtype=torch.float64), (512,), torch.tensor(li["gamma"], dtype=torch.float64),
                        torch.tensor(li["beta"], dtype=torch.float64), eps=1e-6)
    assert float((y - want).abs().max()) < 1e-12
    x = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    assert np.array_equal(P.dropout(x, 0.5, 9, 3), x * dropout_mask(12, 0.5, (9 + 3 * 0x9E3779B9) % 2 ** 32).reshape(3, 4))
    assert P.effective_salt(0xFFFFFFFF, 1) == (0xFFFFFFFF + 0x9E3779B9) % 2 ** 32 and P.effective_salt(5, None) == 5
    sym, fin, mask, allf = P.greedy_update([4, 2, 7, 2], [0, 0, 1, 1], 2)
    assert sym.tolist() == [4, 2, 0, 0] and fin.tolist() == [0, 1, 1, 1] and mask.tolist() == [1, 0, 0, 0] and not allf
    t = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    assert np.array_equal(P.time_sum(t).numpy(), t.numpy().sum(1))
    assert np.array_equal(P.time_sum_grads((2, 3, 4), torch.ones(2, 4, dtype=torch.float64)).numpy(), np.ones((2, 3, 4)))


# ---- headroom ----------------------------------------------------------------------------------------------------------
def test_float32_evaluation_of_every_reference_meets_the_gpu_bounds():
    """For every non-exact family and every case of the GPU tests: |float32 evaluation - float64 evaluation| of the
    reference on the test's own inputs is within the bound the GPU test holds the kernel to."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    count = 0
    for label, thunk, tols in C.headroom_items():
        ref64, ref32 = thunk(np.float64), thunk(np.float32)
        for name, tol in tols.items():
            err, bnd = C.max_err(C.np64(ref32[name]), C.np64(ref64[name])), C.bound(tol, C.np64(ref64[name]))
            assert err <= bnd, "{} {}: float32 evaluation is {:.3g} from float64, bound {:.3g}".format(label, name, err, bnd)
            count += 1
    assert count > 150
    # the issue's spot check: an LSTM cell at [300, 4 * 132] with z ~ 2 N(0, 1) is ~4e-7 from float64 in plain float32
    inp = C.lstm_inputs(300, 132)
    a, b = C.lstm_expect(inp, 1.0, np.float64), C.lstm_expect(inp, 1.0, np.float32)
    assert C.max_err(C.np64(b["h_new"]), C.np64(a["h_new"])) < 2e-6


def test_float32_sums_and_accumulating_calls_meet_the_gpu_bounds():
    """The same for the sum-type bounds (reduce_sum, time_sum, scatter-add with duplicates, the column sums of dyx,
    every member of every gemm_group run) and for the accumulating calls of nm_ew and nm_dropout."""
    count = 0
    for label, err, bnd in C.headroom_sum_items():
        assert err <= bnd, "{}: float32 evaluation is {:.3g} from float64, bound {:.3g}".format(label, err, bnd)
        count += 1
    assert count > 150


def test_exact_families_are_exact_in_float32_numpy():
    """The bit-for-bit comparisons use float32 NumPy as the expected value: the same expression in float64, rounded
    once, gives the same bits (each is one correctly-rounded operation on float32 inputs)."""
    for op in P.EW_EXACT:
        a, b, _ = C.ew_inputs(op, C.MID)
        f32 = P.ew(op, a, b, C.EW_ALPHA.get(op, 0.0))
        alpha32 = float(np.float32(C.EW_ALPHA.get(op, 0.0)))
        f64 = P.ew(op, a.astype(np.float64), None if b is None else b.astype(np.float64), alpha32).astype(np.float32)
        assert f32.dtype == np.float32 and np.array_equal(f32, f64), op


# ---- the coverage ledger -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _functions(path):
    src = open(os.path.join(ROOT, path)).read()
    return {n.name: ast.get_source_segment(src, n) for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}


def _resolve(via):
    """'ops.OptimizerTables.apply' -> the object, looked up in the package's modules."""
    head, *rest = via.split(".")
    mod = None
    for name in ("neuralmonkey_amd." + head, "neuralmonkey_amd.nn." + head):
        try:
            mod = importlib.import_module(name)
            break
        except ImportError:
            continue
    assert mod is not None, via
    obj = mod
    for part in rest:
        obj = getattr(obj, part)
    return obj


def _wrapper_reaches(via, symbol):
    """The wrapper's source names the symbol -- itself, or through an ops wrapper it calls."""
    from neuralmonkey_amd import ops
    src = inspect.getsource(_resolve(via))
    if re.search(r"\b{}\b".format(symbol), src):
        return True
    return any(hasattr(ops, w) and re.search(r"\b{}\b".format(symbol), inspect.getsource(getattr(ops, w)))
               for w in re.findall(r"\bops\.([A-Za-z_0-9]+)\(", src))


def ledger_problems(ledger, symbols):
    problems = []
    if set(ledger) != set(symbols):
        problems.append("ledger and header differ: {}".format(sorted(set(ledger) ^ set(symbols))))
    for symbol, entry in sorted(ledger.items()):
        if isinstance(entry, tuple):
            if entry[0] != "no kernel" or not entry[1].strip():
                problems.append("{}: an excuse is ('no kernel', reason)".format(symbol))
            continue
        where, _, via = entry.partition(" via ")
        path, _, test = where.partition("::")
        if not os.path.exists(os.path.join(ROOT, path)):
            problems.append("{}: no file {}".format(symbol, path))
            continue
        funcs = _functions(path)
        if test not in funcs or not test.startswith("test_"):
            problems.append("{}: no test {} in {}".format(symbol, test, path))
            continue
        # the test's own source, and that of the module's helpers it calls by name
        text = funcs[test] + "".join(src for name, src in funcs.items()
                                     if not name.startswith("test_") and re.search(r"\b{}\(".format(name), funcs[test]))
        if via:
            # called through whatever name the test imported its module under: '<alias>.<function or class>('
            called = re.search(r"\.{}\(".format(re.escape(via.split(".")[-1])), text)
            if not called:
                problems.append("{}: {} does not call {}".format(symbol, test, via))
            elif not _wrapper_reaches(via, symbol):
                problems.append("{}: {} does not reach it".format(symbol, via))
        elif not re.search(r"\b{}\b".format(symbol), text):
            problems.append("{}: {} does not mention it".format(symbol, test))
    return problems


# entry points that may be excused: they launch no arithmetic kernel (what the library's sources say about them is
# restated in the ledger's reasons); everything else needs a test
NO_KERNEL_ALLOWED = re.compile(r"^nm_(last_error|version|create|destroy|ctx_\w+|prof_enable|prof_attn_step|allreduce_\w+|"
                               r"gru_seq_(force_give_up|test_hog|failed|supported)|dec_step_cluster_supported|"
                               r"\w+_(bytes|tile|layout)|proj_split_forget|copy_d2d)$")


def test_ledger_covers_the_header():
    assert ledger_problems(K.LEDGER, header_symbols()) == []
    excused = [s for s, e in K.LEDGER.items() if isinstance(e, tuple)]
    assert all(NO_KERNEL_ALLOWED.match(s) for s in excused), [s for s in excused if not NO_KERNEL_ALLOWED.match(s)]
    # the excused share is bounded by what launches no arithmetic: a third of the header, and none of the point-wise,
    # backward or product entry points
    assert len(excused) <= len(K.LEDGER) // 3
    for s in ("nm_ew", "nm_lstm_cell_bwd", "nm_gemm_f32_group", "nm_reduce_sum", "nm_layer_norm_bwd", "nm_prof_stream_read"):
        assert not isinstance(K.LEDGER[s], tuple)


def test_ledger_check_notices_a_missing_symbol_and_a_deleted_test():
    symbols = header_symbols()
    short = dict(K.LEDGER)
    del short["nm_blend_bwd"]
    assert any("ledger and header differ" in p for p in ledger_problems(short, symbols))
    gone = dict(K.LEDGER, nm_blend_bwd=K.HERE + "test_blend_was_deleted via ops.blend_bwd")
    assert any("no test test_blend_was_deleted" in p for p in ledger_problems(gone, symbols))
    wrong = dict(K.LEDGER, nm_blend_bwd=K.HERE + "test_tanh_bwd via ops.blend_bwd")
    assert any("does not call ops.blend_bwd" in p for p in ledger_problems(wrong, symbols))
    other = dict(K.LEDGER, nm_blend_bwd=K.HERE + "test_tanh_bwd via ops.tanh_bwd")
    assert any("does not reach it" in p for p in ledger_problems(other, symbols))
    excuse = dict(K.LEDGER, nm_blend_bwd=("skipped", ""))
    assert any("an excuse is" in p for p in ledger_problems(excuse, symbols))
