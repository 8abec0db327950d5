"""NumPy restatement of the sentence-level heads of the reference -- encoders/pooling.py, encoders/attentive.py,
decoders/classifier.py, decoders/sequence_regressor.py (with nn/mlp.py and nn/projection.py) and
model/gradient_reversal.py -- as TensorFlow 1.x computes them: test infrastructure, CPU only.  Every function takes the
dtype it computes in (float64: the expected values; float32: the unit of the GPU tolerances and, for the selections of
max pooling, the bit pattern itself).

Forward functions return dictionaries; the ``*_bwd`` functions are the analytic gradients (checked against torch float64
autograd by tests/test_pool_host.py)."""
import numpy as np

from .label_ref import ACT, rows

PAD_VALUE = 1e-15          # pooling.py:50
EPS = 1e-8                 # pooling.py:63, attentive.py:73


# ---- encoders/pooling.py ------------------------------------------------------------------------------------------------
def max_pool(x, mask, dtype=np.float64):
    """x [B, T, D], mask [B, T] -> out [B, D], ties [B, D] (positions of p equal to the maximum, padded ones included)
    and p itself (:44-51)."""
    x = np.asarray(x, dtype=dtype)
    m = np.asarray(mask, dtype=dtype)[:, :, None]
    p = x * m + dtype(PAD_VALUE) * (dtype(1) - m)
    out = p.max(axis=1)
    ties = (p == out[:, None, :]).sum(axis=1).astype(np.int32)
    return {"out": out, "ties": ties, "p": p}


def max_pool_bwd(x, mask, dout, dtype=np.float64):
    """The gradient of tf.reduce_max (an equal share for every position that holds the maximum) through the mask."""
    f = max_pool(x, mask, dtype)
    m = np.asarray(mask, dtype=dtype)[:, :, None]
    eq = (f["p"] == f["out"][:, None, :]).astype(dtype)
    share = np.asarray(dout, dtype=dtype) / f["ties"].astype(dtype)
    return (m * eq * share[:, None, :]).astype(dtype)


def avg_pool(x, mask, dtype=np.float64):
    """(:60-63)."""
    x = np.asarray(x, dtype=dtype)
    m = np.asarray(mask, dtype=dtype)[:, :, None]
    den = m.sum(axis=1) + dtype(EPS)
    return {"out": ((x * m).sum(axis=1) / den).astype(dtype), "den": den}


def avg_pool_bwd(mask, dout, width, dtype=np.float64):
    m = np.asarray(mask, dtype=dtype)[:, :, None]
    den = m.sum(axis=1) + dtype(EPS)
    return (m * (np.asarray(dout, dtype=dtype) / den)[:, None, :] * np.ones((1, 1, width), dtype)).astype(dtype)


# ---- encoders/attentive.py:60-75 ------------------------------------------------------------------------------------------
def time_softmax(e, mask=None, dtype=np.float64):
    """e [B, T, H] -> w [B, T, H] normalised over T; s (the plain softmax) and z [B, H] for the gradient."""
    e = np.asarray(e, dtype=dtype)
    ex = np.exp(e - e.max(axis=1, keepdims=True))
    s = ex / ex.sum(axis=1, keepdims=True)
    if mask is None:
        return {"w": s, "s": s, "z": np.ones((e.shape[0], e.shape[2]), dtype)}
    m = np.asarray(mask, dtype=dtype)[:, :, None]
    u = s * m
    z = u.sum(axis=1) + dtype(EPS)
    return {"w": (u / z[:, None, :]).astype(dtype), "s": s, "z": z}


def time_softmax_bwd(dw, s, z, mask=None, dtype=np.float64):
    dw, s = np.asarray(dw, dtype=dtype), np.asarray(s, dtype=dtype)
    if mask is None:
        ds = dw
    else:
        m = np.asarray(mask, dtype=dtype)[:, :, None]
        z = np.asarray(z, dtype=dtype)[:, None, :]
        u = s * m
        du = dw / z - (dw * u).sum(axis=1, keepdims=True) / (z * z)
        ds = du * m
    return (s * (ds - (ds * s).sum(axis=1, keepdims=True))).astype(dtype)


def sqerr(pred, targets, scale=1.0, dtype=np.float64):
    """pred [R, dim], targets [R] -> loss [R] = sum_k (p - y)^2 and grad [R, dim] = scale * 2 (p - y)."""
    d = np.asarray(pred, dtype=dtype) - np.asarray(targets, dtype=dtype)[:, None]
    return {"loss": (d * d).sum(axis=1).astype(dtype), "grad": (dtype(scale) * dtype(2) * d).astype(dtype)}


def attentive(params, states, mask, name="encoder_att", dtype=np.float64):
    """AttentiveEncoder without dropout: ``params`` holds ``<name>/S1/kernel`` [D, hidden], ``<name>/S2/kernel``
    [hidden, H] and optionally ``<name>/state_projection/{kernel,bias}``, ``<name>/output_projection/{kernel,bias}``."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items() if k.startswith(name + "/")}
    x = np.asarray(states, dtype=dtype)
    bsz, steps, d = x.shape
    hidden = np.tanh(x.reshape(-1, d) @ p[name + "/S1/kernel"])
    energies = (hidden @ p[name + "/S2/kernel"]).reshape(bsz, steps, -1)
    sm = time_softmax(energies, mask, dtype)
    sp_k = name + "/state_projection/kernel"
    proj = (x.reshape(-1, d) @ p[sp_k] + p[name + "/state_projection/bias"]).reshape(bsz, steps, -1) if sp_k in p else x
    temporal = np.einsum("bth,btd->bhd", sm["w"], proj)
    flat = temporal.reshape(bsz, -1)
    op_k = name + "/output_projection/kernel"
    output = flat @ p[op_k] + p[name + "/output_projection/bias"] if op_k in p else flat
    return {"attention_weights": sm["w"], "temporal_states": temporal, "output": output, "energies": energies,
            "_saved": (p, x, mask, hidden, sm, proj, flat)}


def attentive_bwd(fwd, d_output=None, d_temporal=None, name="encoder_att", dtype=np.float64):
    """-> (gradients of the encoder's variables, gradient of the input states)."""
    p, x, mask, hidden, sm, proj, flat = fwd["_saved"]
    bsz, steps, d = x.shape
    grads = {}
    dtemp = np.zeros_like(fwd["temporal_states"]) if d_temporal is None else np.asarray(d_temporal, dtype=dtype).copy()
    if d_output is not None:
        dout = np.asarray(d_output, dtype=dtype)
        op_k = name + "/output_projection/kernel"
        if op_k in p:
            grads[op_k] = flat.T @ dout
            grads[name + "/output_projection/bias"] = dout.sum(axis=0)
            dout = dout @ p[op_k].T
        dtemp += dout.reshape(dtemp.shape)
    dw = np.einsum("bhd,btd->bth", dtemp, proj)
    dproj = np.einsum("bth,bhd->btd", sm["w"], dtemp)
    dx = np.zeros_like(x)
    sp_k = name + "/state_projection/kernel"
    if sp_k in p:
        flat_dp = dproj.reshape(bsz * steps, -1)
        grads[sp_k] = x.reshape(-1, d).T @ flat_dp
        grads[name + "/state_projection/bias"] = flat_dp.sum(axis=0)
        dx += (flat_dp @ p[sp_k].T).reshape(x.shape)
    else:
        dx += dproj
    de = time_softmax_bwd(dw, sm["s"], sm["z"], mask, dtype).reshape(bsz * steps, -1)
    grads[name + "/S2/kernel"] = hidden.T @ de
    dhid = (de @ p[name + "/S2/kernel"].T) * (1 - hidden * hidden)
    grads[name + "/S1/kernel"] = x.reshape(-1, d).T @ dhid
    dx += (dhid @ p[name + "/S1/kernel"].T).reshape(x.shape)
    return grads, dx


# ---- the heads ----------------------------------------------------------------------------------------------------------
def _mlp(p, x, prefix, n_layers, activation):
    fwd, _ = ACT[activation]
    acts = [x]
    for i in range(n_layers):
        acts.append(fwd(acts[-1] @ p["{}/mlp_layer_{}/kernel".format(prefix, i)]
                        + p["{}/mlp_layer_{}/bias".format(prefix, i)]))
    return acts


def _mlp_bwd(p, acts, dtop, prefix, activation, grads):
    _, dfn = ACT[activation]
    for i in reversed(range(len(acts) - 1)):
        dz = dtop * dfn(acts[i + 1])
        grads["{}/mlp_layer_{}/kernel".format(prefix, i)] = acts[i].T @ dz
        grads["{}/mlp_layer_{}/bias".format(prefix, i)] = dz.sum(axis=0)
        dtop = dz @ p["{}/mlp_layer_{}/kernel".format(prefix, i)].T
    return dtop


def classifier(params, inputs, targets, name="classifier", layers=0, activation="relu", dtype=np.float64):
    """decoders/classifier.py over the encoders' ``output`` tensors ``inputs`` (list of [B, d], concatenated):
    ``layers`` hidden layers, no dropout.  targets [B] int class indices, or None.  ``grads``: d cost / d (variables,
    "inputs" -- the concatenation)."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items() if k.startswith(name + "/")}
    x = np.concatenate([np.asarray(i, dtype=dtype) for i in inputs], axis=1)
    deep = name + "/multilayer_perceptron/deep_output_mlp"
    acts = _mlp(p, x, deep, layers, activation)
    ck, cb = name + "/multilayer_perceptron/classification_layer/kernel", \
        name + "/multilayer_perceptron/classification_layer/bias"
    logits = acts[-1] @ p[ck] + p[cb]
    r = rows(logits, targets, pad=-1, scale=1.0, dtype=dtype)
    out = {"logits": logits, "logprobs": r["logprobs"], "decoded": r["argmax"], "mlp_input": x}
    if targets is not None:
        bsz = dtype(x.shape[0])
        out["xents"] = r["loss"]
        out["cost"] = r["loss"].sum() / bsz
        dlogits = r["grad"] / bsz
        grads = {ck: acts[-1].T @ dlogits, cb: dlogits.sum(axis=0)}
        grads["inputs"] = _mlp_bwd(p, acts, dlogits @ p[ck].T, deep, activation, grads)
        out["grads"] = grads
    return out


def regressor(params, inputs, targets, name="regressor", layers=0, activation="relu", dtype=np.float64):
    """decoders/sequence_regressor.py: predictions [B, dim]; cost = mean over B*dim of (pred - y)^2, y [B] broadcast."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items() if k.startswith(name + "/")}
    x = np.concatenate([np.asarray(i, dtype=dtype) for i in inputs], axis=1)
    acts = _mlp(p, x, name + "/mlp", layers, activation)
    ok, ob = name + "/output_projection/kernel", name + "/output_projection/bias"
    pred = acts[-1] @ p[ok] + p[ob]
    out = {"predictions": pred, "mlp_input": x}
    if targets is not None:
        count = dtype(pred.size)
        se = sqerr(pred, targets, 1.0, dtype)
        out["cost"] = se["loss"].sum() / count
        dpred = se["grad"] / count
        grads = {ok: acts[-1].T @ dpred, ob: dpred.sum(axis=0)}
        grads["inputs"] = _mlp_bwd(p, acts, dpred @ p[ok].T, name + "/mlp", activation, grads)
        out["grads"] = grads
    return out


def logits_runner_strings(logits, normalize=True, pick_index=None):
    """runners/logits_runner.py:34-53 as it is: exp without the maximum subtracted; ``if pick_index:`` treats index 0 as
    "all classes"; the classes of a time step are joined by commas, the time steps by tabs.  logits [T, B, K] -> per
    sentence a list holding one string."""
    logits = np.asarray(logits)
    out = [[] for _ in logits[0]]
    for step in logits:
        for row, acc in zip(step, out):
            if normalize:
                row = np.exp(row) / np.sum(np.exp(row), axis=0)
            acc.append(str(row[pick_index]) if pick_index else ",".join(str(v) for v in row))
    return [["\t".join(acc)] for acc in out]


def parse_logits_strings(outputs):
    """The floats of LogitsRunner's strings: [B, values]."""
    return np.asarray([[float(v) for v in sent[0].replace("\t", ",").split(",")] for sent in outputs], np.float64)


def adversarial_topology(params, states, mask, targets, layers=1, activation="relu", dtype=np.float64):
    """The topology of the reference's tests/classifier.ini over given encoder states: an AttentiveEncoder
    ("encoder_att") and a SequenceMaxPooling read the same states; ``classifier`` reads both; ``classifier_adv`` reads
    the pooler through a gradient-reversal StatefulView.  The trained cost is the sum of the two costs; the view hands
    the pooler the NEGATED gradient of the adversary.  -> cost, the two costs, ``grads`` of every variable and of
    ``states``."""
    att = attentive(params, states, mask, "encoder_att", dtype)
    pooled = max_pool(states, mask, dtype)
    main = classifier(params, [att["output"], pooled["out"]], targets, "classifier", layers, activation, dtype)
    adv = classifier(params, [pooled["out"]], targets, "classifier_adv", 0, activation, dtype)
    grads = dict(main["grads"])
    grads.update(adv["grads"])
    d_main = main["grads"]["inputs"]
    width = att["output"].shape[1]
    d_pool = d_main[:, width:] - adv["grads"]["inputs"]                      # the view: exact negation
    g_att, dx = attentive_bwd(att, d_output=d_main[:, :width], name="encoder_att", dtype=dtype)
    grads.update(g_att)
    grads.pop("inputs")
    grads["states"] = dx + max_pool_bwd(states, mask, d_pool, dtype)
    return {"cost": main["cost"] + adv["cost"], "cost_main": main["cost"], "cost_adv": adv["cost"], "grads": grads,
            "d_pool": d_pool, "pooled": pooled["out"], "att_output": att["output"]}
