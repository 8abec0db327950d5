"""NumPy restatement of the sequence-labelling heads of the reference's decoders/sequence_labeler.py and of
runners/label_runner.py as TensorFlow 1.x computes them: test infrastructure, CPU only.  Every function takes the dtype
it computes in (float64: the expected values; float32: the unit of the GPU tolerances).

``rows``: what one row of logits is asked for -- tf.nn.log_softmax, tf.argmax (first maximum),
sparse_softmax_cross_entropy_with_logits * sentence_mask(targets), and the gradient of the summed loss.  A target that
is neither <pad> nor a class gives loss NaN and gradient 0 (the engine's convention for a caller's error, as in its CTC
head; TensorFlow's CPU kernel raises there).  ``head``: the model from the encoders' states to the cost, with the
analytic gradient of the cost w.r.t. every head variable and the states."""
import numpy as np

END = 2           # vocabulary.END_TOKEN_INDEX
PAD = 0           # vocabulary.PAD_TOKEN_INDEX


def rows(logits, targets=None, pad=PAD, scale=1.0, dtype=np.float64, row_mask=None, masked_class=END):
    """logits [R, K] -> dict: logprobs [R, K], argmax [R]; with targets [R]: loss [R] and grad [R, K] = scale *
    d sum(loss) / d logits; with row_mask [R]: labels [R]."""
    x = np.asarray(logits, dtype=dtype)
    k = x.shape[1]
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis=1, keepdims=True)
    lse = np.log(s)
    out = {"logprobs": (x - m) - lse, "argmax": np.argmax(x, axis=1).astype(np.int32)}
    if targets is not None:
        t = np.asarray(targets, dtype=np.int64)
        counted = t != pad
        valid = (t >= 0) & (t < k)
        safe = np.where(valid, t, 0)
        xt = np.take_along_axis(x, safe[:, None], axis=1)[:, 0]
        nll = lse[:, 0] - (xt - m[:, 0])
        out["loss"] = np.where(counted, np.where(valid, nll, np.nan), 0.0).astype(dtype)
        onehot = np.zeros_like(x)
        onehot[np.arange(len(t)), safe] = 1.0
        out["grad"] = (dtype(scale) * (e / s - onehot) * (counted & valid)[:, None]).astype(dtype)
    if row_mask is not None:
        out["labels"] = np.where(np.asarray(row_mask) != 0, out["argmax"], masked_class).astype(np.int32)
    return out


def top_two_gap(logits):
    """[R] difference between the largest and the second largest class of every row (inf for one class)."""
    part = np.sort(np.asarray(logits, dtype=np.float64), axis=-1)
    return part[..., -1] - part[..., -2] if part.shape[-1] > 1 else np.full(part.shape[:-1], np.inf)


ACT = {"relu": (lambda z: np.maximum(z, 0), lambda y: (y > 0)),
       "tanh": (np.tanh, lambda y: 1 - y * y),
       "identity": (lambda z: z, lambda y: np.ones_like(y))}


def head(params, states, targets, kind="sequence", name="tagger", activation="relu", table=None, train_embeddings=True,
         dtype=np.float64, pad=PAD):
    """``states``: list of [B, T, D_e] encoder states (concatenated along the features, :93-98); ``params``: name ->
    array with ``<name>/hidden_layer/kernel|bias`` (optional), ``<name>/logits/kernel|bias`` (kind "sequence") or
    ``<name>/project_for_embeddings/kernel|bias`` (optional, kind "embeddings", with ``table`` [V, E]).  Returns the
    reference's tensors and ``grads``: d cost / d (every variable, ``table``, ``states`` -- the concatenation)."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    cat = np.concatenate([np.asarray(s, dtype=dtype) for s in states], axis=2)
    bsz, steps, width = cat.shape
    flat = cat.reshape(bsz * steps, width)
    hid_k, hid_b = name + "/hidden_layer/kernel", name + "/hidden_layer/bias"
    fwd, dfn = ACT[activation]
    hidden = fwd(flat @ p[hid_k] + p[hid_b]) if hid_k in p else flat
    proj_k, proj_b = name + "/project_for_embeddings/kernel", name + "/project_for_embeddings/bias"
    if kind == "sequence":
        pre = hidden
        logits = pre @ p[name + "/logits/kernel"] + p[name + "/logits/bias"]
    else:
        emb = np.asarray(table, dtype=dtype)
        pre = hidden @ p[proj_k] + p[proj_b] if proj_k in p else hidden
        logits = pre @ emb.T
    tgt = np.asarray(targets).reshape(-1)
    r = rows(logits, tgt, pad, 1.0, dtype)
    mask = (tgt != pad).astype(dtype)
    count = mask.sum()
    cost = r["loss"].sum() / (count + dtype(1e-9))
    out = {"states": hidden.reshape(bsz, steps, -1), "logits": logits.reshape(bsz, steps, -1),
           "logprobs": r["logprobs"].reshape(bsz, steps, -1), "decoded": r["argmax"].reshape(bsz, steps),
           "train_mask": mask.reshape(bsz, steps), "train_xents": r["loss"].reshape(bsz, steps), "cost": cost}
    dlogits = r["grad"] / (count + dtype(1e-9))
    grads = {}
    if kind == "sequence":
        grads[name + "/logits/kernel"] = pre.T @ dlogits
        grads[name + "/logits/bias"] = dlogits.sum(axis=0)
        dpre = dlogits @ p[name + "/logits/kernel"].T
    else:
        grads["table"] = dlogits.T @ pre if train_embeddings else np.zeros_like(emb)
        dpre = dlogits @ emb
        if proj_k in p:
            grads[proj_k] = hidden.T @ dpre
            grads[proj_b] = dpre.sum(axis=0)
            dpre = dpre @ p[proj_k].T
    if hid_k in p:
        dz = dpre * dfn(hidden)
        grads[hid_k] = flat.T @ dz
        grads[hid_b] = dz.sum(axis=0)
        dpre = dz @ p[hid_k].T
    grads["states"] = dpre.reshape(bsz, steps, width)
    out["grads"] = grads
    return out


def runner_sentences(decoded, input_mask, words, end=END):
    """runners/label_runner.py:34-48: masked positions become </s>; every sentence is cut before its first </s>
    (vocabulary.py:257-288).  ``words``: index -> string."""
    labels = np.where(np.asarray(input_mask) != 0, np.asarray(decoded), end)
    out = []
    for row in labels:
        sent = []
        for c in row:
            if c == end:
                break
            sent.append(words[int(c)])
        out.append(sent)
    return out
