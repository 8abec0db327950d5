"""NumPy restatement of the CTC head of the reference's decoders/ctc_decoder.py as TensorFlow 1.x computes it
(tf.nn.ctc_loss with ignore_longer_outputs_than_inputs=True, tf.nn.ctc_greedy_decoder): test infrastructure, CPU only.
Every function takes the dtype it computes in (float64: the expected values; float32: the unit of the GPU tolerances).

Conventions: logits [T, B, K], the blank is class K - 1; ``labels`` is a list of B label lists (pads already removed);
frames t >= frame_lens[b] do not count.  With l' the labels with blanks interleaved (S = 2L + 1 states):
  * start in states 0 and 1, end in the last two;
  * state u keeps itself (self-loop) only if ``merge_repeated`` or l'[u] is the blank;
  * u - 1 -> u always; u - 2 -> u if l'[u] is no blank and not (``merge_repeated`` and l'[u] == l'[u - 2]).
A sentence without a valid alignment (zero frames; more labels -- plus the blanks repeats need when merging -- than
frames) has loss 0 and gradient 0; an empty label sequence is the all-blank path."""
import itertools

import numpy as np

END = 2           # vocabulary.END_TOKEN_INDEX
PAD = 0           # vocabulary.PAD_TOKEN_INDEX


def prepare_labels(ids, merge_repeated_targets):
    """Padded id rows -> label lists: pads removed, then (preprocess_collapse_repeated) adjacent repeats collapsed."""
    out = []
    for row in ids:
        kept = [int(c) for c in row if int(c) != PAD]
        if merge_repeated_targets:
            kept = [c for i, c in enumerate(kept) if i == 0 or c != kept[i - 1]]
        out.append(kept)
    return out


def log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def _lse(stack):
    """log sum exp over axis 0 of a [n, S] stack that may hold -inf (all -inf -> -inf)."""
    m = stack.max(axis=0)
    safe = np.where(np.isfinite(m), m, 0).astype(stack.dtype)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), safe + np.log(np.exp(stack - safe).sum(axis=0)), -np.inf).astype(stack.dtype)


def _transitions(lab, blank, merge):
    ext = np.full(2 * len(lab) + 1, blank, dtype=np.int64)
    ext[1::2] = lab
    odd = np.arange(len(ext)) % 2 == 1
    keep = np.ones(len(ext), bool) if merge else ~odd
    skip = odd.copy()
    skip[:2] = False
    if merge and len(ext) > 2:
        skip[2:] &= ext[2:] != ext[:-2]
    return ext, keep, skip


def has_alignment(lab, frames, merge):
    repeats = sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])
    return frames >= 1 and len(lab) + (repeats if merge else 0) <= frames


def sentence_loss_and_grad(x, lab, merge, dtype=np.float64):
    """x [T, K] logits of the frames that count -> (loss, d loss / d x [T, K]) by alpha-beta; (0, zeros) without an
    alignment."""
    x = np.asarray(x, dtype=dtype)
    frames, k = x.shape
    if not has_alignment(lab, frames, merge):
        return dtype(0.0), np.zeros_like(x)
    lp = log_softmax(x)
    ext, keep, skip = _transitions(lab, k - 1, merge)
    s = len(ext)
    ninf = dtype(-np.inf)
    em = lp[:, ext]                                                  # [T, S]
    alpha = np.full((frames, s), ninf, dtype=dtype)
    alpha[0, :2] = em[0, :2]
    for t in range(1, frames):
        prev = alpha[t - 1]
        one = np.concatenate(([ninf], prev))[:s]
        two = np.concatenate(([ninf, ninf], prev))[:s]
        alpha[t] = em[t] + _lse(np.stack([np.where(keep, prev, ninf), one, np.where(skip, two, ninf)]))
    # beta without the state's own emission: tail[t, u] = log sum over what may follow (t, u)
    tail = np.full((frames, s), ninf, dtype=dtype)
    tail[-1, max(0, s - 2):] = 0.0
    skip_from = np.concatenate((skip, [False, False]))[2:]             # u -> u + 2 allowed
    for t in range(frames - 2, -1, -1):
        nxt = em[t + 1] + tail[t + 1]
        one = np.concatenate((nxt, [ninf]))[1:]
        two = np.concatenate((nxt, [ninf, ninf]))[2:]
        tail[t] = _lse(np.stack([np.where(keep, nxt, ninf), one, np.where(skip_from, two, ninf)]))
    log_z = _lse(alpha[-1, max(0, s - 2):][:, None])[0]
    post = np.exp(alpha + tail - log_z)                              # [T, S] posterior of every state
    occ = np.zeros_like(x)
    for u in range(s):
        occ[:, ext[u]] += post[:, u]
    return dtype(-log_z), (np.exp(lp) - occ).astype(dtype)


def ctc_loss_and_grad(logits, labels, frame_lens, merge, dtype=np.float64, scale=1.0):
    """(loss [B], scale * d sum(loss) / d logits [T, B, K]); frames at or past a sentence's length get zeros."""
    logits = np.asarray(logits, dtype=dtype)
    steps, bsz, _ = logits.shape
    loss = np.zeros(bsz, dtype=dtype)
    grad = np.zeros_like(logits)
    for b in range(bsz):
        n = int(min(max(frame_lens[b], 0), steps))
        loss[b], g = sentence_loss_and_grad(logits[:n, b], list(labels[b]), merge, dtype)
        grad[:n, b] = dtype(scale) * g
    return loss, grad


def brute_force_loss(lp, lab, merge):
    """-log of the summed probability of every path of len(lp) frames that collapses to ``lab`` (torch, differentiable):
    with ``merge`` repeated classes merge before the blanks are removed, without it only the blanks are removed."""
    import torch
    frames, k = lp.shape
    blank = k - 1
    terms = []
    for path in itertools.product(range(k), repeat=frames):
        seq = [c for i, c in enumerate(path) if not (merge and i > 0 and c == path[i - 1])]
        if [c for c in seq if c != blank] == list(lab):
            terms.append(sum(lp[t, c] for t, c in enumerate(path)))
    if not terms:
        return None
    return -torch.logsumexp(torch.stack(terms), 0)


def greedy(logits, frame_lens, merge, end=END):
    """tf.nn.ctc_greedy_decoder + sparse_tensor_to_dense(default END), transposed: ([width, B] int32 time-major with
    width = the longest emitted sequence, the emitted lists).  Ties go to the lowest class; the previous class is the
    previous FRAME's, blanks included."""
    logits = np.asarray(logits)
    steps, bsz, k = logits.shape
    outs = []
    for b in range(bsz):
        prev, seq = None, []
        for t in range(int(min(max(frame_lens[b], 0), steps))):
            c = int(np.argmax(logits[t, b]))
            if c != k - 1 and not (merge and c == prev):
                seq.append(c)
            prev = c
        outs.append(seq)
    width = max([len(s) for s in outs], default=0)
    dense = np.full((width, bsz), end, dtype=np.int32)
    for b, seq in enumerate(outs):
        dense[:len(seq), b] = seq
    return dense, outs


def top_two_gap(logits):
    """[T, B] difference between the largest and the second largest class of every frame."""
    part = np.sort(np.asarray(logits, dtype=np.float64), axis=-1)
    return part[..., -1] - part[..., -2] if part.shape[-1] > 1 else np.full(part.shape[:-1], np.inf)
