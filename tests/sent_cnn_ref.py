"""Float64 torch restatement of the reference's SentenceCNNEncoder (encoders/sentence_cnn_encoder.py:103-196,
nn/highway.py:6-57, tf.nn.bidirectional_dynamic_rnn over OrthoGRUCell): test infrastructure, CPU only.

Conventions are TensorFlow's: conv1d SAME pads (w - 1) // 2 positions before and the rest after; the SAME max-pool pads
(S' s - S) // 2 positions before (padded slots never win); dynamic_rnn emits zeros and carries the state past a
sentence's length; the backward direction runs on the length-reversed sequence (tf.reverse_sequence)."""
import math

import torch
import torch.nn.functional as TF


def conv_relu(x, w, b):
    """relu(conv1d_SAME(x [B, S, E], w [w, E, n]) + b): [B, n, S]."""
    width = w.shape[0]
    pad = (width - 1) // 2
    xp = TF.pad(x.transpose(1, 2), (pad, width - 1 - pad))
    return torch.relu(TF.conv1d(xp, w.permute(2, 1, 0)) + b[None, :, None])


def same_max_pool(r, s):
    """SAME max-pool of [B, n, S] over windows of s, stride s: [B, n, ceil(S / s)]."""
    slen = r.shape[2]
    sp = (slen + s - 1) // s
    pb = (sp * s - slen) // 2
    rp = TF.pad(r, (pb, sp * s - slen - pb), value=-math.inf)
    return rp.view(r.shape[0], r.shape[1], sp, s).max(-1).values


def _reverse(x, lengths):
    """tf.reverse_sequence along axis 1: the first lengths[b] rows of sentence b reversed, the rest in place."""
    steps = x.shape[1]
    idx = torch.arange(steps)[None, :].expand(x.shape[0], steps)
    rev = lengths[:, None] - 1 - idx
    idx = torch.where(rev >= 0, rev, idx)
    return x.gather(1, idx[:, :, None].expand(-1, -1, x.shape[2]))


def gru_layer(x, lengths, p, reverse):
    """One direction of dynamic_rnn over TF GRUCell (r, u = sigmoid([x, h] Wg + bg); c = tanh([x, r h] Wc + bc);
    h' = u h + (1 - u) c): (outputs [B, T, H], final state [B, H])."""
    if reverse:
        x = _reverse(x, lengths)
    hsz = p["candidate/bias"].shape[0]
    h = x.new_zeros(x.shape[0], hsz)
    outs = []
    for t in range(x.shape[1]):
        live = (t < lengths)[:, None]
        g = torch.sigmoid(torch.cat([x[:, t], h], 1) @ p["gates/kernel"] + p["gates/bias"])
        r, u = g[:, :hsz], g[:, hsz:]
        c = torch.tanh(torch.cat([x[:, t], r * h], 1) @ p["candidate/kernel"] + p["candidate/bias"])
        new = u * h + (1 - u) * c
        outs.append(torch.where(live, new, torch.zeros_like(new)))
        h = torch.where(live, new, h)
    out = torch.stack(outs, 1)
    return (_reverse(out, lengths) if reverse else out), h


def encoder(x, mask, lengths, params, filters, segment, depth, drop=None):
    """(temporal_states [B, S', 2H], output [B, 2H], temporal_mask [B, S']) of SentenceCNNEncoder.  ``params``: local
    variable name -> tensor; ``drop``: the input dropout's keep mask already divided by keep_prob (None: no dropout)."""
    if drop is not None:
        x = x * drop
    pooled = [same_max_pool(conv_relu(x, params["conv-maxpool-{}/conv_W".format(w)],
                                      params["conv-maxpool-{}/conv_bias".format(w)]), segment) for w, _ in filters]
    h = torch.cat(pooled, 1).transpose(1, 2)
    for i in range(depth):
        pre = "highway_layer_{}/".format(i)
        t = torch.sigmoid(h @ params[pre + "weight_T"] + params[pre + "bias_T"])
        hh = torch.relu(h @ params[pre + "weight_H"] + params[pre + "bias_H"])
        h = hh * t + h * (1 - t)
    seq = (lengths + segment - 1) // segment
    cell = lambda d: {k: params["bidirectional_rnn/{}/OrthoGRUCell/{}".format(d, k)]
                      for k in ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")}
    fw, fw_final = gru_layer(h, seq, cell("fw"), False)
    bw, bw_final = gru_layer(h, seq, cell("bw"), True)
    pmask = same_max_pool(mask[:, None, :], segment)[:, 0]
    return torch.cat([fw, bw], 2), torch.cat([fw_final, bw_final], 1), pmask
