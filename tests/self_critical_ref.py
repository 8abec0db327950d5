"""Float64 restatement of the self-critical loss (trainers/self_critical_objective.py) for the model of
tests/golden/self_critical: the encoder, attention step and GRU cell of oracle/torch_ref.py, stepped as the greedy loop
steps them -- but with the decoded symbols, the mask and D = reward(runtime) - reward(train) HELD CONSTANT, which is what
the objective differentiates (rewards and argmax have no gradient; tf.stop_gradient on the reward difference):

    loss = -sum_{t,b} D_b * nll[t, b] * mask[t, b] / sum(mask)

with nll the negative log-likelihood of argmax[t, b] under the logits of step t, whose input is <s> at t = 0 and
argmax[t - 1, b] * (sentence b unfinished before step t - 1) afterwards (decoders/autoregressive.py:466-480).

TEST INFRASTRUCTURE ONLY; held to the reference by tests/test_self_critical_host.py: it reproduces the fixture's loss,
and its autograd gradient meets the central differences of the reference's loss."""
import numpy as np
import torch

from oracle import nm_oracle as O
from oracle import torch_ref as TR


def fed_symbols(argmax_tb):
    """symbols[t] = argmax[t] where the sentence had not finished before step t, else <pad>; and the mask the loop
    writes: 1 while the sentence is unfinished AFTER step t (the end token's own position carries 0)."""
    argmax_tb = np.asarray(argmax_tb)
    symbols, mask = np.zeros_like(argmax_tb), np.zeros(argmax_tb.shape, np.float64)
    finished = np.zeros(argmax_tb.shape[1], bool)
    for t in range(argmax_tb.shape[0]):
        symbols[t] = np.where(finished, O.PAD, argmax_tb[t])
        finished = finished | (symbols[t] == O.END)
        mask[t] = ~finished
    return symbols, mask


def runtime_logits(p, src_ids, symbols_tb, enc_name="encoder", dec_name="decoder", att_name="attention"):
    """[T, B, V] logits of the greedy loop fed ``symbols_tb`` (Decoder.next_state, decoders/decoder.py:279-358)."""
    states, mask, final = TR.encoder(p, src_ids, enc_name)
    sym = torch.as_tensor(np.asarray(symbols_tb), dtype=torch.long)
    steps, bsz = sym.shape
    a, n = att_name, dec_name
    hf = states @ p[f"{a}/attn_key_projection"]
    h = final @ p[f"{n}/initial_state/encoders_projection/kernel"] + p[f"{n}/initial_state/encoders_projection/bias"]
    emb = p[f"{n}/word_embeddings"]
    cell = f"{n}/attention_decoder/OrthoGRUCell"
    cw = (p[f"{cell}/gates/kernel"], p[f"{cell}/gates/bias"], p[f"{cell}/candidate/kernel"], p[f"{cell}/candidate/bias"])
    aw = (p[f"{a}/Attention/attn_query_projection"], p[f"{a}/attn_projection_bias"], p[f"{a}/attn_similarity_v"],
          p[f"{a}/attn_bias"])
    ow, ob = p[f"{n}/attention_decoder/dense/kernel"], p[f"{n}/attention_decoder/dense/bias"]
    lw, lb = p[f"{n}/state_to_word_W"], p[f"{n}/state_to_word_b"]
    x = emb[torch.full((bsz,), O.START, dtype=torch.long)]
    logits = []
    for t in range(steps):
        h = TR.gru_cell(x, h, *cw)
        ctx, _ = TR.attention_step(h, hf, states, mask, *aw)
        out = torch.tanh(torch.cat([h, x, ctx], 1) @ ow + ob)
        logits.append(out @ lw + lb)
        x = emb[sym[t]]
    return torch.stack(logits)


def self_critical_loss(p, src_ids, argmax_tb, reward_diff):
    """The loss with the decoding held constant; ``p`` holds torch tensors (TR.to_torch) of either precision."""
    symbols, mask = fed_symbols(argmax_tb)
    logits = runtime_logits(p, src_ids, symbols)
    targets = torch.as_tensor(np.asarray(argmax_tb), dtype=torch.long)
    nll = -torch.log_softmax(logits, -1).gather(2, targets[:, :, None])[:, :, 0]
    m = torch.as_tensor(mask, dtype=logits.dtype)
    d = torch.as_tensor(np.asarray(reward_diff, np.float64), dtype=logits.dtype)
    return -(d[None, :] * nll * m).sum() / m.sum(), logits, mask


def loss_and_gradients(params, src_ids, argmax_tb, reward_diff, dtype=torch.float64):
    """(loss, {variable: gradient}, logits, mask) as NumPy arrays."""
    p = TR.to_torch(params, dtype=dtype)
    loss, logits, mask = self_critical_loss(p, src_ids, argmax_tb, reward_diff)
    loss.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in p.items()}
    return float(loss.detach()), grads, logits.detach().numpy(), mask
