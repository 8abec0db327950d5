"""Float64 / float32 restatement of the REINFORCE loss (trainers/rl_trainer.py) for the model of tests/golden/reinforce
(the one of tests/golden/self_critical): the decoder of tests/self_critical_ref.py stepped as a sampling loop steps it,
with the drawn symbols, the rewards and the baseline HELD CONSTANT -- which is what the objective differentiates:

    sent_logprob[s, b] = -sum_{t < steps_s} nll[s, t, b]        nll under logits / temperature, <pad> rows included
    p                  = softmax_s(alpha * sent_logprob) with normalize, else sent_logprob
    loss               = mean_b sum_s -(reward[s, b] - baseline) * p[s, b]  +  ce_smoothing * cost

with ``cost`` the teacher-forced cross entropy over the target's non-pad positions.

TEST INFRASTRUCTURE ONLY; held to the reference by tests/test_reinforce_host.py: it reproduces each fixture's sentence
log-probabilities and loss, and its autograd gradient meets the central differences of the reference's loss."""
import numpy as np
import torch

from oracle import torch_ref as TR

from .self_critical_ref import runtime_logits


def reinforce_loss(p, src_ids, tgt_ids, symbols, steps, rewards, baseline, mode):
    """``symbols`` [S, T, B] (the loops' output symbols: <pad> for finished sentences), ``steps`` [S], ``rewards``
    [S, B], ``baseline`` a number, ``mode`` the constructor's keyword arguments.  Returns (loss, sent_logprobs)."""
    dtype = next(iter(p.values())).dtype
    temperature = float(mode.get("temperature", 1.0))
    logprobs = []
    for sym, n in zip(np.asarray(symbols), np.asarray(steps)):
        sym = sym[:int(n)]
        logits = runtime_logits(p, src_ids, sym) / temperature
        targets = torch.as_tensor(sym, dtype=torch.long)
        nll = -torch.log_softmax(logits, -1).gather(2, targets[:, :, None])[:, :, 0]
        logprobs.append(-nll.sum(0))
    logprobs = torch.stack(logprobs)
    advantage = torch.as_tensor(np.asarray(rewards, np.float64) - float(baseline), dtype=dtype)
    scored = torch.softmax(logprobs * float(mode.get("alpha", 1.0)), 0) if mode.get("normalize") else logprobs
    loss = (-advantage * scored).sum(0).mean()
    if mode.get("ce_smoothing", 0.0) > 0.0:
        tgt = np.asarray(tgt_ids)
        logits = runtime_logits(p, src_ids, tgt)                       # fed the targets: teacher forcing
        targets = torch.as_tensor(tgt, dtype=torch.long)
        nll = -torch.log_softmax(logits, -1).gather(2, targets[:, :, None])[:, :, 0]
        mask = torch.as_tensor(tgt != 0, dtype=dtype)
        loss = loss + float(mode["ce_smoothing"]) * (nll * mask).sum() / mask.sum()
    return loss, logprobs


def loss_and_gradients(params, src_ids, tgt_ids, symbols, steps, rewards, baseline, mode, dtype=torch.float64):
    """(loss, {variable: gradient}, sent_logprobs) as NumPy values."""
    p = TR.to_torch({k: v for k, v in params.items() if np.asarray(v).dtype.kind == "f"}, dtype=dtype)
    loss, logprobs = reinforce_loss(p, src_ids, tgt_ids, symbols, steps, rewards, baseline, mode)
    loss.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in p.items()}
    return float(loss.detach()), grads, logprobs.detach().numpy()
