"""The policy-gradient objective of ``GPT2.policy_loss`` (PPO-clip / GRPO / REINFORCE), stated once in plain torch.

``policy_reference`` is the rule; the HIP kernels of csrc/policy_loss.hip compute the same loss, per-row values and
(through the existing backward) gradient from one read of the logits, and the tests hold them to this function in fp64.

A row is a (b, t) with label y, aligned as in ``forward(idx, labels)``: ``labels[b, t]`` is the token the logits at
(b, t) are scored on. Rows with ``y == ignore_index`` are not counted; N is the number of counted rows. Per counted row:

    logp = logits[y] - logsumexp(logits)
    r    = exp(logp - old)                 old = old_logprobs[b, t]; None: old = logp detached, r = 1 exactly
    s    = min(r A, clamp(r, 1 - clip_low, 1 + clip_high) A)          A = advantages[b, t]; a tie is the unclipped term
    d    = ref - logp,  k3 = exp(d) - d - 1                           the GRPO KL estimator (Schulman's k3), >= 0
    H    = -sum_v p_v log p_v

    loss = -(1/N) sum_rows (s - kl_coef k3 + entropy_coef H)
    dloss/dlogits_v = (1/N) [c (p_v - [v = y]) + entropy_coef p_v (log p_v + H)]
    c    = (r A if the unclipped term is the minimum, else 0) - kl_coef (1 - exp(d))

k3 enters the loss only with ``ref_logprobs`` and ``kl_coef != 0``. The normalisation is the token mean over the call's
counted rows. A per-sequence or per-group normalisation (GRPO's 1/|o_i|, Dr. GRPO's constant) is the caller's, folded
into ``advantages``: scale row (b, t)'s advantage by N times the weight that row should have.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch


class PolicyReference(NamedTuple):
    loss: torch.Tensor      # scalar, differentiable with respect to logits
    logp: torch.Tensor      # per row, detached, 0 where ignored: log p[label]
    ratio: torch.Tensor     # r
    kl: torch.Tensor        # k3 (0 without ref_logprobs)
    entropy: torch.Tensor   # H
    clipped: torch.Tensor   # 1 where clamp(r) != r, else 0


class PolicyOutput(NamedTuple):
    """What ``GPT2.policy_loss`` returns: the differentiable scalar ``loss``; the detached fp32 [B, T] per-token
    ``logprobs``, ``ratio``, ``kl``, ``entropy`` and ``clipped`` (0 where the label is ignored); ``metrics``, a dict of
    four device scalars, the means over the counted tokens of ratio, clipped, kl and entropy."""
    loss: torch.Tensor
    logprobs: torch.Tensor
    ratio: torch.Tensor
    kl: torch.Tensor
    entropy: torch.Tensor
    clipped: torch.Tensor
    metrics: dict


METRICS = ("ratio", "clip_fraction", "kl", "entropy")


def policy_reference(logits: torch.Tensor, labels: torch.Tensor, advantages: torch.Tensor,
                     old_logprobs: Optional[torch.Tensor] = None, ref_logprobs: Optional[torch.Tensor] = None,
                     clip_low: float = 0.2, clip_high: float = 0.2, kl_coef: float = 0.0, entropy_coef: float = 0.0,
                     ignore_index: int = -100) -> PolicyReference:
    """The rule above on ``logits`` [..., V] and ``labels``, ``advantages``, ``old_logprobs``, ``ref_logprobs`` of the
    leading shape, in the dtype of ``logits`` (fp64 in the tests). The per-row results have the leading shape."""
    shape = labels.shape
    z = logits.reshape(-1, logits.shape[-1])
    y = labels.reshape(-1)
    dt = z.dtype
    keep = y != ignore_index
    n = keep.sum()
    lp_all = torch.log_softmax(z, dim=-1)
    logp = lp_all.gather(1, y.clamp(0, z.shape[1] - 1)[:, None])[:, 0]
    adv = advantages.reshape(-1).to(dt)
    old = logp.detach() if old_logprobs is None else old_logprobs.reshape(-1).to(dt)
    r = torch.exp(logp - old)
    rc = r.clamp(1.0 - clip_low, 1.0 + clip_high)
    u, v = r * adv, rc * adv
    s = torch.where(u <= v, u, v)
    k3 = torch.zeros_like(logp)
    if ref_logprobs is not None:
        d = ref_logprobs.reshape(-1).to(dt) - logp
        k3 = torch.expm1(d) - d
    p = lp_all.exp()
    H = -torch.where(p > 0, p * lp_all, torch.zeros_like(p)).sum(-1)
    obj = s + entropy_coef * H
    if ref_logprobs is not None and kl_coef != 0:
        obj = obj - kl_coef * k3
    zero = torch.zeros_like(obj)
    loss = -torch.where(keep, obj, zero).sum() / n

    def row(t):
        return torch.where(keep, t.detach(), zero.detach()).reshape(shape)

    return PolicyReference(loss, row(logp), row(r), row(k3), row(H), row((rc != r).to(dt)))

