"""The distillation objective of ``GPT2.distill_loss`` (cross entropy + forward or reverse KL to a teacher's logits),
stated once in plain torch.

``distill_reference`` is the rule; the HIP kernels of csrc/distill_loss.hip compute the same loss, per-row values and
(through the existing backward) gradient from one read of the student's and the teacher's logits, and the tests hold them
to this function in fp64.

A row is a (b, t) with label y, aligned as in ``forward(idx, labels)``. Rows with ``y == ignore_index`` are not counted;
N is the number of counted rows. Per counted row, with s the student's logits, t the teacher's and tau = temperature > 0:

    p = softmax(s)      p_tau = softmax(s / tau)      q = softmax(t / tau)
    ce   = -log p[y]
    kd   = tau^2 KL(q || p_tau)          kind = "forward" (Hinton et al., 2015; mode covering)
         = tau^2 KL(p_tau || q)          kind = "reverse" (mode seeking)
    loss = (1/N) sum_rows (ce_coef ce + kd_coef kd)

    dloss/ds_v = (1/N) [ce_coef (p_v - [v = y]) + kd_coef tau (p_tau_v - q_v)]                                  forward
               = (1/N) [ce_coef (p_v - [v = y]) + kd_coef tau p_tau_v (log p_tau_v - log q_v - KL(p_tau || q))]  reverse

The teacher is a constant: nothing flows into ``teacher_logits``. The tau^2 keeps the size of the distillation gradient
independent of the temperature. ``labels`` is always needed, it is the row mask; ``ce_coef = 0`` is pure distillation.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

KINDS = ("forward", "reverse")
METRICS = ("ce", "kd")


class DistillReference(NamedTuple):
    loss: torch.Tensor  # scalar, differentiable with respect to logits
    ce: torch.Tensor    # per row, detached, 0 where ignored: -log p[label]
    kd: torch.Tensor    # tau^2 KL


class DistillOutput(NamedTuple):
    """What ``GPT2.distill_loss`` returns: the differentiable scalar ``loss``; the detached fp32 [B, T] per-token ``ce``
    and ``kd`` (0 where the label is ignored); ``metrics``, a dict of two device scalars, the means of ce and kd over
    the counted tokens."""
    loss: torch.Tensor
    ce: torch.Tensor
    kd: torch.Tensor
    metrics: dict


def distill_reference(logits: torch.Tensor, labels: torch.Tensor, teacher_logits: torch.Tensor,
                      temperature: float = 1.0, ce_coef: float = 0.5, kd_coef: float = 0.5, kind: str = "forward",
                      ignore_index: int = -100) -> DistillReference:
    """The rule above on ``logits`` and ``teacher_logits`` [..., V] and ``labels`` of the leading shape, in the dtype of
    ``logits`` (fp64 in the tests). The per-row results have the leading shape."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS} (got {kind!r})")
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0 (got {temperature})")
    shape = labels.shape
    z = logits.reshape(-1, logits.shape[-1])
    t = teacher_logits.detach().reshape(-1, z.shape[1]).to(z.dtype)
    y = labels.reshape(-1)
    keep = y != ignore_index
    n = keep.sum()
    ce = -torch.log_softmax(z, dim=-1).gather(1, y.clamp(0, z.shape[1] - 1)[:, None])[:, 0]
    lp, lq = torch.log_softmax(z / temperature, dim=-1), torch.log_softmax(t / temperature, dim=-1)
    a, b = (lq, lp) if kind == "forward" else (lp, lq)  # KL(a || b)
    pa = a.exp()
    kl = torch.where(pa > 0, pa * (a - b), torch.zeros_like(pa)).sum(-1)
    kd = temperature * temperature * kl
    obj = ce_coef * ce + kd_coef * kd
    zero = torch.zeros_like(obj)
    loss = torch.where(keep, obj, zero).sum() / n

    def row(v):
        return torch.where(keep, v.detach(), zero.detach()).reshape(shape)

    return DistillReference(loss, row(ce), row(kd))
