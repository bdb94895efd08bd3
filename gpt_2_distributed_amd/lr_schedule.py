"""Learning-rate schedules for the trainer (pure Python: the value is a function of the optimizer-step count, so a
resumed run needs no schedule state beyond the step the checkpoint restores).

``cosine`` is nanoGPT's rule: linear warmup over ``warmup_steps`` steps, cosine decay to ``min_lr`` at ``decay_steps``,
``min_lr`` from there on. The reference trainer keeps the rate constant (its TODO: "Use a cosine annealing scheduler
for the learning rate").
"""
from __future__ import annotations

import math

KINDS = ("constant", "cosine")


def lr_at(step: int, lr: float, warmup_steps: int = 0, decay_steps: int = 0, min_lr: float = 0.0,
          kind: str = "cosine") -> float:
    """The learning rate of the optimizer step taken after ``step`` earlier ones (step 0 is the first)."""
    if kind not in KINDS:
        raise ValueError(f"lr schedule {kind!r}: expected one of {KINDS}")
    if step < 0:
        raise ValueError(f"step={step} must be >= 0")
    if kind == "constant":
        return lr
    if not decay_steps > warmup_steps >= 0:
        raise ValueError(f"need decay_steps > warmup_steps >= 0 (got warmup_steps={warmup_steps}, "
                         f"decay_steps={decay_steps})")
    if not 0 <= min_lr <= lr:
        raise ValueError(f"need 0 <= min_lr <= lr (got min_lr={min_lr}, lr={lr})")
    if step < warmup_steps:
        return lr * (step + 1) / (warmup_steps + 1)
    if step > decay_steps:
        return min_lr
    ratio = (step - warmup_steps) / (decay_steps - warmup_steps)
    return min_lr + 0.5 * (1.0 + math.cos(math.pi * ratio)) * (lr - min_lr)
