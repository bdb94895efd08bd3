"""Generate the gradient-clipping / lr-schedule goldens by running the REFERENCE model (`/root/reference/model.py`)
with torch's own clip_grad_norm_ and AdamW. Build container only, on the CPU:
    python tests/golden/make_clip_golden.py

Outputs (data only):
  tiny_clip_traj.json   TINY config, seed 42, AdamW(lr 1e-3, wd 0.1, betas 0.9/0.95), B=2, grad_accum=2, 12 steps,
                        Zipf tokens (tiny_traj.json's recipe, stored in the file), clip_grad_norm_(params, 1.0) and the
                        lr of lr_schedule.lr_at (cosine, warmup 3, decay 10, min lr/10) set before every step: per-step
                        loss, pre-clip norm, lr, final-parameter fingerprints, and the loss trajectory of the same run
                        with clipping off. The two trajectories must differ by >= 10x the fp32 loss tolerance (1e-4)
                        from step 3 on (counting from 0, as lr_at does), or this script fails.
  clip_ddp_golden.json  ddp_golden.json's configuration and data (DDPCFG, 2 ranks x B=2, grad_accum=2, lr 1e-3, the
                        reference single-process on the concatenated batch) with clip_grad_norm_(params, 1.2): of the
                        unclipped norms 1.855, 1.314, 1.085 two steps clip and one does not. The clipped run must be
                        >= 10x the gating tolerance away from the unclipped one on a field tests/test_clip_ddp_gpu.py
                        gates (loss 1e-4; the parameters' leading values, rtol 1e-4 + atol 1e-2 lr); steps are added
                        until it is, and the count is recorded.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")

import model as ref_model  # noqa: E402  (reference)

from gpt_2_distributed_amd.lr_schedule import lr_at  # noqa: E402

TINY = dict(n_layer=2, n_head=2, n_embd=128, vocab_size=509, n_positions=64, resid_pdrop=0.0, attn_pdrop=0.0)
DDPCFG = dict(n_layer=2, n_head=4, n_embd=256, vocab_size=509, n_positions=64, resid_pdrop=0.0, attn_pdrop=0.0)
LOSS_TOL, PAR_RTOL = 1e-4, 1e-4  # the fp32 gates of tests/test_model_gpu.py and tests/test_ddp_gpu.py


def _param_checks(m):
    out = {}
    for n, p in m.named_parameters():
        d = p.detach().double()
        out[n] = {"sum": float(d.sum()), "sumsq": float((d * d).sum()),
                  "head": [float(v) for v in p.detach().reshape(-1)[:16]]}
    return out


def _run(cfg, batches, steps, grad_accum, lr, max_norm, sched=None):
    torch.manual_seed(42)
    m = ref_model.GPT2(cfg)
    opt = torch.optim.AdamW(m.parameters(), lr=lr, weight_decay=0.1, betas=(0.9, 0.95), fused=True)
    opt.zero_grad()
    losses, norms, lrs = [], [], []
    it = iter(batches)
    for s in range(steps):
        for _a in range(grad_accum):
            x, y = next(it)
            _, loss = m(x, labels=y)
            loss = loss / grad_accum
            loss.backward()
        gn = torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm)
        if sched is not None:
            opt.param_groups[0]["lr"] = lr_at(s, **sched)
        lrs.append(float(opt.param_groups[0]["lr"]))
        opt.step()
        opt.zero_grad()
        losses.append(loss.item() * grad_accum)
        norms.append(float(gn))
    return losses, norms, lrs, m


def tiny_clip_traj(steps=12, grad_accum=2, batch=2, lr=1e-3, max_norm=1.0):
    cfg = ref_model.GPT2Config(**TINY)
    rng = np.random.default_rng(99)
    toks = (np.minimum(rng.zipf(1.2, size=(steps * grad_accum, batch, 65)), cfg.vocab_size) - 1).astype(np.int64)
    batches = [(torch.from_numpy(t[:, :-1].copy()), torch.from_numpy(t[:, 1:].copy())) for t in toks]
    sched = dict(lr=lr, warmup_steps=3, decay_steps=10, min_lr=lr / 10, kind="cosine")
    losses, norms, lrs, m = _run(cfg, batches, steps, grad_accum, lr, max_norm, sched)
    losses_off, norms_off, _, _ = _run(cfg, batches, steps, grad_accum, lr, float("inf"), sched)
    sep = [abs(a - b) / b for a, b in zip(losses, losses_off)]
    # steps are counted as lr_at counts them (the optimizer steps already taken): step 3 is the fourth. The third
    # (step 2) still sits in the warmup, two small updates after the identical start, and differs by 7e-4 only
    assert min(sep[3:]) >= 10 * LOSS_TOL, f"clipping does not separate the trajectories from step 3 on: {sep}"
    assert sum(n > max_norm for n in norms) >= 2, norms
    with open(os.path.join(HERE, "tiny_clip_traj.json"), "w") as f:
        json.dump({"config": TINY, "data": "np.random.default_rng(99).zipf(1.2, (24,2,65)) clipped; micro-batch i = "
                   "row i; stored in 'tokens'", "tokens": toks.tolist(), "batch": batch, "seq_len": 64,
                   "grad_accum": grad_accum, "steps": steps, "lr": lr, "max_grad_norm": max_norm, "schedule": sched,
                   "losses": losses, "grad_norms": norms, "lrs": lrs, "params": _param_checks(m),
                   "losses_unclipped": losses_off, "grad_norms_unclipped": norms_off}, f, indent=0)
    print("tiny_clip_traj norms", norms, "\n  separation", sep)


def _ddp_separation(clip, off, lr):
    """The largest distance between the two runs in units of the test's gate, per gated field."""
    loss = max(abs(a - b) / b for a, b in zip(clip[0], off[0])) / LOSS_TOL
    head = 0.0
    pc, po = _param_checks(clip[3]), _param_checks(off[3])
    for n in pc:
        a, b = np.array(pc[n]["head"]), np.array(po[n]["head"])
        head = max(head, float((np.abs(a - b) / (1e-2 * lr + PAR_RTOL * np.abs(b))).max()))
    return {"loss": loss, "param_head": head}


def clip_ddp_golden(grad_accum=2, world=2, per_rank=2, lr=1e-3, max_norm=1.2):
    cfg = ref_model.GPT2Config(**DDPCFG)
    for steps in range(3, 9):
        # ddp_golden.json's rows: the generator fills step by step, so steps 0..2 are its data at any step count
        g = torch.Generator().manual_seed(5)
        toks = torch.randint(0, 509, (3, grad_accum, world * per_rank, 65), generator=g)
        if steps > 3:
            toks = torch.cat([toks, torch.randint(0, 509, (steps - 3, grad_accum, world * per_rank, 65), generator=g)])
        batches = [(toks[s, a, :, :-1].contiguous(), toks[s, a, :, 1:].contiguous())
                   for s in range(steps) for a in range(grad_accum)]
        clip = _run(cfg, batches, steps, grad_accum, lr, max_norm)
        off = _run(cfg, batches, steps, grad_accum, lr, float("inf"))
        sep = _ddp_separation(clip, off, lr)
        print("clip_ddp_golden", steps, "steps: separation / gate", sep, "norms", clip[1])
        if max(sep.values()) >= 10:
            break
    else:
        raise AssertionError(f"the clipped run is not 10x the gate away from the unclipped one after 8 steps: {sep}")
    assert any(n > max_norm for n in clip[1]) and any(n < max_norm for n in clip[1]), clip[1]
    with open(os.path.join(HERE, "clip_ddp_golden.json"), "w") as f:
        json.dump({"config": DDPCFG, "world": world, "per_rank": per_rank, "grad_accum": grad_accum, "steps": steps,
                   "lr": lr, "max_grad_norm": max_norm,
                   "data": "ddp_golden.json's rows (torch.randint(0,509,(3,grad_accum,world*per_rank,65)), Generator "
                           "seed 5; further steps drawn after them); stored in 'tokens'; rank r takes rows "
                           "r*per_rank..", "tokens": toks.tolist(), "losses": clip[0], "grad_norms": clip[1],
                   "params": _param_checks(clip[3]), "losses_unclipped": off[0],
                   "params_unclipped_head": {n: v["head"] for n, v in _param_checks(off[3]).items()},
                   "separation_over_gate": sep}, f, indent=0)


if __name__ == "__main__":
    tiny_clip_traj()
    clip_ddp_golden()
