"""What global-norm clipping adds to the optimizer step: FusedAdamW.step() with max_grad_norm=None against 1.0,
GPT-2 124M on one MI355X.

One forward + backward at the bench shape (B=64, T=1024, bf16 autocast) fills the gradient arena; then two optimizers
over the same model and the same gradients are stepped in ONE process, interleaved round by round after a warm-up
round of each (tools/README.md, "A/B harnesses"):
  off      max_grad_norm=None: one gpt2mi_adamw launch (the sum of squares folded in) + the norm finalisation.
  clipped  max_grad_norm=1.0: gpt2mi_sumsq_partials over the arena, gpt2mi_clip_coef, one gpt2mi_adamw_clipped launch.
Each arm's time is a host clock around --steps steps ending in a device synchronise; the median round is reported with
every round's figure beside it. A window that takes longer than --limit seconds ends the run with an error.

What the difference is set against: the extra pass reads the fp32 gradient arena once (4 bytes per parameter), at the
6.29 TB/s a device-to-device copy reaches on this chip (MI355X_MICROARCH.md), plus two small launches. That figure is
a derivation; this tool records what the device gives and sets no threshold. Writes one JSON file.

    python tools/clip_bench.py --out profiles/clip/clip_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py and the trainer set it (gpt_2_distributed_amd/__init__.py)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s, measured device-to-device copy rate (MI355X_MICROARCH.md)


def window(opt, steps, limit):
    """Microseconds per step() over one window of `steps` steps."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dt > limit:
        raise SystemExit(f"clip_bench: a window of {steps} steps took {dt:.1f} s (limit {limit} s)")
    return dt / steps * 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=300, help="optimizer steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=30.0, help="seconds one window may take")
    ap.add_argument("--max_grad_norm", type=float, default=1.0)
    ap.add_argument("--out", default="profiles/clip/clip_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**dict(MODEL_SIZES[a.model], n_positions=a.seq_len))
    model = GPT2(cfg).to("cuda:0")
    arms = {"off": model.configure_optimizers(learning_rate=1e-4),
            "clipped": model.configure_optimizers(learning_rate=1e-4, max_grad_norm=a.max_grad_norm)}
    tok = torch.randint(0, cfg.vocab_size, (a.batch, a.seq_len + 1), generator=torch.Generator().manual_seed(0)).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, loss = model(tok[:, :-1], labels=tok[:, 1:])
    loss.backward()
    us = {k: [] for k in arms}
    for r in range(a.rounds + 1):  # round 0 warms the arms up
        for k, opt in arms.items():
            t = window(opt, a.steps, a.limit)
            if r:
                us[k].append(t)
    n = model.arena.numel()
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {"model": a.model, "batch": a.batch, "seq_len": a.seq_len, "steps_per_window": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "max_grad_norm": a.max_grad_norm, "arena_elements": n,
           "grad_norm": float(arms["clipped"].grad_norm), "clip_coef": float(arms["clipped"].clip_coef),
           "step_us_off": med["off"], "step_us_clipped": med["clipped"], "added_us": med["clipped"] - med["off"],
           "rounds_us_off": us["off"], "rounds_us_clipped": us["clipped"],
           "extra_read_bytes": 4 * n, "copy_rate_TBps": COPY_RATE / 1e12, "derived_extra_read_us": 4 * n / COPY_RATE * 1e6}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
