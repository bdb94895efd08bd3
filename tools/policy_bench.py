"""What the policy-gradient head costs beside the cross entropy it stands in for, on one MI355X.

Two pairs, each run in ONE process, interleaved round by round after a warm-up round of each arm (tools/README.md,
"A/B harnesses"); the median round is reported with every round's figure beside it:
  kernel  gpt2mi_xent_fwd against gpt2mi_policy_fwd with every option on (old and reference log-probabilities,
          asymmetric clip, KL and entropy coefficients, every per-row output and the metrics) over the same bf16 logits
          [M = 65536, V = 50257] (GPT-2 124M's head at B = 64, T = 1024): xent_row_kernel + xent_finalize_kernel against
          policy_row_kernel + policy_finalize_kernel. Both read the logits once and write dlogits once.
  step    forward(idx, labels) + backward against policy_loss(...) + backward, GPT-2 124M, bf16 autocast.
Each time is a host clock around --steps calls ending in a device synchronise. Both kernels move the same bytes, so the
expectation is parity; this tool records the ratio and sets no threshold. The bytes a call needs (logits read + dlogits
written) over the kernel time is given as an achieved rate. Writes one JSON file.

    python tools/policy_bench.py --out profiles/policy/policy_bench.json
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
from gpt_2_distributed_amd import _lib as K  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

OPTS = dict(clip_low=0.2, clip_high=0.28, kl_coef=0.04, entropy_coef=0.01)


def window(fn, steps, limit):
    """Microseconds per call over one window of `steps` calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dt > limit:
        raise SystemExit(f"policy_bench: a window of {steps} calls took {dt:.1f} s (limit {limit} s)")
    return dt / steps * 1e6


def interleaved(arms, steps, rounds, limit):
    us = {k: [] for k in arms}
    for r in range(rounds + 1):  # round 0 warms the arms up
        for k, fn in arms.items():
            t = window(fn, steps, limit)
            if r:
                us[k].append(t)
    return us


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--kernel_steps", type=int, default=100, help="head calls per timed window")
    ap.add_argument("--steps", type=int, default=8, help="forward + backward steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=30.0, help="seconds one window may take")
    ap.add_argument("--out", default="profiles/policy/policy_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    dev = "cuda:0"
    cfg = GPT2Config(**dict(MODEL_SIZES[a.model], n_positions=a.seq_len))
    model = GPT2(cfg).to(dev)
    B, T, V = a.batch, a.seq_len, cfg.vocab_size
    M, Vp = B * T, model.engine().vpad
    g = torch.Generator(device=dev).manual_seed(0)
    f32 = dict(dtype=torch.float32, device=dev)

    # ---- the head kernels alone ----
    logits = torch.empty(M, Vp, dtype=torch.bfloat16, device=dev).normal_(0, 3, generator=g)
    dlogits = torch.empty_like(logits)
    labels = torch.randint(0, V, (M,), device=dev, generator=g)
    adv = torch.randn(M, generator=g, **f32)
    rows, lse, loss, inv = torch.empty(6, M, **f32), torch.empty(M, **f32), torch.empty(1, **f32), torch.empty(1, **f32)
    metrics = torch.empty(4, **f32)
    K.xent_fwd(logits, Vp, labels, rows[0], lse, None, Vp, M, V, loss, inv)
    old = -rows[0] + 0.2 * torch.randn(M, generator=g, **f32)  # log p[label] of these logits, moved: ratios around 1
    ref = -rows[0] + 0.2 * torch.randn(M, generator=g, **f32)
    arms = {"xent": lambda: K.xent_fwd(logits, Vp, labels, rows[0], lse, dlogits, Vp, M, V, loss, inv),
            "policy": lambda: K.policy_fwd(logits, Vp, labels, adv, old, ref, OPTS["clip_low"], OPTS["clip_high"],
                                           OPTS["kl_coef"], OPTS["entropy_coef"], *rows, dlogits, Vp, M, V, loss, inv,
                                           metrics)}
    k_us = interleaved(arms, a.kernel_steps, a.rounds, a.limit)
    clip_fraction = float(metrics[1])
    del logits, dlogits
    torch.cuda.empty_cache()

    # ---- the whole step ----
    tok = torch.randint(0, V, (B, T + 1), device=dev, generator=g)
    idx, lab = tok[:, :-1], tok[:, 1:].contiguous()
    adv2 = adv.view(B, T)
    with torch.no_grad():
        lp = -model.score(idx, lab, reduction="none")
    old2, ref2 = lp + 0.2 * torch.randn(B, T, generator=g, **f32), lp + 0.2 * torch.randn(B, T, generator=g, **f32)

    def plain():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _, l = model(idx, labels=lab)
        l.backward()

    def policy():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model.policy_loss(idx, lab, adv2, old2, ref2, **OPTS)
        out.loss.backward()

    s_us = interleaved({"forward_labels": plain, "policy_loss": policy}, a.steps, a.rounds, a.limit)
    med = {k: statistics.median(v) for k, v in {**k_us, **s_us}.items()}
    head_bytes = 2 * M * Vp * 2  # the bf16 logits read once, the bf16 dlogits written once
    res = {"model": a.model, "batch": B, "seq_len": T, "M": M, "V": V, "ld": Vp, "device": torch.cuda.get_device_name(0),
           "options": OPTS, "rounds": a.rounds, "kernel_calls_per_window": a.kernel_steps, "steps_per_window": a.steps,
           "kernel_us_xent": med["xent"], "kernel_us_policy": med["policy"],
           "kernel_ratio_policy_over_xent": med["policy"] / med["xent"],
           "head_bytes": head_bytes, "xent_TBps": head_bytes / med["xent"] / 1e6,
           "policy_TBps": head_bytes / med["policy"] / 1e6, "kernel_clip_fraction": clip_fraction,
           "step_us_forward_labels": med["forward_labels"], "step_us_policy_loss": med["policy_loss"],
           "step_ratio_policy_over_forward": med["policy_loss"] / med["forward_labels"],
           "rounds_us": {**k_us, **s_us}}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
