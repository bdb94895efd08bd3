"""What the distillation head costs beside the cross entropy it stands in for, on one MI355X.

One process; every arm is warmed up, then timed with device events around --launches launches, --rounds times, the arms
interleaved round by round (tools/README.md, "A/B harnesses"); the median round is reported with every round beside it:
  kernel  gpt2mi_xent_fwd (the reference arm, timed first and last in every round) against gpt2mi_distill_fwd forward
          and reverse at tau = 1 and tau = 2, over bf16 logits [M = 65536, V = 50257] (GPT-2 124M's head at B = 64,
          T = 1024): xent_row_kernel against distill_row_kernel, each with its finalize kernel. The cross entropy reads
          one [M, Vp] tensor and writes one; the distillation head reads two and writes one, so by bytes it should take
          about 1.5 times as long.
  step    forward(idx, labels) + backward against distill_loss(...) + backward, GPT-2 124M, bf16 autocast, the teacher's
          logits what another forward returned (read in place).
This tool records the ratios and sets no threshold. Writes one JSON file.

    python tools/distill_bench.py --out profiles/distill/distill_bench.json
"""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py and the trainer set it (gpt_2_distributed_amd/__init__.py)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_2_distributed_amd import _lib as K  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

KERNEL_ARMS = [("forward", 1.0), ("reverse", 1.0), ("forward", 2.0), ("reverse", 2.0)]


def window(fn, launches):
    """Microseconds per call: device events around `launches` calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / launches


def interleaved(arms, launches, rounds):
    """arms: (name, fn) pairs in the order they run in every round; round 0 warms them up."""
    us = {}
    for r in range(rounds + 1):
        for name, fn in arms:
            t = window(fn, launches if r else 2)
            if r:
                us.setdefault(name, []).append(t)
    return us


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=20, help="head calls per timed window")
    ap.add_argument("--steps", type=int, default=4, help="forward + backward steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/distill/distill_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    dev = "cuda:0"
    cfg = GPT2Config(**dict(MODEL_SIZES[a.model], n_positions=a.seq_len))
    model = GPT2(cfg).to(dev)
    B, T, V = a.batch, a.seq_len, cfg.vocab_size
    M, Vp = B * T, model.engine().vpad
    g = torch.Generator(device=dev).manual_seed(0)
    f32 = dict(dtype=torch.float32, device=dev)

    # ---- the head kernels alone ----
    logits = torch.empty(M, Vp, dtype=torch.bfloat16, device=dev).normal_(0, 3, generator=g)
    teacher = (logits.float() + 0.5 * torch.randn(M, Vp, generator=g, **f32)).to(torch.bfloat16)
    dlogits = torch.empty_like(logits)
    labels = torch.randint(0, V, (M,), device=dev, generator=g)
    rows, lse, loss, inv = torch.empty(3, M, **f32), torch.empty(M, **f32), torch.empty(1, **f32), torch.empty(1, **f32)
    metrics = torch.empty(2, **f32)

    def xent():
        K.xent_fwd(logits, Vp, labels, rows[0], lse, dlogits, Vp, M, V, loss, inv)

    def distill(kind, tau):
        return lambda: K.distill_fwd(logits, Vp, teacher, Vp, labels, tau, 0.5, 0.5, kind, *rows, dlogits, Vp, M, V,
                                     loss, inv, metrics)

    arms = [("xent_first", xent)] + [(f"distill_{k}_tau{t:g}", distill(k, t)) for k, t in KERNEL_ARMS] + [("xent_last", xent)]
    k_us = interleaved(arms, a.launches, a.rounds)
    del logits, teacher, dlogits
    torch.cuda.empty_cache()

    # ---- the whole step ----
    tok = torch.randint(0, V, (2, B, T + 1), device=dev, generator=g)
    idx, lab = tok[0, :, :-1], tok[0, :, 1:].contiguous()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        t_logits = model(tok[1, :, :-1])[0]  # [B, T, V] over rows of stride Vp: what a teacher's forward returns

    def plain():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _, l = model(idx, labels=lab)
        l.backward()

    def distilled():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model.distill_loss(idx, lab, t_logits, temperature=2.0)
        out.loss.backward()

    s_us = interleaved([("forward_labels", plain), ("distill_loss", distilled)], a.steps, a.rounds)
    med = {k: statistics.median(v) for k, v in {**k_us, **s_us}.items()}
    x_us = 0.5 * (med["xent_first"] + med["xent_last"])
    stream = M * Vp * 2  # one bf16 [M, Vp] tensor read or written once
    res = {"model": a.model, "batch": B, "seq_len": T, "M": M, "V": V, "ld": Vp, "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "kernel_launches_per_window": a.launches, "steps_per_window": a.steps,
           "kernel_us": {k: med[k] for k in k_us}, "kernel_us_xent": x_us,
           "kernel_ratio_over_xent": {k: med[k] / x_us for k in k_us if k.startswith("distill")},
           "expected_ratio_by_bytes": 1.5, "xent_TBps": 2 * stream / x_us / 1e6,
           "distill_TBps": {k: 3 * stream / med[k] / 1e6 for k in k_us if k.startswith("distill")},
           "step_us_forward_labels": med["forward_labels"], "step_us_distill_loss": med["distill_loss"],
           "step_ratio_distill_over_forward": med["distill_loss"] / med["forward_labels"],
           "rounds_us": {**k_us, **s_us}}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
