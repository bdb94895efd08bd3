"""What document masking costs and saves: the attention kernels of one layer with and without bounds, and the whole
training step, GPT-2 124M widths on one MI355X.

Attention arms, at H = 12, T = 1024, B = 16, dropout 0.1, bf16, forward and backward of one layer timed with device
events, all in ONE process, alternating round by round after a warm-up round of every arm (tools/README.md, "A/B
harnesses"); the median round is reported with every round's figure beside it:
  a  the unmasked entries (gpt2mi_attn_fwd / gpt2mi_attn_bwd): the yardstick
  b  the _doc entries with one document per row: the same work through the masked instantiations
  c  the _doc entries, seeded random documents of mean 256 tokens
  d  the _doc entries, seeded random documents of mean 64 tokens
For each arm the algorithmic FLOPs are counted from the bounds (visible pairs = sum over t of t - start[t] + 1; the
forward is 2 matmuls of 2 * 64 FLOPs per pair and head, the backward 5) and the achieved rate is recorded beside the
time. Then the training step of bench.py's shape (B = 64, T = 1024, bf16 autocast, forward + backward + AdamW), with
plain causal attention and with bounds of mean 256, timed by a host clock around windows that end in a synchronise.
The tool records what the device gives and sets no threshold. Writes one JSON file.

    python tools/docmask_bench.py --out profiles/docmask/docmask_bench.json
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
from gpt_2_distributed_amd.packing import DocBounds  # noqa: E402

D = 64


def random_bounds(B, T, mean, seed):
    """DocBounds (CPU) of B rows of seeded random document lengths (1 + exponential, mean about `mean`); mean None: one
    document per row."""
    start = torch.zeros(B, T, dtype=torch.int32)
    end = torch.full((B, T), T, dtype=torch.int32)
    if mean is None:
        return DocBounds(start, end)
    g = torch.Generator().manual_seed(seed)
    for b in range(B):
        s = 0
        while s < T:
            n = min(int(torch.empty(1).exponential_(1.0 / mean, generator=g).item()) + 1, T - s)
            start[b, s:s + n] = s
            end[b, s:s + n] = s + n
            s += n
    return DocBounds(start, end)


def visible_pairs(bounds):
    T = bounds.start.shape[1]
    return int((torch.arange(T)[None, :] - bounds.start.long() + 1).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--p_drop", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step_batch", type=int, default=64)
    ap.add_argument("--step_iters", type=int, default=4, help="training steps per timed window (0: skip the step arms)")
    ap.add_argument("--step_rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/docmask/docmask_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("docmask_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    dev = "cuda:0"
    B, T, H, p = a.batch, a.seq_len, a.heads, a.p_drop
    C = H * D
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * T, 3 * C, generator=g).bfloat16().to(dev)
    dout = torch.randn(B * T, C, generator=g).bfloat16().to(dev)
    out, dqkv = torch.empty(B * T, C, dtype=torch.bfloat16, device=dev), torch.empty_like(qkv)
    lse, delta = torch.empty(B * H, T, device=dev), torch.empty(B * H, T, device=dev)
    cpu_bounds = {"a": None, "b": random_bounds(B, T, None, 0), "c": random_bounds(B, T, 256, 1),
                  "d": random_bounds(B, T, 64, 2)}
    bounds = {k: None if v is None else DocBounds(v.start.to(dev), v.end.to(dev)) for k, v in cpu_bounds.items()}
    causal_pairs = B * T * (T + 1) // 2
    pairs = {k: causal_pairs if v is None else visible_pairs(v) for k, v in cpu_bounds.items()}

    def fwd(doc):
        K.attn_fwd(qkv, out, lse, B, T, H, D, p, 7, doc=doc)

    def bwd(doc):
        K.attn_bwd(qkv, out, dout, lse, delta, dqkv, B, T, H, D, p, 7, doc=doc)

    def window(fn, doc):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(doc)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters  # microseconds per launch

    us = {k: {"fwd": [], "bwd": []} for k in bounds}
    for r in range(a.rounds + 1):  # round 0 warms every arm up
        for k, doc in bounds.items():
            fwd(doc)  # the backward of this arm reads this arm's out / lse
            for name, fn in (("fwd", fwd), ("bwd", bwd)):
                t = window(fn, doc)
                if r:
                    us[k][name].append(t)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "seq_len": T, "heads": H, "p_drop": p, "iters": a.iters,
           "rounds": a.rounds, "arms": {}}
    for k in bounds:
        arm = {"visible_pairs": pairs[k], "share_of_causal_pairs": pairs[k] / causal_pairs}
        for name, mm in (("fwd", 2), ("bwd", 5)):
            med = statistics.median(us[k][name])
            flops = mm * 2 * D * pairs[k] * H
            arm[name] = {"us": med, "rounds_us": us[k][name], "spread_us": max(us[k][name]) - min(us[k][name]),
                         "flops": flops, "tflops": flops / med / 1e6}
        res["arms"][k] = arm
    ref = res["arms"]["a"]
    res["b_minus_a_us"] = {n: res["arms"]["b"][n]["us"] - ref[n]["us"] for n in ("fwd", "bwd")}
    res["d_faster_than_a"] = {n: res["arms"]["d"][n]["us"] < ref[n]["us"] for n in ("fwd", "bwd")}
    print(json.dumps(res), flush=True)

    if a.step_iters:
        del qkv, dout, out, dqkv
        SB = a.step_batch
        cfg = GPT2Config(**dict(MODEL_SIZES["124M"], n_positions=T))
        model = GPT2(cfg).to(dev)
        opt = model.configure_optimizers(learning_rate=1e-4)
        tok = torch.randint(0, cfg.vocab_size, (SB, T + 1), generator=torch.Generator().manual_seed(0)).to(dev)
        sb = random_bounds(SB, T, 256, 3)
        step_bounds = {"causal": None, "docs_mean_256": DocBounds(sb.start.to(dev), sb.end.to(dev))}

        def step_window(doc):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.step_iters):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    if doc is None:
                        _, loss = model(tok[:, :-1], labels=tok[:, 1:])
                    else:
                        _, loss = model(tok[:, :-1], labels=tok[:, 1:], doc_bounds=doc)
                loss.backward()
                opt.step()
                opt.zero_grad()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.step_iters * 1e3

        ms = {k: [] for k in step_bounds}
        for r in range(a.step_rounds + 1):
            for k, doc in step_bounds.items():
                t = step_window(doc)
                if r:
                    ms[k].append(t)
        res["step"] = {"batch": SB, "seq_len": T, "model": "124M", "steps_per_window": a.step_iters,
                       "share_of_causal_pairs": visible_pairs(sb) / (SB * T * (T + 1) // 2),
                       **{k: {"ms": statistics.median(v), "rounds_ms": v} for k, v in ms.items()}}
        print(json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
