"""What positions per document cost: the embedding kernels with and without the restart, and the whole training step
with bounds, with and without ``reset_positions``, GPT-2 124M widths on one MI355X.

Kernel arms at B = 64, T = 1024, C = 768, dropout 0.1, timed with device events, all in ONE process, alternating round
by round after a warm-up round of every arm (tools/README.md, "A/B harnesses"); the median round is reported with every
round's figure and the spread beside it:
  plain      gpt2mi_embed_fwd / gpt2mi_embed_bwd: the yardstick, the path a step without the keyword takes
  one        the _doc entries, one document per row (the same sums through the new kernels)
  mean_256   the _doc entries, seeded random documents of mean 256 tokens
  mean_64    the _doc entries, seeded random documents of mean 64 tokens
  all_ones   the _doc entries, every token a document of its own: B x T addends on dwpe[0], the worst case
Then the training step of bench.py's shape (B = 64, T = 1024, bf16 autocast, forward + backward + AdamW) with bounds of
mean 256, without and with reset_positions, timed by a host clock around windows that end in a synchronise.
The tool records what the device gives and sets no threshold. Writes one JSON file.

    python tools/docpos_bench.py --out profiles/docmask/docpos_bench.json
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
from tools.docmask_bench import random_bounds  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--p_drop", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=10, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step_iters", type=int, default=4, help="training steps per timed window (0: skip the step arms)")
    ap.add_argument("--step_rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/docmask/docpos_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("docpos_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    dev = "cuda:0"
    B, T, C, p, V = a.batch, a.seq_len, a.width, a.p_drop, 50257
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, V, (B, T), generator=g).to(dev)
    wte, wpe = torch.randn(V, C, generator=g).to(dev), torch.randn(T, C, generator=g).to(dev)
    dres = torch.randn(B * T, C, generator=g).to(dev)
    x = torch.empty(B * T, C, device=dev)
    dwte, dwpe = torch.zeros(V, C, device=dev), torch.zeros(T, C, device=dev)
    ones = torch.arange(T, dtype=torch.int32).expand(B, T).contiguous()
    starts = {"plain": None, "one": random_bounds(B, T, None, 0).start, "mean_256": random_bounds(B, T, 256, 1).start,
              "mean_64": random_bounds(B, T, 64, 2).start, "all_ones": ones}
    docs = {k: None if v is None else int((v == torch.arange(T)[None]).sum()) for k, v in starts.items()}
    starts = {k: None if v is None else v.to(dev) for k, v in starts.items()}

    def fwd(start):
        if start is None:
            K.embed_fwd(idx, wte, wpe, x, B, T, C, p, 7)
        else:
            K.embed_fwd_doc(idx, wte, wpe, x, start, B, T, C, p, 7)

    def bwd(start):
        if start is None:
            K.embed_bwd(idx, dres, dwte, dwpe, B, T, C, p, 7)
        else:
            K.embed_bwd_doc(idx, dres, dwte, dwpe, start, B, T, C, p, 7)

    def window(fn, start):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(start)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters  # microseconds per launch

    us = {k: {"fwd": [], "bwd": []} for k in starts}
    for r in range(a.rounds + 1):  # round 0 warms every arm up
        for k, start in starts.items():
            for name, fn in (("fwd", fwd), ("bwd", bwd)):
                t = window(fn, start)
                if r:
                    us[k][name].append(t)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "seq_len": T, "width": C, "p_drop": p, "iters": a.iters,
           "rounds": a.rounds, "arms": {}}
    for k in starts:
        arm = {"documents": docs[k]}
        for name in ("fwd", "bwd"):
            arm[name] = {"us": statistics.median(us[k][name]), "rounds_us": us[k][name],
                         "spread_us": max(us[k][name]) - min(us[k][name])}
        res["arms"][k] = arm
    ref = res["arms"]["plain"]
    res["minus_plain_us"] = {k: {n: res["arms"][k][n]["us"] - ref[n]["us"] for n in ("fwd", "bwd")}
                             for k in starts if k != "plain"}
    print(json.dumps(res), flush=True)

    if a.step_iters:
        del wte, dwte, dres, x
        cfg = GPT2Config(**dict(MODEL_SIZES["124M"], n_positions=T))
        model = GPT2(cfg).to(dev)
        opt = model.configure_optimizers(learning_rate=1e-4)
        tok = torch.randint(0, cfg.vocab_size, (B, T + 1), generator=torch.Generator().manual_seed(0)).to(dev)
        sb = random_bounds(B, T, 256, 3)
        doc = DocBounds(sb.start.to(dev), sb.end.to(dev))
        arms = {"bounds_only": {}, "reset_positions": {"reset_positions": True}}

        def step_window(kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.step_iters):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    _, loss = model(tok[:, :-1], labels=tok[:, 1:], doc_bounds=doc, **kw)
                loss.backward()
                opt.step()
                opt.zero_grad()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.step_iters * 1e3

        ms = {k: [] for k in arms}
        for r in range(a.step_rounds + 1):
            for k, kw in arms.items():
                t = step_window(kw)
                if r:
                    ms[k].append(t)
        res["step"] = {"batch": B, "seq_len": T, "model": "124M", "steps_per_window": a.step_iters,
                       "bounds": "mean 256", **{k: {"ms": statistics.median(v), "rounds_ms": v} for k, v in ms.items()}}
        res["step"]["reset_over_bounds_only"] = res["step"]["reset_positions"]["ms"] / res["step"]["bounds_only"]["ms"]
        print(json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
