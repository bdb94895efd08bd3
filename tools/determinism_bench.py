"""What the deterministic mode costs: each ordered kernel against the float-atomic one it replaces, and the whole
training step with ``model.deterministic`` off and on, GPT-2 124M widths on one MI355X.

Kernel arms at B = 64, T = 1024, C = 768, dropout 0.1, timed with device events, all in ONE process, alternating round
by round after a warm-up round of every arm (tools/README.md, "A/B harnesses"); the median round is reported with every
round's figure and the spread beside it:
  embed_bwd          gpt2mi_embed_bwd against gpt2mi_embed_bwd_det, uniform tokens and a Zipf draw (exponent 1.2: the
                     head token fills about a fifth of the rows)
  layernorm_bwd      gpt2mi_layernorm_bwd against gpt2mi_layernorm_bwd_det, with the emitted branch and its bias sum
  colsum_qkv         gpt2mi_colsum_f32 against gpt2mi_colsum_det_f32 over the attention backward's [M/32, 3C] partials
  colsum_dU          gpt2mi_colsum_det_bf16 over dU [M, 4C]: the fc1 bias gradient, which the default mode forms inside
                     the fc2 dgrad epilogue (no launch of its own; gpt2mi_colsum_bf16 over the same matrix is timed
                     beside it as the unfused yardstick)
Then the training step of bench.py's shape (B = 64, T = 1024, bf16 autocast, dropout 0.1, forward + backward + AdamW)
on two models of the same initialisation, one with the flag, timed by a host clock around windows that end in a
synchronise, the two arms alternating. The tool records what the device gives and sets no threshold. One JSON file.

    python tools/determinism_bench.py --out profiles/determinism/determinism_bench.json
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--p_drop", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=10, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step_iters", type=int, default=4, help="training steps per timed window (0: skip the step arms)")
    ap.add_argument("--step_rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/determinism/determinism_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("determinism_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    dev = "cuda:0"
    B, T, C, p, V = a.batch, a.seq_len, a.width, a.p_drop, 50257
    M = B * T
    g = torch.Generator().manual_seed(0)
    ws = torch.empty(K.det_workspace_bytes(B, T, C, 4 * C), dtype=torch.uint8, device=dev)
    zipf = torch.multinomial(1.0 / torch.arange(1, V + 1).double() ** 1.2, M, replacement=True, generator=g)
    tokens = {"uniform": torch.randint(0, V, (B, T), generator=g).to(dev), "zipf": zipf.view(B, T).to(dev)}
    dres = torch.randn(M, C, generator=g).to(dev)
    dwte, dwpe = torch.zeros(V, C, device=dev), torch.zeros(T, C, device=dev)
    x, w = torch.randn(M, C, generator=g).to(dev), torch.ones(C, device=dev)
    mean, rstd = x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + 1e-5)
    dy, out = torch.randn(M, C, generator=g).to(dev).bfloat16(), torch.empty(M, C, dtype=torch.bfloat16, device=dev)
    dw, db, dbo = (torch.zeros(C, device=dev) for _ in range(3))
    cs = torch.randn(M // 32, 3 * C, generator=g).to(dev)
    dU = torch.randn(M, 4 * C, generator=g).to(dev).bfloat16()
    b3, b4 = torch.zeros(3 * C, device=dev), torch.zeros(4 * C, device=dev)
    ln = (x, w, mean, rstd, dy, dres, dw, db, out, dbo, M, C, p, 7)
    # name -> {arm: launch}
    kernels = {
        **{f"embed_bwd_{k}": {"atomic": lambda i=i: K.embed_bwd(i, dres, dwte, dwpe, B, T, C, p, 7),
                              "det": lambda i=i: K.embed_bwd_det(i, dres, dwte, dwpe, B, T, C, p, 7, workspace=ws)}
           for k, i in tokens.items()},
        "layernorm_bwd": {"atomic": lambda: K.layernorm_bwd(*ln), "det": lambda: K.layernorm_bwd_det(*ln, workspace=ws)},
        "colsum_qkv": {"atomic": lambda: K.colsum_bf16(cs, b3, M // 32, 3 * C, 3 * C),
                       "det": lambda: K.colsum_det(cs, b3, M // 32, 3 * C, 3 * C, ws)},
        "colsum_dU": {"atomic": lambda: K.colsum_bf16(dU, b4, M, 4 * C, 4 * C),
                      "det": lambda: K.colsum_det(dU, b4, M, 4 * C, 4 * C, ws)},
    }

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters  # microseconds per call (every launch of the entry)

    us = {k: {arm: [] for arm in arms} for k, arms in kernels.items()}
    for r in range(a.rounds + 1):  # round 0 warms every arm up
        for k, arms in kernels.items():
            for arm, fn in arms.items():
                t = window(fn)
                if r:
                    us[k][arm].append(t)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "seq_len": T, "width": C, "p_drop": p, "iters": a.iters,
           "rounds": a.rounds, "kernels": {}}
    for k, arms in us.items():
        res["kernels"][k] = {arm: {"us": statistics.median(v), "rounds_us": v, "spread_us": max(v) - min(v)}
                             for arm, v in arms.items()}
        res["kernels"][k]["det_over_atomic"] = res["kernels"][k]["det"]["us"] / res["kernels"][k]["atomic"]["us"]
    res["kernels"]["colsum_dU"]["note"] = ("the default step forms this sum in the fc2 dgrad epilogue without a launch: "
                                           "the det figure is the mode's added time per layer")
    print(json.dumps(res), flush=True)

    if a.step_iters:
        del dres, dwte, x, dy, out, dU, cs
        cfg = GPT2Config(**dict(MODEL_SIZES["124M"], n_positions=T, resid_pdrop=p, attn_pdrop=p))
        tok = torch.randint(0, cfg.vocab_size, (B, T + 1), generator=torch.Generator().manual_seed(0)).to(dev)
        arms = {}
        for name, flag in (("default", False), ("deterministic", True)):
            model = GPT2(cfg).to(dev).train()
            model.deterministic = flag
            arms[name] = (model, model.configure_optimizers(learning_rate=1e-4))

        def step_window(model, opt):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.step_iters):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    _, loss = model(tok[:, :-1], labels=tok[:, 1:])
                loss.backward()
                opt.step()
                opt.zero_grad()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.step_iters * 1e3, float(loss.detach())

        ms, last = {k: [] for k in arms}, {}
        for r in range(a.step_rounds + 1):
            for k, (model, opt) in arms.items():
                t, last[k] = step_window(model, opt)
                if r:
                    ms[k].append(t)
        res["step"] = {"batch": B, "seq_len": T, "model": "124M", "p_drop": p, "steps_per_window": a.step_iters,
                       **{k: {"ms": statistics.median(v), "rounds_ms": v, "spread_ms": max(v) - min(v),
                              "last_loss": last[k]} for k, v in ms.items()}}
        res["step"]["deterministic_over_default"] = res["step"]["deterministic"]["ms"] / res["step"]["default"]["ms"]
        print(json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
