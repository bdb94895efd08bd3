"""What the forward-only evaluation path costs against the parent's way of getting a loss without a backward, on one
MI355X, in ONE process:

  model   ms per batch and peak memory above the weights of
            parent  model.eval() + torch.no_grad() + model(idx, labels): the training workspace, bf16 logits in HBM, the
                    cross-entropy kernel over them;
            score   model.score(idx, labels): the evaluation workspace and the fused lm_head + cross-entropy kernel,
          at GPT-2 124M and at the GPT-2 1.5B widths (C = 1600, 25 heads; --layers_15b blocks, not all 48: the head and
          the per-block cost are what differ, and the memory figures are reported per arm with the depth beside them).
  head    the head alone at M = 8192 and M = 65536 rows, C = 768 and C = 1600: gpt2mi_gemm (EPI_BF16, [M, Vp] logits)
          + gpt2mi_xent_fwd with dlogits = NULL, against gpt2mi_lm_loss; and, to say where the difference comes from,
          the pair's two kernels alone and the same GEMM forced onto the 128x128 kernel whose main loop gpt2mi_lm_loss
          shares (sched low byte 1).

Timing: device events around --iters (>= 20) launches after a warm-up of each arm; the product path (score / lm_loss) is
timed first and last with the parent between, and both of its figures are recorded. Peak memory: the rise of
torch.cuda.max_memory_allocated over the allocation with only the model and its engine resident. Records what the
device gives and sets no threshold. The algorithmic counts beside the head figures are computed from the shapes:
2 M Vp C flops; the parent pair writes and re-reads M Vp bf16 logits that the fused kernel never forms.

    python tools/eval_bench.py --out profiles/eval/eval_bench.json
"""
import argparse
import json
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py and the trainer set it (gpt_2_distributed_amd/__init__.py)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_2_distributed_amd import _lib as K  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

V, VP = 50257, 50432


def timed(fn, iters):
    """Milliseconds per call: device events around `iters` calls."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def head_case(M, C, iters):
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g).bfloat16().cuda()
    w = (0.02 * torch.randn(VP, C, generator=g)).bfloat16().cuda()
    w[V:] = 0
    labels = torch.randint(0, V, (M,), generator=g).cuda()
    rows, lse = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    s, n, mean = (torch.empty(1, device="cuda") for _ in range(3))
    ws = torch.empty(K.lm_loss_workspace(M, V), device="cuda")
    prow, plse, ploss, pinv = torch.empty(M, device="cuda"), torch.empty(M, device="cuda"), \
        torch.empty((), device="cuda"), torch.empty(1, device="cuda")

    def fused():
        K.lm_loss(x, C, w, C, VP, labels, M, V, C, rows, lse, ws, loss_sum=s, count=n, loss_mean=mean)

    def parent():
        logits = torch.empty(M, VP, dtype=torch.bfloat16, device="cuda")  # fresh per forward, as Engine._forward
        K.gemm(K.FWD, K.EPI_BF16, M, VP, C, x, C, w, C, logits, VP)
        K.xent_fwd(logits, VP, labels, prow, plse, None, VP, M, V, ploss, pinv)

    logits = torch.empty(M, VP, dtype=torch.bfloat16, device="cuda")
    parts = {"gemm_planner_ms": lambda: K.gemm(K.FWD, K.EPI_BF16, M, VP, C, x, C, w, C, logits, VP),
             "gemm_128x128_ms": lambda: K.gemm(K.FWD, K.EPI_BF16, M, VP, C, x, C, w, C, logits, VP, sched=1),
             "xent_fwd_ms": lambda: K.xent_fwd(logits, VP, labels, prow, plse, None, VP, M, V, ploss, pinv)}

    fused(), parent()  # warm-up
    torch.cuda.synchronize()
    diff = abs(mean.item() - ploss.item())
    first, par = timed(fused, iters), timed(parent, iters)
    alone = {}
    for k, fn in parts.items():
        fn()
        alone[k] = timed(fn, iters)
    last = timed(fused, iters)
    del x, w, logits
    return {"M": M, "C": C, "lm_loss_ms_first": first, "parent_gemm_xent_ms": par, "lm_loss_ms_last": last,
            "ratio_lm_loss_over_parent": min(first, last) / par, **alone, "flops": 2 * M * VP * C,
            "lm_loss_TFLOPs": 2 * M * VP * C / (min(first, last) * 1e-3) / 1e12,
            "parent_logits_bytes": M * VP * 2, "lm_loss_workspace_bytes": ws.numel() * 4,
            "mean_loss_abs_diff": diff}


def model_case(name, dims, B, T, iters):
    cfg = GPT2Config(n_positions=T, **dims)
    model = GPT2(cfg).to("cuda:0")
    eng = model.engine()
    tok = torch.randint(0, V, (B, T + 1), generator=torch.Generator().manual_seed(1)).cuda()
    x, y = tok[:, :-1].contiguous(), tok[:, 1:].contiguous()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()

    def score():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return model.score(x, y)

    def parent():
        with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
            return model(x, labels=y)[1]

    torch.cuda.reset_peak_memory_stats()
    a = score().item()
    mem_score = torch.cuda.max_memory_allocated() - base
    first = timed(score, iters)
    eng._eval_ws.clear()  # the parent arm's memory is measured without the evaluation workspace
    model.eval()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    b = parent().item()
    mem_parent = torch.cuda.max_memory_allocated() - base
    par = timed(parent, iters)
    model.train()
    score()
    last = timed(score, iters)
    res = {"model": name, "n_layer": cfg.n_layer, "n_embd": cfg.n_embd, "B": B, "T": T,
           "score_ms_first": first, "parent_nograd_forward_ms": par, "score_ms_last": last,
           "score_peak_bytes_above_weights": mem_score, "parent_peak_bytes_above_weights": mem_parent,
           "eval_workspace_bytes": eng.eval_workspace_bytes(B, T), "loss_score": a, "loss_parent": b}
    del model, eng
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window (>= 20)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq_len", type=int, default=1024)
    ap.add_argument("--layers_15b", type=int, default=6, help="blocks of the 1.5B-width model (the full model has 48)")
    ap.add_argument("--out", default="profiles/eval/eval_bench.json")
    a = ap.parse_args()
    if a.iters < 20:
        raise SystemExit("--iters must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "head": [], "model": []}
    for C in (768, 1600):
        for M in (8192, 65536):
            res["head"].append(head_case(M, C, a.iters))
            print(json.dumps(res["head"][-1]), flush=True)
    for name, dims in (("124M", dict(MODEL_SIZES["124M"])),
                       ("1.5B-width", dict(MODEL_SIZES["1.5B"], n_layer=a.layers_15b))):
        res["model"].append(model_case(name, dims, a.batch, a.seq_len, a.iters))
        print(json.dumps(res["model"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
