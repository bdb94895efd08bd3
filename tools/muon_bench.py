"""Muon at the 124M widths, one process, arms interleaved, median of 3 rounds after a warm-up:
(a) Muon.step()  (b) FusedAdamW.step()  (c) the 15-launch Newton-Schulz chain alone  (d) the same chain over the same
72 matrices through torch.matmul in bf16. Writes profiles/muon/muon_bench.json."""
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402
from gpt_2_distributed_amd.muon import NS_COEFFS  # noqa: E402

PEAK_BF16 = 2.5166e15  # the dense bf16 peak the trainer's MFU uses (train_gpt2_distributed.py)
ITERS = 10


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / ITERS  # us


def main():
    cfg = GPT2Config(**MODEL_SIZES["124M"], n_positions=128)
    m = GPT2(cfg).to("cuda")
    idx = torch.randint(0, cfg.vocab_size, (2, 128), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, loss = m(idx, labels=idx)
    loss.backward()
    muon, adamw = m.fused_muon(lr=1e-4, adamw_lr=1e-6), m.configure_optimizers(learning_rate=1e-6)
    muon.step()  # leaves a normalised X0 in muon.x[0]
    rows = muon.tables["mats"].cpu().tolist()
    xs = [muon.x[0][r[4]:r[4] + r[1] * r[2]].view(min(r[1], r[2]), max(r[1], r[2])).clone() for r in rows]
    a, b, c = NS_COEFFS

    def torch_chain():
        for X in xs:
            for _ in range(5):
                A = X @ X.T
                B = torch.addmm(A, A, A, beta=b, alpha=c)
                X = torch.addmm(X, B, X, beta=a)

    arms = {"muon_step": muon.step, "adamw_step": adamw.step, "ns_chain_hip": lambda: muon.newton_schulz(5),
            "ns_chain_torch_matmul": torch_chain}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            rounds[k].append(timed(fn))
    flop = 5 * sum(2 * min(r[1], r[2]) ** 2 * (2 * max(r[1], r[2]) + min(r[1], r[2])) for r in rows)
    res = {k + "_us": round(statistics.median(v), 1) for k, v in rounds.items()}
    res.update(matrices=len(rows), chain_flop=flop, rounds={k: [round(x, 1) for x in v] for k, v in rounds.items()},
               ns_chain_hip_tflops=round(flop / statistics.median(rounds["ns_chain_hip"]) / 1e6, 1),
               ns_chain_hip_of_peak=round(flop / statistics.median(rounds["ns_chain_hip"]) / 1e-6 / PEAK_BF16, 4))
    os.makedirs(os.path.join(REPO, "profiles", "muon"), exist_ok=True)
    out = os.environ.get("MUON_BENCH_OUT", os.path.join(REPO, "profiles", "muon", "muon_bench.json"))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
