#!/usr/bin/env python
"""Prices one deferred weight-gradient launch for the whole trunk before building it. GPT-2 124M, 65536 tokens.

Arm A is what the step runs: per layer two grouped launches (fc2 + fc1, proj + qkv) at the split the engine asks for,
each with its slab reduction; 12 layers with 12 distinct operand sets, so nothing is L2/MALL-warm that the step would
not find warm. Arm B stands in for the batched plan through the existing entries: gemm_wgrad(splits=1) on one problem
of 1280 full tiles (10240 x 8192: every block owns a tile, loops over all tokens, writes fp32 once; no slabs) plus the
18-tile tail (two proj problems, grouped) at the split that fills one round. Both arms alternate in one process, HIP
events, medians; arm A is timed a second time in every round so that its own repeat spread stands beside the gap."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_2_distributed_amd import _lib as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join("profiles", "wgrad_batch", "probe.txt"))
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=2)
args = ap.parse_args()

dev = "cuda"
Mt, C, L = 65536, 768, 12
g = torch.Generator(device=dev).manual_seed(0)


def bf(rows, cols, scale=1.0):
    return (torch.randn(rows, cols, device=dev, generator=g) * scale).to(torch.bfloat16)


# (m, n) of dW = dY[:, :m]^T X[:, :n]
mlp = [(C, 4 * C), (4 * C, C)]  # fc2, fc1
att = [(C, C), (3 * C, C)]  # proj, qkv
layers = []
for _ in range(L):
    pairs = []
    for shapes in (mlp, att):
        pairs.append([(m, n, bf(Mt, m, 0.1), m, bf(Mt, n), n, torch.empty(m, n, device=dev)) for m, n in shapes])
    layers.append(pairs)
ws = torch.empty(32 * 3072 * 768, device=dev)
split_mlp = K.wgrad_group_splits(mlp, Mt)
split_att = K.wgrad_group_splits(att, Mt)

BM, BN = 10240, 8192  # 40 x 32 = 1280 tiles = 5 rounds of 256 CUs
bA, bB, bC = bf(Mt, BM, 0.1), bf(Mt, BN), torch.empty(BM, BN, device=dev)
tail = [layers[i][1][0] for i in (0, 1)]  # two proj problems: 18 tiles
# the split that fills one round of 256 CUs with 18 tiles: minimise ceil(18 s / 256) / s + the slab term
tail_split = min(range(1, 33), key=lambda s: -(-18 * s // 256) * (Mt / s) * 22e-9 + s * 2 * C * C * 8 / 5e12)


def arm_a():
    for pairs in layers:
        K.gemm_wgrad_grouped(pairs[0], Mt, accumulate=False, workspace=ws, splits=split_mlp)
        K.gemm_wgrad_grouped(pairs[1], Mt, accumulate=False, workspace=ws, splits=split_att)


def body():
    K.gemm_wgrad(BM, BN, Mt, bA, BM, bB, BN, bC, BN, accumulate=False, workspace=ws, splits=1)


def tail_only():
    K.gemm_wgrad_grouped(tail, Mt, accumulate=False, workspace=ws, splits=tail_split)


def arm_b():
    body()
    tail_only()


cases = {f"A: 12 x (fc2+fc1 @{split_mlp}, proj+qkv @{split_att}) + reductions": arm_a,
         f"B: 1280 tiles unsplit + 18-tile tail @{tail_split}": arm_b,
         "B body alone (10240 x 8192, splits=1)": body,
         f"B tail alone (2 x proj grouped @{tail_split})": tail_only,
         "A again": arm_a}
times = {k: [] for k in cases}
for f in cases.values():
    f()
torch.cuda.synchronize()
for _ in range(args.rounds):
    for k, f in cases.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _r in range(args.reps):
            f()
        e.record()
        torch.cuda.synchronize()
        times[k].append(s.elapsed_time(e) / args.reps * 1e3)

flop_a = 2 * Mt * L * sum(m * n for m, n in mlp + att)
flop = {k: flop_a for k in cases}
names = list(cases)
flop[names[1]] = 2 * Mt * (BM * BN + 2 * C * C)
flop[names[2]] = 2 * Mt * BM * BN
flop[names[3]] = 2 * Mt * 2 * C * C
lines = [f"{torch.cuda.get_device_name(0)}; {Mt} tokens; {args.rounds} alternating rounds x {args.reps} reps; "
         f"median [min .. max] us"]
med = {}
for k, v in times.items():
    v = sorted(v)
    med[k] = v[len(v) // 2]
    lines.append(f"{k:62s} {med[k]:9.1f} [{v[0]:9.1f} .. {v[-1]:9.1f}] us  {flop[k] / med[k] / 1e6:6.0f} TF")
a, b, a2 = med[names[0]], med[names[1]], med[names[4]]
# arm B does 1298 tiles where arm A does 1296: scale it to A's work before comparing
b_eq = b * flop_a / flop[names[1]]
lines.append(f"A - B (B scaled to A's FLOPs: {b_eq:.1f} us) = {a - b_eq:.1f} us; A - A again = {a - a2:.1f} us")
text = "\n".join(lines)
print(text, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(text + "\n")
