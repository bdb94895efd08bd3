"""Decode step time over the fp8 key/value cache against the bf16 cache, GPT-2 124M on one MI355X.

The method is tools/decode_bench.py's decode arm, once per cache format: for each batch size B (default 1, 8, 64) a
random prompt of 512 tokens, DecodeSession.prefill once (not timed), then 128 x (argmax + DecodeSession.step). The two
arms run in ONE process, interleaved round by round after a warm-up round of each (tools/README.md, "A/B harnesses");
an arm's time is a host clock around its 128 tokens ending in a device synchronise; the median round is reported with
every round's figure beside it. Random weights: the greedy tokens of the two arms part early (nearly tied logits), which
says nothing about correctness (tests/test_kv_fp8_generation_gpu.py does).

Reported per B: ms/token of both arms and their ratio, cache_bytes of both sessions, the K/V bytes a step streams at the
mean timed position in each format, and the bf16 arm against the figure --baseline holds for that B
(profiles/decode/decode_bench.json, which states 7 % box-to-box repeatability: a bf16 arm outside it means the bf16
path changed). Writes one JSON file.

    python tools/kv_bench.py --out profiles/decode/kv_fp8_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py and the trainer set it (gpt_2_distributed_amd/__init__.py)

import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gpt_2_distributed_amd.generation import sample_next  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

ROW_BYTES = {"bf16": 128, "fp8": 68}  # per (layer, K or V, sequence, head, position)
REPEATABILITY = 0.07


def decode_arm(model, prompt, n_new, kv_dtype):
    """(seconds for n_new tokens, the session's cache_bytes): prefill outside the clock."""
    sess = model.decoder(prompt.size(0), prompt.size(1) + n_new, kv_dtype=kv_dtype)
    logits = sess.prefill(prompt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_new):
        nxt = sample_next(logits, 0.0)
        if i + 1 < n_new:
            logits = sess.step(nxt)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, sess.cache_bytes


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline", default=os.path.join(REPO, "profiles", "decode", "decode_bench.json"))
    ap.add_argument("--out", default="profiles/decode/kv_fp8_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    base = {}
    if a.baseline and os.path.exists(a.baseline):
        with open(a.baseline) as f:
            base = {s["B"]: s["decode_ms_per_token"] for s in json.load(f)["shapes"]}
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    res = {"model": a.model, "prompt": a.prompt, "new_tokens": a.new, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "baseline": os.path.relpath(a.baseline, REPO) if base else None,
           "shapes": []}
    for B in [int(b) for b in a.batches.split(",")]:
        prompt = torch.randint(0, cfg.vocab_size, (B, a.prompt), generator=torch.Generator().manual_seed(B)).cuda()
        ms = {"bf16": [], "fp8": []}
        size = {}
        for r in range(a.rounds + 1):  # round 0 warms the arms up
            for kv_dtype in ms:
                t, size[kv_dtype] = decode_arm(model, prompt, a.new, kv_dtype)
                if r:
                    ms[kv_dtype].append(t / a.new * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        mean_pos = a.prompt + a.new / 2
        row = {"B": B, "bf16_ms_per_token": med["bf16"], "fp8_ms_per_token": med["fp8"],
               "fp8_over_bf16": med["fp8"] / med["bf16"], "bf16_rounds_ms": ms["bf16"], "fp8_rounds_ms": ms["fp8"],
               "bf16_cache_bytes": size["bf16"], "fp8_cache_bytes": size["fp8"],
               "cache_bytes_ratio": size["fp8"] / size["bf16"]}
        for k, nbytes in ROW_BYTES.items():
            row[f"{k}_kv_bytes_per_token"] = cfg.n_layer * 2 * B * cfg.n_head * mean_pos * nbytes
        if B in base:
            row["baseline_bf16_ms_per_token"] = base[B]
            row["bf16_over_baseline"] = med["bf16"] / base[B]
            row["bf16_within_repeatability"] = abs(med["bf16"] / base[B] - 1) <= REPEATABILITY
        print(json.dumps(row), flush=True)
        res["shapes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
