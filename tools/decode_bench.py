"""Decode throughput: the KV-cache decode step against the full-recompute loop, GPT-2 124M on one MI355X.

For each batch size B (default 1, 8, 64): a random prompt of 512 tokens, 128 greedy new tokens.
  decode     DecodeSession.prefill once (not timed), then 128 x (argmax + DecodeSession.step): gpt2mi_decode_step.
  recompute  128 x (model(idx) on the whole growing sequence in eval mode under bf16 autocast, argmax of its last
             row, append): the only way to continue a prompt without the decode path. It includes what that loop pays
             in the engine: padding to the 64-token attention tile, the full [B*T, Vp] lm_head, and a workspace
             re-allocation each time the padded length grows (512 -> 576 -> 640).
  recompute_padded  the same loop as a careful caller would write it without the decode path: idx kept zero-padded to
             the next multiple of 64 (causality hides the padding) and the logits row of the last real token read, so
             every tensor keeps its shape for 64 tokens and the caching allocator re-uses its blocks. (In the plain
             loop the engine's compaction of the [B, T, Vp] logits changes size with every token, and each token pays
             a multi-gigabyte device allocation at large B.)
All arms run in ONE process, interleaved round by round after a warm-up round of each (tools/README.md, "A/B
harnesses"); each arm's time is a host clock around its 128 tokens ending in a device synchronise; the median round is
reported with every round's figure beside it.

streamed bytes per token = the bf16 weights a step reads once (12 C^2 per layer + the [Vp, C] tied head) + the cached
K and V of every layer at the mean position of the timed tokens; divided by the decode time per token it is set against
the 6.29 TB/s a device-to-device copy reaches on this chip (MI355X_MICROARCH.md). Writes one JSON file.

    python tools/decode_bench.py --out profiles/decode/decode_bench.json
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
from gpt_2_distributed_amd.generation import sample_next  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s, measured device-to-device copy rate (MI355X_MICROARCH.md)


def streamed_bytes(cfg, vpad, B, mean_pos):
    C, L = cfg.n_embd, cfg.n_layer
    weights = 2 * (L * 12 * C * C + vpad * C)
    kv = 2 * L * 2 * B * mean_pos * C
    return weights, kv


def launches_per_token(cfg, vpad):
    """Kernel launches of one gpt2mi_decode_step: a skinny GEMM is one launch from 128 strips of 16 columns on
    (N >= 2048) and two (the K slices' partial sums, then their sum) below; attention is the key ranges + their combine."""
    C = cfg.n_embd
    gemm = lambda n: 1 if n // 16 >= 128 else 2  # noqa: E731
    layer = 2 + gemm(3 * C) + 2 + gemm(C) + gemm(4 * C) + gemm(C)  # LN1, LN2, qkv, attention, proj, fc1, fc2
    return 1 + cfg.n_layer * layer + 1 + gemm(vpad)  # embedding, blocks, ln_f, lm_head


def decode_arm(model, prompt, n_new):
    """(seconds for n_new tokens, the tokens): prefill outside the clock."""
    sess = model.decoder(prompt.size(0), prompt.size(1) + n_new)
    logits = sess.prefill(prompt)
    out = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_new):
        nxt = sample_next(logits, 0.0)
        out.append(nxt)
        if i + 1 < n_new:
            logits = sess.step(nxt)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.stack(out, 1)


def recompute_arm(model, prompt, n_new):
    idx, out = prompt, []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for i in range(n_new):
            logits, _ = model(idx)
            nxt = logits[:, -1].float().argmax(-1)
            out.append(nxt)
            if i + 1 < n_new:
                idx = torch.cat([idx, nxt[:, None]], dim=1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.stack(out, 1)


def recompute_padded_arm(model, prompt, n_new):
    B, P = prompt.shape
    buf = torch.zeros(B, (P + n_new + 63) // 64 * 64, dtype=torch.int64, device=prompt.device)
    buf[:, :P] = prompt
    out = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for i in range(n_new):
            cur = P + i
            logits, _ = model(buf[:, :(cur + 63) // 64 * 64])
            nxt = logits[:, cur - 1].float().argmax(-1)
            out.append(nxt)
            if i + 1 < n_new:
                buf[:, cur] = nxt
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.stack(out, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/decode/decode_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    res = {"model": a.model, "prompt": a.prompt, "new_tokens": a.new, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12,
           "launches_per_token": launches_per_token(cfg, model.vpad), "shapes": []}
    for B in [int(b) for b in a.batches.split(",")]:
        prompt = torch.randint(0, cfg.vocab_size, (B, a.prompt), generator=torch.Generator().manual_seed(B)).cuda()
        dec, rec, recp, agree = [], [], [], None
        for r in range(a.rounds + 1):  # round 0 warms the arms up
            td, tok_d = decode_arm(model, prompt, a.new)
            tr, tok_r = recompute_arm(model, prompt, a.new)
            tp, _ = recompute_padded_arm(model, prompt, a.new)
            if r:
                dec.append(td / a.new * 1e3)
                rec.append(tr / a.new * 1e3)
                recp.append(tp / a.new * 1e3)
            # share of equal greedy tokens of the two paths. With the random weights used here logits are nearly tied
            # (and the recompute arm's are bf16, with exact ties), so the paths part early and stay apart: reported
            # for the record, it says nothing about correctness (tests/test_generation_gpu.py does)
            agree = float((tok_d == tok_r).float().mean())
        ms_d, ms_r, ms_p = statistics.median(dec), statistics.median(rec), statistics.median(recp)
        w, kv = streamed_bytes(cfg, model.vpad, B, a.prompt + a.new / 2)
        row = {"B": B, "decode_ms_per_token": ms_d, "recompute_ms_per_token": ms_r, "speedup": ms_r / ms_d,
               "recompute_padded_ms_per_token": ms_p, "speedup_over_padded": ms_p / ms_d,
               "decode_rounds_ms": dec, "recompute_rounds_ms": rec, "recompute_padded_rounds_ms": recp, "decode_tokens_per_s": B / ms_d * 1e3,
               "weight_bytes": w, "kv_bytes": kv, "streamed_TBps": (w + kv) / (ms_d * 1e-3) / 1e12,
               "share_of_copy_rate": (w + kv) / (ms_d * 1e-3) / COPY_RATE, "greedy_token_agreement": agree}
        print(json.dumps(row), flush=True)
        res["shapes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
