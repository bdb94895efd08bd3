"""Beam search on the device against the closest existing loop over the same rows, GPT-2 124M widths (random weights) on
one MI355X.

For each configuration G x W (G distinct random prompts of 512 tokens, W rows of each, B = G * W rows) one session is
filled the way both callers fill it (refill the prompt once, fork it to its W rows: one share group per prompt) and then
issues 128 tokens per row in one C call:
  samples   num_samples=W: gpt2mi_decode_generate_ragged with the device sampler (temperature 1, top_k 50, one seed),
            the loop of the parent commit over the same rows and the same shared cache
  beams     num_beams=W: gpt2mi_decode_beam_search (per token: top-W, select, the two reorder launches, the step)
Both arms run in ONE process, interleaved round by round after a warm-up round (tools/README.md, "A/B harnesses"); the
figure is the median of the rounds. Per configuration: ms per token of both arms and their ratio, the share of steps
in which any row took another row's suffix (a non-identity parent), and the cache and token bytes the reorder moved:
for each moved row L x 2 x H x (pos - prompt) rows of 128 bytes and (pos - prompt) tokens of 8, read and written twice
(cache -> staging -> cache).

    python tools/beam_bench.py --out profiles/decode/beam_bench.json
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
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

SAMPLER = dict(temperature=1.0, top_k=50, seed=0)


def fill(sess, prompts, W):
    sess.reset()
    for g, p in enumerate(prompts):
        sess.refill(g * W, p)
        sess.fork(g * W, range(g * W + 1, (g + 1) * W))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--configs", default="1x4,1x8,8x8,4x16", help="GxW: distinct prompts x rows (samples, beams) of each")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kv_dtype", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--out", default="profiles/decode/beam_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    row_bytes = 128 if a.kv_dtype == "bf16" else 68
    res = {"model": a.model, "prompt": a.prompt, "new_tokens": a.new, "rounds": a.rounds, "kv_dtype": a.kv_dtype,
           "device": torch.cuda.get_device_name(0), "sampler": SAMPLER, "argv": sys.argv[1:], "configs": []}
    for conf in a.configs.split(","):
        G, W = (int(v) for v in conf.split("x"))
        B = G * W
        gen = torch.Generator().manual_seed(B + G)
        prompts = [torch.randint(0, cfg.vocab_size, (a.prompt,), generator=gen).cuda() for _ in range(G)]
        sess = model.decoder(B, a.prompt + a.new, kv_dtype=a.kv_dtype)
        times = {"samples": [], "beams": []}
        parents = torch.zeros(a.new, B, dtype=torch.int32, device="cuda:0")
        for r in range(a.rounds + 1):  # round 0 warms both arms up
            for name in ("samples", "beams"):
                seq = torch.zeros(B, a.prompt + a.new, dtype=torch.int64, device="cuda:0")
                for g, p in enumerate(prompts):
                    seq[g * W:(g + 1) * W, :a.prompt] = p
                cum = torch.full((B,), float("-inf"), device="cuda:0")
                cum[::W] = 0.0
                done = torch.zeros(B, dtype=torch.uint8, device="cuda:0")
                fill(sess, prompts, W)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "samples":
                    sess.generate(a.new, seq=seq, **SAMPLER)
                else:
                    sess.beam_search(a.new, W, None, seq, cum, done, parents=parents)
                torch.cuda.synchronize()
                if r:
                    times[name].append((time.perf_counter() - t0) / a.new * 1e3)
        moved = parents.cpu() != torch.arange(B, dtype=torch.int32)[None]  # [new, B]: step i, row r took another row's
        window = torch.arange(a.new)[:, None]                             # suffix of i positions
        rows_moved = int((moved * window).sum())                          # (row, position) pairs copied, all steps
        per_pos = cfg.n_layer * 2 * cfg.n_head * row_bytes + 8
        ms = {k: statistics.median(v) for k, v in times.items()}
        row = {"config": conf, "B": B, "prompts": G, "beams": W,
               "samples_ms_per_token": ms["samples"], "beams_ms_per_token": ms["beams"],
               "ratio": ms["beams"] / ms["samples"], "rounds_ms_per_token": times,
               "steps_with_a_moved_row": float(moved.any(1).float().mean()),
               "rows_moved_per_step": float(moved.sum(1).float().mean()),
               "bytes_moved_total": rows_moved * per_pos, "bytes_read_and_written_total": 4 * rows_moved * per_pos,
               "bytes_moved_per_step": rows_moved * per_pos / a.new}
        print(json.dumps(row), flush=True)
        res["configs"].append(row)
        del sess
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
