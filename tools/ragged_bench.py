"""Many prompts of unequal length: generate_many (continuous batching) against one generate per prompt, GPT-2 124M widths
on one MI355X.

Workload: 64 prompts with lengths spread evenly over [16, 512] (random tokens from a seed), 128 new tokens each, no eos,
temperature 0.8 / top_k 50 on the device sampler.
  one_by_one    what a caller does without ragged batches: model.generate(prompt[None], 128, seed=...) per prompt, B = 1.
  many_B        model.generate_many(prompts, 128, batch_size=B) for B in 8, 32, 64: every prompt enters a row of one
                session through DecodeSession.refill (a prefill of one sequence) and the rows decode together.
Both arms include their prefills: the figure is what the caller waits for. All arms run in ONE process, interleaved round
by round after a warm-up round of each (tools/README.md, "A/B harnesses"); an arm's time is a host clock around the
whole arm ending in a device synchronise; the median round is reported with every round's figure beside it.
ms per generated token = arm time / (64 x 128); tokens/s its inverse. The ratio is one_by_one / many_B.
The arms compute the same thing for prompt i only where its draw key agrees: generate_many draws prompt i with key i,
generate at B = 1 with key 0, so only prompt 0's tokens are comparable, and they are compared (bitwise) as a check that
the arms run the same model. Writes one JSON file.

    python tools/ragged_bench.py --out profiles/decode/ragged_bench.json
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
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

SAMPLER = dict(temperature=0.8, top_k=50, seed=11)


def make_prompts(vocab, count, lo, hi, seed=0):
    """`count` prompts with lengths evenly spaced over [lo, hi], in an order shuffled by the seed."""
    g = torch.Generator().manual_seed(seed)
    lens = [lo + round(i * (hi - lo) / max(count - 1, 1)) for i in range(count)]
    lens = [lens[i] for i in torch.randperm(count, generator=g).tolist()]
    return [torch.randint(0, vocab, (n,), generator=g).cuda() for n in lens]


def one_by_one(model, prompts, n_new):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = [model.generate(p[None], n_new, **SAMPLER)[0] for p in prompts]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, outs


def many(model, prompts, n_new, batch_size):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = model.generate_many(prompts, n_new, batch_size=batch_size, **SAMPLER)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, outs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--prompts", type=int, default=64)
    ap.add_argument("--min_len", type=int, default=16)
    ap.add_argument("--max_len", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--batches", default="8,32,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/decode/ragged_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    prompts = make_prompts(cfg.vocab_size, a.prompts, a.min_len, a.max_len)
    batches = [int(b) for b in a.batches.split(",")]
    total = a.prompts * a.new
    times = {"one_by_one": [], **{f"many_{b}": [] for b in batches}}
    same_prompt0, same_across_batches = True, True
    for r in range(a.rounds + 1):  # round 0 warms the arms up
        t, base = one_by_one(model, prompts, a.new)
        if r:
            times["one_by_one"].append(t)
        first = None
        for b in batches:
            t, outs = many(model, prompts, a.new, b)
            if r:
                times[f"many_{b}"].append(t)
            same_prompt0 &= bool(torch.equal(outs[0], base[0]))
            first = outs if first is None else first
            same_across_batches &= all(torch.equal(x, y) for x, y in zip(outs, first))
    ms = {k: statistics.median(v) / total * 1e3 for k, v in times.items()}
    res = {"model": a.model, "prompts": a.prompts, "prompt_lens": [p.numel() for p in prompts], "new_tokens": a.new,
           "rounds": a.rounds, "sampler": SAMPLER, "device": torch.cuda.get_device_name(0),
           "generated_tokens_per_arm": total, "prompt0_equal_to_one_by_one": same_prompt0,
           "outputs_equal_across_batch_sizes": same_across_batches, "arms": []}
    for k, v in times.items():
        row = {"arm": k, "ms_per_generated_token": ms[k], "tokens_per_s": 1e3 / ms[k],
               "speedup_over_one_by_one": ms["one_by_one"] / ms[k], "rounds_s": v}
        print(json.dumps(row), flush=True)
        res["arms"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
