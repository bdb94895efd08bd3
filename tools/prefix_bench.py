"""Prefill over a live cache, measured at 124M widths (12 layers, C = 768, 12 heads, V = 50257, 1024 positions), random
weights; writes profiles/decode/prefix_bench.json.

Appending runs: n = 16, 64, 256, 512 tokens appended to a row that holds base = 64 or 512, through
  append   DecodeSession.append (one pass of the trunk over the chunk, the chunk attention over the cache),
  extend   DecodeSession.extend (decode rows, 64 a call),
  refill   DecodeSession.refill of the base + n tokens from position 0,
and with --nosplit_lib (a build of the library whose chunk attention never splits the keys,
``bash tools/variant_lib.sh nosplit prefill_cached.hip -DGPT2MI_CHUNK_SPLIT_TILES=1024 -Xclang -target-feature -Xclang
-packed-fp32-ops``) the append arm over that library as well: what the key split buys.
Shared prefix: generate_many over 64 prompts (a 384-token prefix, a 32-token suffix each, 32 new tokens, 32 rows) with and
without a SharedPrefix; the JSON records whether the two arms' tokens are equal (they need not be: the arithmetic differs).

All arms run in one process, interleaved, a warm-up round and then the median of 3 rounds; a timing is a host clock
around work that ends in a device synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_2_distributed_amd import _lib as K  # noqa: E402
from gpt_2_distributed_amd.generation import SharedPrefix  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config  # noqa: E402

WIDTHS = dict(n_layer=12, n_head=12, n_embd=768, vocab_size=50257, n_positions=1024, resid_pdrop=0.0, attn_pdrop=0.0)


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3  # ms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="profiles/decode/prefix_bench.json")
    ap.add_argument("--nosplit_lib", default=None)
    ap.add_argument("--kv_dtype", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("prefix_bench measures on the GPU: none found")
    dev = "cuda"
    torch.manual_seed(0)
    model = GPT2(GPT2Config(**WIDTHS)).to(dev)
    tok = torch.randint(0, WIDTHS["vocab_size"], (1024,), device=dev)
    nosplit = K.open_library(a.nosplit_lib) if a.nosplit_lib else None
    sess = model.decoder(1, kv_dtype=a.kv_dtype)

    def rewind(base):  # the row back at `base` tokens: what lies above is overwritten by the next arm
        sess.lens[0] = base

    def arm_append(base, n):
        rewind(base)
        sess.append(0, tok[base:base + n])

    def arm_extend(base, n):
        rewind(base)
        sess.extend(tok[None, base:base + n])

    arms = {"append": arm_append, "extend": arm_extend, "refill": lambda base, n: sess.refill(0, tok[:base + n])}
    if nosplit is not None:
        def arm_nosplit(base, n):
            with K.using(nosplit):
                arm_append(base, n)
        arms["append_nosplit"] = arm_nosplit
    points = [(base, n) for base in (64, 512) for n in (16, 64, 256, 512)]
    times = {(p, name): [] for p in points for name in arms}
    for rnd in range(4):  # round 0 warms every shape up
        for p in points:
            sess.refill(0, tok[:p[0]])
            for name, fn in arms.items():
                ms = timed(lambda: fn(*p), a.reps)
                if rnd:
                    times[(p, name)].append(ms)
    rows = []
    for base, n in points:
        med = {name: statistics.median(times[((base, n), name)]) for name in arms}
        row = dict(base=base, n=n, splits=K.attn_chunk_splits(base + n), ms=med,
                   append_over_extend=med["append"] / med["extend"], append_over_refill=med["append"] / med["refill"])
        if nosplit is not None:
            row["split_over_nosplit"] = med["append"] / med["append_nosplit"]
        rows.append(row)
        print(json.dumps(row))

    # the chunk attention alone (H = 12, one sequence), 50 calls back to back: the launches of one layer without the
    # trunk around them, over the product library and over the one that never splits
    kernel = []
    if nosplit is not None:
        H, C, Tcap = WIDTHS["n_head"], WIDTHS["n_embd"], 1024
        kc, vc = (torch.randn(1, H, Tcap, 64, device=dev).bfloat16() for _ in range(2))
        kt = {(p, name): [] for p in points for name in ("split", "nosplit")}
        for rnd in range(4):
            for base, n in points:
                Tp = (n + 63) // 64 * 64
                qkv = torch.randn(1, Tp, 3 * C, device=dev).bfloat16()
                out = torch.empty(1, Tp, C, dtype=torch.bfloat16, device=dev)
                ws = torch.empty(K.attn_chunk_workspace(1, H, Tcap, Tp), device=dev)
                call = lambda: K.attn_chunk(qkv, kc, vc, out, ws, 1, H, 64, Tcap, Tp, [0], [base], [n])  # noqa: E731
                for name, ctx in (("split", None), ("nosplit", nosplit)):
                    if ctx is None:
                        ms = timed(call, 50)
                    else:
                        with K.using(ctx):
                            ms = timed(call, 50)
                    if rnd:
                        kt[((base, n), name)].append(ms)
        for base, n in points:
            us = {name: 1e3 * statistics.median(kt[((base, n), name)]) for name in ("split", "nosplit")}
            kernel.append(dict(base=base, n=n, splits=K.attn_chunk_splits(base + n), us=us,
                               split_over_nosplit=us["split"] / us["nosplit"]))
            print(json.dumps(kernel[-1]))

    # shared prefix
    g = torch.Generator().manual_seed(1)
    prefix = torch.randint(0, WIDTHS["vocab_size"], (384,), generator=g).to(dev)
    suffixes = [torch.randint(0, WIDTHS["vocab_size"], (32,), generator=g).to(dev) for _ in range(64)]
    kw = dict(batch_size=32, seed=3, temperature=0.8, top_k=50, kv_dtype=a.kv_dtype)
    shared = {"with_prefix": lambda: model.generate_many(SharedPrefix(prefix, suffixes), 32, **kw),
              "without": lambda: model.generate_many([torch.cat([prefix, s]) for s in suffixes], 32, **kw)}
    st, outs = {n: [] for n in shared}, {}
    for rnd in range(4):
        for name, fn in shared.items():
            box = []
            ms = timed(lambda: box.append(fn()), 1)
            outs[name] = box[0]
            if rnd:
                st[name].append(ms)
    med = {n: statistics.median(v) for n, v in st.items()}
    equal = all(torch.equal(x, y) for x, y in zip(outs["with_prefix"], outs["without"]))
    share = dict(prompts=64, prefix=384, suffix=32, new_tokens=32, batch_size=32, ms=med,
                 with_over_without=med["with_prefix"] / med["without"], tokens_equal=equal)
    print(json.dumps(share))
    result = dict(widths=WIDTHS, kv_dtype=a.kv_dtype, reps=a.reps, rounds=3, device=torch.cuda.get_device_name(0),
                  nosplit_lib=bool(nosplit), appending=rows, chunk_attention=kernel, shared_prefix=share)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments from device memory (see __init__.py)
    sys.exit(main())
