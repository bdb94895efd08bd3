"""Several samples per prompt over one shared prompt cache: what DecodeSession.fork saves, GPT-2 124M on one MI355X.

For each configuration G x S (G distinct random prompts of 512 tokens, S samples of each, B = G * S rows) one session is filled three ways and then draws 128 tokens per row in the device loop
(gpt2mi_decode_generate_ragged, temperature 1, top_k 50, one seed):
  refill     every row refilled with its prompt: B prefills of one sequence, the only way before fork
  fork       each distinct prompt refilled once, fork(share=False) to its other rows: the same step as `refill`
  share_<c>  fork(share=True), the loop through a library built with GPT2MI_SHARE_CHUNK=<c> members per wave
             and no row threshold (tools/variant_lib.sh chunk<c> decode.hip -DGPT2MI_SHARE_CHUNK=<c>
             -DGPT2MI_SHARE_MIN_ROWS=2; a missing variant is skipped). `share_default` always runs the product
             library: its chunk size, and the unshared launches below its row threshold
All arms run in ONE process, interleaved round by round after a warm-up round (tools/README.md, "A/B harnesses"), and
the warm-up round asserts that every arm produced the same tokens. Per arm: the fill time (prompt to first logits,
host clock ending in a device synchronise), ms per token of the loop, every round's figure, and the algorithmic K/V
bytes a step reads at the mean position of the timed tokens. share_* is to be compared with `fork` of the same run.

The defaults are the run behind profiles/decode/share_bench.json: the issue's three configurations, then 1x16, 2x8 and
4x8 for the row threshold, and chunks 2 and 4 beside the 8, 16 and 64 that were asked for:

    for c in 2 4 8 16 64; do
        bash tools/variant_lib.sh chunk$c decode.hip -DGPT2MI_SHARE_CHUNK=$c -DGPT2MI_SHARE_MIN_ROWS=2
    done
    python tools/share_bench.py --out profiles/decode/share_bench.json
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
from gpt_2_distributed_amd import _lib as K  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

SAMPLER = dict(temperature=1.0, top_k=50, seed=0)


def variant(chunk):
    """The library built with GPT2MI_SHARE_CHUNK=chunk, typed like the product library, or None if it was not built."""
    path = os.path.join(REPO, "tools", "ab", f"lib_chunk{chunk}.so")
    return K.open_library(path) if os.path.exists(path) else None


def loop(lib, sess, n, seq):
    """sess.generate(n, seq=seq) with every C call issued by `lib`: the same plan, buffers and share map."""
    with K.using(lib):
        sess.generate(n, seq=seq, **SAMPLER)


def fill(sess, prompts, S, how):
    sess.reset()
    for g, p in enumerate(prompts):
        if how == "refill":
            for j in range(S):
                sess.refill(g * S + j, p)
        else:
            sess.refill(g * S, p)
            sess.fork(g * S, range(g * S + 1, (g + 1) * S), share=(how == "share"))


def kv_bytes(cfg, G, S, prompt, mean_pos, chunk):
    """K and V bytes one step reads (bf16): chunk None: every row its whole stream; else a shared range once per chunk."""
    per_key = 2 * cfg.n_layer * cfg.n_embd * 2
    if chunk is None:
        return G * S * mean_pos * per_key
    shared = 32 * (prompt // 32)
    return G * (-(-S // chunk) * shared + S * (mean_pos - shared)) * per_key


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--configs", default="1x64,8x8,1x8,1x16,2x8,4x8", help="GxS: distinct prompts x samples of each")
    ap.add_argument("--chunks", default="2,4,8,16,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/decode/share_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("share_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    product = K.load()
    arms = [("refill", "refill", product, None), ("fork", "fork", product, None)]
    for c in [int(c) for c in a.chunks.split(",")]:
        lib = variant(c)
        if lib is not None:
            arms.append((f"share_{c}", "share", lib, c))
    arms.append(("share_default", "share", product, None))
    res = {"model": a.model, "prompt": a.prompt, "new_tokens": a.new, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "sampler": SAMPLER, "argv": sys.argv[1:],
           "configs": []}
    for conf in a.configs.split(","):
        G, S = (int(v) for v in conf.split("x"))
        B = G * S
        gen = torch.Generator().manual_seed(B + G)
        prompts = [torch.randint(0, cfg.vocab_size, (a.prompt,), generator=gen).cuda() for _ in range(G)]
        sess = model.decoder(B, a.prompt + a.new)
        times = {name: dict(fill=[], loop=[]) for name, *_ in arms}
        first = None
        for r in range(a.rounds + 1):  # round 0 warms the arms up and compares their tokens
            for name, how, lib, _ in arms:
                seq = torch.zeros(B, a.prompt + a.new, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fill(sess, prompts, S, how)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                loop(lib, sess, a.new, seq)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if r == 0:
                    first = seq if first is None else first
                    assert torch.equal(seq, first), f"{conf}: arm {name} drew other tokens than arm {arms[0][0]}"
                else:
                    times[name]["fill"].append((t1 - t0) * 1e3)
                    times[name]["loop"].append((t2 - t1) / a.new * 1e3)
        row = {"config": conf, "B": B, "prompts": G, "samples": S, "tokens_equal_across_arms": True, "arms": {}}
        base = statistics.median(times["fork"]["loop"])
        for name, how, _, chunk in arms:
            ms = statistics.median(times[name]["loop"])
            eff = chunk if chunk is not None else (None if how != "share" else "default")
            row["arms"][name] = {
                "ms_per_token": ms, "rounds_ms_per_token": times[name]["loop"],
                "fill_ms": statistics.median(times[name]["fill"]), "rounds_fill_ms": times[name]["fill"],
                "vs_fork": ms / base,
                "kv_bytes_per_step": None if eff == "default" else kv_bytes(cfg, G, S, a.prompt, a.prompt + a.new / 2, eff)}
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
