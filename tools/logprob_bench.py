"""What per-token log-probabilities cost: gpt2mi_sample_logprobs alone and inside the device loop, on one MI355X.

The protocol of tools/sample_bench.py and tools/penalty_bench.py: ONE process, the arms interleaved round by round after
a warm-up round of each, the median of the rounds reported with every round beside it.

Kernel alone: HIP events around 200 back-to-back launches at V = 50257 (ldl 50432), B = 1 and 64, for "top_k 50 +
top_p 0.95" (temperature 0.8) and greedy. Arms: `null` (gpt2mi_sample_logprobs with lp = NULL: gpt2mi_sample_penalized's
launches), `top0` / `top5` / `top20` (the LP kernels with top_n = 0, 5, 20). The launches are issued from Python through
ctypes with every argument built beforehand, so a figure is an upper bound on the kernel's time: `issue_us_per_launch`,
the host time per call, is the floor a figure cannot go below.

Device loop: ms per token of DecodeSession.generate, GPT-2 124M, a random prompt of 512 tokens, 128 new tokens, B = 1 / 8
/ 64, sampling (0.8, top_k 50, top_p 0.95), with and without a LogprobBuffer of top_n = 5.

--parent_lib: a libgpt2mi.so built from the parent commit (the same ABI version, minor 0), opened with
_lib.open_library(path, min_minor=0). Its gpt2mi_sample_penalized then runs as two further arms, `parent_a` and
`parent_b`, alternating with `null` in every round, and the device loop runs over it twice as well (_lib.using). The
two parent arms are the same code: the distance between their medians, and of their rounds from their medians, is the
spread of this run, which `null` over `parent_a` has to stay within (`null_within_parent_spread`).

    python tools/logprob_bench.py --out profiles/decode/logprob_bench.json [--parent_lib /path/to/libgpt2mi.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py and the trainer set it (gpt_2_distributed_amd/__init__.py)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_2_distributed_amd import _lib as K  # noqa: E402
from gpt_2_distributed_amd.generation import LogprobBuffer  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402
from tools.penalty_bench import prepared, timed  # noqa: E402

MODES = {"top_k50_top_p0.95": (0.8, 50, 0.95), "greedy": (0.0, None, None)}
TOPS = (0, 5, 20)
POS = 17


def spread(rounds_by_arm):
    """The largest distance of a round from its arm's median, relative, over the given arms."""
    return max(abs(x - statistics.median(v)) / statistics.median(v) for v in rounds_by_arm for x in v)


def verdict(us, mine, a, b):
    """`mine` against the parent arm `a`, beside what the two parent arms (the same code) differ by in this run."""
    med = {k: statistics.median(v) for k, v in us.items()}
    noise = max(abs(med[a] - med[b]) / med[a], spread([us[a], us[b]]))
    return {"null_over_parent": med[mine] / med[a], "parent_b_over_parent_a": med[b] / med[a], "parent_spread": noise,
            "null_within_parent_spread": med[mine] / med[a] <= 1 + noise}


def kernel_alone(B, V, ldl, launches, rounds, parent):
    logits = torch.randn(B, ldl, generator=torch.Generator().manual_seed(B)).cuda() * 3
    tok = torch.empty(B, dtype=torch.int64, device="cuda")
    lib = K.load()
    stream = torch.cuda.current_stream().cuda_stream
    pos = (ctypes.c_int * B)(*([POS] * B))
    bufs = {n: (torch.zeros(B, POS + 1, device="cuda"), torch.zeros(B, POS + 1, n, dtype=torch.int32, device="cuda"),
                torch.zeros(B, POS + 1, n, device="cuda")) for n in TOPS}
    structs = {n: K.Logprobs(lp.data_ptr(), POS + 1, n, ids.data_ptr() if n else None, tl.data_ptr() if n else None, None)
               for n, (lp, ids, tl) in bufs.items()}
    out = {}
    for mode, (t, k, p) in MODES.items():
        head = (logits.data_ptr(), ldl, B, V, t, k or 0, 1.0 if p is None else p, 0, pos, None, -1, None, tok.data_ptr(),
                None, 0, None, None, None)  # ... probs_out, pen, logits_out
        arms = {"null": prepared(lib.gpt2mi_sample_logprobs, *head, None, stream)}
        for n in TOPS:
            arms[f"top{n}"] = prepared(lib.gpt2mi_sample_logprobs, *head, ctypes.byref(structs[n]), stream)
        if parent is not None:
            arms["parent_a"] = prepared(parent.gpt2mi_sample_penalized, *head, stream)
            arms["parent_b"] = prepared(parent.gpt2mi_sample_penalized, *head, stream)
        us = {a: [] for a in arms}
        issue = {a: [] for a in arms}
        for r in range(rounds + 1):  # round 0 warms the arms up
            for a, launch in arms.items():
                u, h = timed(launch, launches)
                if r:
                    us[a].append(u)
                    issue[a].append(h)
        med = {a: statistics.median(v) for a, v in us.items()}
        out[mode] = {"us_per_launch": med, "rounds_us": us,
                     "issue_us_per_launch": {a: statistics.median(v) for a, v in issue.items()},
                     "cost_us_over_null": {a: med[a] - med["null"] for a in med if a.startswith("top")},
                     "round_spread": spread(list(us.values()))}
        if parent is not None:
            out[mode]["against_parent"] = verdict(us, "null", "parent_a", "parent_b")
    return out


def loop_arm(model, prompt, n_new, top_n, seed):
    import time
    B, P = prompt.shape
    sess = model.decoder(B, P + n_new)
    sess.prefill(prompt)
    seq = torch.empty(B, P + n_new, dtype=torch.int64, device=prompt.device)
    seq[:, :P] = prompt
    lp = {} if top_n is None else {"logprobs": LogprobBuffer(B, P + n_new, top_n, prompt.device)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess.generate(n_new, 0.8, 50, 0.95, seed, seq=seq, **lp)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n_new * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default="profiles/decode/logprob_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logprob_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    parent = K.open_library(a.parent_lib, min_minor=0) if a.parent_lib else None
    res = {"model": a.model, "prompt": a.prompt, "new_tokens": a.new, "rounds": a.rounds, "launches": a.launches,
           "device": torch.cuda.get_device_name(0), "parent_lib": bool(parent), "kernel_alone": [], "loops": []}
    V, ldl = cfg.vocab_size, model.vpad
    for B in (1, 64):
        row = {"B": B, "V": V, "ldl": ldl, **kernel_alone(B, V, ldl, a.launches, a.rounds, parent)}
        print(json.dumps(row), flush=True)
        res["kernel_alone"].append(row)
    for B in [int(b) for b in a.batches.split(",")]:
        prompt = torch.randint(0, cfg.vocab_size, (B, a.prompt), generator=torch.Generator().manual_seed(B)).cuda()
        arms = [("plain", None, None), ("logprobs5", 5, None)]
        if parent is not None:
            arms += [("parent_a", None, parent), ("parent_b", None, parent)]
        times = {arm: [] for arm, _, _ in arms}
        for r in range(a.rounds + 1):
            for arm, top_n, lib in arms:
                if lib is None:
                    ms = loop_arm(model, prompt, a.new, top_n, seed=r)
                else:
                    with K.using(lib):
                        ms = loop_arm(model, prompt, a.new, top_n, seed=r)
                if r:
                    times[arm].append(ms)
        row = {"B": B, **{f"{arm}_ms_per_token": statistics.median(ts) for arm, ts in times.items()},
               **{f"{arm}_rounds_ms": ts for arm, ts in times.items()}}
        row["logprobs5_over_plain"] = row["logprobs5_ms_per_token"] / row["plain_ms_per_token"]
        if parent is not None:
            row["against_parent"] = verdict(times, "plain", "parent_a", "parent_b")
        print(json.dumps(row), flush=True)
        res["loops"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
