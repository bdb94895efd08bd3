"""What the sampler's penalties cost: gpt2mi_sample_penalized alone and inside the device loop, on one MI355X.

The protocol of tools/sample_bench.py: ONE process, the arms interleaved round by round after a warm-up round of each,
the median of 3 rounds reported with every round beside it.

Kernel alone: HIP events around 200 back-to-back launches at V = 50257 (ldl 50432), B = 1 and 64, for "top_k 50 +
top_p 0.95" (temperature 0.8) and greedy. Arms: `plain` (gpt2mi_sample_ragged), `neutral` (gpt2mi_sample_penalized with
1, 0, 0: the same kernels), and penalised (1.3, 0.5, 0.2) at history lengths 16 / 512 / 1023 with all-distinct and with
all-equal tokens. The launches are issued from Python through ctypes with every argument built beforehand (the greedy
kernel is shorter than a call through the package's wrappers takes to issue), so a figure is an upper bound on the
kernel's time: `issue_us_per_launch`, the host time per call, is the floor a figure cannot go below.

Device loop: ms per token of DecodeSession.generate, GPT-2 124M, a random prompt of 512 tokens, 128 new tokens, B = 1 / 8
/ 64, sampling (0.8, top_k 50, top_p 0.95), with and without repetition_penalty=1.3, frequency_penalty=0.2.

--parent_lib: a libgpt2mi.so built from the parent commit. Its gpt2mi_sample_ragged (the same signature) then runs as a
further arm `parent_plain`, alternating with `plain` in every round: the neutral path against the tree before this
feature, with the round-to-round spread of the same run beside it.

    python tools/penalty_bench.py --out profiles/decode/penalty_bench.json [--parent_lib /path/to/libgpt2mi.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py and the trainer set it (gpt_2_distributed_amd/__init__.py)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_2_distributed_amd import _lib as K  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

MODES = {"top_k50_top_p0.95": (0.8, 50, 0.95), "greedy": (0.0, None, None)}
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2)
LOOP_PEN = dict(repetition_penalty=1.3, frequency_penalty=0.2)
HIST_LENS = (16, 512, 1023)


def entries(path):
    """(gpt2mi_sample_ragged, gpt2mi_sample_penalized or None, ABI version) of a build of the library, typed."""
    lib = ctypes.CDLL(path)
    out = []
    for name in ("gpt2mi_sample_ragged", "gpt2mi_sample_penalized"):
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = K._SIGS[name], ctypes.c_int
        out.append(fn)
    return out[0], out[1], lib.gpt2mi_abi_version()


def prepared(fn, *args):
    """launch(i) calling the C entry with arguments converted once."""
    def launch(i):
        rc = fn(*args)
        assert rc == 0, rc
    return launch


def timed(launch, launches):
    """(us per launch between two HIP events, host us per call) of `launches` back-to-back calls of launch(i)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    h0 = time.perf_counter()
    for i in range(launches):
        launch(i)
    issue = time.perf_counter() - h0
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / launches * 1e3, issue / launches * 1e6


def kernel_alone(B, V, ldl, launches, rounds, parent):
    logits = torch.randn(B, ldl, generator=torch.Generator().manual_seed(B)).cuda() * 3
    tok = torch.empty(B, dtype=torch.int64, device="cuda")
    g = torch.Generator().manual_seed(1)
    distinct = torch.stack([torch.randperm(V, generator=g)[:1024] for _ in range(B)]).cuda()
    equal = torch.full((B, 1024), 1234, dtype=torch.int64, device="cuda")
    plain, penalized, _ = entries(K.LIB_PATH)
    stream = torch.cuda.current_stream().cuda_stream
    keep = []  # the host arrays and structs the prepared calls point at

    def ints(vals):
        keep.append((ctypes.c_int * len(vals))(*vals))
        return keep[-1]

    def pen_struct(hist, n, values):
        keep.append(K.Penalties(*values, None if hist is None else hist.data_ptr(), 1024, B, None,
                                ctypes.cast(ints([n // 2] * B), ctypes.c_void_p)))
        return ctypes.byref(keep[-1])
    out = {}
    for mode, (t, k, p) in MODES.items():
        def head(n):  # gpt2mi_sample_ragged's arguments up to probs_out, every row at position n
            return (logits.data_ptr(), ldl, B, V, t, k or 0, 1.0 if p is None else p, 0, ints([n] * B), None, -1, None,
                    tok.data_ptr(), None, 0, None)
        arms = {"plain": prepared(plain, *head(1023), stream),
                "neutral": prepared(penalized, *head(1023), pen_struct(None, 0, (1.0, 0.0, 0.0)), None, stream)}
        if parent:
            arms["parent_plain"] = prepared(parent, *head(1023), stream)
        for n in HIST_LENS:
            for name, hist in (("distinct", distinct), ("equal", equal)):
                arms[f"penalised_{name}_{n}"] = prepared(penalized, *head(n), pen_struct(hist, n, PEN.values()), None,
                                                         stream)
        us = {a: [] for a in arms}
        issue = {a: [] for a in arms}
        for r in range(rounds + 1):  # round 0 warms the arms up
            for a, launch in arms.items():
                u, h = timed(launch, launches)
                if r:
                    us[a].append(u)
                    issue[a].append(h)
        out[mode] = {"us_per_launch": {a: statistics.median(v) for a, v in us.items()}, "rounds_us": us,
                     "issue_us_per_launch": {a: statistics.median(v) for a, v in issue.items()},
                     # the largest distance of a round from its arm's median, over the plain arms: the spread a
                     # difference between them has to exceed to mean anything
                     "plain_round_spread": max(abs(x - statistics.median(us[a])) / statistics.median(us[a])
                                               for a in us if "plain" in a or a == "neutral" for x in us[a])}
    return out


def loop_arm(model, prompt, n_new, pen, seed):
    B, P = prompt.shape
    sess = model.decoder(B, P + n_new)
    sess.prefill(prompt)
    seq = torch.empty(B, P + n_new, dtype=torch.int64, device=prompt.device)
    seq[:, :P] = prompt
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess.generate(n_new, 0.8, 50, 0.95, seed, seq=seq, gen_start=[P] * B if pen else None, **pen)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n_new * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default="profiles/decode/penalty_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("penalty_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    parent, _, parent_abi = entries(a.parent_lib) if a.parent_lib else (None, None, None)
    res = {"model": a.model, "prompt": a.prompt, "new_tokens": a.new, "rounds": a.rounds, "launches": a.launches,
           "device": torch.cuda.get_device_name(0), "penalties": PEN, "loop_penalties": LOOP_PEN,
           "parent_lib_abi": parent_abi, "kernel_alone": [], "loops": []}
    V, ldl = cfg.vocab_size, model.vpad
    for B in (1, 64):
        row = {"B": B, "V": V, "ldl": ldl, **kernel_alone(B, V, ldl, a.launches, a.rounds, parent)}
        print(json.dumps(row), flush=True)
        res["kernel_alone"].append(row)
    for B in [int(b) for b in a.batches.split(",")]:
        prompt = torch.randint(0, cfg.vocab_size, (B, a.prompt), generator=torch.Generator().manual_seed(B)).cuda()
        times = {"plain": [], "penalised": []}
        for r in range(a.rounds + 1):
            for arm, pen in (("plain", {}), ("penalised", LOOP_PEN)):
                ms = loop_arm(model, prompt, a.new, pen, seed=r)
                if r:
                    times[arm].append(ms)
        row = {"B": B, **{f"{arm}_ms_per_token": statistics.median(ts) for arm, ts in times.items()},
               **{f"{arm}_rounds_ms": ts for arm, ts in times.items()}}
        row["penalised_over_plain"] = row["penalised_ms_per_token"] / row["plain_ms_per_token"]
        print(json.dumps(row), flush=True)
        res["loops"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
