"""What the sampler's constraints cost: gpt2mi_sample_constrained alone and inside the device loop, on one MI355X.

The protocol of tools/penalty_bench.py: ONE process, the arms interleaved round by round after a warm-up round of each,
the median of 3 rounds reported with every round beside it.

Kernel alone: HIP events around 200 back-to-back launches at V = 50257 (ldl 50432), B = 1 / 8 / 64, position 1023, for
"top_k 50 + top_p 0.95" (temperature 0.8) and greedy. Arms: `plain` (gpt2mi_sample_ragged), `neutral`
(gpt2mi_sample_constrained with nothing on: the same kernels), `bias` (one shared fp32 row), `min_p` (0.05), `stop` (8
sequences of 16 tokens beside a history of 1023, none of which matches) and `all` (those, min_new 2048 and
the penalties 1.3 / 0.5 / 0.2 of tools/penalty_bench.py beside them: `penalised` is that arm without the constraints).
The launches are issued from Python through ctypes with every argument built beforehand, so a figure is an upper bound on
the kernel's time: `issue_us_per_launch`, the host time per call, is the floor a figure cannot go below.

Device loop: ms per token of DecodeSession.generate, GPT-2 124M, a random prompt of 512 tokens, 128 new tokens, B = 1 / 8
/ 64, sampling (0.8, top_k 50, top_p 0.95), without and with logit_bias, min_p = 0.05, min_new_tokens = 64 and 8 stop
sequences (of tokens the bias bans, so that no row ends early).

    python tools/constraint_bench.py --out profiles/decode/constraint_bench.json
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
from tools.penalty_bench import MODES, PEN, prepared, timed  # noqa: E402

POS, EOS, BANNED = 1023, 50256, 777
STOPS = [[BANNED + s] * 15 + [BANNED] for s in range(K.STOP_MAX_SEQS)]


def kernel_alone(B, V, ldl, launches, rounds):
    lib = K.load()
    logits = torch.randn(B, ldl, generator=torch.Generator().manual_seed(B)).cuda() * 3
    tok = torch.empty(B, dtype=torch.int64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(1)
    hist = torch.stack([torch.randperm(V, generator=g)[:1024] for _ in range(B)]).cuda()
    bias = (torch.randn(1, V, generator=g) * 0.5).cuda()
    bias[0, BANNED] = float("-inf")  # (the stop sequences' last token: the done flags stay 0 from launch to launch)
    stream = torch.cuda.current_stream().cuda_stream
    keep = []  # the host arrays and structs the prepared calls point at

    def ints(vals, ctype=ctypes.c_int):
        keep.append((ctype * len(vals))(*vals))
        return keep[-1]

    def pen_struct(values):
        keep.append(K.Penalties(*values, hist.data_ptr(), 1024, B, None, ctypes.cast(ints([POS // 2] * B), ctypes.c_void_p)))
        return ctypes.byref(keep[-1])

    def con_struct(with_bias=False, min_p=0.0, min_new=0, stops=()):
        table = ints([t for s in stops for t in s], ctypes.c_int32) if stops else None
        lens = ints([len(s) for s in stops]) if stops else None
        keep.append(K.Constraints(bias.data_ptr() if with_bias else None, V, 1,
                                  ctypes.cast(ints([0] * B), ctypes.c_void_p) if with_bias else None, min_p, min_new,
                                  len(stops), ctypes.cast(table, ctypes.c_void_p) if stops else None,
                                  ctypes.cast(lens, ctypes.c_void_p) if stops else None))
        return ctypes.byref(keep[-1])
    out = {}
    for mode, (t, k, p) in MODES.items():
        head = (logits.data_ptr(), ldl, B, V, t, k or 0, 1.0 if p is None else p, 0, ints([POS] * B), None, EOS,
                done.data_ptr(), tok.data_ptr(), None, 0, None)
        off, on = pen_struct((1.0, 0.0, 0.0)), pen_struct(PEN.values())

        def con_arm(pen, con):
            return prepared(lib.gpt2mi_sample_constrained, *head, pen, None, None, con, stream)
        arms = {"plain": prepared(lib.gpt2mi_sample_ragged, *head, stream),
                "neutral": con_arm(off, con_struct()),
                "bias": con_arm(off, con_struct(with_bias=True)),
                "min_p": con_arm(off, con_struct(min_p=0.05)),
                "stop": con_arm(off, con_struct(stops=STOPS)),
                "penalised": con_arm(on, con_struct()),
                "all": con_arm(on, con_struct(True, 0.05, 2048, STOPS))}
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
                     "over_plain": {a: med[a] / med["plain"] for a in med},
                     "plain_round_spread": max(abs(x - med[a]) / med[a] for a in ("plain", "neutral") for x in us[a])}
        assert int(done.sum()) == 0
    return out


def loop_arm(model, prompt, n_new, con, seed):
    B, P = prompt.shape
    sess = model.decoder(B, P + n_new)
    sess.prefill(prompt)
    seq = torch.empty(B, P + n_new, dtype=torch.int64, device=prompt.device)
    seq[:, :P] = prompt
    done = torch.zeros(B, dtype=torch.uint8, device=prompt.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess.generate(n_new, 0.8, 50, 0.95, seed, EOS, seq, done, gen_start=[P] * B if con else None, **con)
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
    ap.add_argument("--out", default="profiles/decode/constraint_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("constraint_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    batches = [int(b) for b in a.batches.split(",")]
    res = {"model": a.model, "prompt": a.prompt, "new_tokens": a.new, "rounds": a.rounds, "launches": a.launches,
           "device": torch.cuda.get_device_name(0), "penalties": PEN, "kernel_alone": [], "loops": []}
    V, ldl = cfg.vocab_size, model.vpad
    for B in batches:
        row = {"B": B, "V": V, "ldl": ldl, **kernel_alone(B, V, ldl, a.launches, a.rounds)}
        print(json.dumps(row), flush=True)
        res["kernel_alone"].append(row)
    bias = torch.zeros(1, V, device="cuda")
    bias[0, BANNED], bias[0, 198] = float("-inf"), 2.5
    for B in batches:
        prompt = torch.randint(0, V, (B, a.prompt), generator=torch.Generator().manual_seed(B)).cuda()
        con = dict(logit_bias=bias, bias_row=[0] * B, min_p=0.05, min_new_tokens=a.new // 2, stop=STOPS)
        times = {"plain": [], "constrained": []}
        for r in range(a.rounds + 1):
            for arm, kw in (("plain", {}), ("constrained", con)):
                ms = loop_arm(model, prompt, a.new, kw, seed=r)
                if r:
                    times[arm].append(ms)
        row = {"B": B, **{f"{arm}_ms_per_token": statistics.median(ts) for arm, ts in times.items()},
               **{f"{arm}_rounds_ms": ts for arm, ts in times.items()}}
        row["constrained_over_plain"] = row["constrained_ms_per_token"] / row["plain_ms_per_token"]
        print(json.dumps(row), flush=True)
        res["loops"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
