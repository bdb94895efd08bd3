"""The sampling tail of a decode step: the host-driven PyTorch loop against the device loop, GPT-2 124M on one MI355X.

The protocol of tools/decode_bench.py: a random prompt of 512 tokens, 128 new tokens, B = 1, 8, 64; the arms run in ONE
process, interleaved round by round after a warm-up round of each; an arm's time is a host clock around its 128 tokens
(prefill outside) ending in one device synchronise; the median of 3 rounds is reported with every round beside it.
  torch    the loop of GPT2.generate without a seed: DecodeSession.step (which clones the logits) + sample_next in
           PyTorch per token, the tokens collected in a list and concatenated.
  device   the loop with a seed: one gpt2mi_decode_generate call (gpt2mi_sample + gpt2mi_decode_step per token, issued
           from C into one [B, P + n] buffer), nothing read back.
Each arm greedy (temperature 0) and sampling (temperature 0.8, top_k 50, top_p 0.95).

Separately, gpt2mi_sample alone: HIP events around 200 back-to-back launches at B = 1 and 64, V = 50257 (ldl 50432),
for five settings: greedy, temperature only, top-k 50, top-p 0.95 without top-k (the longest search), and top-k 50 +
top-p 0.95. The launches are issued from Python through ctypes, so a figure is an UPPER BOUND on the kernel's time that
includes the issue of a launch: `issue_us_per_launch`, the host time per call of the same loop measured beside it, says
how near a figure is to that floor (a figure at the floor measures the issue rate, not the kernel). Beside it, as a
DERIVATION and not a target: the time to read one 200 KB row per workgroup at the 6.29 TB/s device-to-device copy rate.

    python tools/sample_bench.py --out profiles/decode/sample_bench.json
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
from gpt_2_distributed_amd import _lib as K  # noqa: E402
from gpt_2_distributed_amd.generation import sample_next  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s, measured device-to-device copy rate (MI355X_MICROARCH.md)
MODES = {"greedy": dict(temperature=0.0, top_k=None, top_p=None),
         "sample": dict(temperature=0.8, top_k=50, top_p=0.95)}


def torch_arm(model, prompt, n_new, mode, seed):
    sess = model.decoder(prompt.size(0), prompt.size(1) + n_new)
    logits = sess.prefill(prompt)
    gen = torch.Generator(device=prompt.device).manual_seed(seed)
    out = [prompt]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_new):
        nxt = sample_next(logits, mode["temperature"], mode["top_k"], gen, mode["top_p"])
        out.append(nxt[:, None])
        if i + 1 < n_new:
            logits = sess.step(nxt)
    seq = torch.cat(out, dim=1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, seq


def device_arm(model, prompt, n_new, mode, seed):
    B, P = prompt.shape
    sess = model.decoder(B, P + n_new)
    sess.prefill(prompt)
    seq = torch.empty(B, P + n_new, dtype=torch.int64, device=prompt.device)
    seq[:, :P] = prompt
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess.generate(n_new, mode["temperature"], mode["top_k"], mode["top_p"], seed, seq=seq)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, seq


def kernel_alone(B, V, ldl, launches):
    logits = torch.randn(B, ldl, generator=torch.Generator().manual_seed(B)).cuda() * 3
    tok = torch.empty(B, dtype=torch.int64, device="cuda")
    rows, issued = {}, {}
    for name, (t, k, p) in {"greedy": (0.0, None, None), "top_k50_top_p0.95": (0.8, 50, 0.95),
                            "top_p0.95": (0.8, None, 0.95), "top_k50": (0.8, 50, None),
                            "temperature_only": (0.8, None, None)}.items():
        for _ in range(10):
            K.sample(logits, V, t, k, p, 0, 0, tok)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        h0 = time.perf_counter()
        for i in range(launches):
            K.sample(logits, V, t, k, p, 0, i, tok)
        issue = time.perf_counter() - h0  # host time to issue the launches (they run behind it)
        end.record()
        torch.cuda.synchronize()
        rows[name] = start.elapsed_time(end) / launches * 1e3  # us per launch between the events
        issued[name] = issue / launches * 1e6
    return rows, issued


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default="profiles/decode/sample_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    res = {"model": a.model, "prompt": a.prompt, "new_tokens": a.new, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "modes": MODES, "loops": [], "kernel_alone": []}
    for B in [int(b) for b in a.batches.split(",")]:
        prompt = torch.randint(0, cfg.vocab_size, (B, a.prompt), generator=torch.Generator().manual_seed(B)).cuda()
        times = {(arm, mode): [] for arm in ("torch", "device") for mode in MODES}
        greedy_equal = None
        for r in range(a.rounds + 1):  # round 0 warms the arms up
            for mode, kw in MODES.items():
                tt, seq_t = torch_arm(model, prompt, a.new, kw, seed=r)
                td, seq_d = device_arm(model, prompt, a.new, kw, seed=r)
                if r:
                    times[("torch", mode)].append(tt / a.new * 1e3)
                    times[("device", mode)].append(td / a.new * 1e3)
                if mode == "greedy":
                    greedy_equal = bool(torch.equal(seq_t, seq_d))
        row = {"B": B, "greedy_tokens_equal": greedy_equal}
        for (arm, mode), ts in times.items():
            row[f"{arm}_{mode}_ms_per_token"] = statistics.median(ts)
            row[f"{arm}_{mode}_rounds_ms"] = ts
        for mode in MODES:
            row[f"{mode}_torch_over_device"] = row[f"torch_{mode}_ms_per_token"] / row[f"device_{mode}_ms_per_token"]
        print(json.dumps(row), flush=True)
        res["loops"].append(row)
    V, ldl = cfg.vocab_size, model.vpad
    for B in (1, 64):
        per_launch, issued = kernel_alone(B, V, ldl, a.launches)
        row = {"B": B, "V": V, "ldl": ldl, "launches": a.launches, "us_per_launch": per_launch,
               "issue_us_per_launch": issued,
               # a derivation, not a measurement: B rows of V fp32 at the device-to-device copy rate
               "derived_row_read_us_at_copy_rate": B * V * 4 / COPY_RATE * 1e6}
        print(json.dumps(row), flush=True)
        res["kernel_alone"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
