"""Speculative generation against the plain device loop, and the cost of a verify call, GPT-2 124M on one MI355X.

The protocol of tools/sample_bench.py: random weights, a random prompt of 512 tokens, 128 new tokens, B = 1 and 4; the
arms run in ONE process, interleaved round by round after a warm-up round of each; an arm's time is a host clock around
its 128 tokens (prefill outside) ending in one device synchronise; the median of 3 rounds is reported with every round
beside it. Sampling at temperature 0.8, top_k 50, top_p 0.95.
  plain        DecodeSession.generate: one gpt2mi_decode_generate_ragged call, nothing read back.
  k / right    DecodeSession.speculate with k = 2, 4, 7 drafts that are always right (the continuation recorded from the
               plain arm), so every verify call yields k + 1 tokens;
  k / wrong    ... never right (every call yields 1 token: the whole cost of verifying, none of the gain);
  k / half     ... right at every other call of the draft function.
  k / ngram    ngram_draft on a prompt made of a repeated 32-token block, against the plain loop on that prompt.
Every speculative arm's tokens are compared with its plain arm's (`tokens_equal`).

Separately, one call alone: HIP events around back-to-back gpt2mi_decode_extend calls over R = 1, 2, 3, 5, 8, 16, 64 rows of
one sequence at positions 512.., as tools/lib_ab.py times gpt2mi_decode_step, with gpt2mi_decode_step_ragged at B = 1 (and
at B = R sequences) beside it. From those, as a DERIVATION: the mean number of accepted drafts per call from which a
verify call of k + 1 rows beats k + 1 plain steps, A* = extend_us(k + 1) / step_us(1) - 1, and A* / k as a rate. The
same from the loops, which include the sampler, the read-back and the host's bookkeeping: the `wrong` arm's time per call
over the plain arm's time per token, minus 1.

    python tools/spec_bench.py --out profiles/decode/spec_bench.json
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
from gpt_2_distributed_amd.generation import ngram_draft  # noqa: E402
from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES  # noqa: E402

MODE = dict(temperature=0.8, top_k=50, top_p=0.95)
KS = (2, 4, 7)
ROWS = (1, 2, 3, 5, 8, 16, 64)


def session(model, prompt, n_new):
    B, P = prompt.shape
    sess = model.decoder(B, P + n_new)
    sess.prefill(prompt)
    seq = torch.zeros(B, P + n_new, dtype=torch.int64, device=prompt.device)
    seq[:, :P] = prompt
    torch.cuda.synchronize()
    return sess, seq


def plain_arm(model, prompt, n_new, seed):
    sess, seq = session(model, prompt, n_new)
    t0 = time.perf_counter()
    sess.generate(n_new, MODE["temperature"], MODE["top_k"], MODE["top_p"], seed, seq=seq)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, seq


def spec_arm(model, prompt, n_new, seed, k, draft_fn):
    sess, seq = session(model, prompt, n_new)
    t0 = time.perf_counter()
    stats = sess.speculate(n_new, k, draft_fn, MODE["temperature"], MODE["top_k"], MODE["top_p"], seed, seq=seq)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, seq, stats


def scripted(kind, rows, V):
    """draft_fn over the recorded rows: right always, never, or at every other call."""
    calls = [0]

    def fn(history, m):
        calls[0] += 1
        n = len(history)
        row = next(r for r in rows if r[n - 1] == history[-1] and r[:n] == history)
        out = row[n:n + m]
        if kind == "wrong" or (kind == "half" and calls[0] % 2 == 0):
            out = [(t + 1) % V for t in out]
        return out
    return fn


def loops(model, cfg, B, a):
    g = torch.Generator().manual_seed(B)
    prompts = {"random": torch.randint(0, cfg.vocab_size, (B, a.prompt), generator=g).cuda(),
               "repeated32": torch.randint(0, cfg.vocab_size, (B, 32), generator=g).repeat(1, a.prompt // 32).cuda()}
    arms = [("random", k, kind) for k in KS for kind in ("right", "wrong", "half")] + [("repeated32", k, "ngram") for k in KS]
    times = {arm: [] for arm in arms}
    times.update({(p, 0, "plain"): [] for p in prompts})
    last, equal = {}, {}
    for r in range(a.rounds + 1):  # round 0 warms the arms up
        plain = {}
        for p, prompt in prompts.items():
            t, plain[p] = plain_arm(model, prompt, a.new, seed=r)
            if r:
                times[(p, 0, "plain")].append(t / a.new * 1e3)
        for arm in arms:
            p, k, kind = arm
            fn = ngram_draft if kind == "ngram" else scripted(kind, plain[p].tolist(), cfg.vocab_size)
            t, seq, stats = spec_arm(model, prompts[p], a.new, r, k, fn)
            equal[arm] = equal.get(arm, True) and bool(torch.equal(seq, plain[p]))
            last[arm] = stats
            if r:
                times[arm].append(t / a.new * 1e3)
    rows = []
    for (p, k, kind), ts in times.items():
        row = {"B": B, "prompt": p, "k": k, "drafts": kind, "ms_per_token": statistics.median(ts), "rounds_ms": ts}
        if kind != "plain":
            base = statistics.median(times[(p, 0, "plain")])
            st = last[(p, k, kind)]
            row.update(tokens_equal=equal[(p, k, kind)], speedup_over_plain=base / row["ms_per_token"], **st,
                       ms_per_call=row["ms_per_token"] * a.new / max(st["calls"], 1),
                       accepted_per_call=st["accepted"] / max(st["calls"], 1))
            if kind == "wrong":  # every call yields one token: its time per call over the plain time per token
                row["loop_break_even_accepted_per_call"] = row["ms_per_call"] / base - 1
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def timed(call, rounds=5, reps=20):
    """us per call: HIP events around `reps` back-to-back calls, the median of `rounds` after a warm-up round."""
    out = []
    for r in range(rounds + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            call()
        e.record()
        torch.cuda.synchronize()
        if r:
            out.append(s.elapsed_time(e) / reps * 1e3)
    return statistics.median(out)


def calls_alone(model, cfg, pos0, tcap):
    """gpt2mi_decode_extend over R rows of one sequence at pos0.., gpt2mi_decode_step_ragged at B = 1 and at B = R."""
    one = model.decoder(1, tcap)
    one._ready(True)
    scratch, plan = one._rows_plan()
    g = torch.Generator().manual_seed(0)
    rows = []
    step1 = None
    for R in ROWS:
        tok = torch.randint(0, cfg.vocab_size, (R,), generator=g).cuda()
        seq, pos = [0] * R, list(range(pos0, pos0 + R))
        ext = timed(lambda: K.decode_extend(plan, tok, seq, pos))
        many = model.decoder(R, tcap)
        step = timed(lambda: K.decode_step_ragged(many._plan, tok, [pos0] * R))
        step1 = step if R == 1 else step1
        row = {"R": R, "pos0": pos0, "decode_extend_us": ext, "decode_step_ragged_B=R_us": step,
               "decode_step_ragged_B=1_us": step1, "extend_over_one_step": ext / step1}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del many
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES))
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/decode/spec_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spec_bench needs the MI355X: there is no CPU measurement of a GPU rate")
    cfg = GPT2Config(**MODEL_SIZES[a.model])
    model = GPT2(cfg).to("cuda:0").eval()
    res = {"model": a.model, "prompt": a.prompt, "new_tokens": a.new, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "mode": MODE, "loops": [], "calls_alone": []}
    for B in [int(b) for b in a.batches.split(",")]:
        res["loops"] += loops(model, cfg, B, a)
    res["calls_alone"] = calls_alone(model, cfg, a.prompt, a.prompt + a.new)
    by_rows = {r["R"]: r for r in res["calls_alone"]}
    # a derivation from the figures above, not a measurement: a call of k + 1 rows yields 1 + A tokens
    res["break_even"] = [{"k": k, "rows": k + 1, "accepted_per_call": by_rows[k + 1]["extend_over_one_step"] - 1,
                          "acceptance_rate": (by_rows[k + 1]["extend_over_one_step"] - 1) / k}
                         for k in KS if k + 1 in by_rows]
    print(json.dumps(res["break_even"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
