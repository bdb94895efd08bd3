"""Repetition, presence and frequency penalties on the MI355X: gpt2mi_sample_penalized against its executable
specification (generation.apply_penalties, then generation.sample_reference), and the penalised token loops.

logits_out must equal apply_penalties bit for bit (the rule is a handful of single fp32 operations, none contracted).
Tokens and probs_out are held to the exact cases of tests/test_sampling_gpu.py, with the margins computed on the penalised
fp32 logits of the reference, so the reference alone decides which seeds qualify. Everything about the loops is
bitwise: the device loop against a manual loop with the reference, generate_many against single-prompt runs, speculative
generation against the plain loop."""
import json
import subprocess
import sys

import pytest
import torch

from gpt_2_distributed_amd import _lib as K
from gpt_2_distributed_amd.generation import apply_penalties, sample_reference, uniform_at
from tests.conftest import REPO
from tests.test_sampling_gpu import MARGIN, TINY, make_logits, make_model, margins, padded

pytestmark = pytest.mark.gpu

dev = "cuda"
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2)
PEN_KW = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2)
TRAP, TRAP_LOGIT = 7, 1000.0   # a valid token that fills everything a row must not read; any penalty moves 1000 visibly
LD = 1032                       # the history buffers' row stride (>= the longest window, 1023)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- helpers -----------------------------------------------------------------------------------------------------------
def make_history(lens, V, seed, equal_rows=(), hot=None):
    """(hist int64 [2B, LD], hist_row, gen_start): row b's window is hist[hist_row[b], :lens[b]], hist_row a permutation of
    the odd rows; every even row and every position at or beyond a window holds TRAP. A window holds random tokens
    (never TRAP), one token R at every third position (repeated through the whole window), and, where it is long enough,
    a token and the same thread's token of the next chunk (t, t + 1024), V - 1, -1 and V. Rows in `equal_rows` hold one
    token throughout; `hot` [B, 2] are two more tokens per row (its most likely ones, so that the penalties decide what is
    kept), at positions 3 and 6. gen_start is the middle of the window, but 0 for rows b % 4 == 1 and lens for rows
    b % 4 == 2."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    hist = torch.full((2 * B, LD), TRAP, dtype=torch.int64)
    hist_row = [2 * ((b * 3 + 1) % B) + 1 for b in range(B)] if B % 3 else [2 * b + 1 for b in range(B)]
    assert sorted(hist_row) == list(range(1, 2 * B, 2))
    gen_start = []
    R, t0 = 11, 0
    for b, n in enumerate(lens):
        w = torch.randint(8, V, (n,), generator=g)          # (8..V-1: never TRAP)
        w[::3] = R
        plant = [(1, t0), (4, V - 1), (5, -1), (7, V), (8, t0)] + ([(2, t0 + 1024)] if t0 + 1024 < V else [])
        if hot is not None:
            plant += [(3, int(hot[b, 0])), (6, int(hot[b, 1]))]
        for at, tok in plant:
            if at < n:
                w[at] = tok
        if b in equal_rows:
            w[:] = V - 2
        hist[hist_row[b], :n] = w
        gen_start.append(0 if b % 4 == 1 else n if b % 4 == 2 else n // 2)
    return hist, hist_row, gen_start


def windows(hist, hist_row):
    """The rows' histories in batch order, [B, LD] (what apply_penalties takes)."""
    return hist[torch.tensor(hist_row)]


def penalized(buf, V, temperature, top_k, top_p, seed, pos, hist_dev, hist_row, gen_start, pen=PEN, row_id=None,
              want_probs=True, want_logits=True, seq_out=None):
    B = buf.size(0)
    tok = torch.full((B,), -7, dtype=torch.int64, device=dev)
    probs = torch.full((B, V), -1.0, device=dev) if want_probs else None
    out = torch.full((B, V), -1.0, device=dev) if want_logits else None
    K.sample_penalized(buf, V, temperature, top_k, top_p, seed, pos, tok, row_id=row_id, seq_out=seq_out,
                       probs_out=probs, hist=hist_dev, hist_row=hist_row, gen_start=gen_start, logits_out=out, **pen)
    torch.cuda.synchronize()
    return tok.cpu(), None if probs is None else probs.cpu(), None if out is None else out.cpu()


def row_uniforms(seed, pos):
    return torch.tensor([uniform_at(seed, b, p) for b, p in enumerate(pos)], dtype=torch.float64)


def pick_seed(lg, temperature, top_k, top_p, pos):
    """tests/test_sampling_gpu.py's pick_seed with a position per row."""
    for seed in range(40):
        d_u, d_p = margins(lg, temperature, top_k, top_p, row_uniforms(seed, pos))
        if d_u >= MARGIN and d_p >= MARGIN:
            return seed, d_u, d_p
    raise AssertionError("no seed in 0..39 keeps every row 1e-5 away from a boundary")


# ---- exact bits of the penalised logits --------------------------------------------------------------------------------
BIT_LENS = [0, 1, 63, 64, 65, 1023, 1023, 200]   # (row 6: one token throughout, c = 1023)


@pytest.mark.parametrize("pen", [PEN, dict(repetition=0.75, presence=-0.25, frequency=0.0),
                                 dict(repetition=1.0, presence=0.0, frequency=0.2)], ids=["all", "rp-pp", "fp"])
@pytest.mark.parametrize("V", [509, 1025, 2049, 50257])
def test_logits_out_has_the_bits_of_apply_penalties(V, pen):
    """Both kernels (greedy, sampled), one launch each. Every history sits among TRAP tokens (positions >= pos, the rows
    of other sequences): a block that read one of them would move logit TRAP, which must come out untouched."""
    B = len(BIT_LENS)
    lg = make_logits(B, V, seed=300 + V % 97)
    lg[:, TRAP] = TRAP_LOGIT
    lg[:, 11] = 1.0                 # R: counts of many sizes, among them those at which fp32(0.2) * c is inexact
    lg[:, 0] = 0.0                  # t: a logit of exactly 0 is divided
    lg[0::2, V - 1] = float("-inf")
    lg[1::2, V - 2] = -0.0
    hist, hist_row, gen_start = make_history(BIT_LENS, V, seed=V, equal_rows=(6,))
    want = apply_penalties(lg, windows(hist, hist_row), BIT_LENS, gen_start, pen["repetition"], pen["presence"],
                           pen["frequency"])
    assert not torch.equal(bits(want[2:]), bits(lg[2:]))
    assert torch.equal(bits(want[0]), bits(lg[0])) and bool((want[:, TRAP] == TRAP_LOGIT).all())
    buf = padded(lg, V + 7 if V == 509 else -(-V // 64) * 64)
    before = buf.clone()
    for temperature in (0.0, 0.8):
        _, _, got = penalized(buf, V, temperature, 8, None, 3, BIT_LENS, hist.to(dev), hist_row, gen_start, pen,
                              want_probs=False)
        diff = (bits(got) != bits(want)).nonzero()
        assert diff.numel() == 0, (temperature, diff[:8].tolist(), got[tuple(diff[0])], want[tuple(diff[0])])
        assert torch.equal(bits(buf), bits(before))          # the logits buffer is not modified


def test_the_product_is_not_contracted():
    """fp32(0.2) * 5 rounds to 1, the exact product lies above it: 1 - that is 0 in two roundings, -2^-26 fused."""
    V = 509
    lg = torch.zeros(1, V)
    lg[0, 33] = 1.0
    hist = torch.full((1, 16), 33, dtype=torch.int64)
    pen = dict(repetition=1.0, presence=0.0, frequency=0.2)
    want = apply_penalties(lg, hist, [5], [0], 1.0, 0.0, 0.2)
    assert float(want[0, 33]) == 0.0
    for temperature in (0.0, 1.0):
        _, _, got = penalized(lg.to(dev), V, temperature, None, None, 0, [5], hist.to(dev), [0], [0], pen,
                              want_probs=False)
        assert float(got[0, 33]) == 0.0 and torch.equal(bits(got), bits(want))


def test_a_history_at_the_cap():
    """pos = GPT2MI_PENALTY_MAX_HISTORY, one token throughout (the largest count a table entry holds) beside a row of
    distinct tokens; one past the cap is refused and raises."""
    V, cap = 509, K.PENALTY_MAX_HISTORY
    lg = make_logits(2, V, seed=5)
    hist = torch.stack([torch.full((cap + 8,), 77, dtype=torch.int64), torch.arange(cap + 8) % V])
    pos, gs = [cap, cap - 3], [0, 100]
    want = apply_penalties(lg, hist, pos, gs, **{k + "_penalty": v for k, v in PEN.items()})
    _, _, got = penalized(lg.to(dev), V, 0.0, None, None, 0, pos, hist.to(dev), [0, 1], gs, want_probs=False)
    assert torch.equal(bits(got), bits(want))
    with pytest.raises(K.KernelError, match="cap"):
        penalized(lg.to(dev), V, 0.0, None, None, 0, [cap + 1, 5], hist.to(dev), [0, 1], [0, 0], want_probs=False)


# ---- tokens and probabilities ------------------------------------------------------------------------------------------
def check_tokens(B, V, top_k, top_p, temperature=0.8):
    lens = [(37 * b + 5) % 300 for b in range(B)]            # per-row history lengths that differ (5, 42, 79, ...)
    lg = make_logits(B, V, seed=400 + B)
    hist, hist_row, gen_start = make_history(lens, V, seed=B + V, hot=lg.topk(2, dim=-1).indices)
    pen_lg = apply_penalties(lg, windows(hist, hist_row), lens, gen_start, *PEN.values())
    seed, d_u, d_p = pick_seed(pen_lg, temperature, top_k, top_p, lens)
    want_tok, want_probs = sample_reference(pen_lg, temperature, top_k, top_p, row_uniforms(seed, lens))
    tok, probs, _ = penalized(padded(lg, -(-V // 64) * 64), V, temperature, top_k, top_p, seed, lens, hist.to(dev),
                              hist_row, gen_start, want_logits=False)
    print(f"V={V} B={B} k={top_k} p={top_p}: seed {seed}, margins u {d_u:.2e} top_p {d_p:.2e}")
    assert torch.equal(tok, want_tok), (tok.tolist(), want_tok.tolist())
    big = want_probs >= 2e-38                                 # (as tests/test_sampling_gpu.py check_exact)
    assert bool((probs[big] > 0).all()) and bool((probs[want_probs == 0] == 0).all())
    assert bool((probs[~big] <= 4e-38).all())
    rel = (probs.double() - want_probs).abs()[big] / want_probs[big]
    assert float(rel.max()) <= 1e-5, float(rel.max())
    # the penalties decide something here: the plain sampler's distribution differs
    plain = sample_reference(lg, temperature, top_k, top_p, row_uniforms(seed, lens))[1]
    assert not torch.equal(plain, want_probs)


@pytest.mark.parametrize("top_p", [None, 0.9], ids=["p-off", "p0.9"])
@pytest.mark.parametrize("top_k", [8, 50])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_tokens_small_vocab(B, top_k, top_p):
    check_tokens(B, 509, top_k, top_p)


@pytest.mark.parametrize("B,top_k,top_p", [(1, 8, None), (3, 50, 0.9), (64, 8, 0.9), (64, 50, None)])
def test_tokens_gpt2_vocab(B, top_k, top_p):
    check_tokens(B, 50257, top_k, top_p)


def test_greedy_argmax_moves():
    """Row 0: A = 5 > B = 4, A in the history, 5 / 2 < 4: B. Row 1: all negative, A = -1 > B = -1.5, -1 * 2 < -1.5: B.
    Row 2: row 0's logits with A only at position pos, beyond its window: A stays. Row 3: A generated 3 times: B under
    repetition, and B under frequency and presence alone (5 - 0.2 * 3 - 0.5 < 4), which leave rows 0 and 1 at A (no
    generated A: gen_start at or past it)."""
    V, A, Bt = 2049, 1500, 40
    lg = torch.full((4, V), -9.0)
    lg[:, A], lg[:, Bt] = 5.0, 4.0
    lg[1, A], lg[1, Bt] = -1.0, -1.5
    hist = torch.full((4, 32), 3, dtype=torch.int64)
    hist[0, 2] = hist[1, 0] = hist[2, 10] = A
    hist[3, 4:7] = A
    pos, gs = [6, 6, 10, 9], [6, 0, 0, 2]
    pen = dict(repetition=2.0, presence=0.0, frequency=0.0)
    want = apply_penalties(lg, hist, pos, gs, 2.0, 0.0, 0.0)
    assert want.argmax(-1).tolist() == [Bt, Bt, A, Bt] and lg.argmax(-1).tolist() == [A] * 4
    tok, probs, got = penalized(lg.to(dev), V, 0.0, None, None, 0, pos, hist.to(dev), [0, 1, 2, 3], gs, pen)
    assert tok.tolist() == [Bt, Bt, A, Bt] and torch.equal(bits(got), bits(want))
    assert torch.equal(probs, torch.zeros(4, V).scatter_(1, tok[:, None], 1.0))
    plain = torch.empty(4, dtype=torch.int64, device=dev)
    K.sample_ragged(lg.to(dev), V, 0.0, None, None, 0, pos, plain)
    assert plain.tolist() == [A] * 4
    # presence and frequency alone: rows 0..2 have no generated A (gen_start at or past it, or A outside the window)
    pen = dict(repetition=1.0, presence=0.5, frequency=0.2)
    tok, _, _ = penalized(lg.to(dev), V, 0.0, None, None, 0, pos, hist.to(dev), [0, 1, 2, 3], [6, 1, 0, 2], pen)
    assert tok.tolist() == [A, A, A, Bt]


# ---- neutral values, determinism, the buffers it writes ----------------------------------------------------------------
@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_neutral_values_are_the_plain_sampler(temperature):
    V, B = 50257, 3
    lg = make_logits(B, V, seed=9)
    buf = padded(lg, 50432)
    pos = [4, 90, 17]
    tok = torch.full((B,), -7, dtype=torch.int64, device=dev)
    probs = torch.full((B, V), -1.0, device=dev)
    K.sample_ragged(buf, V, temperature, 50, 0.9, 5, pos, tok, probs_out=probs)
    neutral = dict(repetition=1.0, presence=0.0, frequency=0.0)
    got_tok, got_probs, got_lg = penalized(buf, V, temperature, 50, 0.9, 5, pos, None, None, None, neutral)
    assert torch.equal(got_tok, tok.cpu()) and torch.equal(bits(got_probs), bits(probs.cpu()))
    assert torch.equal(bits(got_lg), bits(lg))                # logits_out: the logits themselves
    # ... and with a history given, it is not read: one full of out-of-range values and TRAP changes nothing
    hist = torch.full((B, 128), 2 ** 40, dtype=torch.int64, device=dev)
    again, _, _ = penalized(buf, V, temperature, 50, 0.9, 5, pos, hist, None, None, neutral, want_logits=False)
    assert torch.equal(again, got_tok)


def test_two_penalised_runs_are_bit_identical_and_write_only_their_outputs():
    V, B = 50257, 5
    lens = [0, 300, 1023, 64, 9]
    lg = make_logits(B, V, seed=21)
    buf = padded(lg, 50432)
    before = buf.clone()
    hist, hist_row, gen_start = make_history(lens, V, seed=2, equal_rows=(2,))
    hist_dev = hist.to(dev)
    hist_before = hist_dev.clone()
    runs = [penalized(buf, V, 0.8, 50, 0.9, 4, lens, hist_dev, hist_row, gen_start) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b)
    assert torch.equal(bits(buf), bits(before)) and torch.equal(hist_dev, hist_before)
    # seq_out aliasing hist, as in the loop: row b writes hist[b, pos[b]] and nothing else (hist_row: the identity)
    own = hist_dev[torch.tensor(hist_row, device=dev)].contiguous()
    own_before = own.clone()
    tok, _, _ = penalized(buf, V, 0.8, 50, 0.9, 4, lens, own, None, gen_start, seq_out=own, want_probs=False,
                          want_logits=False)
    assert torch.equal(tok, runs[0][0])
    changed = (own != own_before).nonzero().tolist()
    assert own[torch.arange(B), torch.tensor(lens)].cpu().tolist() == tok.tolist()
    assert all(c == lens[r] for r, c in changed)


# ---- the loops on the tiny model ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    model = make_model()
    S = torch.randint(0, TINY["vocab_size"], (8, 150), generator=torch.Generator().manual_seed(17)).to(dev)
    return model, S


def test_device_loop_equals_a_manual_loop_with_the_reference(tiny):
    """prefill + (apply_penalties + sample_reference on the session's logits + step) per token, the exact-case margins
    checked on the CPU copy of every step's penalised logits; the seed is the first for which they hold at every step."""
    model, S = tiny
    prompt = S[:3, :5].contiguous()
    n, T, k, p = 24, 0.8, 50, 0.9
    P = prompt.size(1)
    for seed in range(20):
        sess = model.decoder(3, P + n)
        logits = sess.prefill(prompt)
        hist = torch.zeros(3, P + n, dtype=torch.int64)
        hist[:, :P] = prompt.cpu()
        ok = True
        for i in range(n):
            lg = apply_penalties(logits.cpu(), hist, [P + i] * 3, [P] * 3, **PEN_KW)
            u = torch.tensor([uniform_at(seed, b, P + i) for b in range(3)], dtype=torch.float64)
            d_u, d_p = margins(lg, T, k, p, u)
            if d_u < MARGIN or d_p < MARGIN:
                ok = False
                break
            hist[:, P + i] = sample_reference(lg, T, k, p, u)[0]
            if i + 1 < n:
                logits = sess.step(hist[:, P + i].to(dev))
        if ok:
            break
    assert ok, "no seed in 0..19 keeps every step 1e-5 away from a boundary"
    got = model.generate(prompt, n, temperature=T, top_k=k, top_p=p, seed=seed, **PEN_KW)
    assert torch.equal(got.cpu(), hist), (seed, got.tolist(), hist.tolist())
    assert not torch.equal(got, model.generate(prompt, n, temperature=T, top_k=k, top_p=p, seed=seed))
    # the session interface: sample(history=) + step, and generate() in two calls over the same buffer
    sess = model.decoder(3, P + n)
    sess.prefill(prompt)
    seq = torch.zeros(3, P + n, dtype=torch.int64, device=dev)
    seq[:, :P] = prompt
    first = sess.sample(T, k, p, seed, history=seq, gen_start=[P] * 3, **PEN_KW)
    assert torch.equal(first.cpu(), hist[:, P])
    seq[:, P] = first
    sess.step(first)
    sess.generate(9, T, k, p, seed, seq=seq, gen_start=[P] * 3, **PEN_KW)
    sess.generate(n - 10, T, k, p, seed, seq=seq, gen_start=[P] * 3, **PEN_KW)
    assert torch.equal(seq.cpu(), hist)
    fresh = model.decoder(3, P + n)
    fresh.prefill(prompt)
    with pytest.raises(ValueError, match="seq"):
        fresh.generate(1, T, k, p, seed, **PEN_KW)
    with pytest.raises(ValueError, match="history"):
        fresh.sample(T, k, p, seed, repetition_penalty=1.3)


def test_greedy_device_loop_equals_the_host_sampler_path(tiny):
    model, S = tiny
    prompt = S[:3, :9].contiguous()
    for kw in (dict(repetition_penalty=1.3), PEN_KW):
        want = model.generate(prompt, 40, temperature=0.0, **kw)
        got = model.generate(prompt, 40, temperature=0.0, seed=0, **kw)
        assert got.shape == (3, 49) and torch.equal(got, want), kw
    assert not torch.equal(got, model.generate(prompt, 40, temperature=0.0, seed=0))
    # ragged prompts and eos through both paths
    eos = int(got[1, 20])
    kw = dict(temperature=0.0, prompt_lens=[9, 3, 6], eos_token_id=eos, **PEN_KW)
    assert torch.equal(model.generate(prompt, 40, seed=0, **kw), model.generate(prompt, 40, **kw))


MANY_LENS = [1, 5, 33, 9, 30, 2, 17]


@pytest.mark.parametrize("sampler", ["greedy", "sampled"])
def test_generate_many_does_not_depend_on_the_batch(tiny, sampler):
    """Prompts of unequal length, more prompts than rows (refills): each output is the one-prompt run's."""
    model, S = tiny
    n = 40
    prompts = [S[i, :L].contiguous() for i, L in enumerate(MANY_LENS)]
    kw = dict(temperature=0.0) if sampler == "greedy" else dict(temperature=0.8, top_k=20, top_p=0.95)
    runs = [model.generate_many(prompts, n, batch_size=bs, seed=3, **kw, **PEN_KW) for bs in (2, 8)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    plain = model.generate_many(prompts, n, batch_size=8, seed=3, **kw)
    assert not all(torch.equal(a, b) for a, b in zip(runs[0], plain))
    for i, p in enumerate(prompts):
        if sampler == "greedy":
            one = model.generate(p[None], n, seed=3, **kw, **PEN_KW)[0]
        else:  # (generate draws row 0 with key 0: the session takes prompt i's key)
            sess = model.decoder(1, p.numel() + n)
            sess.prefill(p[None])
            seq = torch.zeros(1, p.numel() + n, dtype=torch.int64, device=dev)
            seq[0, :p.numel()] = p
            sess.generate(n, kw["temperature"], kw["top_k"], kw["top_p"], 3, seq=seq, row_id=[i],
                          gen_start=[p.numel()], **PEN_KW)
            one = seq[0]
        assert torch.equal(runs[0][i], one), (sampler, i)


SAMPLERS = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.8, top_k=50, top_p=0.95)}


@pytest.mark.parametrize("s", SAMPLERS)
def test_speculative_generation_stays_exact(tiny, s):
    from tests.test_speculative_gpu import scripted
    model, S = tiny
    n, lens = 40, [3, 17, 9]
    idx = S[:3, :17].contiguous()
    kw = dict(seed=1, prompt_lens=lens, **SAMPLERS[s], **PEN_KW)
    want = model.generate(idx, n, **kw)
    assert not torch.equal(want, model.generate(idx, n, seed=1, prompt_lens=lens, **SAMPLERS[s]))
    rows = [row[:lens[i] + n] for i, row in enumerate(want.tolist())]
    for draft in ("right", "wrong", None):
        fn = None if draft is None else scripted(draft, rows)
        got = model.generate(idx, n, draft_tokens=3, draft_fn=fn, **kw)
        assert torch.equal(got, want), (s, draft)
    eos = int(want[0, lens[0] + 9])
    want = model.generate(idx, n, eos_token_id=eos, **kw)
    assert torch.equal(model.generate(idx, n, eos_token_id=eos, draft_tokens=3, **kw), want)


def test_cli_takes_the_penalties(tmp_path):
    from gpt_2_distributed_amd.train_gpt2_distributed import save_checkpoint
    model = make_model()
    ckpt = save_checkpoint(model, model.configure_optimizers(), 3, str(tmp_path))
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.generate", "--checkpoint", ckpt, "--model", "auto",
           "--prompt_ids", "11,12,13", "--max_new_tokens", "24", "--batch", "2", "--temperature", "0.8", "--seed", "5",
           "--sampler", "device", "--top_p", "0.9", "--repetition_penalty", "1.3", "--presence_penalty", "0.5",
           "--frequency_penalty", "0.2"]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("[")]
    idx = torch.tensor([[11, 12, 13]] * 2, device=dev)
    assert rows == model.generate(idx, 24, temperature=0.8, top_p=0.9, seed=5, **PEN_KW).tolist()
    assert rows != model.generate(idx, 24, temperature=0.8, top_p=0.9, seed=5).tolist()
