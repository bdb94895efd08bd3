"""Logit bias, min-p, minimum length and stop sequences on the MI355X: gpt2mi_sample_constrained against its executable
specification (generation.apply_penalties, apply_constraints, sample_reference with min_p, stop_match).

logits_out must equal apply_constraints(apply_penalties(...)) bit for bit and the min-p kept set is exact (one fp32 add
and compares). Tokens and probs_out are held to the exact cases of tests/test_sampling_gpu.py, the margins computed on the
reference's constrained fp32 logits, so the reference alone decides which seeds qualify."""
import numpy as np
import pytest
import torch

from gpt_2_distributed_amd import _lib as K
from gpt_2_distributed_amd.generation import (apply_constraints, apply_penalties, log_min_p, sample_reference, stop_match,
                                              token_logprobs)
from tests.test_penalties_gpu import PEN, TRAP, TRAP_LOGIT, make_history, row_uniforms, windows
from tests.test_sampling_gpu import MARGIN, exclusive_mass, make_logits, padded

pytestmark = pytest.mark.gpu

dev = "cuda"
INF = float("inf")
NEUTRAL = dict(repetition=1.0, presence=0.0, frequency=0.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.contiguous().view(torch.int32)


def constrained(buf, V, temperature, top_k, top_p, seed, pos, hist=None, hist_row=None, gen_start=None, pen=NEUTRAL,
                eos=None, done=None, lp=None, want_probs=True, want_logits=True, seq_out=None, row_id=None, **con):
    """One gpt2mi_sample_constrained call; everything it writes, on the CPU: (tok, probs, logits_out, done, lp values)."""
    B = buf.size(0)
    tok = torch.full((B,), -7, dtype=torch.int64, device=dev)
    probs = torch.full((B, V), -1.0, device=dev) if want_probs else None
    out = torch.full((B, V), -1.0, device=dev) if want_logits else None
    done_d = None if done is None else torch.tensor(done, dtype=torch.uint8, device=dev)
    lpk = {}
    if lp is not None:
        lpk = dict(logprob=torch.full((B, 1), -3.0, device=dev), col=[0] * B,
                   top_ids=torch.full((B, 1, lp), -3, dtype=torch.int32, device=dev) if lp else None,
                   top_logprobs=torch.full((B, 1, lp), -3.0, device=dev) if lp else None)
    if "logit_bias" in con and con["logit_bias"] is not None:
        con["logit_bias"] = con["logit_bias"].to(dev)
    K.sample_constrained(buf, V, temperature, top_k, top_p, seed, pos, tok, row_id=row_id, eos=eos, done=done_d,
                         seq_out=seq_out, probs_out=probs, hist=None if hist is None else hist.to(dev), hist_row=hist_row,
                         gen_start=gen_start, logits_out=out, **pen, **lpk, **con)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
    return (tok.cpu(), cpu(probs), cpu(out), cpu(done_d),
            None if lp is None else tuple(cpu(lpk[k]) for k in ("logprob", "top_ids", "top_logprobs")))


# ---- exact bits of the dumped row -----------------------------------------------------------------------------------------
BIT_LENS = [0, 1, 63, 64, 65, 1023]
EOS = 21


def make_bias(V, seed):
    """Three bias rows: -inf on two tokens, -0.0 on two (one of them a logit of +0.0), a value on the token the history
    repeats (11: a penalised token) and on TRAP, random elsewhere in row 1, zero elsewhere in rows 0 and 2."""
    g = torch.Generator().manual_seed(seed)
    bias = torch.zeros(3, V)
    bias[1] = torch.randn(V, generator=g)
    bias[:, 11] = torch.tensor([0.7, -1.3, 2.5])
    bias[:, 5], bias[:, V - 1] = -INF, -INF
    bias[:, 0], bias[:, 9] = -0.0, -0.0
    bias[1, TRAP], bias[2, TRAP] = 0.0, 1.0
    return bias


@pytest.mark.parametrize("pen", [PEN, NEUTRAL], ids=["penalised", "unpenalised"])
@pytest.mark.parametrize("V", [509, 1025, 2049, 50257])
def test_logits_out_has_the_bits_of_the_rule(V, pen):
    """Both kernel forms, one launch each: rows with no bias row, rows sharing one and rows with their own; the eos held
    back in the rows below min_new; every history among TRAP tokens (tests/test_penalties_gpu.py: a block that read one
    would move logit TRAP). The logits buffer is not modified."""
    B = len(BIT_LENS)
    lg = make_logits(B, V, seed=700 + V % 97)
    lg[:, TRAP] = TRAP_LOGIT
    lg[:, 11], lg[:, 0], lg[:, 9] = 1.0, 0.0, 3.0
    lg[0::2, V - 2] = -INF
    hist, hist_row, gen_start = make_history(BIT_LENS, V, seed=V)
    bias, bias_row = make_bias(V, V), [-1, 0, 0, 1, 2, -1]
    min_new = 30  # pos - gen_start: 0, 1, 0 (b % 4 == 2: gen_start = lens), 32, 33, 1023 (b % 4 == 1: gen_start = 0)
    held = [p - g < min_new for p, g in zip(BIT_LENS, gen_start)]
    assert held == [True, True, True, False, False, False]
    want = apply_constraints(apply_penalties(lg, windows(hist, hist_row), BIT_LENS, gen_start, *pen.values()), BIT_LENS,
                             gen_start, bias, bias_row, min_new, EOS)
    assert torch.equal(bits(want[5]), bits(apply_penalties(lg, windows(hist, hist_row), BIT_LENS, gen_start,
                                                           *pen.values())[5]))
    assert bool((want[:3, EOS] == -INF).all()) and bool((want[3:, EOS] > -INF).all())
    assert bool((want[[0, 1, 2, 3, 5], TRAP] == TRAP_LOGIT).all()) and float(want[4, TRAP]) == TRAP_LOGIT + 1.0
    buf = padded(lg, V + 7 if V == 509 else -(-V // 64) * 64)
    before = buf.clone()
    for temperature in (0.0, 0.8):
        _, _, got, _, _ = constrained(buf, V, temperature, 8, None, 3, BIT_LENS, hist, hist_row, gen_start, pen, eos=EOS,
                                      want_probs=False, logit_bias=bias, bias_row=bias_row, min_new_tokens=min_new)
        diff = (bits(got) != bits(want)).nonzero()
        assert diff.numel() == 0, (temperature, diff[:8].tolist(), got[tuple(diff[0])], want[tuple(diff[0])])
        assert torch.equal(bits(buf), bits(before))


def margins_min_p(lg, temperature, top_k, top_p, u, min_p):
    """tests/test_sampling_gpu.py's margins with the min-p rule in the reference's CDF (the top-p search is what it was:
    it runs before min-p, on the same values; the min-p comparison itself is exact)."""
    _, probs = sample_reference(lg, temperature, top_k, top_p, u, min_p=min_p)
    cdf = probs.cumsum(-1)[:, :-1]
    d = (cdf - u[:, None]).abs() + (probs[:, :-1] == 0) * 1.0
    d_p = float("inf")
    if top_p is not None and top_p < 1:
        d_p = float((exclusive_mass(lg, temperature, top_k)[1] - top_p).abs().min())
    return float(d.min()), d_p


# ---- the min-p kept set, exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k,top_p", [(None, None), (40, 0.999)], ids=["alone", "with-k-p"])
@pytest.mark.parametrize("V", [509, 50257])
def test_min_p_keeps_the_logit_at_the_threshold_and_drops_the_one_below(V, top_k, top_p):
    """Temperature 1, maximum 0: a logit of exactly lmp is kept, nextafter(lmp, -inf) is dropped."""
    mp = 0.01
    lmp = np.float32(log_min_p(mp))
    below = float(np.nextafter(lmp, np.float32(-INF)))
    lg = torch.full((2, V), -30.0)
    lg[:, 100] = 0.0
    lg[0, [3, V - 1]], lg[0, [4, 1030 % V]] = float(lmp), below
    lg[1, 7], lg[1, 8], lg[1, 200:210] = below, float(lmp), -1.0
    seed = next(s for s in range(40) if min(margins_min_p(lg, 1.0, top_k, top_p, row_uniforms(s, [9, 9]), mp)) >= MARGIN)
    want_tok, want = sample_reference(lg, 1.0, top_k, top_p, row_uniforms(seed, [9, 9]), min_p=mp)
    assert (want[0] > 0).nonzero()[:, 0].tolist() == sorted({3, 100, V - 1}) and int((want[1] > 0).sum()) == 12
    tok, probs, _, _, _ = constrained(lg.to(dev), V, 1.0, top_k, top_p, seed, [9, 9], want_logits=False, min_p=mp)
    assert torch.equal(probs > 0, want > 0)
    assert float(((probs.double() - want).abs()[want > 0] / want[want > 0]).max()) <= 1e-5
    assert torch.equal(tok, want_tok)


# ---- tokens and probabilities -------------------------------------------------------------------------------------------
def check_tokens(B, V, top_k, top_p, temperature=0.8, min_p=0.02):
    lens = [(37 * b + 5) % 300 for b in range(B)]
    lg = make_logits(B, V, seed=800 + B)
    hist, hist_row, gen_start = make_history(lens, V, seed=B + V, hot=lg.topk(2, dim=-1).indices)
    bias = make_bias(V, B)
    bias_row = [((b + 1) % 4) - 1 for b in range(B)]         # rows 0, 1, 2, none, 0, ...
    bias[bias_row[B // 2], lg[B // 2].argmax()] = -INF       # the most likely token of a row: banned
    min_new = 20
    pen_lg = apply_penalties(lg, windows(hist, hist_row), lens, gen_start, *PEN.values())
    con_lg = apply_constraints(pen_lg, lens, gen_start, bias, bias_row, min_new, EOS)
    for seed in range(40):
        d_u, d_p = margins_min_p(con_lg, temperature, top_k, top_p, row_uniforms(seed, lens), min_p)
        if d_u >= MARGIN and d_p >= MARGIN:
            break
    else:
        raise AssertionError("no seed in 0..39 keeps every row 1e-5 away from a boundary")
    want_tok, want_probs = sample_reference(con_lg, temperature, top_k, top_p, row_uniforms(seed, lens), min_p=min_p)
    tok, probs, _, _, _ = constrained(padded(lg, -(-V // 64) * 64), V, temperature, top_k, top_p, seed, lens, hist, hist_row,
                                      gen_start, PEN, eos=EOS, want_logits=False, logit_bias=bias, bias_row=bias_row,
                                      min_p=min_p, min_new_tokens=min_new)
    print(f"V={V} B={B} k={top_k} p={top_p}: seed {seed}, margins u {d_u:.2e} top_p {d_p:.2e}")
    assert torch.equal(tok, want_tok), (tok.tolist(), want_tok.tolist())
    big = want_probs >= 2e-38
    assert bool((probs[big] > 0).all()) and bool((probs[want_probs == 0] == 0).all())
    assert bool((probs[~big] <= 4e-38).all())
    rel = (probs.double() - want_probs).abs()[big] / want_probs[big]
    assert float(rel.max()) <= 1e-5, float(rel.max())
    # the constraints decide something here: the penalised sampler's distribution differs, and so does min-p's share
    assert not torch.equal(sample_reference(pen_lg, temperature, top_k, top_p, row_uniforms(seed, lens))[1], want_probs)
    if top_k is None:
        assert not torch.equal(sample_reference(con_lg, temperature, None, top_p, row_uniforms(seed, lens))[1], want_probs)


@pytest.mark.parametrize("top_k,top_p", [(None, None), (50, 0.9)], ids=["min-p", "k50-p0.9"])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_tokens_small_vocab(B, top_k, top_p):
    check_tokens(B, 509, top_k, top_p)


@pytest.mark.parametrize("B,top_k,top_p", [(1, None, None), (64, 50, 0.9)])
def test_tokens_gpt2_vocab(B, top_k, top_p):
    check_tokens(B, 50257, top_k, top_p)


# ---- greedy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [0.0, 0.8], ids=["greedy", "sampled"])
def test_suppressed_and_banned_tokens_done_rows_and_rows_with_nothing_finite(temperature):
    """Row 0: the argmax is eos and it is held back: the next best. Row 1: the argmax is banned by the bias: the next best.
    Row 2: already done: eos, whatever the row holds. Row 3: everything banned: token 0. Row 4: the only finite token is the
    held-back eos: token 0. Row 5: past min_new, eos is drawn and sets done. (Sampled: top_k = 1 draws the maximum.)"""
    V, A, Bt = 2049, 1500, 40
    lg = torch.full((6, V), -9.0)
    lg[:, EOS], lg[:, Bt] = 5.0, 4.0
    lg[1, A] = 6.0
    lg[4] = -INF
    lg[4, EOS] = 1.0
    bias = torch.zeros(2, V)
    bias[0, A] = -INF
    bias[1] = -INF
    pos, gs = [6, 6, 6, 6, 6, 9], [4, 0, 4, 4, 4, 4]
    out = constrained(lg.to(dev), V, temperature, 1 if temperature else None, None, 0, pos, gen_start=gs, eos=EOS,
                      done=[0, 0, 1, 0, 0, 0], logit_bias=bias, bias_row=[-1, 0, -1, 1, -1, -1], min_new_tokens=5)
    tok, probs, got, done, _ = out
    assert tok.tolist() == [Bt, EOS, EOS, 0, 0, EOS], tok.tolist()
    assert done.tolist() == [0, 1, 1, 0, 0, 1]
    want = apply_constraints(lg, pos, gs, bias, [-1, 0, -1, 1, -1, -1], 5, EOS)
    assert torch.equal(bits(got), bits(want)) and want[0, EOS] == -INF and want[1, EOS] == 5.0 and want[5, EOS] == 5.0
    assert bool((want[3:5] == -INF).all())
    assert torch.equal(probs[[0, 1, 5]], torch.zeros(3, V).scatter_(1, torch.tensor([[Bt], [EOS], [EOS]]), 1.0))
    assert torch.equal(tok[[0, 1, 3, 4, 5]], sample_reference(want, temperature, 1 if temperature else None, None,
                                                              row_uniforms(0, pos))[0][[0, 1, 3, 4, 5]])


# ---- stop sequences --------------------------------------------------------------------------------------------------------
def run_forced(V, rows, stops, min_new=0, temperature=0.0, hist_row=None):
    """Rows of (prompt, the tokens to force, one per launch): every launch draws from logits that are one-hot after the
    bias (everything but the forced token banned). Returns the tokens and done flags after each launch; seq is the
    history, row b's in row hist_row[b] of a buffer twice as tall whose other rows hold TRAP."""
    B, n = len(rows), len(rows[0][1])
    hist_row = list(range(B)) if hist_row is None else hist_row
    seq = torch.full((2 * B, 64), TRAP, dtype=torch.int64)
    for b, (prompt, _) in enumerate(rows):
        seq[hist_row[b], :len(prompt)] = torch.tensor(prompt)
    seq = seq.to(dev)
    gs = [len(p) for p, _ in rows]
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    lg = make_logits(B, V, seed=1).to(dev)
    toks, flags = [], []
    for i in range(n):
        bias = torch.full((B, V), -INF)
        for b, (_, forced) in enumerate(rows):
            bias[b, forced[i]] = 0.0
        tok = torch.full((B,), -7, dtype=torch.int64, device=dev)
        pos = [g + i for g in gs]
        K.sample_constrained(lg, V, temperature, None, None, 3, pos, tok, eos=EOS, done=done, hist=seq, hist_row=hist_row,
                             gen_start=gs, logit_bias=bias.to(dev), min_new_tokens=min_new, stop=stops)
        for b in range(B):                                   # the history of the next launch
            seq[hist_row[b], pos[b]] = tok[b]
        toks.append(tok.tolist())
        flags.append(done.tolist())
    return toks, flags, seq.cpu()


@pytest.mark.parametrize("temperature", [0.0, 0.8], ids=["greedy", "sampled"])
def test_stop_sequences_of_length_1_2_and_16(temperature):
    V = 509
    long16 = list(range(300, 316))
    stops = [[77], [60, 61], long16]
    forced18 = lambda head: head + [400 + i for i in range(18 - len(head))]  # noqa: E731
    rows = [([5, 6], forced18([9, 77])),                     # length 1: done at launch 1, eos from launch 2 on
            ([5, 60], forced18([61, 8, 60, 61])),            # a would-be match whose first token is the prompt's: not at
                                                             # launch 0; the one inside the generated part: launch 3
            ([300], forced18(long16[1:] + long16[:1])),      # 15 of 16 after a prompt token 300: no match
            ([4, 4, 4], forced18(long16)),                   # the whole 16 generated: done at launch 15
            ([8], forced18([60, 62, 61]))]                   # interrupted: never
    hist_row = [3, 9, 1, 6, 4]
    toks, flags, seq = run_forced(V, rows, stops, temperature=temperature, hist_row=hist_row)
    first_done = [next((i for i, f in enumerate(flags) if f[b]), None) for b in range(5)]
    assert first_done == [1, 3, None, 15, None], first_done
    for b, (prompt, forced) in enumerate(rows):
        d = first_done[b]
        got = [t[b] for t in toks]
        assert got == (forced if d is None else forced[:d + 1] + [EOS] * (17 - d)), (b, got)
        hist = prompt + got                                  # stop_match agrees launch by launch
        for i in range(18 if d is None else d + 1):
            assert stop_match(hist[:len(prompt) + i + 1], len(prompt), stops) == (i == d), (b, i)
    assert bool((seq[[0, 2, 5, 7, 8]] == TRAP).all())        # the rows of no sequence are untouched


def test_the_min_new_gate_and_position_zero():
    """A match that completes before the row holds min_new tokens does not fire; the same tokens later do. pos = 0 with a
    16-token sequence (and a 1-token one that matches there) is safe."""
    V = 509
    rows = [([5], [60, 61, 9, 60, 61, 9])]
    toks, flags, _ = run_forced(V, rows, [[60, 61]], min_new=4)
    assert [f[0] for f in flags] == [0, 0, 0, 0, 1, 1] and [t[0] for t in toks] == [60, 61, 9, 60, 61, EOS]
    lg = torch.full((2, V), -9.0)
    lg[:, 300] = 5.0
    hist = torch.full((2, 32), TRAP, dtype=torch.int64)
    tok, _, _, done, _ = constrained(lg.to(dev), V, 0.0, None, None, 0, [0, 0], hist, gen_start=[0, 0], eos=EOS,
                                     done=[0, 0], want_probs=False, want_logits=False,
                                     stop=[list(range(285, 301))], min_p=0.5)
    assert tok.tolist() == [300, 300] and done.tolist() == [0, 0]
    tok, _, _, done, _ = constrained(lg.to(dev), V, 0.0, None, None, 0, [0, 0], hist, gen_start=[0, 0], eos=EOS,
                                     done=[0, 0], want_probs=False, want_logits=False,
                                     stop=[list(range(285, 301)), [300]])
    assert done.tolist() == [1, 1]


# ---- neutral constraints, determinism, the buffers it writes ------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_neutral_constraints_are_sample_logprobs(temperature):
    V, B = 50257, 3
    lg = make_logits(B, V, seed=9)
    buf = padded(lg, 50432)
    pos = [40, 90, 17]
    hist, hist_row, gen_start = make_history(pos, V, seed=3)

    def call(fn, **con):
        tok = torch.full((B,), -7, dtype=torch.int64, device=dev)
        probs, out = torch.full((B, V), -1.0, device=dev), torch.full((B, V), -1.0, device=dev)
        done = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
        lp = dict(logprob=torch.full((B, 1), -3.0, device=dev), col=[0] * B,
                  top_ids=torch.full((B, 1, 4), -3, dtype=torch.int32, device=dev),
                  top_logprobs=torch.full((B, 1, 4), -3.0, device=dev))
        fn(buf, V, temperature, 50, 0.9, 5, pos, tok, eos=EOS, done=done, probs_out=probs, logits_out=out,
           hist=hist.to(dev), hist_row=hist_row, gen_start=gen_start, **PEN, **lp, **con)
        torch.cuda.synchronize()
        return [t.cpu() for t in (tok, probs, out, done, lp["logprob"], lp["top_ids"], lp["top_logprobs"])]
    want = call(K.sample_logprobs)
    for con in ({}, dict(min_p=0.0, min_new_tokens=0, stop=[]),
                dict(logit_bias=torch.ones(1, V, device=dev), bias_row=[-1] * B)):
        got = call(K.sample_constrained, **con)
        assert all(torch.equal(bits(g) if g.dtype == torch.float32 else g, bits(w) if w.dtype == torch.float32 else w)
                   for g, w in zip(got, want)), con.keys()


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_two_runs_have_the_same_bits_and_write_only_their_outputs(temperature):
    V, B = 50257, 4
    lens = [5, 700, 64, 33]
    lg = make_logits(B, V, seed=11)
    buf = padded(lg, 50432)
    hist, hist_row, gen_start = make_history(lens, V, seed=4)
    hist_d = hist.to(dev)
    bias = make_bias(V, 2).to(dev)
    guard = 16

    def run():
        tok = torch.full((B + 2 * guard,), -7, dtype=torch.int64, device=dev)
        probs = torch.full((B + 2, V), -1.0, device=dev)
        out = torch.full((B + 2, V), -1.0, device=dev)
        done = torch.full((B + 2 * guard,), 0, dtype=torch.uint8, device=dev)
        done[:guard], done[guard + B:] = 9, 9
        lpb = torch.full((B + 2, 1), -3.0, device=dev)
        ids, lps = torch.full((B + 2, 1, 3), -3, dtype=torch.int32, device=dev), torch.full((B + 2, 1, 3), -3.0, device=dev)
        K.sample_constrained(buf, V, temperature, 50, 0.9, 5, lens, tok[guard:guard + B], eos=EOS, done=done[guard:guard + B],
                             probs_out=probs[1:B + 1], logits_out=out[1:B + 1], hist=hist_d, hist_row=hist_row,
                             gen_start=gen_start, logprob=lpb[1:B + 1], top_ids=ids[1:B + 1], top_logprobs=lps[1:B + 1],
                             col=[0] * B, logit_bias=bias, bias_row=[0, 1, 2, -1], min_p=0.05, min_new_tokens=3,
                             stop=[[11, 12], [13]], **PEN)
        torch.cuda.synchronize()
        return [t.cpu() for t in (tok, probs, out, done, lpb, ids, lps)]
    before = (buf.clone(), hist_d.clone(), bias.clone())
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(bits(x) if x.dtype == torch.float32 else x, bits(y) if y.dtype == torch.float32 else y)
    tok, probs, out, done, lpb, ids, lps = a
    assert bool((tok[:guard] == -7).all()) and bool((tok[guard + B:] == -7).all()) and bool((tok[guard:guard + B] >= 0).all())
    assert bool((done[:guard] == 9).all()) and bool((done[guard + B:] == 9).all())
    for t, fill in ((probs, -1.0), (out, -1.0), (lpb, -3.0), (ids, -3), (lps, -3.0)):
        assert bool((t[0] == fill).all()) and bool((t[B + 1] == fill).all()) and not bool((t[1:B + 1] == fill).all())
    assert all(torch.equal(bits(x), bits(y)) if x.dtype == torch.float32 else torch.equal(x, y)
               for x, y in zip((buf, hist_d, bias), before))
    # the log-probabilities are the raw row's
    want_lp, want_ids, _ = token_logprobs(lg, tok[guard:guard + B], 3)
    assert torch.equal(ids[1:B + 1, 0].long(), want_ids)
    assert float((lpb[1:B + 1, 0].double() - want_lp).abs().max()) < 1e-4
