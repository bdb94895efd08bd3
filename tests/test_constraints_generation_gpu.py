"""Logit bias, min-p, minimum length and stop sequences through the token loops on the MI355X, on the tiny model of
tests/test_penalties_gpu.py (L2 H2 C128 V509). Everything is bitwise: the device loop against a manual loop of step + the
reference rules, the greedy device path against the host sampler's, generate_many against itself at another batch size,
speculative generation and num_samples against the plain calls, the CLI against the API."""
import json
import subprocess
import sys

import pytest
import torch

from gpt_2_distributed_amd.generation import (apply_constraints, apply_penalties, sample_reference, stop_match,
                                              uniform_at)
from tests.conftest import REPO
from tests.test_constraints_kernels_gpu import margins_min_p
from tests.test_sampling_gpu import MARGIN, TINY, make_model

pytestmark = pytest.mark.gpu

dev = "cuda"
V = TINY["vocab_size"]
EOS = 500
PEN_KW = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2)
# (the tiny model's logits lie within about one unit of each other: a bias of this size matters and does not decide alone)
BIAS = {EOS: 0.4, 17: -float("inf"), 40: 0.6, 41: -0.5}
SAMPLERS = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.8, top_k=50, top_p=0.95)}
MIN_P, MIN_NEW = 0.05, 6


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tiny():
    model = make_model()
    S = torch.randint(0, V, (8, 150), generator=torch.Generator().manual_seed(17)).to(dev)
    return model, S


def bias_row():
    b = torch.zeros(1, V)
    for t, v in BIAS.items():
        b[0, t] = v
    return b


def pick(gen, at, n):
    """n consecutive tokens of the generated tokens `gen`, from index `at` or as near to it as `gen` is long."""
    a = max(0, min(at, len(gen) - n))
    return [int(t) for t in gen[a:a + n]]


def ended(row, start, stops, min_new, eos):
    """Whether the row drew eos or completed a stop sequence in its generated part."""
    return any(row[i] == eos or stop_match(row[:i + 1], start, stops, min_new) for i in range(start, len(row)))


def end_rows(rows, starts, stops, min_new, eos):
    """The rows of a run without stop sequences as the run with them leaves them: from the column after the token that
    completes a stop sequence (before any eos) the row holds eos."""
    out = [list(r) for r in rows]
    for r, g in zip(out, starts):
        for i in range(g, len(r)):
            if r[i] == eos:
                break
            if stop_match(r[:i + 1], g, stops, min_new):
                r[i + 1:] = [eos] * (len(r) - i - 1)
                break
    return out


@pytest.mark.parametrize("s", SAMPLERS)
def test_device_loop_equals_a_manual_loop_with_the_reference(tiny, s):
    """prefill + (apply_penalties + apply_constraints + sample_reference(min_p) on the session's logits + step) per
    token with all four options on, the exact-case margins checked on every step's constrained logits; the stop sequences
    are taken from what that loop drew, and the row then goes on with eos."""
    model, S = tiny
    prompt = S[:3, :5].contiguous()
    n, P = 24, 5
    T, k, p = (SAMPLERS[s].get(x) for x in ("temperature", "top_k", "top_p"))
    bias = bias_row()
    for seed in range(20):
        sess = model.decoder(3, P + n)
        logits = sess.prefill(prompt)
        hist = torch.zeros(3, P + n, dtype=torch.int64)
        hist[:, :P] = prompt.cpu()
        done = [False] * 3
        ok = True
        for i in range(n):
            lg = apply_penalties(logits.cpu(), hist, [P + i] * 3, [P] * 3, **PEN_KW)
            lg = apply_constraints(lg, [P + i] * 3, [P] * 3, bias, [0] * 3, MIN_NEW, EOS)
            u = torch.tensor([uniform_at(seed, b, P + i) for b in range(3)], dtype=torch.float64)
            if T and min(margins_min_p(lg, T, k, p, u, MIN_P)) < MARGIN:
                ok = False
                break
            tok = sample_reference(lg, T, k, p, u, min_p=MIN_P)[0]
            tok = torch.where(torch.tensor(done), torch.full_like(tok, EOS), tok)
            done = [d or int(t) == EOS for d, t in zip(done, tok)]
            hist[:, P + i] = tok
            if i + 1 < n:
                logits = sess.step(tok.to(dev))
        if ok:
            break
    assert ok, "no seed in 0..19 keeps every step 1e-5 away from a boundary"
    assert not bool((hist[:, P:P + MIN_NEW] == EOS).any()) and not bool((hist[:, P:] == 17).any())
    opts = dict(logit_bias=BIAS, min_p=MIN_P, min_new_tokens=MIN_NEW, eos_token_id=EOS, seed=seed, **SAMPLERS[s], **PEN_KW)
    got = model.generate(prompt, n, **opts)
    assert torch.equal(got.cpu(), hist[:, :got.size(1)]), (seed, got.tolist(), hist.tolist())
    assert bool((hist[:, got.size(1):] == EOS).all())        # (cut where every row has emitted eos)
    assert not torch.equal(got, model.generate(prompt, n, eos_token_id=EOS, seed=seed, **SAMPLERS[s], **PEN_KW)[:, :got.size(1)])
    # stop sequences from the run itself: a 2-token one of row 0 past min_new, a 1-token one of row 1 before it (gated)
    rows = hist.tolist()
    stops = [rows[0][P + 8:P + 10], [rows[1][P + 2]]]
    want = torch.tensor(end_rows(rows, [P] * 3, stops, MIN_NEW, EOS))
    got = model.generate(prompt, n, stop=stops, **opts)
    assert torch.equal(got.cpu(), want[:, :got.size(1)]) and bool((want[:, got.size(1):] == EOS).all())
    # the session interface: sample() + step, then generate() over the same buffer, the flags carried
    sess = model.decoder(3, P + n)
    sess.prefill(prompt)
    seq = torch.zeros(3, P + n, dtype=torch.int64, device=dev)
    seq[:, :P] = prompt
    flags = torch.zeros(3, dtype=torch.uint8, device=dev)
    con = dict(logit_bias=bias.to(dev), bias_row=[0] * 3, min_p=MIN_P, min_new_tokens=MIN_NEW, stop=stops,
               gen_start=[P] * 3, **PEN_KW)
    first = sess.sample(T, k, p, seed, history=seq, eos_token_id=EOS, done=flags, **con)
    seq[:, P] = first
    sess.step(first)
    sess.generate(9, T, k, p, seed, EOS, seq, flags, **con)
    sess.generate(n - 10, T, k, p, seed, EOS, seq, flags, **con)
    assert torch.equal(seq.cpu(), want)
    assert flags.tolist() == [int(ended(r, P, stops, MIN_NEW, EOS)) for r in want.tolist()]
    fresh = model.decoder(3, P + n)
    fresh.prefill(prompt)
    with pytest.raises(ValueError, match="seq"):
        fresh.generate(1, T, k, p, seed, EOS, None, flags, stop=stops)
    with pytest.raises(ValueError, match="eos_token_id"):
        fresh.sample(T, k, p, seed, min_new_tokens=2)


def test_greedy_device_loop_equals_the_host_sampler_path(tiny):
    model, S = tiny
    prompt = S[:3, :9].contiguous()
    opts = dict(temperature=0.0, logit_bias=BIAS, min_p=MIN_P, min_new_tokens=MIN_NEW, eos_token_id=EOS, **PEN_KW)
    want = model.generate(prompt, 40, **opts)
    got = model.generate(prompt, 40, seed=0, **opts)
    assert torch.equal(got, want)
    assert not torch.equal(got, model.generate(prompt, 40, temperature=0.0, seed=0, eos_token_id=EOS, **PEN_KW)[:, :got.size(1)])
    rows = got.tolist()
    stops = [pick(rows[0][9:], 7, 2), pick(rows[2][9:], 10, 1)]
    want = model.generate(prompt, 40, stop=stops, **opts)
    got = model.generate(prompt, 40, seed=0, stop=stops, **opts)
    assert torch.equal(got, want)
    assert got.tolist() == [r[:got.size(1)] for r in end_rows(rows, [9] * 3, stops, MIN_NEW, EOS)]
    # ragged prompts, a [B, V] bias and an allowed list through both paths
    per_row = torch.zeros(3, V)
    per_row[0, 33], per_row[1, 44], per_row[2, EOS] = 9.0, 9.0, 1.0
    kw = dict(temperature=0.0, prompt_lens=[9, 3, 6], eos_token_id=EOS, logit_bias=per_row, min_new_tokens=3,
              allowed_token_ids=list(range(20, 60)) + [EOS], stop=[[33, 33, 33]])
    a, b = model.generate(prompt, 12, seed=0, **kw), model.generate(prompt, 12, **kw)
    assert torch.equal(a, b) and a[0, 9:12].tolist() == [33, 33, 33] and a[1, 3:6].tolist() == [44, 44, 44]


MANY_LENS = [1, 5, 33, 9, 30, 2, 17]


@pytest.mark.parametrize("s", SAMPLERS)
def test_generate_many_does_not_depend_on_the_batch(tiny, s):
    model, S = tiny
    n = 40
    prompts = [S[i, :L].contiguous() for i, L in enumerate(MANY_LENS)]
    opts = dict(seed=3, eos_token_id=EOS, logit_bias=BIAS, min_p=MIN_P, min_new_tokens=MIN_NEW, **SAMPLERS[s], **PEN_KW)
    free = model.generate_many(prompts, n, batch_size=8, **opts)
    stops = [pick(free[2][MANY_LENS[2]:].tolist(), 8, 2), pick(free[5][MANY_LENS[5]:].tolist(), 3, 1)]
    runs = [model.generate_many(prompts, n, batch_size=bs, stop=stops, **opts) for bs in (2, 8)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    for i, (out, full) in enumerate(zip(runs[0], free)):     # each is its stop-free run, cut after the completing token
        want = end_rows([full.tolist()], [MANY_LENS[i]], stops, MIN_NEW, EOS)[0]
        cut = next((j + 1 for j in range(MANY_LENS[i], len(want)) if want[j] == EOS or
                    stop_match(want[:j + 1], MANY_LENS[i], stops, MIN_NEW)), len(want))
        assert out.tolist() == want[:cut], i
    assert runs[0][2].numel() <= MANY_LENS[2] + 10 and not any(17 in o[m:].tolist() for o, m in zip(runs[0], MANY_LENS))
    plain = model.generate_many(prompts, n, batch_size=8, seed=3, eos_token_id=EOS, **SAMPLERS[s], **PEN_KW)
    assert not all(torch.equal(a, b) for a, b in zip(runs[0], plain))
    if s == "greedy":                                         # (generate draws row 0 with key 0: greedy has no key)
        for i in (0, 2, 5):
            one = model.generate(prompts[i][None], n, stop=stops, **opts)[0]
            assert torch.equal(runs[0][i], one[:runs[0][i].numel()]), i


@pytest.mark.parametrize("s,kv_dtype", [("greedy", "bf16"), ("sampled", "bf16"), ("sampled", "fp8")])
def test_speculative_generation_stays_exact(tiny, s, kv_dtype):
    """draft_tokens=4 with drafts that are always right: every run of 5 tokens is accepted whole, so the stop sequence
    fires in the middle of one. Also with the default drafts. (fp8: the one case with the quantised cache.)"""
    from tests.test_speculative_gpu import scripted
    model, S = tiny
    n, lens = 30, [3, 17, 9]
    idx = S[:3, :17].contiguous()
    opts = dict(seed=1, prompt_lens=lens, eos_token_id=EOS, logit_bias=BIAS, min_p=MIN_P, min_new_tokens=MIN_NEW,
                kv_dtype=kv_dtype, **SAMPLERS[s], **PEN_KW)
    free = model.generate(idx, n, **opts)
    rows = [r[:lens[i] + free.size(1) - 17] for i, r in enumerate(free.tolist())]
    stops = [pick(rows[0][3:], 7, 2), pick(rows[1][17:], 11, 3)]  # they end inside the 2nd and 3rd run of 5
    want = model.generate(idx, n, stop=stops, **opts)
    made = want.size(1) - 17
    assert [r[:m + made] for r, m in zip(want.tolist(), lens)] == [r[:m + made] for r, m in zip(
        end_rows(rows, lens, stops, MIN_NEW, EOS), lens)]
    for fn in (scripted("right", rows), scripted("half", rows), None):
        got = model.generate(idx, n, draft_tokens=4, draft_fn=fn, stop=stops, **opts)
        assert torch.equal(got, want), (s, fn)


def test_num_samples_equals_generate_many_over_the_repeated_prompts(tiny):
    model, S = tiny
    prompts = [S[0, :7].contiguous(), S[1, :12].contiguous()]
    opts = dict(temperature=0.8, top_k=50, seed=5, logit_bias=BIAS, min_p=MIN_P)
    out = model.generate(prompts, 20, num_samples=4, pad_token_id=0, **opts)
    many = model.generate_many([p for p in prompts for _ in range(4)], 20, batch_size=8, **opts)
    for r, (row, one) in enumerate(zip(out, many)):
        assert torch.equal(row[:one.numel()], one), r
    assert len({tuple(o.tolist()) for o in many[:4]}) > 1 and not bool((out[:, 12:] == 17).any())
    plain = model.generate(prompts, 20, num_samples=4, pad_token_id=0, temperature=0.8, top_k=50, seed=5)
    assert not torch.equal(out, plain)


def test_min_new_tokens_holds_an_argmax_eos_back(tiny):
    model, S = tiny
    prompt, P, n = S[:3, :6].contiguous(), 6, 7
    for how in (dict(seed=0), {}):                             # the device sampler and the host sampler
        out = model.generate(prompt, 20, temperature=0.0, eos_token_id=EOS, logit_bias={EOS: 50.0}, min_new_tokens=n, **how)
        assert out.shape == (3, P + n + 1), out.shape
        assert not bool((out[:, P:P + n] == EOS).any()) and bool((out[:, P + n] == EOS).all())
        assert bool((model.generate(prompt, 20, temperature=0.0, eos_token_id=EOS, logit_bias={EOS: 50.0}, **how)[:, P] == EOS).all())


def test_allowed_token_ids_confine_every_generated_token(tiny):
    model, S = tiny
    allowed = [3, 99, 100, 257, 508]
    for how in (dict(seed=2), dict(generator=torch.Generator(device=dev).manual_seed(2))):
        out = model.generate(S[:4, :5].contiguous(), 30, temperature=1.5, allowed_token_ids=allowed, **how)
        new = out[:, 5:]
        assert bool(torch.isin(new, torch.tensor(allowed, device=dev)).all()) and len(set(new.flatten().tolist())) > 1
    many = model.generate_many([S[0, :4], S[1, :9]], 12, batch_size=2, temperature=1.5, seed=2, allowed_token_ids=allowed,
                               logit_bias=torch.zeros(V))
    assert all(set(o[m:].tolist()) <= set(allowed) for o, m in zip(many, (4, 9)))


def test_cli_takes_the_flags(tmp_path):
    from gpt_2_distributed_amd.train_gpt2_distributed import save_checkpoint
    model = make_model()
    ckpt = save_checkpoint(model, model.configure_optimizers(), 3, str(tmp_path))
    api = dict(temperature=0.8, top_p=0.9, seed=5, eos_token_id=EOS, logit_bias={EOS: 0.5, 40: 0.75, 17: -100.0}, min_p=0.05,
               min_new_tokens=8)
    idx = torch.tensor([[11, 12, 13]] * 2, device=dev)
    free = model.generate(idx, 24, **api)
    stops = [pick(free[0, 3:].tolist(), 9, 2), pick(free[1, 3:].tolist(), 12, 1)]
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.generate", "--checkpoint", ckpt, "--model", "auto",
           "--prompt_ids", "11,12,13", "--max_new_tokens", "24", "--batch", "2", "--temperature", "0.8", "--seed", "5",
           "--sampler", "device", "--top_p", "0.9", "--eos_token_id", str(EOS), "--logit_bias", f"{EOS}:0.5,40:0.75,17:-100",
           "--min_p", "0.05", "--min_new_tokens", "8"] + [a for s in stops for a in ("--stop", ",".join(map(str, s)))]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("[")]
    want = model.generate(idx, 24, stop=stops, **api)
    assert rows == want.tolist()
    assert want.tolist() == [r[:want.size(1)] for r in end_rows(free.tolist(), [3, 3], stops, 8, EOS)]
    assert rows != model.generate(idx, 24, temperature=0.8, top_p=0.9, seed=5, eos_token_id=EOS).tolist()
