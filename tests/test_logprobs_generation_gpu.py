"""Token log-probabilities through GPT2.generate / generate_many / the CLI on the MI355X (the TINY model of
tests/test_sampling_gpu.py: 2 layers, 128 wide, V = 509).

The tokens are those of the call without ``logprobs``; each value is token_logprobs (float64) of the logits row the token
was drawn from, to the kernels' tolerance (tests/test_logprobs_kernels_gpu.py); and because a value is a function of its
logits row alone, the paths that are proved to form the same rows give the same log-probability bits: another batch
size, num_samples against the repeated prompt list, draft_tokens with right and wrong drafts, penalties, the fp8 cache."""
import json
import subprocess
import sys

import pytest
import torch

from gpt_2_distributed_amd.generation import LogprobBuffer, token_logprobs
from tests.conftest import REPO
from tests.test_logprobs_kernels_gpu import bits, tolerance
from tests.test_sampling_gpu import TINY, make_model

pytestmark = pytest.mark.gpu

dev = "cuda"
V = TINY["vocab_size"]
SAMPLERS = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.8, top_k=50, top_p=0.95)}
PEN_KW = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tiny():
    model = make_model()
    S = torch.randint(0, V, (8, 40), generator=torch.Generator().manual_seed(17)).to(dev)
    return model, S


def same(a, b):
    """Two GenerateOutputs, bit for bit."""
    return (torch.equal(a.tokens, b.tokens) and torch.equal(bits(a.logprobs), bits(b.logprobs))
            and torch.equal(a.top_ids, b.top_ids) and torch.equal(bits(a.top_logprobs), bits(b.top_logprobs)))


@pytest.mark.parametrize("s", SAMPLERS)
def test_tokens_are_unchanged_and_padding_is_zero(tiny, s):
    model, S = tiny
    prompt, n = S[:3, :9].contiguous(), 24
    want = model.generate(prompt, n, seed=2, **SAMPLERS[s])
    out = model.generate(prompt, n, seed=2, logprobs=5, **SAMPLERS[s])
    assert torch.equal(out.tokens, want)
    assert out.logprobs.shape == want.shape and out.logprobs.dtype == torch.float32
    assert out.top_ids.shape == out.top_logprobs.shape == want.shape + (5,) and out.top_ids.dtype == torch.int32
    assert bool((out.logprobs[:, :9] == 0).all()) and bool((out.logprobs[:, 9:] < 0).all())
    assert bool((out.top_ids[:, :9] == 0).all()) and bool((out.top_logprobs[:, :9] == 0).all())
    assert torch.equal(model.generate(prompt, n, seed=2, logprobs=True, **SAMPLERS[s]).logprobs, out.logprobs)
    if s == "greedy":                                         # the argmax is the first alternative
        assert torch.equal(out.top_ids[:, 9:, 0].long(), want[:, 9:])
        assert torch.equal(bits(out.top_logprobs[:, 9:, 0]), bits(out.logprobs[:, 9:]))
    # ragged prompts with eos and a pad token: prompt columns, pad columns and what follows a row's eos hold 0
    lens = [9, 3, 6]
    free = model.generate(prompt, n, seed=2, prompt_lens=lens, **SAMPLERS[s])
    eos = int(free[1, 3 + 4])                                 # row 1's fifth token
    kw = dict(seed=2, prompt_lens=lens, eos_token_id=eos, pad_token_id=1, **SAMPLERS[s])
    want = model.generate(prompt, n, **kw)
    out = model.generate(prompt, n, logprobs=5, **kw)
    assert torch.equal(out.tokens, want)
    for b, m in enumerate(lens):
        row = want[b, m:].tolist()
        end = m + (row.index(eos) + 1 if eos in row else want.size(1) - m)
        end = min(end, m + (want.size(1) - max(lens)))
        assert bool((out.logprobs[b, m:end] < 0).all()), (b, m, end)
        for t in (out.logprobs, out.top_ids, out.top_logprobs):
            assert bool((t[b, :m] == 0).all()) and bool((t[b, end:] == 0).all()), (b, m, end)
    assert float(out.logprobs.sum(1)[1]) == pytest.approx(float(out.logprobs[1, 3:3 + 5].sum()))


@pytest.mark.parametrize("s", SAMPLERS)
def test_values_are_those_of_the_logits_row_each_token_was_drawn_from(tiny, s):
    """A manual sample / step loop over a session captures every logits row; the device loop's values are
    token_logprobs of those rows (raw: the penalties move the draw, not the value)."""
    model, S = tiny
    lens, n = [9, 3, 6], 12
    prompt = S[:3, :9].contiguous()
    for pen in ({}, PEN_KW):
        out = model.generate(prompt, n, seed=4, prompt_lens=lens, logprobs=20, **SAMPLERS[s], **pen)
        sess = model.decoder(3, 9 + n)
        logits = sess.prefill(prompt, lens)
        for i in range(n):
            rows = logits.cpu()
            cols = torch.tensor(lens) + i
            tok = out.tokens[torch.arange(3), cols.to(dev)]
            want_lp, want_ids, want_top = token_logprobs(rows, tok.cpu(), 20)
            lse = torch.logsumexp(rows.double(), -1)
            got = out.logprobs[torch.arange(3), cols.to(dev)].cpu().double()
            assert bool(((got - want_lp).abs() <= tolerance(rows[torch.arange(3), tok.cpu()].double(), lse)).all()), i
            assert torch.equal(out.top_ids[torch.arange(3), cols.to(dev)].cpu().long(), want_ids), i
            got_top = out.top_logprobs[torch.arange(3), cols.to(dev)].cpu().double()
            l = rows.double().gather(1, want_ids)
            assert bool(((got_top - want_top).abs() <= tolerance(l, lse[:, None].expand_as(l))).all()), i
            if i + 1 < n:
                logits = sess.step(tok)
    # DecodeSession.sample(logprobs=n): the same launch, the session's own logits row
    sess = model.decoder(3, 9 + n)
    rows = sess.prefill(prompt, lens).cpu()
    plain = sess.sample(seed=4, **SAMPLERS[s])
    tok, lp, ids, top = sess.sample(seed=4, logprobs=5, **SAMPLERS[s])
    assert torch.equal(tok, plain) and lp.shape == (3,) and ids.shape == top.shape == (3, 5)
    want_lp, want_ids, _ = token_logprobs(rows, tok.cpu(), 5)
    assert torch.equal(ids.cpu().long(), want_ids) and float((lp.cpu().double() - want_lp).abs().max()) < 2e-5


@pytest.mark.parametrize("s", SAMPLERS)
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_bits_do_not_depend_on_the_batch_or_on_num_samples(tiny, s, kv_dtype):
    model, S = tiny
    n = 20
    prompts = [S[i, :L].contiguous() for i, L in enumerate([5, 17, 9, 2, 30])]
    kw = dict(seed=3, kv_dtype=kv_dtype, logprobs=5, **SAMPLERS[s])
    runs = [model.generate_many(prompts, n, batch_size=bs, **kw) for bs in (2, 8)]
    for a, b, p in zip(*runs, prompts):
        assert same(a, b) and a.tokens.shape == (p.numel() + n,) and a.logprobs.shape == (p.numel() + n,)
        assert a.top_ids.shape == (p.numel() + n, 5) and bool((a.logprobs[:p.numel()] == 0).all())
        assert bool((a.logprobs[p.numel():] < 0).all())
    plain = model.generate_many(prompts, n, batch_size=8, seed=3, kv_dtype=kv_dtype, **SAMPLERS[s])
    assert all(torch.equal(a.tokens, t) for a, t in zip(runs[0], plain))
    # generate of a batch against generate_many at another batch size (greedy: the draw key does not enter)
    if s == "greedy":
        batch = model.generate(S[:3, :9].contiguous(), n, **kw)
        many = model.generate_many([S[i, :9].contiguous() for i in range(3)], n, batch_size=2, **kw)
        for b in range(3):
            assert torch.equal(batch.tokens[b], many[b].tokens) and torch.equal(bits(batch.logprobs[b]), bits(many[b].logprobs))
            assert torch.equal(batch.top_ids[b], many[b].top_ids)
            assert torch.equal(bits(batch.top_logprobs[b]), bits(many[b].top_logprobs))
    # num_samples = s against the list in which each prompt appears s times (same keys: the output row numbers)
    two = [S[0, :7].contiguous(), S[1, :7].contiguous()]
    out = model.generate(torch.stack(two), n, num_samples=3, **kw)
    many = model.generate_many([p for p in two for _ in range(3)], n, batch_size=6, **kw)
    for r in range(6):
        assert torch.equal(out.tokens[r], many[r].tokens) and torch.equal(bits(out.logprobs[r]), bits(many[r].logprobs))
        assert torch.equal(out.top_ids[r], many[r].top_ids)
    best = out.logprobs.sum(1).view(2, 3).argmax(1)                         # the README's best-of-n line
    assert best.shape == (2,) and bool((best >= 0).all())
    if s == "sampled":
        assert len({tuple(r) for r in out.tokens.tolist()}) > 2             # (the samples differ, so do their sums)


@pytest.mark.parametrize("s", SAMPLERS)
@pytest.mark.parametrize("pen", [{}, PEN_KW], ids=["plain", "penalised"])
def test_speculative_generation_gives_the_same_bits(tiny, s, pen):
    from tests.test_speculative_gpu import scripted
    model, S = tiny
    n, lens = 24, [3, 17, 9]
    idx = S[:3, :17].contiguous()
    kw = dict(seed=1, prompt_lens=lens, logprobs=5, **SAMPLERS[s], **pen)
    want = model.generate(idx, n, **kw)
    rows = [row[:lens[i] + n] for i, row in enumerate(want.tokens.tolist())]
    for draft in ("right", "wrong", None):
        fn = None if draft is None else scripted(draft, rows)
        got = model.generate(idx, n, draft_tokens=3, draft_fn=fn, **kw)
        assert same(got, want), (s, draft)
    eos = int(want.tokens[0, lens[0] + 9])
    want = model.generate(idx, n, eos_token_id=eos, **kw)
    got = model.generate(idx, n, eos_token_id=eos, draft_tokens=3, **kw)
    assert same(got, want)
    fp8 = model.generate(idx, n, kv_dtype="fp8", **kw)
    assert same(model.generate(idx, n, kv_dtype="fp8", draft_tokens=3, **kw), fp8)       # (its own tokens: n-gram drafts)


def test_host_sampler_agrees_with_the_device(tiny):
    """Greedy decoding through the host sampler (token_logprobs in float64, stored as fp32) and through the kernel:
    the same tokens, the same alternatives, values within the kernel tolerance; with penalties and eos too."""
    model, S = tiny
    prompt, n = S[:3, :9].contiguous(), 24
    free = model.generate(prompt, n, temperature=0.0, seed=0)
    eos = int(free[2, 9 + 6])
    for kw in (dict(), PEN_KW, dict(prompt_lens=[9, 3, 6], eos_token_id=eos, **PEN_KW)):
        host = model.generate(prompt, n, temperature=0.0, logprobs=5, **kw)
        devi = model.generate(prompt, n, temperature=0.0, seed=0, logprobs=5, **kw)
        assert torch.equal(host.tokens, devi.tokens) and torch.equal(host.top_ids, devi.top_ids), kw
        assert torch.equal(host.logprobs == 0, devi.logprobs == 0)
        bound = 1e-5 + 4 * 2.0 ** -23 * 20 + 2.0 ** -22                    # |l|, |lse| < 20 here; the host's fp32 store
        assert float((host.logprobs - devi.logprobs).abs().max()) <= bound
        assert float((host.top_logprobs - devi.top_logprobs).abs().max()) <= bound
    sampled = model.generate(prompt, n, temperature=0.8, top_k=20, logprobs=0,
                             generator=torch.Generator(device=dev).manual_seed(1))
    again = model.generate(prompt, n, temperature=0.8, top_k=20, generator=torch.Generator(device=dev).manual_seed(1))
    assert torch.equal(sampled.tokens, again) and bool((sampled.logprobs[:, 9:] < 0).all())


def test_session_buffer_is_column_aligned_with_seq(tiny):
    model, S = tiny
    lens, n = [9, 3, 6], 10
    T = 9 + 2 * n + 4
    sess = model.decoder(3, T)
    sess.prefill(S[:3, :9].contiguous(), lens)
    seq = torch.zeros(3, T, dtype=torch.int64, device=dev)
    buf = LogprobBuffer(3, T, 3, dev)
    sess.generate(n, 0.8, 50, 0.95, 7, seq=seq, logprobs=buf)
    sess.generate(n, 0.8, 50, 0.95, 7, seq=seq, logprobs=buf)              # a second call goes on where the first ended
    whole = model.generate(S[:3, :9].contiguous(), 2 * n, temperature=0.8, top_k=50, top_p=0.95, seed=7, prompt_lens=lens,
                           logprobs=3)
    for b, m in enumerate(lens):
        assert torch.equal(seq[b, m:m + 2 * n], whole.tokens[b, m:m + 2 * n])
        assert torch.equal(bits(buf.logprob[b, m:m + 2 * n]), bits(whole.logprobs[b, m:m + 2 * n]))
        assert torch.equal(buf.top_ids[b, m:m + 2 * n], whole.top_ids[b, m:m + 2 * n])
        assert bool((buf.logprob[b, :m] == 0).all()) and bool((buf.logprob[b, m + 2 * n:] == 0).all())
    with pytest.raises(ValueError, match="LogprobBuffer"):
        sess.generate(1, 0.8, 50, 0.95, 7, seq=seq, logprobs=LogprobBuffer(2, 64, 3, dev))       # two rows for three
    with pytest.raises(ValueError, match="LogprobBuffer"):
        sess.generate(1, 0.8, 50, 0.95, 7, seq=seq, logprobs=LogprobBuffer(3, 9 + 2 * n, 3, dev))  # a column short


def test_cli_prints_logprobs(tmp_path):
    from gpt_2_distributed_amd.train_gpt2_distributed import save_checkpoint
    model = make_model()
    ckpt = save_checkpoint(model, model.configure_optimizers(), 3, str(tmp_path))
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.generate", "--checkpoint", ckpt, "--model", "auto",
           "--prompt_ids", "11,12,13", "--max_new_tokens", "12", "--batch", "2", "--temperature", "0.8", "--seed", "5",
           "--sampler", "device", "--top_p", "0.9", "--logprobs", "2"]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    idx = torch.tensor([[11, 12, 13]] * 2, device=dev)
    want = model.generate(idx, 12, temperature=0.8, top_p=0.9, seed=5, logprobs=2)
    assert len(lines) == 2
    for r, line in enumerate(lines):
        assert line["tokens"] == want.tokens[r].tolist()
        assert len(line["logprobs"]) == 12 and line["cum_logprob"] == pytest.approx(sum(line["logprobs"]), abs=1e-9)
        assert line["logprobs"] == pytest.approx(want.logprobs[r, 3:].tolist(), abs=1e-6)
        assert [[i for i, _ in step] for step in line["top_logprobs"]] == want.top_ids[r, 3:].tolist()
