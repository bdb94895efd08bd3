"""DecodeSession.extend and speculative generation on the MI355X, on the tiny configuration. Everything here is bitwise:
extend leaves the logits, lengths and cache of as many step calls, and generate(draft_tokens=k) returns the tensor the
plain device loop returns, whatever the drafts are worth."""
import math
import random

import pytest
import torch

from tests.test_generation_gpu import TINY, make_model
from tests.test_ragged_generation_gpu import _train_step

pytestmark = pytest.mark.gpu

dev = "cuda"
V = TINY["vocab_size"]
B = 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tiny():
    model = make_model(TINY)
    S = torch.randint(0, V, (B, 150), generator=torch.Generator().manual_seed(17)).to(dev)
    return model, S


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_state(a, b):
    """lens, logits and the cache below lens (the caches are torch.empty above it)."""
    assert a.lens == b.lens
    assert torch.equal(bits(a.logits), bits(b.logits))
    for row, n in enumerate(a.lens):
        assert torch.equal(bits(a.kcache[:, row, :, :n]), bits(b.kcache[:, row, :, :n])), row
        assert torch.equal(bits(a.vcache[:, row, :, :n]), bits(b.vcache[:, row, :, :n])), row


def stepped(sess, S, lens, n):
    """n step calls feeding row b the token S[b, lens[b] + i]: the logits after each, [B, n, V]."""
    at = torch.tensor(lens, device=dev)
    return torch.stack([sess.step(S.gather(1, (at + i)[:, None]).squeeze(1)) for i in range(n)], dim=1)


def turn(S, lens, n):
    """tokens [B, n]: row b's next n tokens of S from lens[b] on."""
    at = torch.tensor(lens, device=dev)[:, None] + torch.arange(n, device=dev)[None]
    return S.gather(1, at)


# ---- extend ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 40])  # 3 * 40 rows: split along the token axis into calls of at most 64
def test_extend_has_the_bits_of_as_many_steps(tiny, n):
    model, S = tiny
    a, b = model.decoder(B, max_len=70), model.decoder(B, max_len=70)
    a.prefill(S[:, :7].contiguous()), b.prefill(S[:, :7].contiguous())
    got = a.extend(S[:, 7:7 + n].contiguous())
    want = stepped(b, S, [7] * B, n)
    assert got.shape == (B, n, V) and got.dtype == torch.float32
    assert torch.equal(bits(got), bits(want))
    same_state(a, b)
    assert a.lens == [7 + n] * B and torch.equal(a.logits[:, :V], got[:, -1])


def test_extend_with_counts_leaves_a_row_of_count_zero_alone(tiny):
    model, S = tiny
    a, b = model.decoder(B, max_len=70), model.decoder(B, max_len=70)
    a.prefill(S[:, :7].contiguous()), b.prefill(S[:, :7].contiguous())
    before = (a.logits[0].clone(), a.kcache[:, 0].clone(), a.vcache[:, 0].clone())
    counts = [0, 3, 5]
    got = a.extend(S[:, 7:12].contiguous(), counts)
    assert a.lens == [7, 10, 12]
    assert torch.equal(bits(a.logits[0]), bits(before[0]))
    assert torch.equal(bits(a.kcache[:, 0]), bits(before[1])) and torch.equal(bits(a.vcache[:, 0]), bits(before[2]))
    for row, c in enumerate(counts):  # each row against a one-row session stepped c times
        one = model.decoder(1, max_len=70)
        one.prefill(S[row:row + 1, :7].contiguous())
        for j in range(c):
            assert torch.equal(bits(one.step(S[row:row + 1, 7 + j])[0]), bits(got[row, j])), (row, j)
        assert bool(torch.isnan(got[row, c:]).all()) and bool(torch.isfinite(got[row, :c]).all())
        if c:
            assert torch.equal(bits(one.logits[0]), bits(a.logits[row]))
            assert torch.equal(bits(one.kcache[:, 0, :, :7 + c]), bits(a.kcache[:, row, :, :7 + c]))


def test_extend_after_a_ragged_prefill_is_a_second_turn(tiny):
    model, S = tiny
    lens = [3, 17, 40]
    a, b = model.decoder(B, max_len=70), model.decoder(B, max_len=70)
    a.prefill(S[:, :40].contiguous(), lens), b.prefill(S[:, :40].contiguous(), lens)
    got = a.extend(turn(S, lens, 5))
    assert torch.equal(bits(got), bits(stepped(b, S, lens, 5)))
    same_state(a, b)
    # and the sessions go on alike: 5 tokens of the device loop on both sides
    seqs = [torch.zeros(B, 70, dtype=torch.int64, device=dev) for _ in range(2)]
    toks = [s.generate(5, 0.8, 20, None, 3, seq=q).clone() for s, q in zip((a, b), seqs)]
    assert torch.equal(toks[0], toks[1]) and torch.equal(seqs[0], seqs[1])
    same_state(a, b)


def test_extend_from_an_empty_cache_and_after_a_drawn_token(tiny):
    model, S = tiny
    a, b = model.decoder(B, max_len=70), model.decoder(B, max_len=70)
    got = a.extend(S[:, :6].contiguous())
    first = b.extend(S[:, :1].contiguous())
    assert torch.equal(bits(got[:, :1]), bits(first)) and torch.equal(bits(got[:, 1:]), bits(stepped(b, S, [1] * B, 5)))
    same_state(a, b)
    # a token generate() drew and has not stepped is stepped first, as refill does
    for s in (a, b):
        s.generate(3, 0.0, seed=0)
    tok = a._tok.clone()
    assert a._drawn and a.lens == [8] * B
    a.extend(S[:, 20:22].contiguous())
    b.step(tok), b.step(S[:, 20]), b.step(S[:, 21])
    assert not a._drawn
    same_state(a, b)
    with pytest.raises(ValueError, match="do not fit"):
        a.extend(S[:, :60].contiguous())
    with pytest.raises(ValueError, match="counts"):
        a.extend(S[:, :4].contiguous(), [1, 2, 5])
    assert a.lens == b.lens


# ---- generate(draft_tokens=k) ------------------------------------------------------------------------------------------
N, KD = 40, 4
SAMPLERS = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.8, top_k=50, top_p=0.95)}
PROMPTS = {"B1": (slice(0, 1), None), "B3-ragged": (slice(0, 3), [3, 17, 9])}


@pytest.fixture(scope="module")
def plain(tiny):
    """The plain device loop's result of every case, computed once: (sampler, prompts, eos?) -> tensor."""
    model, S = tiny
    out = {}
    for s, kw in SAMPLERS.items():
        for p, (rows, lens) in PROMPTS.items():
            idx = S[rows, :17].contiguous()
            full = model.generate(idx, N, seed=1, prompt_lens=lens, **kw)
            out[s, p, None] = full
            # an eos that stops some rows early: what row 0 emits as its 10th token
            eos = int(full[0, (lens[0] if lens else 17) + 9])
            out[s, p, "eos"] = (eos, model.generate(idx, N, seed=1, prompt_lens=lens, eos_token_id=eos, **kw))
    return out


def continuation(rows):
    """draft_fn that replays recorded sequences: the tokens that follow `history` in the row that starts with it."""
    def fn(history, m):
        for row in rows:
            if row[:len(history)] == history:
                return row[len(history):len(history) + m]
        raise AssertionError("a history that no recorded row starts with")
    return fn


def scripted(kind, rows):
    right = continuation(rows)
    rng = random.Random(11)
    if kind == "right":
        return right
    wrong = lambda h, m: [(t + 1) % V for t in right(h, m)]  # noqa: E731
    if kind == "wrong":
        return wrong
    return lambda h, m: (right if rng.random() < 0.5 else wrong)(h, m)


@pytest.mark.parametrize("draft", [None, "right", "wrong", "half"])
@pytest.mark.parametrize("eos", [None, "eos"])
@pytest.mark.parametrize("p", PROMPTS)
@pytest.mark.parametrize("s", SAMPLERS)
def test_generate_with_draft_tokens_returns_the_plain_loops_tokens(tiny, plain, s, p, eos, draft):
    model, S = tiny
    rows, lens = PROMPTS[p]
    idx = S[rows, :17].contiguous()
    want = plain[s, p, eos]
    eos_id = None
    if eos:
        eos_id, want = want
        assert bool((want == eos_id).any()) and want.size(1) <= 17 + N
    if draft is None:
        fn = None  # ngram_draft
    else:  # the eos-free run's rows without their padding: the eos run agrees with them up to its eos
        fn = scripted(draft, [row[:(lens[i] if lens else 17) + N] for i, row in enumerate(plain[s, p, None].tolist())])
    got = model.generate(idx, N, seed=1, prompt_lens=lens, eos_token_id=eos_id, draft_tokens=KD, draft_fn=fn,
                         **SAMPLERS[s])
    assert torch.equal(got, want)


@pytest.mark.parametrize("s", SAMPLERS)
def test_speculate_counts_its_calls_and_leaves_the_plain_calls_state(tiny, s):
    """B = 1: an always-right draft needs ceil((n - 1) / (k + 1)) verify calls, an always-wrong one n - 1, a half-right
    one a number in between; tokens and the final session state are the plain call's in all three."""
    model, S = tiny
    kw = SAMPLERS[s]
    args = (kw["temperature"], kw.get("top_k"), kw.get("top_p"), 1)
    prompt = S[:1, :17].contiguous()
    ref = model.decoder(1, max_len=17 + N)
    ref.prefill(prompt)
    seq0 = torch.zeros(1, 17 + N, dtype=torch.int64, device=dev)
    seq0[:, :17] = prompt
    tok0 = ref.generate(N, *args, seq=seq0).clone()
    rows = seq0.tolist()
    calls = {}
    for kind in ("right", "wrong", "half"):
        sess = model.decoder(1, max_len=17 + N)
        sess.prefill(prompt)
        seq = torch.zeros(1, 17 + N, dtype=torch.int64, device=dev)
        seq[:, :17] = prompt
        stats = sess.speculate(N, KD, scripted(kind, rows), *args, seq=seq)
        assert torch.equal(seq, seq0) and torch.equal(sess._tok, tok0) and sess._drawn
        same_state(sess, ref)
        assert stats["tokens"] == N and 0 <= stats["accepted"] <= stats["drafted"]
        calls[kind] = stats["calls"]
        if kind == "right":
            assert stats["accepted"] == stats["drafted"] == N - 1 - stats["calls"]
        if kind == "wrong":
            assert stats["accepted"] == 0
    assert calls["right"] == math.ceil((N - 1) / (KD + 1)) and calls["wrong"] == N - 1
    assert calls["right"] < calls["half"] < calls["wrong"], calls
    # the sessions go on alike after the drawn token is flushed
    sess.flush(), ref.flush()
    same_state(sess, ref)
    with pytest.raises(ValueError, match="64 rows"):
        model.decoder(13, max_len=20).speculate(2, 4)  # (the row budget is checked before anything runs)


def test_speculate_refuses_out_of_vocabulary_drafts(tiny):
    model, S = tiny
    sess = model.decoder(1, max_len=30)
    sess.prefill(S[:1, :5].contiguous())
    with pytest.raises(ValueError, match="vocab_size"):
        sess.speculate(8, 2, lambda h, m: [V] * m, 0.0)


# ---- training is not perturbed -----------------------------------------------------------------------------------------
def test_speculative_generate_between_steps_leaves_training_bit_identical():
    batches = torch.randint(0, 509, (2, 2, 65), generator=torch.Generator().manual_seed(3)).to(dev)
    runs = []
    for with_generate in (False, True):
        model = make_model(TINY)
        opt = model.configure_optimizers(learning_rate=1e-2)
        _train_step(model, opt, batches[0])
        if with_generate:
            seed, token = model.engine()._step_seed, model.engine()._fwd_token
            model.generate(batches[0, :, :12].contiguous(), 20, temperature=0.8, top_k=20, seed=1, draft_tokens=4)
            assert (model.engine()._step_seed, model.engine()._fwd_token) == (seed, token)
            assert model.training
        loss = _train_step(model, opt, batches[1])
        runs.append((loss, model.transformer.h[0].attn.qkv.weight.detach().clone(), model.engine()._step_seed))
    (l0, w0, s0), (l1, w1, s1) = runs
    assert torch.equal(l0, l1) and torch.equal(w0, w1) and s0 == s1
