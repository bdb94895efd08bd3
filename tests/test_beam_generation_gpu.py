"""Beam search on the MI355X: GPT2.generate(num_beams=) and DecodeSession.beam_search (gpt2mi_decode_beam_search).

The device loop is held, bit for bit, to the same search composed on the host from pieces that have tests of their own:
gpt2mi_sample_logprobs (greedy, top_n = W) on the session's logits, generation.beam_select, torch.index_select on the
session's cache tensors and on the token rows, and DecodeSession.step. A wrong tie order, a reorder that reads what it
is writing (rows swap all the time), a window off by one position or a moved prompt all change tokens within a few
steps. Beside that: one beam is the greedy call, a prompt's result does not depend on its batch, the cumulative
log-probability is what a fresh session assigns to the returned tokens, and training is not perturbed."""
import functools

import pytest
import torch

from gpt_2_distributed_amd import _lib as K
from gpt_2_distributed_amd.generation import EOS_CHUNK, LogprobBuffer, beam_rank, beam_select, token_logprobs
from tests.test_generation_gpu import TINY, _train_step, make_model

pytestmark = pytest.mark.gpu

dev = "cuda"
V = TINY["vocab_size"]
LENS = (1, 31, 33, 64)  # one ragged batch: every group crosses a boundary between two ranges of 32 keys within N tokens
N = 40
assert N > EOS_CHUNK  # generate() with eos issues more than one chunk


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def model():
    torch.manual_seed(11)
    return make_model(TINY)


def prompts():
    g = torch.Generator().manual_seed(21)
    return [torch.randint(0, V, (n,), generator=g).to(dev) for n in LENS]


def beams_of(m, ps, W, kv, share=True):
    """A session whose rows b W .. b W + W - 1 are forks of prompt b, and the token buffer that holds the prompts."""
    sess = m.decoder(len(ps) * W, max(p.numel() for p in ps) + N, kv_dtype=kv)
    seq = torch.zeros(sess.B, sess.Tcap, dtype=torch.int64, device=dev)
    for b, p in enumerate(ps):
        sess.refill(b * W, p)
        sess.fork(b * W, range(b * W + 1, b * W + W), share=share)
        seq[b * W:b * W + W, :p.numel()] = p
    return sess, seq


def first_state(R, W):
    cum = torch.full((R,), float("-inf"), device=dev)
    cum[::W] = 0.0
    return cum, torch.zeros(R, dtype=torch.uint8, device=dev)


@functools.lru_cache(maxsize=None)
def host_search(W, kv, eos):
    """The search composed on the host: (seq, cum, done, parents [N, R]) on the CPU, and whether a step re-parented a
    beam and whether a beam was finished while another of its group was live."""
    m, ps = model(), prompts()
    sess, seq = beams_of(m, ps, W, kv, share=False)  # (unshared: the composition does not lean on the share map)
    R = sess.B
    cum, done = (t.cpu().numpy() for t in first_state(R, W))
    parents, mixed = [], False
    tok_d = torch.empty(R, dtype=torch.int64, device=dev)
    for i in range(N):
        buf = LogprobBuffer(R, 1, W, dev)
        K.sample_logprobs(sess.logits, V, 0.0, None, None, 0, sess.lens, tok_d, **buf.tensors(), col=[0] * R)
        tok, parent, cum, done = beam_select(cum, done, buf.top_ids[:, 0], buf.top_logprobs[:, 0], eos, W)
        par = torch.from_numpy(parent).long().to(dev)
        for t in (sess.kcache, sess.vcache, sess.kscale, sess.vscale):
            if t is not None:
                t.copy_(t.index_select(1, par))
        seq = seq.index_select(0, par)
        new = torch.from_numpy(tok).to(dev)
        seq[torch.arange(R, device=dev), torch.tensor(sess.lens, device=dev)] = new
        parents.append(parent)
        fin = done.reshape(-1, W)
        mixed = mixed or bool(((fin.sum(1) > 0) & (fin.sum(1) < W)).any())
        if i + 1 < N:
            sess.step(new)
    parents = torch.tensor([p.tolist() for p in parents], dtype=torch.int32)
    moved = bool((parents != torch.arange(R, dtype=torch.int32)[None]).any())
    return seq.cpu(), torch.from_numpy(cum), torch.from_numpy(done), parents, moved, mixed


def frequent_token(W, kv):
    """The token that occurs most often in what the eos-free search generated."""
    seq = host_search(W, kv, None)[0]
    new = torch.cat([seq[b * W:b * W + W, n:n + N].reshape(-1) for b, n in enumerate(LENS)])
    return int(new.bincount().argmax())


def device_search(W, kv, eos):
    sess, seq = beams_of(model(), prompts(), W, kv)
    cum, done = first_state(sess.B, W)
    parents = torch.full((N, sess.B), -1, dtype=torch.int32, device=dev)
    sess.beam_search(N, W, eos, seq, cum, done, parents=parents)
    return seq.cpu(), cum.cpu(), done.cpu(), parents.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def check_against_host(W, kv):
    for eos in (None, frequent_token(W, kv)):
        want = host_search(W, kv, eos)
        seq, cum, done, parents = device_search(W, kv, eos)
        where = f"W={W} kv={kv} eos={eos}"
        assert torch.equal(parents, want[3]), where
        assert torch.equal(seq, want[0]), where
        assert torch.equal(bits(cum), bits(want[1])) and torch.equal(done, want[2]), where
        assert want[4], f"{where}: no step re-parented a beam: the comparison proves nothing about the reorder"
        if eos is not None:
            assert want[5], f"{where}: no beam finished while another was live"
        # generate(): the same search in chunks of EOS_CHUNK tokens, then the ranking
        out = model().generate(prompts(), N, num_beams=W, num_return_sequences=W, eos_token_id=eos, kv_dtype=kv)
        m = out.tokens.size(2) - max(LENS)
        for b, n in enumerate(LENS):
            rows = slice(b * W, b * W + W)
            new = seq[rows, n:n + N]
            length = torch.full((W,), N)
            if eos is not None:
                hit = new == eos
                length = torch.where(hit.any(1), hit.int().argmax(1) + 1, length)
            order = beam_rank(cum[rows], length, 1.0)[0]
            assert torch.equal(bits(out.cum_logprob[b].cpu()), bits(cum[rows][order])), where
            assert torch.equal(out.lengths[b].cpu(), length[order]), where
            for j, r in enumerate(order.tolist()):
                k = int(length[r])
                assert torch.equal(out.tokens[b, j, :n + k].cpu(), seq[b * W + r, :n + k]), where
                pad = 0 if eos is None else eos
                assert bool((out.tokens[b, j, n + k:] == pad).all()), where
        assert m <= N


# ---- 1. one beam is greedy -----------------------------------------------------------------------------------------------
def test_one_beam_is_the_greedy_call():
    m, ps = model(), prompts()
    greedy = m.generate(ps, 24, temperature=0.0, seed=0, logprobs=True)
    out = m.generate(ps, 24, num_beams=1)
    assert out.tokens.shape == (len(ps), 1, max(LENS) + 24)
    assert torch.equal(out.tokens[:, 0], greedy.tokens)
    acc = torch.zeros(len(ps))
    for b, n in enumerate(LENS):
        for c in range(n, n + 24):  # the sequential fp32 sum, in column order
            acc[b] = acc[b] + greedy.logprobs[b, c].cpu()
    assert torch.equal(bits(out.cum_logprob[:, 0].cpu()), bits(acc))
    assert out.lengths.tolist() == [[24]] * len(ps)
    assert torch.equal(out.scores.cpu(), out.cum_logprob.double().cpu() / 24)


# ---- 2. the device loop equals the host composition; 4. with an fp8 cache ---------------------------------------------------
@pytest.mark.parametrize("W", [2, 4, 5])
def test_device_loop_equals_the_host_composition(W):
    check_against_host(W, "bf16")


@pytest.mark.parametrize("W", [2, 4, 5])
def test_device_loop_equals_the_host_composition_fp8(W):
    check_against_host(W, "fp8")


# ---- 3. batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_eos", [False, True], ids=["no-eos", "eos"])
def test_a_prompts_beams_do_not_depend_on_the_batch(with_eos):
    m, ps, W = model(), prompts(), 4
    eos = frequent_token(W, "bf16") if with_eos else None
    kw = dict(num_beams=W, num_return_sequences=W, eos_token_id=eos, length_penalty=0.7)
    batch = m.generate(ps, N, **kw)
    for b, p in enumerate(ps):
        alone = m.generate([p], N, **kw)
        assert torch.equal(alone.lengths[0], batch.lengths[b])
        assert torch.equal(bits(alone.cum_logprob[0]), bits(batch.cum_logprob[b]))
        assert torch.equal(alone.scores[0], batch.scores[b])
        for j in range(W):
            k = p.numel() + int(alone.lengths[0, j])
            assert torch.equal(alone.tokens[0, j, :k], batch.tokens[b, j, :k]), (b, j)


# ---- fewer returned sequences are the head of the ranking --------------------------------------------------------------------
@pytest.mark.parametrize("with_eos", [False, True], ids=["no-eos", "eos"])
def test_num_return_sequences_returns_the_best_beams(with_eos):
    """r < W, the default call among them, against the first r entries of the r = W result, bitwise in every field; with
    eos and a length penalty that puts the beams in another order than their raw sums do."""
    m, ps, W = model(), prompts(), 4
    eos = frequent_token(W, "bf16") if with_eos else None
    reordered = False
    for lp in (1.0, 2.0) if with_eos else (1.0,):
        kw = dict(num_beams=W, eos_token_id=eos, length_penalty=lp)
        full = m.generate(ps, N, num_return_sequences=W, **kw)
        reordered = reordered or not torch.equal(full.cum_logprob.sort(1, descending=True).values, full.cum_logprob)
        assert bool((full.scores[:, :-1] >= full.scores[:, 1:]).all())
        want = full.cum_logprob.double().cpu() / full.lengths.double().cpu().clamp_min(1) ** lp  # (where beam_rank is)
        assert torch.equal(full.scores.cpu(), want)
        for r in (1, 2):
            part = m.generate(ps, N, **kw) if r == 1 else m.generate(ps, N, num_return_sequences=r, **kw)
            assert part.tokens.shape == (len(ps), r, full.tokens.size(2))
            assert torch.equal(part.tokens, full.tokens[:, :r]) and torch.equal(part.lengths, full.lengths[:, :r])
            assert torch.equal(bits(part.cum_logprob), bits(full.cum_logprob[:, :r]))
            assert torch.equal(part.scores, full.scores[:, :r])
    if with_eos:  # beams of unequal length under a penalty that rewards length: the order is not the raw sums'
        assert reordered, "the length penalty reordered no prompt's beams: the case proves less than it says"


def test_cli_prints_the_returned_beams(monkeypatch, capsys):
    """--num_beams through main(): the lines are those of generate() on the same prompts, prompt-major, best first."""
    import json
    from gpt_2_distributed_amd import generate as cli
    m = model()
    monkeypatch.setattr(cli, "load_model", lambda ckpt, size: m)
    a, b = [3, 1, 4, 1, 5], [9, 2, 6]
    argv = ["--checkpoint", "unused", "--prompt_ids", ",".join(map(str, a)), "--prompt_ids", ",".join(map(str, b)),
            "--max_new_tokens", "12", "--num_beams", "3", "--num_return_sequences", "2", "--length_penalty", "0.5",
            "--kv_dtype", "fp8"]
    assert cli.main(argv) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines()]
    out = m.generate([torch.tensor(q, device=dev) for q in (a, b)], 12, num_beams=3, num_return_sequences=2,
                     length_penalty=0.5, kv_dtype="fp8")
    assert [(x["prompt"], x["beam"]) for x in lines] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for x in lines:
        q, i, j = (a, b)[x["prompt"]], x["prompt"], x["beam"]
        assert x["tokens"] == out.tokens[i, j, :len(q) + 12].tolist() and x["tokens"][:len(q)] == q
        assert x["score"] == float(out.scores[i, j]) and x["cum_logprob"] == float(out.cum_logprob[i, j])
    with pytest.raises(ValueError, match="temperature"):  # a sampler flag the user did give is refused by its name
        cli.main(argv + ["--temperature", "0.7"])


# ---- 5. teacher forcing -------------------------------------------------------------------------------------------------------
def test_cum_logprob_is_what_a_fresh_session_assigns_the_tokens():
    m, ps, W = model(), prompts(), 4
    out = m.generate(ps, N, num_beams=W, num_return_sequences=W)
    R = len(ps) * W
    lens = [n for n in LENS for _ in range(W)]
    toks = out.tokens.reshape(R, -1)
    sess = m.decoder(R, max(LENS) + N)
    idx = torch.where(torch.arange(max(LENS), device=dev)[None] < torch.tensor(lens, device=dev)[:, None],
                      toks[:, :max(LENS)], torch.zeros_like(toks[:, :max(LENS)]))
    logits = sess.prefill(idx, lens)
    total, big = torch.zeros(R, dtype=torch.float64, device=dev), 0.0
    at = torch.tensor(lens, device=dev)
    for i in range(N):
        nxt = toks.gather(1, (at + i)[:, None])[:, 0]
        total += token_logprobs(logits, nxt)[0]
        big = max(big, float(logits.abs().max()))
        if i + 1 < N:
            logits = sess.step(nxt)
    bound = N * (1e-5 + 4 * 2.0 ** -23 * big)
    err = (out.cum_logprob.reshape(R).double() - total).abs().max().item()
    print(f"teacher forcing: max |cum_logprob - sum| = {err:.3e}, bound {bound:.3e}, max |l| = {big:.3f}")
    assert err <= bound


# ---- 6. training is untouched ----------------------------------------------------------------------------------------------
def test_beam_search_between_steps_leaves_training_bit_identical():
    batches = torch.randint(0, 509, (2, 2, 65), generator=torch.Generator().manual_seed(3)).to(dev)
    prompt = batches[0, :, :5].contiguous()
    runs = []
    for with_generate in (False, True):
        m = make_model(TINY)
        opt = m.configure_optimizers(learning_rate=1e-2)
        _train_step(m, opt, batches[0])
        if with_generate:
            seed, token = m.engine()._step_seed, m.engine()._fwd_token
            out = m.generate(prompt, 20, num_beams=4)
            assert out.tokens.shape == (2, 1, 25)
            assert (m.engine()._step_seed, m.engine()._fwd_token) == (seed, token)
            assert m.training
        loss = _train_step(m, opt, batches[1])
        runs.append((loss, m.transformer.h[0].attn.qkv.weight.detach().clone(), m.engine()._step_seed))
    (l0, w0, s0), (l1, w1, s1) = runs
    assert torch.equal(l0, l1) and torch.equal(w0, w1) and s0 == s1
