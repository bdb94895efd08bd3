"""Ragged batched generation on the MI355X: a DecodeSession whose rows sit at different positions, refill, generate with
prompt_lens and generate_many.

Accuracy is held to the project's existing rule (tests/test_generation_gpu.py): teacher-forced on a token matrix S, the
decode path's error against the fp32 oracle is at most twice the error of the eval-mode full forward against the same
oracle, overall and for the worst row. Everything else here is bitwise: a row of a ragged session has the bits that row
has in an equal-length session, a refilled row those of a fresh one-row session, and generate_many's outputs do not
depend on the batch size."""
import json
import subprocess
import sys

import pytest
import torch

from tests.conftest import REPO
from tests.test_generation_gpu import TINY, errs, full_forward, make_model, oracle_logits

pytestmark = pytest.mark.gpu

dev = "cuda"
V = TINY["vocab_size"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tiny():
    """The tiny model, the existing fixture's token matrix, and the two references shared by the tests below."""
    model = make_model(TINY)
    S = torch.randint(0, V, (3, 150), generator=torch.Generator().manual_seed(17)).to(dev)
    full, ref = full_forward(model, S), oracle_logits(model, TINY, S)
    return model, S, full, ref


def ragged_logits(model, S, P, lens, steps):
    """prefill(S[:, :P], lens), then `steps` steps feeding row b the token S[b, lens[b] + i]: [B, steps + 1, V], entry i
    of row b = the logits of position lens[b] - 1 + i."""
    sess = model.decoder(S.size(0))
    lens_t = torch.tensor(lens, device=dev)
    rows = [sess.prefill(S[:, :P].contiguous(), lens)]
    assert sess.lens == list(lens) and (sess.pos is None) == (len(set(lens)) > 1)
    for i in range(steps):
        rows.append(sess.step(S.gather(1, (lens_t + i)[:, None]).squeeze(1)))
    assert sess.lens == [n + steps for n in lens]
    return torch.stack(rows, dim=1)


def equal_length_logits(model, S, P, steps):
    sess = model.decoder(S.size(0))
    rows = [sess.prefill(S[:, :P].contiguous())]
    for i in range(steps):
        rows.append(sess.step(S[:, P + i]))
    return torch.stack(rows, dim=1)


# ---- the session -------------------------------------------------------------------------------------------------------
def test_teacher_forced_parity_of_a_ragged_session(tiny):
    model, S, full, ref = tiny
    lens, steps = [1, 37, 70], 60  # one token, inside a tile, across the 64-token tile edge
    dec = ragged_logits(model, S, 70, lens, steps)
    take = lambda x: torch.stack([x[b, n - 1:n + steps] for b, n in enumerate(lens)])  # noqa: E731
    e_full, e_full_row = errs(take(full), take(ref))
    e_dec, e_dec_row = errs(dec, take(ref))
    print(f"ragged lens={lens}: E_full {e_full:.3e} (row max {e_full_row:.3e}), E_dec {e_dec:.3e} "
          f"(row max {e_dec_row:.3e})")
    assert e_dec <= 2 * e_full, (e_dec, e_full)
    assert e_dec_row <= 2 * e_full_row, (e_dec_row, e_full_row)


def test_rows_of_a_ragged_session_have_the_bits_of_an_equal_length_one(tiny):
    """lens within one 64-token tile, so the padded prefill has the shape of an equal-length one: row b's logits at the
    prefill and at every step are bit-identical to row b of a session prefilled with S[:, :lens[b]] and stepped with
    the same tokens."""
    model, S, _, _ = tiny
    lens, steps = [3, 17, 40], 30
    dec = ragged_logits(model, S, 40, lens, steps)
    for b, n in enumerate(lens):
        want = equal_length_logits(model, S, n, steps)
        assert torch.equal(dec[b, 0], want[b, 0]), (b, "prefill")
        assert torch.equal(dec[b], want[b]), (b, "steps")


def test_refill_replaces_one_row_and_leaves_the_others(tiny):
    model, S, _, _ = tiny
    prompt = S[1, 100:123].contiguous()  # 23 tokens
    toks = S[:, 60:80]

    def run(refill):
        sess = model.decoder(3, 120)
        sess.prefill(S[:, :9].contiguous())
        out = [sess.step(toks[:, i]) for i in range(4)]
        if refill:
            sess.refill(1, prompt)
            assert sess.lens == [13, 23, 13] and sess.pos is None
            out.append(sess.logits[:, :V].clone())
        else:
            out.append(out[-1])
        out += [sess.step(toks[:, i]) for i in range(4, 20)]
        return torch.stack(out, dim=1)
    base, got = run(False), run(True)
    for b in (0, 2):
        assert torch.equal(got[b], base[b]), b
    # row 1: a function of the prompt alone = a fresh one-row session prefilled with it
    one = model.decoder(1, 120)
    want = [one.prefill(prompt[None])] + [one.step(toks[1:2, i]) for i in range(4, 20)]
    assert torch.equal(got[1, 4:], torch.cat(want, dim=0))
    # and sampling: the refilled row draws from (seed, its key, its position)
    sess = model.decoder(3, 120)
    sess.prefill(S[:, :9].contiguous())
    sess.refill(1, prompt)
    tok = sess.sample(0.8, 20, None, 5, row_id=[0, 7, 2])
    one.reset()
    one.prefill(prompt[None])
    assert int(one.sample(0.8, 20, None, 5, row_id=[7])[0]) == int(tok[1])


# ---- generate(prompt_lens=) --------------------------------------------------------------------------------------------
LENS = [3, 17, 40]
SAMPLERS = [dict(temperature=0.0, seed=0), dict(temperature=0.8, top_k=20, top_p=0.9, seed=7)]


@pytest.mark.parametrize("kw", SAMPLERS, ids=["greedy", "seeded"])
def test_generate_with_prompt_lens_equals_equal_length_batches(tiny, kw):
    model, S, _, _ = tiny
    n, pad = 24, 508
    out = model.generate(S[:, :40].contiguous(), n, prompt_lens=LENS, pad_token_id=pad, **kw)
    assert out.shape == (3, 40 + n) and out.dtype == torch.int64
    as_list = model.generate([S[b, :L] for b, L in enumerate(LENS)], n, pad_token_id=pad, **kw)
    assert torch.equal(out, as_list)
    for b, L in enumerate(LENS):
        want = model.generate(S[:, :L].contiguous(), n, **kw)  # an equal-length batch whose row b is the same prompt
        assert torch.equal(out[b, :L], S[b, :L])
        assert torch.equal(out[b, L:L + n], want[b, L:]), b
        assert bool((out[b, L + n:] == pad).all())
    assert model.training


def test_generate_with_prompt_lens_host_sampler_and_eos(tiny):
    model, S, _, _ = tiny
    n = 24
    idx = S[:, :40].contiguous()
    greedy = model.generate(idx, n, prompt_lens=LENS, temperature=0.0, seed=0)
    assert torch.equal(model.generate(idx, n, prompt_lens=LENS, temperature=0.0), greedy)  # the host loop
    new = torch.stack([greedy[b, L:L + n] for b, L in enumerate(LENS)])
    # an eos that row 0 emits first at step 5 (if its earlier tokens differ from it), else wherever it first occurs
    eos = int(new[0, 5])
    first = [(new[b].tolist() + [eos]).index(eos) for b in range(3)]
    m = min(n, max(first) + 1)  # the existing cut: the step by which every row has emitted eos
    for how in (dict(seed=0), dict()):
        out = model.generate(idx, n, prompt_lens=LENS, temperature=0.0, eos_token_id=eos, **how)
        assert out.shape == (3, 40 + m), (how, out.shape, first)
        for b, L in enumerate(LENS):
            got, stop = out[b, L:L + m].tolist(), min(first[b], m)
            assert torch.equal(out[b, :L], S[b, :L])
            assert got[:stop] == new[b, :stop].tolist() and all(t == eos for t in got[stop:]), (how, b)
            assert bool((out[b, L + m:] == eos).all())  # pad_token_id defaults to eos_token_id
    # the equal-length paths give the same cut for the same rows
    same = model.generate(S[:, :17].contiguous(), n, temperature=0.0, eos_token_id=eos, seed=0)
    ragged = model.generate(S[:, :17].contiguous(), n, prompt_lens=[17] * 3, temperature=0.0, eos_token_id=eos, seed=0)
    assert torch.equal(same, ragged)
    with pytest.raises(ValueError, match="n_positions"):
        model.generate(S[:, :150], 43, prompt_lens=[1, 2, 150])
    assert model.generate(S[:, :150], 42, prompt_lens=[1, 2, 150], temperature=0.0, seed=0).shape == (3, 192)


# ---- generate_many -----------------------------------------------------------------------------------------------------
MANY = dict(temperature=0.8, top_k=20, seed=3)
MANY_LENS = [1, 5, 64, 65, 9, 30, 2]


@pytest.fixture(scope="module")
def many(tiny):
    model, S, _, _ = tiny
    src = torch.randint(0, V, (7, 65), generator=torch.Generator().manual_seed(29)).to(dev)
    prompts = [src[i, :L].contiguous() for i, L in enumerate(MANY_LENS)]
    return prompts, model.generate_many(prompts, 20, batch_size=3, **MANY)


def test_generate_many_does_not_depend_on_the_batch_size(tiny, many):
    model = tiny[0]
    prompts, at3 = many
    assert len(at3) == 7
    for o, p in zip(at3, prompts):
        assert o.dtype == torch.int64 and o.numel() == p.numel() + 20 and torch.equal(o[:p.numel()], p)
    for bs in (2, 7):
        got = model.generate_many(prompts, 20, batch_size=bs, **MANY)
        assert all(torch.equal(g, w) for g, w in zip(got, at3)), bs
    assert model.training


def test_generate_many_equals_single_prompt_runs_with_the_same_row_id(tiny, many):
    """Prompt i alone in a one-row session, drawing with key i: sample, step, sample, ... through the session."""
    model = tiny[0]
    prompts, at3 = many
    for i, p in enumerate(prompts):
        sess = model.decoder(1, p.numel() + 20)
        sess.prefill(p[None])
        seq = torch.zeros(1, p.numel() + 20, dtype=torch.int64, device=dev)
        sess.generate(20, MANY["temperature"], MANY["top_k"], None, MANY["seed"], seq=seq, row_id=[i])
        assert torch.equal(seq[0, p.numel():], at3[i][p.numel():]), i


def test_generate_many_with_eos_is_cut_and_still_batch_independent(tiny, many):
    model = tiny[0]
    prompts, at3 = many
    new = [o[p.numel():].tolist() for o, p in zip(at3, prompts)]
    eos = new[2][7]  # a token some rows emit early (row 2 by step 7 at the latest) and others never
    stops = [(t + [eos]).index(eos) for t in new]
    assert min(stops) < 20
    runs = [model.generate_many(prompts, 20, batch_size=bs, eos_token_id=eos, **MANY) for bs in (2, 3, 7)]
    for got in runs[1:]:
        assert all(torch.equal(g, w) for g, w in zip(got, runs[0]))
    for o, p, t, stop in zip(runs[0], prompts, new, stops):
        assert o.tolist() == p.tolist() + t[:stop + 1]  # the tokens of the run without eos, through the first eos
        if stop < 20:
            assert int(o[-1]) == eos and eos not in o[p.numel():-1].tolist()


# ---- training is not perturbed -----------------------------------------------------------------------------------------
def _train_step(model, opt, batch):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, loss = model(batch[:, :-1], labels=batch[:, 1:])
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss.detach().clone()


def test_generate_many_between_steps_leaves_training_bit_identical():
    batches = torch.randint(0, 509, (2, 2, 65), generator=torch.Generator().manual_seed(3)).to(dev)
    prompts = [batches[0, 0, :5].contiguous(), batches[0, 1, :12].contiguous(), batches[1, 0, :2].contiguous()]
    runs = []
    for with_generate in (False, True):
        model = make_model(TINY)
        opt = model.configure_optimizers(learning_rate=1e-2)
        _train_step(model, opt, batches[0])
        if with_generate:
            seed, token = model.engine()._step_seed, model.engine()._fwd_token
            model.generate_many(prompts, 12, batch_size=2, temperature=1.0, top_k=10, seed=1)
            model.generate(prompts, 6, temperature=0.0, seed=1)
            assert (model.engine()._step_seed, model.engine()._fwd_token) == (seed, token)
            assert model.training
        loss = _train_step(model, opt, batches[1])
        runs.append((loss, model.transformer.h[0].attn.qkv.weight.detach().clone(), model.engine()._step_seed))
    (l0, w0, s0), (l1, w1, s1) = runs
    assert torch.equal(l0, l1) and torch.equal(w0, w1) and s0 == s1


# ---- the CLI: a fresh child process ------------------------------------------------------------------------------------
def test_cli_serves_several_prompts_through_generate_many(tmp_path):
    from gpt_2_distributed_amd.train_gpt2_distributed import save_checkpoint
    model = make_model(TINY)
    ckpt = save_checkpoint(model, model.configure_optimizers(), 3, str(tmp_path))
    (tmp_path / "prompts.txt").write_text("21,22,23,24,25,26,27\n\n31\n")
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.generate", "--checkpoint", ckpt, "--model", "auto",
           "--prompt_ids", "11,12,13", "--prompts_file", str(tmp_path / "prompts.txt"), "--max_new_tokens", "9",
           "--batch", "2", "--temperature", "0.8", "--top_k", "20", "--seed", "5", "--sampler", "device"]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("[")]
    prompts = [[11, 12, 13], [21, 22, 23, 24, 25, 26, 27], [31]]
    want = model.generate_many([torch.tensor(p, device=dev) for p in prompts], 9, batch_size=3, temperature=0.8,
                               top_k=20, seed=5)
    assert rows == [w.tolist() for w in want]  # input order; (seed, prompt index, position) decide the draws
    assert [r[:len(p)] for r, p in zip(rows, prompts)] == prompts and all(len(r) == len(p) + 9 for r, p in zip(rows, prompts))
