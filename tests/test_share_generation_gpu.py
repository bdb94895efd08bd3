"""DecodeSession.fork and GPT2.generate(num_samples=) on the MI355X: several samples of one prompt over one shared
prompt cache give, bit for bit, what the same rows give when each is filled and read on its own.

The plan entries (step, generate) launch the shared kernel only from 16 sharing rows on (rows of a group with two
members and a full range of 32 shared keys; csrc/decode.hip GPT2MI_SHARE_MIN_ROWS). So every session case here runs
twice: at the few rows the feature was specified with, where ``fork``'s copies and the bookkeeping are what is under
test and the launch is the unshared one, and at 16 or more sharing rows ("shared-launch" in the ids), where the plan
does launch the shared kernel and the comparison with a session that does not share is a test of that launch. The
prompts of the large cases are 40 and 70 tokens and the runs go past position 96, so shared ranges, the range that
straddles shared_len and range boundaries above it are all crossed while sharing."""
import pytest
import torch

from tests.test_generation_gpu import TINY, make_model

pytestmark = pytest.mark.gpu

dev = "cuda"
KV = ("bf16", "fp8")
SAMPLER = dict(temperature=0.8, top_k=20, seed=3)
FEW_AND_SHARED = [pytest.param(5, id="5-rows"), pytest.param(17, id="17-rows-shared-launch")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(11)
    return make_model(TINY)


@pytest.fixture(scope="module")
def wide():
    """L2 H12 C768 V50257: the head count and vocabulary of the production model."""
    torch.manual_seed(3)
    return make_model(dict(n_layer=2, n_head=12, n_embd=768, vocab_size=50257, n_positions=128, resid_pdrop=0.0,
                           attn_pdrop=0.0))


def prompt_of(n, seed=0):
    return torch.randint(0, TINY["vocab_size"], (n,), generator=torch.Generator().manual_seed(100 + seed)).to(dev)


def filled(model, kv, B, prompt, how, max_len=None):
    """A session of B rows that all hold ``prompt``: "refill" every row, or refill row 0 and fork it with share = how."""
    sess = model.decoder(B, max_len, kv_dtype=kv)
    if how == "refill":
        for b in range(B):
            sess.refill(b, prompt)
    else:
        sess.refill(0, prompt)
        sess.fork(0, range(1, B), share=how)
    return sess


def seq_for(sess, prompts, width):
    seq = torch.zeros(sess.B, width, dtype=torch.int64, device=dev)
    for b, p in enumerate(prompts):
        seq[b, :p.numel()] = p
    return seq


def state(sess):
    """logits, lens and the caches below lens (they are torch.empty above)."""
    out = [sess.logits.clone(), list(sess.lens)]
    for t in (sess.kcache, sess.vcache, sess.kscale, sess.vscale):
        if t is not None:
            out.append([t[:, b, :, :n].clone() for b, n in enumerate(sess.lens)])
    return out


def assert_same_state(a, b):
    assert a[1] == b[1]
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    for ta, tb in zip(a[2:], b[2:]):
        for xa, xb in zip(ta, tb):
            assert torch.equal(xa.view(torch.uint8), xb.view(torch.uint8))


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("rows", FEW_AND_SHARED)
def test_fork_against_refill(tiny, kv, rows):
    """Positions 70 .. 109: two shared ranges, the straddling one, and the boundary at 96 above them."""
    prompt = prompt_of(70)
    got = []
    for how in ("refill", True, False):
        sess = filled(tiny, kv, rows, prompt, how)
        assert sess.share_len == ([70] * rows if how is True else [0] * rows)
        assert sess.share_group == ([0] * rows if how is True else list(range(rows)))
        seq = seq_for(sess, [prompt] * rows, 70 + 40)
        sess.generate(40, seq=seq, **SAMPLER)
        sess.flush()
        got.append((seq, state(sess)))
    assert len({tuple(r) for r in got[0][0][:, 70:].tolist()}) > 1  # the samples differ: the rows are not one row
    for seq, st in got[1:]:
        assert torch.equal(seq, got[0][0])
        assert_same_state(st, got[0][1])


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("rows", FEW_AND_SHARED)
def test_steps_of_a_shared_session_are_those_of_an_unshared_one(tiny, kv, rows):
    prompt = prompt_of(70, 1)
    a, b = filled(tiny, kv, rows, prompt, True), filled(tiny, kv, rows, prompt, False)
    gen = torch.Generator().manual_seed(2)
    for _ in range(40):
        tok = torch.randint(0, TINY["vocab_size"], (rows,), generator=gen).to(dev)
        la, lb = a.step(tok), b.step(tok)
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert a.lens == b.lens == [110] * rows and a.share_len == [70] * rows
    assert_same_state(state(a), state(b))


def two_prompts(model, kv, share, s, short):
    """Rows 0 .. s-1 samples of a ``short``-token prompt, rows s .. 2s-1 of a 70-token one; in the large layout a last
    row alone with a prompt of its own, which is in no group."""
    alone = s > 3
    sess = model.decoder(2 * s + alone, kv_dtype=kv)
    prompts = [prompt_of(short, 2)] * s + [prompt_of(70, 3)] * s + [prompt_of(9, 15)] * alone
    for b in (0, s):
        sess.refill(b, prompts[b])
        sess.fork(b, range(b + 1, b + s), share=share)
    if alone:
        sess.refill(2 * s, prompts[2 * s])
    return sess, prompts


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("s, short", [pytest.param(3, 5, id="2x3"), pytest.param(9, 40, id="2x9+1-shared-launch")])
def test_two_prompts_and_a_refill_of_a_source_row_mid_run(tiny, kv, s, short):
    """2 x 3 with prompts of 5 and 70 tokens is the layout the feature was specified with (6 rows, of which the 5-token
    group has no full range: the unshared launch). 2 x 9 + 1 with prompts of 40 and 70 shares in both groups, at
    different lengths, beside a row in no group, and stays above the row threshold when the second group's lowest row
    is refilled (9 + 8 = 17 sharing rows): its next row becomes the one the shared ranges are read from."""
    n, lone = 16, [2 * s] * (s > 3)
    runs = {}
    for name, share, refill in (("plain", False, False), ("shared", True, False), ("refilled", True, True)):
        sess, prompts = two_prompts(tiny, kv, share, s, short)
        if share:
            assert sess.share_group == [0] * s + [s] * s + lone
            assert sess.share_len == [short] * s + [70] * s + [0] * len(lone)
        seq = seq_for(sess, prompts, 120)
        sess.generate(n, seq=seq, **SAMPLER)
        if refill:  # the source of the second group is replaced: its other rows go on, row s + 1 now the lowest
            other = prompt_of(9, 4)
            sess.refill(s, other)
            assert sess.share_group == [0] * s + [s] + [s + 1] * (s - 1) + lone
            assert sess.share_len == [short] * s + [0] + [70] * (s - 1) + [0] * len(lone)
            assert sess.lens == [short + n] * s + [9] + [70 + n] * (s - 1) + [9 + n] * len(lone)
            seq[s] = 0
            seq[s, :9] = other
        else:
            sess.flush()
        sess.generate(n, seq=seq, **SAMPLER)  # to positions 70 + 32: past 96
        runs[name] = seq
    assert torch.equal(runs["shared"], runs["plain"])
    keep = [b for b in range(2 * s + len(lone)) if b != s]
    assert torch.equal(runs["refilled"][keep], runs["plain"][keep])
    assert not torch.equal(runs["refilled"][s], runs["plain"][s])


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("rows", [pytest.param(4, id="4-rows"), pytest.param(17, id="17-rows-shared-launch")])
def test_extend_on_a_forked_session_equals_as_many_steps(tiny, kv, rows):
    """``extend`` itself is unshared; at 17 rows the steps it is compared with, and the step after it, are shared, and
    the unshared session ``c`` says that they are right and not only equal to each other."""
    prompt = prompt_of(40, 5)
    a, b, c = (filled(tiny, kv, rows, prompt, share) for share in (True, True, False))
    toks = torch.randint(0, TINY["vocab_size"], (rows, 3), generator=torch.Generator().manual_seed(6)).to(dev)
    la = a.extend(toks)
    for j in range(3):
        lb, lc = b.step(toks[:, j]), c.step(toks[:, j])
        assert torch.equal(la[:, j].view(torch.int32), lb.view(torch.int32))
        assert torch.equal(lc.view(torch.int32), lb.view(torch.int32))
    assert a.share_len == [40] * rows
    assert_same_state(state(a), state(b))
    assert_same_state(state(a), state(c))
    tok = prompt_of(rows, 7)
    after = a.step(tok).view(torch.int32).clone()  # and the step after an extend goes on over the shared prompt
    assert torch.equal(after, b.step(tok).view(torch.int32)) and torch.equal(after, c.step(tok).view(torch.int32))


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("rows", [pytest.param(4, id="4-rows"), pytest.param(16, id="16-rows-shared-launch")])
def test_speculate_on_a_forked_session_returns_the_plain_loops_tokens(tiny, kv, rows):
    """The verify calls of ``speculate`` are unshared; the plain loop it is compared with shares at 16 rows (the
    threshold itself, and with 3 drafts the 64 rows a verify call may have), and the loop of a session that does not
    share gives the tokens of both."""
    prompt = torch.cat([prompt_of(10, 8)] * 4)  # repeats: prompt-lookup drafts get accepted
    out = []
    for share, spec in ((True, False), (True, True), (False, False)):
        sess = filled(tiny, kv, rows, prompt, share)
        seq = seq_for(sess, [prompt] * rows, 40 + 24)
        if spec:
            stats = sess.speculate(24, 3, seq=seq, **SAMPLER)
            assert stats["tokens"] == rows * 24
        else:
            sess.generate(24, seq=seq, **SAMPLER)
        out.append(seq)
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("pen", [{}, dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2)],
                         ids=["plain", "penalties"])
@pytest.mark.parametrize("s, short", [pytest.param(3, 5, id="2x3"), pytest.param(9, 40, id="2x9-shared-launch")])
def test_num_samples_equals_generate_many_over_the_repeated_list(tiny, kv, pen, s, short):
    """``generate_many`` refills every row and never shares, so at 2 x 9 (18 sharing rows, groups of 40 and 70 shared
    tokens, positions up to 93) it is the unshared reference of the loop ``num_samples`` runs shared."""
    prompts = [prompt_of(short, 9), prompt_of(70, 10)]
    out = tiny.generate(prompts, 24, seed=1, num_samples=s, kv_dtype=kv, **pen)
    assert out.shape == (2 * s, 70 + 24)
    many = tiny.generate_many([p for p in prompts for _ in range(s)], 24, batch_size=2 * s, seed=1, kv_dtype=kv, **pen)
    for r, m in enumerate(many):
        n = m.numel()
        assert n == prompts[r // s].numel() + 24
        assert torch.equal(out[r, :n], m), r
    assert not torch.equal(out[0], out[1])
    # the padded form of the same call, and the host sampler, take the same route
    idx = torch.zeros(2, 70, dtype=torch.int64, device=dev)
    idx[0, :short], idx[1] = prompts[0], prompts[1]
    assert torch.equal(tiny.generate(idx, 24, seed=1, num_samples=s, prompt_lens=[short, 70], kv_dtype=kv, **pen), out)
    host = tiny.generate(idx[1:], 6, temperature=0.0, num_samples=2, kv_dtype=kv, **pen)
    assert host.shape == (2, 76) and torch.equal(host[0], host[1])
    assert torch.equal(host, tiny.generate(idx[1:], 6, temperature=0.0, seed=0, num_samples=2, kv_dtype=kv, **pen))


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("s, reps", [pytest.param(4, 3, id="1x4"), pytest.param(16, 5, id="1x16-shared-launch")])
def test_num_samples_with_eos_and_with_drafts(tiny, kv, s, reps):
    """A prompt of 24 tokens has no full range to share; the one of 40 at 16 samples has, and just enough rows (with 3
    drafts a verify call is then 64 rows, the most it may be)."""
    prompt = torch.cat([prompt_of(8, 11)] * reps)[None]
    P = prompt.shape[1]
    how = dict(temperature=0.8, top_k=20, seed=4, kv_dtype=kv)
    plain = tiny.generate(prompt, 20, num_samples=s, **how)
    eos = int(plain[1, P + 6])  # a token sample 1 draws: that row finishes there at the latest
    a = tiny.generate(prompt, 20, num_samples=s, eos_token_id=eos, **how)
    many = tiny.generate_many([prompt[0]] * s, 20, batch_size=s, eos_token_id=eos, **how)
    assert int((a[1, P:] == eos).nonzero()[0]) <= 6
    for r, m in enumerate(many):  # a row: the prompt, its tokens up to its first eos, then eos as padding
        assert torch.equal(a[r, :m.numel()], m) and bool((a[r, m.numel():] == eos).all()), r
    d = tiny.generate(prompt, 20, num_samples=s, draft_tokens=3, **how)
    assert torch.equal(d, plain)


def test_num_samples_one_is_the_call_without_it(tiny):
    idx = torch.stack([prompt_of(12, 12), prompt_of(12, 13)])
    assert torch.equal(tiny.generate(idx, 10, seed=5, num_samples=1), tiny.generate(idx, 10, seed=5))


def test_refusals(tiny):
    with pytest.raises(ValueError, match="64"):
        tiny.generate(torch.zeros(13, 4, dtype=torch.int64, device=dev), 4, seed=0, num_samples=5)  # 65 rows
    sess = tiny.decoder(4)
    with pytest.raises(ValueError, match="empty"):
        sess.fork(0, [1])
    sess.refill(0, prompt_of(6))
    for dst, words in (([0, 1], "among"), ([1, 4], r"\[0, B=4\)"), ([-1], r"\[0, B=4\)"), ([1, 2, 1], "duplicates")):
        with pytest.raises(ValueError, match=words):
            sess.fork(0, dst)
    with pytest.raises(ValueError, match=r"\[0, B=4\)"):
        sess.fork(4, [1])
    assert sess.share_group == [0, 1, 2, 3] and sess.lens == [6, 0, 0, 0]
    sess.fork(0, [1, 2])
    assert sess.share_group == [0, 0, 0, 3] and sess.share_len == [6, 6, 6, 0] and sess.lens == [6, 6, 6, 0]
    sess.reset()
    assert sess.share_group == [0, 1, 2, 3] and sess.share_len == [0] * 4


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("rows, n", [pytest.param(8, 16, id="1x8"), pytest.param(17, 28, id="1x17-shared-launch")])
def test_shared_equals_unshared_at_124m_widths(wide, kv, rows, n):
    """One group over a 40-token prompt: of 8 rows and 16 tokens, the case the feature was specified with (below the row
    threshold: the unshared launch), and of 17 rows and 28 tokens, where the plan entries take the shared launch with
    12 heads and the positions 40 .. 67 cross the range boundary at 64."""
    prompt = torch.randint(0, 50257, (40,), generator=torch.Generator().manual_seed(8)).to(dev)
    out = []
    for share in (True, False):
        sess = filled(wide, kv, rows, prompt, share, max_len=40 + n + 8)
        seq = seq_for(sess, [prompt] * rows, 40 + n)
        sess.generate(n, seq=seq, **SAMPLER)
        sess.flush()
        out.append((seq, state(sess)))
    assert torch.equal(out[0][0], out[1][0])
    assert_same_state(out[0][1], out[1][1])
    assert len({tuple(r) for r in out[0][0][:, 40:].tolist()}) > 1


def test_cli_prints_one_line_per_sample_prompt_major(tiny, tmp_path):
    import json
    import subprocess
    import sys

    from gpt_2_distributed_amd.train_gpt2_distributed import save_checkpoint
    from tests.conftest import REPO
    ckpt = save_checkpoint(tiny, tiny.configure_optimizers(), 3, str(tmp_path))
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.generate", "--checkpoint", ckpt, "--model", "auto",
           "--prompt_ids", "11,12,13", "--prompt_ids", "21,22,23,24,25", "--max_new_tokens", "7", "--num_samples", "3",
           "--sampler", "device", "--seed", "5", "--top_k", "20"]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [(r["prompt"], r["sample"]) for r in rows] == [(b, j) for b in range(2) for j in range(3)]
    prompts = [torch.tensor(p, device=dev) for p in ([11, 12, 13], [21, 22, 23, 24, 25])]
    want = tiny.generate(prompts, 7, top_k=20, seed=5, num_samples=3)
    for r, row in enumerate(rows):
        n = prompts[r // 3].numel() + 7
        assert row["tokens"] == want[r, :n].tolist()


@pytest.mark.parametrize("kv", KV)
def test_the_step_reads_a_shared_prompt_from_its_lowest_row_only(tiny, kv):
    """This is what shows that the "shared-launch" cases above do take the shared launch behind a plan. 17 rows of one
    70-token prompt: with the two full ranges of every row but the lowest poisoned (NaN values, or NaN scales with
    fp8) the loop still draws the tokens, and ends on the logits, of a session that does not share and is not
    poisoned, because those lines are not read; a session that does not share reads them."""
    prompt = prompt_of(70, 14)

    def poisoned(sess):
        for t in ((sess.kscale, sess.vscale) if kv == "fp8" else (sess.kcache, sess.vcache)):
            t[:, 1:, :, :64] = float("nan")
        return sess

    runs = []
    for share, make in ((False, lambda s: s), (True, lambda s: s), (True, poisoned)):
        sess = make(filled(tiny, kv, 17, prompt, share))
        seq = seq_for(sess, [prompt] * 17, 70 + 30)
        sess.generate(30, seq=seq, **SAMPLER)  # positions 70 .. 99
        sess.flush()
        assert bool(torch.isfinite(sess.logits).all())
        runs.append((seq, sess.logits.clone()))
    for seq, logits in runs[1:]:
        assert torch.equal(seq, runs[0][0]) and torch.equal(logits.view(torch.int32), runs[0][1].view(torch.int32))
    sess = poisoned(filled(tiny, kv, 17, prompt, False))
    logits = sess.step(runs[0][0][:, 70].contiguous())
    assert bool(torch.isfinite(logits[0]).all()) and not bool(torch.isfinite(logits[1:]).any())
