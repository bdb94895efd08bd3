"""KV-cache generation on the MI355X: DecodeSession (prefill + one-token steps) and GPT2.generate.

The yardstick of the decode path is code that predates it. For a token matrix S the existing full forward (eval mode,
bf16 autocast, one call) has an error E_full against the fp32 oracle (oracle/model_ref.py); the decode path, teacher-
forced on the same S, is held to E_dec <= 2 E_full over the same positions, overall and for the worst row. The decode
kernels round to bf16 where the training kernels do, so only summation orders and the split combines differ; a wrong
position, a stale or shifted cache row or an off-by-one key gives errors of order 1, a hundred times E_full.

Measured (MI355X), overall / worst row: see the table in DESIGN.md ("Decode")."""
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import model_ref
from tests.conftest import REPO
from tests.test_kernels_gpu import rel_err

pytestmark = pytest.mark.gpu

dev = "cuda"
TINY = dict(n_layer=2, n_head=2, n_embd=128, vocab_size=509, n_positions=192, resid_pdrop=0.1, attn_pdrop=0.1)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_model(cfg):
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    return GPT2(GPT2Config(**cfg)).to(dev)  # (left in train mode: generation must not care)


def full_forward(model, S):
    """The path that exists without generation: eval mode under bf16 autocast, one call on the whole sequence."""
    was = model.training
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        logits, _ = model(S)
    model.train(was)
    return logits.float()


def oracle_logits(model, cfg, S):
    params = {n: p.detach().cpu().float() for n, p in model.named_parameters() if n != "lm_head.weight"}
    with torch.no_grad():
        logits, _ = model_ref.forward(params, model_ref.Cfg(**cfg), S.cpu(), None, "fp32")
    return logits.to(dev)


def decode_logits(model, S, P):
    """prefill(S[:, :P]) then step(S[:, t]) for t = P..T-1: logits of positions P-1..T-1, [B, T-P+1, V]."""
    B, T = S.shape
    sess = model.decoder(B)
    rows = [sess.prefill(S[:, :P])]
    for t in range(P, T):
        rows.append(sess.step(S[:, t]))
    assert sess.pos == T
    return torch.stack(rows, dim=1)


def errs(x, ref):
    """(rel_err over everything, the largest rel_err of one [V] row)."""
    x, ref = x.double(), ref.double()
    rows = (x - ref).norm(dim=-1) / (ref.norm(dim=-1) + 1e-30)
    return rel_err(x, ref), float(rows.max())


def parity(model, cfg, S, prompts):
    full, ref = full_forward(model, S), oracle_logits(model, cfg, S)
    out = {}
    for P in prompts:
        dec = decode_logits(model, S, P)
        e_full, e_full_row = errs(full[:, P - 1:], ref[:, P - 1:])
        e_dec, e_dec_row = errs(dec, ref[:, P - 1:])
        print(f"C={cfg['n_embd']} V={cfg['vocab_size']} P={P}: E_full {e_full:.3e} (row max {e_full_row:.3e}), "
              f"E_dec {e_dec:.3e} (row max {e_dec_row:.3e})")
        out[P] = (e_full, e_full_row, e_dec, e_dec_row)
    return out


@pytest.fixture(scope="module")
def tiny():
    """The tiny model, a fixed token matrix, and the two references shared by the tests below."""
    model = make_model(TINY)
    S = torch.randint(0, TINY["vocab_size"], (3, 150), generator=torch.Generator().manual_seed(17)).to(dev)
    full, ref = full_forward(model, S), oracle_logits(model, TINY, S)
    return model, S, full, ref


@pytest.mark.parametrize("P", [1, 5, 64, 70])
def test_teacher_forced_parity(tiny, P):
    model, S, full, ref = tiny
    assert model.training  # dropout 0.1 configured and train mode on: the decode path runs at p = 0 regardless
    dec = decode_logits(model, S, P)
    e_full, e_full_row = errs(full[:, P - 1:], ref[:, P - 1:])
    e_dec, e_dec_row = errs(dec, ref[:, P - 1:])
    print(f"tiny P={P}: E_full {e_full:.3e} (row max {e_full_row:.3e}), E_dec {e_dec:.3e} (row max {e_dec_row:.3e})")
    assert e_dec <= 2 * e_full, (e_dec, e_full)
    assert e_dec_row <= 2 * e_full_row, (e_dec_row, e_full_row)


@pytest.mark.parametrize("cfg", [
    dict(n_layer=2, n_head=12, n_embd=768, vocab_size=50257, n_positions=64),  # GPT-2 124M's widths (Vp = 50432)
    dict(n_layer=1, n_head=25, n_embd=1600, vocab_size=509, n_positions=64),   # 1.5B's widths: no multiples of 256
], ids=["124M-widths", "1.5B-widths"])
def test_teacher_forced_parity_at_production_widths(cfg):
    cfg = dict(cfg, resid_pdrop=0.1, attn_pdrop=0.1)
    model = make_model(cfg)
    S = torch.randint(0, cfg["vocab_size"], (2, 20), generator=torch.Generator().manual_seed(23)).to(dev)
    e_full, e_full_row, e_dec, e_dec_row = parity(model, cfg, S, [3])[3]
    assert e_dec <= 2 * e_full, (e_dec, e_full)
    assert e_dec_row <= 2 * e_full_row, (e_dec_row, e_full_row)


def test_step_raises_when_the_cache_is_full_and_reset_rewinds(tiny):
    model, S, _, _ = tiny
    sess = model.decoder(3, max_len=8)
    first = sess.prefill(S[:, :7])
    sess.step(S[:, 7])
    with pytest.raises(ValueError, match="full"):
        sess.step(S[:, 8])
    sess.reset()
    assert sess.pos == 0
    assert torch.equal(sess.prefill(S[:, :7]), first)
    with pytest.raises(ValueError):
        model.decoder(3, max_len=TINY["n_positions"] + 1)
    with pytest.raises(ValueError):
        model.decoder(65)


def test_scalar_step_and_generate_entries_are_the_per_row_ones_at_equal_positions(tiny):
    """gpt2mi_decode_step / gpt2mi_decode_generate have no caller in the package (a session always passes lens): called
    here directly against their _ragged forms on a second session, across the 32-key range edge. Bitwise."""
    from gpt_2_distributed_amd import _lib as K
    model, S, _, _ = tiny
    B, V = 3, TINY["vocab_size"]
    a, b = model.decoder(B, max_len=70), model.decoder(B, max_len=70)
    assert torch.equal(a.prefill(S[:, :31]), b.prefill(S[:, :31]))

    def same_state(n):  # the logits and the n cached positions (the caches are torch.empty beyond them)
        return (torch.equal(a.logits, b.logits) and torch.equal(a.kcache[:, :, :, :n], b.kcache[:, :, :, :n])
                and torch.equal(a.vcache[:, :, :, :n], b.vcache[:, :, :, :n]))
    for pos in (31, 32, 33):
        tok = S[:, pos].contiguous()
        K.decode_step(a._plan, tok, pos)
        K.decode_step_ragged(b._plan, tok, [pos] * B)
        assert same_state(pos + 1), pos
    assert not torch.equal(a.kcache[:, :, :, 33], a.kcache[:, :, :, 30])  # (the steps did write their positions)
    tok_a, tok_b = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(2))
    seq_a, seq_b = (torch.zeros(B, 70, dtype=torch.int64, device=dev) for _ in range(2))
    K.decode_generate(a._plan, V, 0.8, 8, None, 5, 34, 4, tok_a, seq=seq_a)
    K.decode_generate_ragged(b._plan, V, 0.8, 8, None, 5, [34] * B, 4, tok_b, row_id=None, seq=seq_b)
    assert torch.equal(tok_a, tok_b) and torch.equal(seq_a, seq_b) and same_state(37)  # (token 37 is not stepped)
    assert bool((seq_a[:, 34:38] < V).all()) and torch.equal(seq_a[:, 37], tok_a) and not bool(seq_a[:, 38:].any())


# ---- generate --------------------------------------------------------------------------------------------------
def test_greedy_generate_emits_an_argmax_of_the_full_forward(tiny):
    """Every emitted token's logit in the existing full forward of the sequence so far is within 2 E_full |row|_inf of
    that row's maximum: an argmax up to the measured logit error (no near-tie exclusion needed)."""
    model, S, full, ref = tiny
    e_full = errs(full, ref)[0]
    prompt = S[:, :5].contiguous()
    out = model.generate(prompt, 40, temperature=0.0)
    assert out.shape == (3, 45) and out.dtype == torch.int64
    assert torch.equal(out[:, :5], prompt)
    assert model.training
    logits = full_forward(model, out)  # causal: row t-1 is the full forward of the sequence so far
    for t in range(5, 45):
        row = logits[:, t - 1]
        gap = row.max(-1).values - row.gather(1, out[:, t:t + 1]).squeeze(1)
        bound = 2 * e_full * row.abs().max(-1).values
        assert bool((gap <= bound).all()), (t, gap.tolist(), bound.tolist())


def test_sampling_is_seeded_and_top1_is_greedy(tiny):
    model, S, _, _ = tiny
    prompt = S[:, :5].contiguous()
    gen = lambda s: torch.Generator(device=dev).manual_seed(s)  # noqa: E731
    a = model.generate(prompt, 24, temperature=1.0, top_k=50, generator=gen(7))
    b = model.generate(prompt, 24, temperature=1.0, top_k=50, generator=gen(7))
    assert torch.equal(a, b)
    assert a.shape == (3, 29) and int(a.min()) >= 0 and int(a.max()) < TINY["vocab_size"]
    greedy = model.generate(prompt, 24, temperature=0.0)
    assert torch.equal(model.generate(prompt, 24, temperature=0.8, top_k=1, generator=gen(1)), greedy)


def test_eos_stops_early_and_pads(tiny):
    model, S, _, _ = tiny
    prompt = S[:, :5].contiguous()
    greedy = model.generate(prompt, 12, temperature=0.0)
    eos = int(greedy[0, 5])
    out = model.generate(prompt, 12, temperature=0.0, eos_token_id=eos)
    assert out.shape[1] <= 17 and torch.equal(out[:, :5], prompt)
    for b in range(3):
        new, want = out[b, 5:].tolist(), greedy[b, 5:].tolist()
        stop = new.index(eos) if eos in new else len(new)
        assert new[:stop] == want[:stop]                 # greedy until the first eos ...
        assert all(t == eos for t in new[stop:])         # ... which the row then keeps emitting
    assert out[0, 5:].tolist() == [eos] * (out.shape[1] - 5)
    # one sequence whose first token is eos: generation ends after that token
    one = model.generate(prompt[:1], 12, temperature=0.0, eos_token_id=eos)
    assert one.shape == (1, 6) and int(one[0, 5]) == eos


def test_generate_refuses_what_it_cannot_do(tiny):
    model, S, _, _ = tiny
    with pytest.raises(ValueError, match="n_positions"):
        model.generate(S[:, :150], 43)  # 150 + 43 > 192
    assert model.generate(S[:, :150], 42, temperature=0.0).shape == (3, 192)  # the last slot is usable
    model.precision = "fp32"
    try:
        with pytest.raises(NotImplementedError):
            model.generate(S[:, :5], 4)
        with pytest.raises(NotImplementedError):
            model.decoder(3)
    finally:
        model.precision = "auto"
    with pytest.raises(RuntimeError):
        model.generate(S[:, :5].cpu(), 4)


# ---- training is not perturbed -----------------------------------------------------------------------------------
def _train_step(model, opt, batch):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, loss = model(batch[:, :-1], labels=batch[:, 1:])
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss.detach().clone()


def test_generate_between_steps_leaves_training_bit_identical():
    batches = torch.randint(0, 509, (2, 2, 65), generator=torch.Generator().manual_seed(3)).to(dev)
    prompt = batches[0, :, :5].contiguous()
    runs = []
    for with_generate in (False, True):
        model = make_model(TINY)
        opt = model.configure_optimizers(learning_rate=1e-2)
        _train_step(model, opt, batches[0])
        if with_generate:
            seed, token = model.engine()._step_seed, model.engine()._fwd_token
            model.generate(prompt, 20, temperature=1.0, top_k=10, generator=torch.Generator(device=dev).manual_seed(1))
            assert (model.engine()._step_seed, model.engine()._fwd_token) == (seed, token)
            assert model.training
        loss = _train_step(model, opt, batches[1])
        runs.append((loss, model.transformer.h[0].attn.qkv.weight.detach().clone(), model.engine()._step_seed))
    (l0, w0, s0), (l1, w1, s1) = runs
    assert torch.equal(l0, l1) and torch.equal(w0, w1) and s0 == s1


def test_generate_uses_the_weights_of_the_latest_optimizer_step():
    batch = torch.randint(0, 509, (2, 65), generator=torch.Generator().manual_seed(4)).to(dev)
    prompt = batch[:, :9].contiguous()
    model = make_model(TINY)
    opt = model.configure_optimizers(learning_rate=1e-2)
    before = model.decoder(2).prefill(prompt)
    _train_step(model, opt, batch)
    after = model.decoder(2).prefill(prompt)
    assert not torch.equal(before, after)
    fresh = make_model(TINY)
    fresh.load_state_dict(model.state_dict())
    assert torch.equal(fresh.decoder(2).prefill(prompt), after)
    assert torch.equal(fresh.generate(prompt, 16, temperature=0.0), model.generate(prompt, 16, temperature=0.0))


# ---- wrappers and the CLI: fresh child processes ------------------------------------------------------------------
WRAPPERS = r"""
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, os.environ["REPO"])
from gpt_2_distributed_amd.parallel import init_distributed, DistributedDataParallel, FullyShardedDataParallel
from gpt_2_distributed_amd.model import GPT2, GPT2Config
init_distributed()  # a world of one rank
cfg = GPT2Config(**json.loads(os.environ["CFG"]))
prompt = torch.randint(0, cfg.vocab_size, (2, 5), generator=torch.Generator().manual_seed(0)).cuda()
plain = GPT2(cfg).to("cuda:0")
want = plain.generate(prompt, 8, temperature=0.0)
ddp = DistributedDataParallel(GPT2(cfg).to("cuda:0"))
res = {"ddp_equal": bool(torch.equal(ddp.module.generate(prompt, 8, temperature=0.0), want))}
fsdp = FullyShardedDataParallel(GPT2(cfg).to("cuda:0"))
try:
    fsdp.module.generate(prompt, 8)
    res["fsdp"] = "ran"
except NotImplementedError as e:
    res["fsdp"] = "NotImplementedError: " + str(e)
print("RESULT", json.dumps(res), flush=True)
dist.destroy_process_group()
"""


def test_wrappers(tmp_path):
    """DistributedDataParallel(model).module.generate equals the plain model's; a FullyShardedDataParallel-wrapped model
    (sharded parameters) raises NotImplementedError. One rank with a gloo process group (the wrappers need one)."""
    script = tmp_path / "wrappers.py"
    script.write_text(WRAPPERS)
    env = dict(os.environ, REPO=REPO, CFG=json.dumps(TINY), GPT2MI_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29571", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][0][7:])
    assert res["ddp_equal"] is True
    assert res["fsdp"].startswith("NotImplementedError") and "FullyShardedDataParallel" in res["fsdp"]


def test_cli_samples_from_a_checkpoint(tmp_path):
    from gpt_2_distributed_amd.train_gpt2_distributed import save_checkpoint
    model = make_model(TINY)
    ckpt = save_checkpoint(model, model.configure_optimizers(), 3, str(tmp_path))
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.generate", "--checkpoint", ckpt, "--model", "auto",
           "--prompt_ids", "11,12,13", "--max_new_tokens", "9", "--batch", "2", "--temperature", "0", "--seed", "5"]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("[")]
    assert len(rows) == 2
    # greedy on the same weights in this process: the CLI's output is the model's
    want = model.generate(torch.tensor([[11, 12, 13]], device=dev), 9, temperature=0.0)[0].tolist()
    for row in rows:
        assert len(row) == 12 and row[:3] == [11, 12, 13]
        assert all(isinstance(t, int) and 0 <= t < TINY["vocab_size"] for t in row)
        assert row == want
