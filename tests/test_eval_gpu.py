"""GPT2.score / GPT2.evaluate on the MI355X: the forward-only evaluation path (Engine.score on an EvalWorkspace, the
fused lm_head + cross-entropy kernel under bf16) against the logits path, the oracle, and its promises: no side effect
on a training run, dropout off, a workspace without a term in n_layer or an [M, Vp] logits tensor."""
import contextlib
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests.conftest import REPO

pytestmark = pytest.mark.gpu
dev = "cuda"

TINY = dict(n_layer=2, n_head=2, n_embd=128, vocab_size=509, n_positions=64, resid_pdrop=0.0, attn_pdrop=0.0)
DROP = dict(TINY, resid_pdrop=0.1, attn_pdrop=0.1)
bf16 = lambda: torch.autocast("cuda", dtype=torch.bfloat16)  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_model(cfg):
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    return GPT2(GPT2Config(**cfg)).to(dev)


def batch(B, T, seed, V=509, ignore=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V, (B, T + 1), generator=g)
    x, y = t[:, :-1].contiguous(), t[:, 1:].contiguous()
    if ignore:
        y.view(-1)[torch.randperm(B * T, generator=g)[:ignore]] = -100
    return x.to(dev), y.to(dev)


@pytest.mark.parametrize("B,T", [(2, 64), (3, 50)])
def test_score_agrees_with_the_logits_path(B, T):
    """Per token, |score - F.cross_entropy(bf16 logits of the existing eval-mode forward)| <= 2^-8 max|logit| of the
    batch: a bf16 half-ulp (2^-9 relative) on the label's logit plus at most the same on the log-sum-exp. T = 50 is
    padded to the attention tile inside the engine; seven labels are -100."""
    m = make_model(TINY)
    x, y = batch(B, T, seed=21, ignore=7)
    m.eval()
    with bf16(), torch.no_grad():
        logits = m(x)[0].float()
    m.train()
    want = F.cross_entropy(logits.reshape(-1, 509), y.reshape(-1), reduction="none", ignore_index=-100).view(B, T)
    with bf16():
        got = m.score(x, y, reduction="none")
        mean, tot = m.score(x, y), m.score(x, y, reduction="sum")
    assert got.shape == (B, T) and got.dtype == torch.float32 and not got.requires_grad
    bound = 2.0 ** -8 * logits.abs().max().item()
    diff = (got - want).abs().max().item()
    print(f"B={B} T={T}: max per-token diff {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound
    assert (got[y == -100] == 0).all() and (got[y != -100] > 0).all()
    n = (y != -100).sum().item()
    assert n == B * T - 7
    s64 = got.double().sum().item()
    assert abs(tot.item() - s64) <= 1e-6 * s64 and abs(mean.item() - s64 / n) <= 1e-6 * s64 / n
    assert mean.shape == () and tot.shape == ()


@pytest.mark.parametrize("prec,gate", [("bf16", 2e-2), ("fp32", 1e-4)])
def test_score_mean_against_the_oracle(prec, gate):
    """The project's gates (README): bf16 within 2e-2, fp32 (no autocast) within 1e-4 of the oracle's fp32 loss for the
    same weights (the seed-42 init) and batch."""
    from oracle import model_ref
    x, y = batch(2, 64, seed=22, ignore=5)
    cfg = model_ref.Cfg(**TINY)
    with torch.no_grad():
        _, ref = model_ref.forward(model_ref.init_params(cfg), cfg, x.cpu(), y.cpu(), "fp32")
    m = make_model(TINY)
    with (bf16() if prec == "bf16" else contextlib.nullcontext()):
        got = m.score(x, y).item()
        rows = m.score(x, y, reduction="none")
    rel = abs(got - ref.item()) / ref.item()
    print(f"{prec}: score {got:.6f} oracle {ref.item():.6f} rel {rel:.2e}")
    assert rel < gate
    assert abs(rows.double().sum().item() / (y != -100).sum().item() - got) <= 1e-6 * got


def test_fp32_score_chunks_rows(monkeypatch):
    """The fp32 head walks the rows in chunks into one reused logits buffer: the same values whatever the chunk, to
    fp32 GEMM resolution (the planner may pick another fp32 kernel for a 64-row GEMM than for a 192-row one)."""
    from gpt_2_distributed_amd import engine as E
    x, y = batch(3, 64, seed=23, ignore=3)
    m = make_model(TINY)
    whole, mean = m.score(x, y, reduction="none"), m.score(x, y)
    unchunked = m.engine().eval_workspace_bytes(3, 64, torch.float32)
    monkeypatch.setattr(E, "EVAL_F32_CHUNK", 64)
    m2 = make_model(TINY)
    assert m2.engine().eval_workspace_bytes(3, 64, torch.float32) < unchunked
    torch.testing.assert_close(m2.score(x, y, reduction="none"), whole, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(m2.score(x, y), mean, rtol=1e-5, atol=1e-5)


def _batches(n, B=2, T=64, V=509):
    out = []
    for s in range(n):
        t = torch.randint(0, V, (B, T + 1), generator=torch.Generator().manual_seed(100 + s))
        out.append((t[:, :-1].contiguous().to(dev), t[:, 1:].contiguous().to(dev)))
    return out


def _step(model, opt, b):
    with bf16():
        _, loss = model(b[0], labels=b[1])
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss.detach().clone()


def _evaluate_between(m):
    ex, ey = batch(3, 50, seed=31, ignore=4)  # another (B, T) than the training batches
    eng = m.engine()
    seed = eng._step_seed
    with bf16():
        m.score(ex, ey)
        assert eng._step_seed == seed
        r = m.evaluate([(ex, ey), (ex, ey)])
    assert r["tokens"] == 2 * (3 * 50 - 4) and math.isfinite(r["loss"])


def test_evaluation_leaves_every_piece_of_training_state_untouched():
    """train(), dropout 0.1, after two steps: score and evaluate on a batch of another (B, T) change nothing a later
    step reads. Compared bit for bit across the evaluation, in one process: the fp32 master weights, the bf16 shadow
    and its transpose, the grad arena, every optimizer state tensor, the dropout stream (_step_seed), _fwd_token,
    _saved, gemm_sched, the engine's gradient flags, model.training, and the cached training Workspace (the same
    object, its buffers untouched). A training step is a function of exactly this state and its batch, so the steps
    after the evaluation are the computation they would have been without it. (The parent's no-grad forward fails this:
    it advances _step_seed, replaces _saved and, at another (B, T), evicts the Workspace.)"""
    bs = _batches(2)
    m = make_model(DROP)
    opt = m.configure_optimizers(learning_rate=1e-2)
    for b in bs:
        _step(m, opt, b)
    eng = m.engine()

    def tensors():
        t = {"arena": m.arena, "shadow": eng.shadow, "shadowT": eng.shadowT, "grad": eng.grad}
        for k, v in opt.state_dict().items():
            if torch.is_tensor(v):
                t["opt." + k] = v
        ws = eng._ws[(2, 64, torch.bfloat16)]
        t.update({"ws.x": ws.x, "ws.lnf": ws.lnf, "ws.dlogits": ws.dlogits, "ws.h0": ws.blocks[0].h})
        return t

    def scalars():
        return (eng._step_seed, eng._fwd_token, eng.gemm_sched, eng.grad_dirty, eng._grad_fresh, eng._grad_dead,
                eng._shadow_versions, eng._shadowT_stale, m.training, [id(w) for w in eng._ws.values()], id(eng._saved),
                {k: v for k, v in opt.state_dict().items() if not torch.is_tensor(v) and k != "param_groups"})

    assert len([k for k in tensors() if k.startswith("opt.")]) >= 2  # the AdamW moments are among them
    before_t = {k: v.detach().clone() for k, v in tensors().items()}
    before_s = scalars()
    _evaluate_between(m)
    assert scalars() == before_s
    for k, v in tensors().items():  # as bytes: never-written gaps of the buffers may hold NaN bit patterns
        assert torch.equal(v.detach().contiguous().view(torch.uint8), before_t[k].contiguous().view(torch.uint8)), k
    assert m.training and eng._ws[(2, 64, torch.bfloat16)] is not None


def test_evaluation_between_steps_leaves_the_losses_and_final_weights():
    """Steps 1-2, evaluation, steps 3-4 (train(), dropout 0.1) against the same four steps without the evaluation, as
    two runs: the four losses agree to 1e-6 relative, every final parameter to 1e-6 absolute, and the dropout stream
    ends at the same position.

    Not "bit-identical losses and final weights" between the two runs, because two runs of the parent's own training
    steps are not: the LayerNorm backward adds its weight / bias / branch-bias column sums with one float atomic per
    workgroup (norm_embed.hip) and the embedding backward adds token rows atomically, so those gradients vary in the last
    bits from run to run. Measured on an MI355X with this model: after ONE step of two fresh models on one batch 8-10 of
    the 28 parameters' gradients differ (ln1 / ln2 weights and biases, fc2 bias, wte); over these four steps, three runs
    WITHOUT evaluation agreed on 4/4 losses but only on 18/28 final parameters, and which parameters agree changes from
    pair to pair. So the unconditional, exact statement is made on the state instead
    (test_evaluation_leaves_every_piece_of_training_state_untouched), and this test holds the outcome to the bound
    tests/test_trainer_gpu.py::test_checkpoint_resume_matches_uninterrupted_run sets for the same steps run twice in one
    process, with that test's learning rate (1e-3): 1e-6 relative on the losses, 1e-6 absolute on every final parameter.
    The parent's no-grad forward misses both by orders of magnitude: it advances the dropout stream, so steps 3-4 draw
    other masks."""
    bs = _batches(4)
    runs = []
    for with_eval in (False, True):
        m = make_model(DROP)
        opt = m.configure_optimizers(learning_rate=1e-3)
        losses = [_step(m, opt, b) for b in bs[:2]]
        if with_eval:
            _evaluate_between(m)
        losses += [_step(m, opt, b) for b in bs[2:]]
        runs.append((torch.stack(losses).double(), m.engine()._step_seed,
                     {n: p.detach().clone() for n, p in m.named_parameters()}))
    (la, sa, wa), (le, se, we) = runs
    worst = max((we[n] - wa[n]).abs().max().item() for n in wa)
    print(f"losses without / with evaluation: {la.tolist()} / {le.tolist()}; largest final-parameter difference {worst:.3e}")
    assert sa == se
    assert ((la - le).abs() <= 1e-6 * la.abs()).all()
    for n in wa:
        assert (we[n] - wa[n]).abs().max().item() <= 1e-6, n


def test_dropout_is_off_in_score():
    m = make_model(DROP)
    x, y = batch(2, 64, seed=41)
    assert m.training
    with bf16():
        a, b = m.score(x, y, reduction="none"), m.score(x, y, reduction="none")
        m.eval()
        c = m.score(x, y, reduction="none")
        m.train()
        # (the logits path in train mode does drop: the two differ there)
        _, dropped = m(x, labels=y)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert abs(dropped.item() - a[y != -100].mean().item()) > 1e-4


def test_argument_checks_are_forwards():
    m = make_model(TINY)
    x, y = batch(2, 64, seed=42)
    with pytest.raises(ValueError, match="Sequence length 65 > model max 64"):
        m.score(torch.zeros(1, 65, dtype=torch.int64, device=dev), torch.zeros(1, 65, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.score(x.cpu(), y.cpu())
    with pytest.raises(ValueError, match="labels shape"):
        m.score(x, y[:, :32])
    with pytest.raises(ValueError, match="reduction"):
        m.score(x, y, reduction="avg")
    with bf16(), torch.enable_grad():
        out = m.score(x, y)
    assert not out.requires_grad and out.grad_fn is None  # documented: no graph, whatever the grad mode


def test_workspace_has_no_term_in_depth_and_no_logits_tensor():
    a, b = make_model(dict(TINY, n_layer=2)), make_model(dict(TINY, n_layer=6))
    for act in (torch.bfloat16, torch.float32):
        assert a.engine().eval_workspace_bytes(4, 64, act) == b.engine().eval_workspace_bytes(4, 64, act) > 0
    del a, b
    # the real vocabulary at a small width: M = 1024 rows; the parent path would allocate M * Vp * 2 bytes of logits
    cfg = dict(n_layer=1, n_head=2, n_embd=128, vocab_size=50257, n_positions=256, resid_pdrop=0.0, attn_pdrop=0.0)
    m = make_model(cfg)
    x, y = batch(4, 256, seed=43, V=50257)
    m.engine()  # (the shadows and the grad arena are the engine's, not the evaluation's)
    with bf16():
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        first = m.score(x, y).item()  # warm-up: allocates the evaluation workspace
        torch.cuda.synchronize()
        # eval_workspace_bytes is what the workspace holds: the allocation it caused, to the allocator's 512-byte
        # rounding of each of its ~25 tensors
        grown = torch.cuda.memory_allocated() - held
        want = m.engine().eval_workspace_bytes(4, 256)
        ws = m.engine()._eval_ws[(4, 256, torch.bfloat16)]
        assert want == sum(t.numel() * t.element_size() for t in ws.tensors())
        assert want <= grown <= want + 512 * len(ws.tensors()), (grown, want)
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        second = m.score(x, y).item()
        rise = torch.cuda.max_memory_allocated() - before
    logits_bytes = 1024 * m.vpad * 2
    print(f"peak rise of a warm score: {rise} B; the logits tensor would be {logits_bytes} B; "
          f"eval workspace {m.engine().eval_workspace_bytes(4, 256)} B")
    assert rise < logits_bytes / 4
    assert m.engine().eval_workspace_bytes(4, 256) < logits_bytes
    assert first == second and abs(first - math.log(50257)) < 0.5  # an untrained model: about ln V
    assert not m.engine()._ws  # the training workspace was never built


def test_evaluate_is_the_token_weighted_mean():
    m = make_model(TINY)
    bs = [batch(2, 64, seed=51, ignore=9), batch(2, 64, seed=52), batch(2, 64, seed=53, ignore=40)]
    with bf16():
        sums = [m.score(x, y, reduction="sum").double().item() for x, y in bs]
        r = m.evaluate(iter(bs))
        capped = m.evaluate(iter(bs), max_batches=2)
    counts = [(y != -100).sum().item() for _, y in bs]
    want = sum(sums) / sum(counts)
    assert r["tokens"] == sum(counts) and capped["tokens"] == sum(counts[:2])
    assert abs(r["loss"] - want) <= 3 * torch.finfo(torch.float32).eps * want  # fp32 running sum of three terms
    assert r["ppl"] == math.exp(r["loss"])
    assert abs(capped["loss"] - sum(sums[:2]) / sum(counts[:2])) <= 3 * torch.finfo(torch.float32).eps * want
    means = [s / c for s, c in zip(sums, counts)]
    assert abs(r["loss"] - sum(means) / 3) > 1e-6  # not a mean of batch means (the counts differ)


WRAPPERS = r"""
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, os.environ["REPO"])
from gpt_2_distributed_amd.parallel import init_distributed, DistributedDataParallel, FullyShardedDataParallel
from gpt_2_distributed_amd.model import GPT2, GPT2Config
init_distributed()  # a world of one rank, collectives forced on
cfg = GPT2Config(**json.loads(os.environ["CFG"]))
g = torch.Generator().manual_seed(61)
bs = []
for _ in range(3):
    t = torch.randint(0, cfg.vocab_size, (2, 51), generator=g)
    bs.append((t[:, :-1].contiguous().cuda(), t[:, 1:].contiguous().cuda()))
res = {}
def run(name, model):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        r = model.evaluate(iter(bs))
        r["score"] = model.score(*bs[0], reduction="sum").item()
        if name != "plain":  # a training step still works after the evaluation, and evaluating again sees its update
            opt = model.configure_optimizers(learning_rate=1e-2)
            _, loss = model(bs[1][0], labels=bs[1][1])
            loss.backward(); opt.step(); opt.zero_grad()
            r["after_step"] = model.evaluate(iter(bs))["loss"]
    res[name] = r
run("plain", GPT2(cfg).to("cuda:0"))
rounded = GPT2(cfg).to("cuda:0")  # the bare model with every parameter at its bf16 value, as FSDP's bf16 gather leaves them
with torch.no_grad():
    for p in rounded.parameters():
        p.copy_(p.bfloat16().float())
rounded.engine().refresh_shadow()
with torch.autocast("cuda", dtype=torch.bfloat16):
    res["rounded"] = rounded.evaluate(iter(bs))
    res["rounded"]["score"] = rounded.score(*bs[0], reduction="sum").item()
run("ddp", DistributedDataParallel(GPT2(cfg).to("cuda:0")))
run("fsdp_resident", FullyShardedDataParallel(GPT2(cfg).to("cuda:0"), reshard_after_forward=False))
run("fsdp_reshard", FullyShardedDataParallel(GPT2(cfg).to("cuda:0"), reshard_after_forward=True))
print("RESULT", json.dumps(res), flush=True)
dist.barrier(); dist.destroy_process_group()
"""


def test_wrappers_evaluate_as_the_bare_model(tmp_path):
    """DistributedDataParallel and FullyShardedDataParallel (resident and resharding) route score / evaluate to the
    module and engine: one rank over RCCL with the collectives forced on (the all-gathers and evaluate's all-reduce
    really run). DDP equals the bare model exactly. Under autocast FSDP gathers every parameter of a unit in bf16
    (torch FSDP's param_dtype), so the parameters the kernels read in fp32 (the embedding tables in the embedding
    kernel, LayerNorm weights, biases) are bf16-rounded there and fp32 masters in the bare model, in training forwards
    as well; the GEMMs' bf16 shadow is the same bits in both. So both FSDP modes must equal, exactly, the bare model
    whose parameters were rounded to bf16 (a stale or wrong unit cannot), and against the unrounded bare model they are
    held to 1e-4 relative, four times the 2.5e-5 that rounding measures here."""
    script = tmp_path / "wrappers.py"
    script.write_text(WRAPPERS)
    env = dict(os.environ, REPO=REPO, CFG=json.dumps(TINY), GPT2MI_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29581", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][0][7:])
    plain = res["plain"]
    assert plain["tokens"] == 300 and plain["ppl"] == math.exp(plain["loss"])
    key = lambda r: (r["loss"], r["ppl"], r["tokens"], r["score"])  # noqa: E731
    assert key(res["ddp"]) == key(plain), (res["ddp"], plain)
    assert key(res["fsdp_resident"]) == key(res["fsdp_reshard"]) == key(res["rounded"]), res
    for name in ("fsdp_resident", "fsdp_reshard"):
        r = res[name]
        print(f"{name}: loss {r['loss']!r} vs bare {plain['loss']!r}")
        assert r["tokens"] == plain["tokens"] and r["ppl"] == math.exp(r["loss"])
        assert abs(r["loss"] - plain["loss"]) <= 1e-4 * plain["loss"]
        assert abs(r["score"] - plain["score"]) <= 1e-4 * plain["score"]
    for name in ("ddp", "fsdp_resident", "fsdp_reshard"):
        r = res[name]
        assert math.isfinite(r["after_step"]) and r["after_step"] != r["loss"], (name, r)
