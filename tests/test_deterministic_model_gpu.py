"""``model.deterministic`` through the public interface: two runs of the same training steps give the same bits (loss,
parameters, gradients), in bf16 and fp32, with dropout, with doc_bounds and restarting positions, for a sub-module
backward and for the trainer; the mode differs from the default one by summation order only; the default launches none
of the ordered kernels."""
import contextlib
import io
import json

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
CFG = dict(n_layer=2, n_head=2, n_embd=128, vocab_size=509, n_positions=64, resid_pdrop=0.1, attn_pdrop=0.1)
DET_BINDINGS = ("colsum_det", "layernorm_bwd_det", "embed_bwd_det", "embed_bwd_doc_det")
PRECISIONS = pytest.mark.parametrize("prec", ["bf16", "fp32"])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(prec, det, **over):
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    m = GPT2(GPT2Config(**dict(CFG, **over))).to(dev).train()
    m.precision, m.deterministic = prec, det
    return m


def _batches(n, B=4, T=64):
    g = torch.Generator().manual_seed(11)
    t = torch.randint(0, 509, (n, B, T + 1), generator=g)
    t[:, :, ::17] = 5  # the separator of the packed case; tokens repeat (509 values over 256 positions)
    return [(b[:, :-1].contiguous().to(dev), b[:, 1:].contiguous().to(dev)) for b in t]


def _train(prec, det, doc, steps):
    """steps FusedAdamW steps of a fresh model: (losses, parameters after the last step, gradients of the last step)."""
    from gpt_2_distributed_amd.packing import doc_bounds
    m = _model(prec, det)
    opt = m.configure_optimizers(learning_rate=1e-3)
    losses = []
    for x, y in _batches(steps):
        opt.zero_grad()
        kw = dict(doc_bounds=doc_bounds(x, 5), reset_positions=True) if doc else {}
        loss = m(x, labels=y, **kw)[1]
        loss.backward()
        grads = {k: p.grad.clone() for k, p in m.named_parameters()}
        opt.step()
        losses.append(loss.detach().clone())
    return losses, {k: p.detach().clone() for k, p in m.named_parameters()}, grads


@pytest.mark.parametrize("doc", [False, True], ids=["plain", "doc_reset"])
@PRECISIONS
def test_two_runs_are_bit_equal(prec, doc):
    a, b = _train(prec, True, doc, 3), _train(prec, True, doc, 3)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])), (a[0], b[0])
    for part in (1, 2):
        diff = [k for k in a[part] if not torch.equal(a[part][k], b[part][k])]
        assert not diff, (("losses", "parameters", "gradients")[part], diff)


@PRECISIONS
def test_block_backward_is_bit_equal(prec):
    def run():
        m = _model(prec, True)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(4, 64, 128, generator=g).to(dev).requires_grad_(True)
        m.transformer.h[1](x).backward(torch.randn(4, 64, 128, generator=g).to(dev))
        return [x.grad] + [p.grad for p in m.transformer.h[1].parameters()]
    assert all(torch.equal(s, t) for s, t in zip(run(), run()))


@PRECISIONS
def test_deterministic_against_default(prec):
    """One step: the forward is the same launches (equal loss bits); every gradient within the absolute 1e-6 that
    tests/test_trainer_gpu.py allows between two in-process runs (the modes differ by summation order only)."""
    det, default = _train(prec, True, False, 1), _train(prec, False, False, 1)
    assert torch.equal(det[0][0], default[0][0])
    worst = {k: float((det[2][k] - default[2][k]).abs().max()) for k in det[2]}
    print("largest gradient difference", max(worst.items(), key=lambda kv: kv[1]))
    assert max(worst.values()) <= 1e-6, {k: v for k, v in worst.items() if v > 1e-6}


def test_width_96_bf16_is_refused():
    m = _model("bf16", True, n_embd=96, n_head=2)
    x, y = _batches(1)[0]
    with pytest.raises(NotImplementedError, match="multiples of 64"):
        m(x, labels=y)[1].backward()


@pytest.mark.parametrize("det", [False, True])
def test_default_model_calls_no_ordered_kernel(monkeypatch, det):
    from gpt_2_distributed_amd import _lib
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    assert GPT2(GPT2Config(**CFG)).deterministic is False
    calls = dict.fromkeys(DET_BINDINGS, 0)

    def counted(name, fn):
        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapper
    for name in DET_BINDINGS:
        monkeypatch.setattr(_lib, name, counted(name, getattr(_lib, name)))
    _train("bf16", det, False, 1)
    if det:  # ln_f + 2 per block; qkv, fc1 per block
        assert (calls["layernorm_bwd_det"], calls["colsum_det"], calls["embed_bwd_det"]) == (5, 4, 1), calls
    else:
        assert not any(calls.values()), calls


def test_trainer_logs_identical_values(tmp_path):
    from gpt_2_distributed_amd import train_gpt2_distributed as trainer

    def run(tag):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            trainer.main(["--data_dir", str(tmp_path / "data"), "--synthetic", "2", "--synthetic_tokens", "60000",
                          "--seq_len", "128", "--batch", "4", "--grad_accum_steps", "1", "--max_steps", "4",
                          "--workers", "0", "--log_every", "1", "--training_mode", "local", "--deterministic",
                          "--save_every", "100", "--save_dir", str(tmp_path / tag)])
        steps = [json.loads(l) for l in out.getvalue().splitlines() if l.startswith("{")]
        return [(s["step"], s["loss"], s["grad_norm"]) for s in steps]
    first, second = run("a"), run("b")
    assert [s[0] for s in first] == [1, 2, 3, 4] and first == second, (first, second)
