"""Generation over the fp8 key/value cache (kv_dtype="fp8") on the MI355X.

Parity. The yardsticks are references, none the code under test: E_full is the error of the existing bf16 full forward
against the fp32 oracle (the yardstick of tests/test_generation_gpu.py) and E_q the error, against the same oracle, of
the fp32 oracle with generation.kv_quantize / kv_dequantize applied to k and v inside causal_attention: what the format
costs when nothing else is rounded. The fp8 decode path, teacher-forced, is held to E_fp8 <= E_q + 2 E_full, overall
and for the worst row; 2 E_full is the margin the bf16 decode path is granted. A stale scale, a shifted row or a wrong
exponent gives errors of order 1. It is not held to the quantised oracle directly: bf16 rounding of k flips some of the
e4m3 rounding decisions, so that distance is a few E_full by itself; it is printed.

Exactness. Everything the bf16 cache guarantees bit for bit holds over the fp8 cache: extend equals steps, a row does
not depend on its batch, a refilled row is a fresh one-row prefill, speculative generation returns the plain loop's
tokens.

Measured (MI355X): see the table in DESIGN.md ("FP8 key/value cache")."""
import json
import subprocess
import sys

import pytest
import torch

from gpt_2_distributed_amd.generation import kv_dequantize, kv_quantize
from oracle import model_ref
from tests.conftest import REPO
from tests.test_generation_gpu import TINY, errs, full_forward, make_model, oracle_logits

pytestmark = pytest.mark.gpu

dev = "cuda"
B, V = 3, TINY["vocab_size"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def quantised_oracle_logits(model, cfg, S):
    """oracle_logits with every attention's k and v passed through the cache format."""
    plain = model_ref.causal_attention

    def quantised(q, k, v, mode="fp32", drop=None):
        return plain(q, kv_dequantize(*kv_quantize(k)), kv_dequantize(*kv_quantize(v)), mode, drop)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(model_ref, "causal_attention", quantised)
        return oracle_logits(model, cfg, S)


def decode_logits_fp8(model, S, P):
    """prefill(S[:, :P]) then step(S[:, t]) for t = P..T-1 over an fp8 cache: logits of positions P-1..T-1."""
    sess = model.decoder(S.size(0), kv_dtype="fp8")
    rows = [sess.prefill(S[:, :P])]
    for t in range(P, S.size(1)):
        rows.append(sess.step(S[:, t]))
    assert sess.pos == S.size(1)
    return torch.stack(rows, dim=1)


def check_parity(name, dec, full, ref, ref_q, P):
    (e_full, r_full), (e_q, r_q) = errs(full[:, P - 1:], ref[:, P - 1:]), errs(ref_q[:, P - 1:], ref[:, P - 1:])
    (e_fp8, r_fp8), (d_q, dr_q) = errs(dec, ref[:, P - 1:]), errs(dec, ref_q[:, P - 1:])
    print(f"{name} P={P}: E_full {e_full:.3e} (row max {r_full:.3e}), E_q {e_q:.3e} ({r_q:.3e}), E_fp8 {e_fp8:.3e} "
          f"({r_fp8:.3e}), share of bound {e_fp8 / (e_q + 2 * e_full):.2f} ({r_fp8 / (r_q + 2 * r_full):.2f}); to the "
          f"quantised oracle {d_q:.3e} ({dr_q:.3e}) = {d_q / e_full:.1f} ({dr_q / r_full:.1f}) E_full")
    assert e_fp8 <= e_q + 2 * e_full, (e_fp8, e_q, e_full)
    assert r_fp8 <= r_q + 2 * r_full, (r_fp8, r_q, r_full)


@pytest.fixture(scope="module")
def tiny():
    """The tiny model, a fixed token matrix and the three references shared by the tests below."""
    model = make_model(TINY)
    S = torch.randint(0, V, (B, 150), generator=torch.Generator().manual_seed(17)).to(dev)
    return model, S, full_forward(model, S), oracle_logits(model, TINY, S), quantised_oracle_logits(model, TINY, S)


@pytest.mark.parametrize("P", [1, 5, 70])
def test_teacher_forced_parity_fp8(tiny, P):
    model, S, full, ref, ref_q = tiny
    check_parity("tiny", decode_logits_fp8(model, S, P), full, ref, ref_q, P)


@pytest.mark.parametrize("cfg", [
    dict(n_layer=2, n_head=12, n_embd=768, vocab_size=50257, n_positions=64),  # GPT-2 124M's widths (Vp = 50432)
    dict(n_layer=1, n_head=25, n_embd=1600, vocab_size=509, n_positions=64),   # 1.5B's widths: no multiples of 256
], ids=["124M-widths", "1.5B-widths"])
def test_teacher_forced_parity_fp8_at_production_widths(cfg):
    cfg = dict(cfg, resid_pdrop=0.1, attn_pdrop=0.1)
    model = make_model(cfg)
    S = torch.randint(0, cfg["vocab_size"], (2, 20), generator=torch.Generator().manual_seed(23)).to(dev)
    check_parity(f"C={cfg['n_embd']}", decode_logits_fp8(model, S, 3), full_forward(model, S),
                 oracle_logits(model, cfg, S), quantised_oracle_logits(model, cfg, S), 3)


# ---- exactness -----------------------------------------------------------------------------------------------------
def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def cache_rows(sess, row, n):
    """Codes and scales of the first n positions of `row`, every layer."""
    return [bits(t[:, row, :, :n]) for t in (sess.kcache, sess.vcache, sess.kscale, sess.vscale)]


def test_extend_equals_steps_over_the_fp8_cache(tiny):
    model, S = tiny[:2]
    counts = [7, 0, 3]
    a = model.decoder(B, max_len=70, kv_dtype="fp8")
    a.prefill(S[:, :5].contiguous())
    got = a.extend(S[:, 5:12].contiguous(), counts)
    assert a.lens == [12, 5, 8] and a.kcache.dtype == torch.uint8
    for row, c in enumerate(counts):  # each row against a one-row session stepped c times
        one = model.decoder(1, max_len=70, kv_dtype="fp8")
        one.prefill(S[row:row + 1, :5].contiguous())
        for j in range(c):
            assert torch.equal(bits(one.step(S[row:row + 1, 5 + j])[0]), bits(got[row, j])), (row, j)
        assert bool(torch.isnan(got[row, c:]).all()) and bool(torch.isfinite(got[row, :c]).all())
        assert torch.equal(bits(one.logits[0]), bits(a.logits[row]))
        for x, y in zip(cache_rows(one, 0, 5 + c), cache_rows(a, row, 5 + c)):
            assert torch.equal(x, y), row


KW = dict(temperature=0.8, top_k=20, seed=1)


def test_fp8_generation_does_not_depend_on_the_batch(tiny):
    model, S = tiny[:2]
    prompts = [S[i, :n].contiguous() for i, n in enumerate((3, 17, 70))]
    many = model.generate_many(prompts, 20, batch_size=2, kv_dtype="fp8", **KW)
    for i, p in enumerate(prompts):  # prompt i alone in a one-row session, drawing with key i
        sess = model.decoder(1, p.numel() + 20, kv_dtype="fp8")
        sess.prefill(p[None])
        seq = torch.zeros(1, p.numel() + 20, dtype=torch.int64, device=dev)
        sess.generate(20, KW["temperature"], KW["top_k"], None, KW["seed"], seq=seq, row_id=[i])
        assert torch.equal(seq[0, p.numel():], many[i][p.numel():]), i
        assert torch.equal(many[i][:p.numel()], p)


def test_refill_over_the_fp8_cache_is_a_one_row_prefill(tiny):
    model, S = tiny[:2]
    sess = model.decoder(B, max_len=100, kv_dtype="fp8")
    sess.prefill(S[:, :9].contiguous())
    for row, n in ((1, 3), (2, 70), (0, 17)):
        prompt = S[row, 20:20 + n].contiguous()
        sess.refill(row, prompt)
        one = model.decoder(1, max_len=100, kv_dtype="fp8")
        one.prefill(prompt[None])
        assert sess.lens[row] == n and torch.equal(bits(sess.logits[row]), bits(one.logits[0]))
        for x, y in zip(cache_rows(sess, row, n), cache_rows(one, 0, n)):
            assert torch.equal(x, y), (row, n)


@pytest.mark.parametrize("pen", [{}, dict(repetition_penalty=1.3)], ids=["plain", "repetition"])
def test_speculative_generation_is_exact_over_the_fp8_cache(tiny, pen):
    model, S = tiny[:2]
    idx = S[:, :9].contiguous()
    kw = dict(seed=3, temperature=0.8, top_k=20, kv_dtype="fp8", **pen)
    assert torch.equal(model.generate(idx, 24, draft_tokens=4, **kw), model.generate(idx, 24, **kw))


def test_session_state(tiny):
    model, S = tiny[:2]
    L, H, Tcap = TINY["n_layer"], TINY["n_head"], 40
    fp8, bf16, default = (model.decoder(B, Tcap, kv_dtype="fp8"), model.decoder(B, Tcap, kv_dtype="bf16"),
                          model.decoder(B, Tcap))
    assert fp8.cache_bytes == L * 2 * B * H * Tcap * 68
    assert bf16.cache_bytes == default.cache_bytes == L * 2 * B * H * Tcap * 128
    assert fp8.kscale.shape == (L, B, H, Tcap) and bf16.kscale is None
    for sess in (bf16, default):
        sess.prefill(S[:, :7].contiguous())
        sess.step(S[:, 7].contiguous())
    assert torch.equal(bits(bf16.logits), bits(default.logits))
    assert torch.equal(bits(bf16.kcache[:, :, :, :8]), bits(default.kcache[:, :, :, :8]))
    assert torch.equal(bits(bf16.vcache[:, :, :, :8]), bits(default.vcache[:, :, :, :8]))
    with pytest.raises(ValueError, match="int4"):
        model.decoder(B, kv_dtype="int4")


def test_cli_with_an_fp8_cache(tmp_path):
    from gpt_2_distributed_amd.train_gpt2_distributed import save_checkpoint
    model = make_model(TINY)
    ckpt = save_checkpoint(model, model.configure_optimizers(), 3, str(tmp_path))
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.generate", "--checkpoint", ckpt, "--model", "auto",
           "--prompt_ids", "11,12,13", "--max_new_tokens", "9", "--batch", "2", "--temperature", "0", "--seed", "5",
           "--kv_dtype", "fp8"]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("[")]
    want = model.generate(torch.tensor([[11, 12, 13]], device=dev), 9, temperature=0.0, kv_dtype="fp8")[0].tolist()
    assert len(rows) == 2 and all(row == want for row in rows)
    assert len(want) == 12 and want[:3] == [11, 12, 13] and all(0 <= t < V for t in want)
