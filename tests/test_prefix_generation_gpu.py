"""DecodeSession.append / prefix / refill(prefix=) and generate_many over a SharedPrefix: a run of tokens appended to a live row in
one pass over the weights (the trunk over a chunk, csrc/prefill_cached.hip), and a prompt prefix computed once.

Accuracy is measured against the fp32 oracle at the same position, and bounded by twice the error of the path that
existed before: the one-shot refill of the concatenation (bf16), or the same tokens through extend (fp8: the path whose
key rule, quantised keys for the chunk's own tokens, append shares)."""
import pytest
import torch

from gpt_2_distributed_amd import generation
from tests.test_generation_gpu import TINY, make_model, oracle_logits
from tests.test_kernels_gpu import rel_err

pytestmark = pytest.mark.gpu

dev = "cuda"
V = TINY["vocab_size"]


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    model = make_model(TINY)
    S = torch.randint(0, V, (3, 150), generator=torch.Generator().manual_seed(23)).to(dev)
    return model, S, oracle_logits(model, TINY, S)


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def caches(sess):
    return [t for t in (sess.kcache, sess.vcache, sess.kscale, sess.vscale) if t is not None]


def values(sess, t, scale):
    from gpt_2_distributed_amd.generation import kv_dequantize
    return (t if scale is None else kv_dequantize(t, scale)).double()


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("P, n", [(5, 1), (5, 70), (64, 64), (70, 59)])
def test_append_matches_the_oracle_as_the_earlier_paths_do(tiny, P, n, kv):
    model, S, ref = tiny
    row, T = 1, P + n
    sess, ext = model.decoder(3, kv_dtype=kv), model.decoder(3, kv_dtype=kv)
    sess.prefill(S[:, :P]), ext.prefill(S[:, :P])
    before = [t.clone() for t in caches(sess)] + [sess.logits.clone()]
    sess.append(row, S[row, P:T])
    ext.extend(S[:, P:T].contiguous(), counts=[0, n, 0])
    assert sess.lens == [P, T, P] == ext.lens
    # the other rows keep their logits and cache bits
    pick = lambda t: t[:, [0, 2]] if t.dim() > 2 else t[[0, 2]]  # noqa: E731  (caches [L][B]..., logits [B][Vp])
    for b, a in zip(before, caches(sess) + [sess.logits]):
        assert torch.equal(bits(pick(a)), bits(pick(b)))
    # accuracy against the oracle, bounded by the reference path's
    if kv == "bf16":
        one = model.decoder(1)
        one.refill(0, S[row, :T])
        base_logits = one.logits[0, :V]
    else:
        base_logits = ext.logits[row, :V]
    want = ref[row, T - 1]
    err, base = rel_err(sess.logits[row, :V], want), rel_err(base_logits, want)
    print(f"append {kv} P={P} n={n}: rel_err {err:.3e}, reference path {base:.3e}")
    assert err <= 2 * base, (err, base)
    # the cache below lens holds the appended tokens' keys and values: those extend stores. Layer 0's bf16 keys depend
    # on the embedding and LN1 only; elsewhere both are roundings of nearby values: a few units in the last place of
    # the format (bf16 2^-8: 2e-2; e4m3 2^-3, where a flipped code moves one element by a step: 0.125 in norm)
    if kv == "bf16":
        assert torch.equal(bits(sess.kcache[0, row, :, P:T]), bits(ext.kcache[0, row, :, P:T]))
    tol = 2e-2 if kv == "bf16" else 0.125
    for name, a, b, sa, sb in (("k", sess.kcache, ext.kcache, sess.kscale, ext.kscale),
                               ("v", sess.vcache, ext.vcache, sess.vscale, ext.vscale)):
        cut = lambda t: None if t is None else t[:, row, :, :T]  # noqa: E731
        e = rel_err(values(sess, cut(a), cut(sa)), values(ext, cut(b), cut(sb)))
        print(f"  cache {name} against extend's: rel_err {e:.3e}")
        assert e < tol, (name, e)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_refill_with_a_prefix_is_refill_then_append(tiny, kv):
    model, S, _ = tiny
    p, suffix = S[0, :70], S[1, :37]
    a, b = model.decoder(3, kv_dtype=kv), model.decoder(3, kv_dtype=kv)
    pre = a.prefix(p)
    assert pre.length == 70 and tuple(pre.k.shape) == (TINY["n_layer"], TINY["n_head"], 70, 64)
    a.refill(1, suffix, prefix=pre)
    b.refill(1, p)
    b.append(1, suffix)
    assert a.lens[1] == b.lens[1] == 107
    assert torch.equal(bits(a.logits[1]), bits(b.logits[1]))
    for x, y in zip(caches(a), caches(b)):
        assert torch.equal(bits(x[:, 1, :, :107]), bits(y[:, 1, :, :107]))
    a.refill(2, suffix[:0], prefix=pre)  # an empty suffix: the prefix's own logits
    assert a.lens[2] == 70 and torch.equal(bits(a.logits[2]), bits(pre.logits))


@pytest.mark.parametrize("how", [dict(temperature=0.8, top_k=50), dict(kv_dtype="fp8")], ids=["top_k", "fp8"])
def test_generate_many_with_a_prefix_does_not_depend_on_the_batch(tiny, how):
    model, S, _ = tiny
    p = S[2, :40]
    prompts = [S[0, :9], S[1, :1], S[0, :0], S[1, 20:85], S[2, 50:73]]
    one = model.generate_many(generation.SharedPrefix(p, prompts), 12, seed=1, batch_size=1, **how)
    four = model.generate_many(generation.SharedPrefix(p, prompts), 12, seed=1, batch_size=4, **how)
    for q, x, y in zip(prompts, one, four):
        assert torch.equal(x, y)
        assert x.numel() == 40 + q.numel() + 12 and torch.equal(x[:40 + q.numel()], torch.cat([p, q]))


def test_refusals(tiny):
    model, S, _ = tiny
    sess = model.decoder(2, max_len=80)
    sess.refill(0, S[0, :70])
    with pytest.raises(ValueError, match="empty"):
        sess.append(1, S[0, :4])
    with pytest.raises(ValueError, match="exceed"):
        sess.append(0, S[0, :11])
    with pytest.raises(ValueError, match="beam"):
        model.generate(generation.SharedPrefix(S[1, :8], [S[0, :4]]), 4, num_beams=2)
