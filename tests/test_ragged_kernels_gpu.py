"""The ragged decode kernels (gpt2mi_*_ragged: one position per row) against fp64 references, against their scalar
twins bit for bit, and for what they must not touch.

Everything above them (DecodeSession with rows at different positions, refill, generate_many's "a prompt's continuation
does not depend on what it was batched with") rests on one claim: row b of a ragged call has the bits the scalar entry
gives that row at pos = pos[b]. Shapes are the smallest that show it: B = 4, H = 2, a cache of 70 positions (three key
ranges of 32, the last one partial), positions on both sides of a range edge and at both ends of the cache, a row with
one range next to a row with three."""
import pytest
import torch

from gpt_2_distributed_amd.generation import sample_reference, uniform_at
from tests.test_kernels_gpu import rel_err
from tests.test_sampling_gpu import MARGIN, make_logits, margins, padded

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
SENTINEL_BITS = 0x7FC1  # a bf16 NaN: poisons whatever reads it, and no kernel writes it
B, H, TCAP, C = 4, 2, 70, 128
POSITIONS = ([0, 31, 32, 69], [63, 64, 5, 33])


@pytest.fixture(scope="module", autouse=True)
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


# ---- attn_decode_ragged ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attn_inputs():
    """Random bf16 qkv and caches, full to the last position: a row reads only what lies below its position."""
    g = torch.Generator().manual_seed(41)
    qkv = torch.randn(B, 3 * C, generator=g).to(BF16).to(dev)
    kc = torch.randn(B, H, TCAP, 64, generator=g).to(BF16).to(dev)
    vc = torch.randn(B, H, TCAP, 64, generator=g).to(BF16).to(dev)
    return qkv, kc, vc


def run_ragged(K, qkv, kc, vc, pos):
    kc, vc = kc.clone(), vc.clone()
    out = torch.full((B, C), -12288.0, dtype=BF16, device=dev)
    ws = torch.full((K.attn_decode_workspace(B, H, TCAP),), float("nan"), device=dev)  # unwritten slots poison a reader
    K.attn_decode_ragged(qkv, kc, vc, out, ws, B, H, 64, TCAP, pos)
    torch.cuda.synchronize()
    return out, kc, vc


def run_scalar(K, qkv, kc, vc, pos):
    kc, vc = kc.clone(), vc.clone()
    out = torch.full((B, C), -12288.0, dtype=BF16, device=dev)
    ws = torch.full((K.attn_decode_workspace(B, H, TCAP),), float("nan"), device=dev)
    K.attn_decode(qkv, kc, vc, out, ws, B, H, 64, TCAP, pos)
    torch.cuda.synchronize()
    return out, kc, vc


@pytest.mark.parametrize("pos", POSITIONS, ids=str)
def test_attn_decode_ragged_against_fp64(K, attn_inputs, pos):
    qkv, kc, vc = attn_inputs
    out, _, _ = run_ragged(K, qkv, kc, vc, pos)
    q, kn, vn = (qkv.view(B, 3, H, 64)[:, i].double() for i in range(3))
    for b, p in enumerate(pos):
        keys = torch.cat([kc[b, :, :p].double(), kn[b, :, None]], dim=1)  # the key / value at pos[b]: the new token's
        vals = torch.cat([vc[b, :, :p].double(), vn[b, :, None]], dim=1)
        att = torch.softmax(torch.einsum("hd,htd->ht", q[b], keys) / 8.0, dim=-1)
        ref = torch.einsum("ht,htd->hd", att, vals).reshape(C)
        err = rel_err(out[b], ref)
        print(f"attn_decode_ragged pos={pos} row {b}: rel_err {err:.3e}")
        assert err < 6e-3, (b, p, err)  # the scalar kernel's bound (test_decode_kernels_gpu.py): the same arithmetic


@pytest.mark.parametrize("pos", POSITIONS, ids=str)
def test_attn_decode_ragged_rows_have_the_scalar_kernels_bits(K, attn_inputs, pos):
    """out[b] and row b's caches after the ragged call are those of gpt2mi_attn_decode on the same inputs at pos[b]."""
    qkv, kc, vc = attn_inputs
    out, kc1, vc1 = run_ragged(K, qkv, kc, vc, pos)
    for b, p in enumerate(pos):
        want, kcs, vcs = run_scalar(K, qkv, kc, vc, p)
        assert torch.equal(bits(out[b]), bits(want[b])), (b, p)
        assert torch.equal(bits(kc1[b]), bits(kcs[b])) and torch.equal(bits(vc1[b]), bits(vcs[b])), (b, p)


@pytest.mark.parametrize("p", [0, 31, 32, 69])
def test_attn_decode_ragged_at_equal_positions_is_the_scalar_call(K, attn_inputs, p):
    qkv, kc, vc = attn_inputs
    got, want = run_ragged(K, qkv, kc, vc, [p] * B), run_scalar(K, qkv, kc, vc, p)
    for g, w in zip(got, want):
        assert torch.equal(bits(g), bits(w)), p


@pytest.mark.parametrize("pos", POSITIONS, ids=str)
def test_attn_decode_ragged_writes_one_cache_position_per_stream(K, attn_inputs, pos):
    """Caches pre-filled with a sentinel bit pattern above each row's position (what is below is read): afterwards only
    position pos[b] of each (b, h) stream differs from before, and it holds the row's k / v bits; nothing above pos[b]
    was read (the sentinel is a NaN: it would poison the output)."""
    qkv, kc, vc = attn_inputs
    kc, vc = kc.clone(), vc.clone()
    for b, p in enumerate(pos):
        bits(kc)[b, :, p:] = SENTINEL_BITS
        bits(vc)[b, :, p:] = SENTINEL_BITS
    out, kc1, vc1 = run_ragged(K, qkv, kc, vc, pos)
    assert bool(torch.isfinite(out.float()).all())
    new = qkv.view(B, 3, H, 64)
    for c0, c1, which in ((kc, kc1, 1), (vc, vc1, 2)):
        changed = (bits(c0) != bits(c1)).any(-1)  # [B, H, Tcap]
        for b, p in enumerate(pos):
            assert changed[b, :, p].all() and int(changed[b].sum()) == H, (which, b, p)
            assert torch.equal(bits(c1[b, :, p]), bits(new[b, which])), (which, b, p)


# ---- embed_decode_ragged -----------------------------------------------------------------------------------------------
def test_embed_decode_ragged(K):
    V, T, pos = 509, 192, [0, 1, 191, 64]
    g = torch.Generator().manual_seed(5)
    wte, wpe = torch.randn(V, C, generator=g).to(dev), torch.randn(T, C, generator=g).to(dev)
    tok = torch.randint(0, V, (B,), generator=g).to(dev)
    x = torch.full((B * C + 256,), -12288.0, device=dev)
    K.embed_decode_ragged(tok, wte, wpe, x, B, C, pos)
    torch.cuda.synchronize()
    assert torch.equal(x[:B * C].view(B, C), wte[tok] + wpe[torch.tensor(pos, device=dev)])
    assert bool((x[B * C:] == -12288.0).all())
    same = torch.empty(B, C, device=dev)
    K.embed_decode_ragged(tok, wte, wpe, same, B, C, [7] * B)
    want = torch.empty(B, C, device=dev)
    K.embed_decode(tok, wte, wpe, want, B, C, 7)
    assert torch.equal(same, want)


# ---- sample_ragged -----------------------------------------------------------------------------------------------------
V, LDL, LSEQ = 509, 512, 40
SAMPLER = dict(temperature=0.8, top_k=20, top_p=0.9)


def ragged_sample(K, buf, pos, row_id, seed, seq=None, want_probs=True):
    n = buf.size(0)
    tok = torch.full((n,), -7, dtype=torch.int64, device=dev)
    probs = torch.full((n, V), -1.0, device=dev) if want_probs else None
    K.sample_ragged(buf, V, SAMPLER["temperature"], SAMPLER["top_k"], SAMPLER["top_p"], seed, pos, tok, row_id=row_id,
                    seq_out=seq, probs_out=probs)
    torch.cuda.synchronize()
    return tok.cpu(), (probs.cpu() if want_probs else None)


def keyed_uniforms(seed, row_id, pos):
    return torch.tensor([uniform_at(seed, r, p) for r, p in zip(row_id, pos)], dtype=torch.float64)


def test_sample_ragged_matches_the_reference_with_per_row_keys(K):
    """Tokens and probs_out against sample_reference fed uniform_at(seed, row_id[b], pos[b]); the comparison rule is
    the sampling test's exact case (the seed is the first that keeps every row's u 1e-5 from a CDF boundary and every
    exclusive mass 1e-5 from top_p, checked in float64 on the CPU before anything runs)."""
    lg = make_logits(B, V, seed=301)
    pos, row_id = [3, 17, 0, 39], [11, 2, 70000, 5]
    T, k, p = SAMPLER["temperature"], SAMPLER["top_k"], SAMPLER["top_p"]
    for seed in range(40):
        u = keyed_uniforms(seed, row_id, pos)
        d_u, d_p = margins(lg, T, k, p, u)
        if d_u >= MARGIN and d_p >= MARGIN:
            break
    else:
        raise AssertionError("no seed in 0..39 keeps every row 1e-5 away from a boundary")
    want_tok, want_probs = sample_reference(lg, T, k, p, u)
    seq = torch.full((B, LSEQ), -99, dtype=torch.int64, device=dev)
    tok, probs = ragged_sample(K, padded(lg, LDL), pos, row_id, seed, seq=seq)
    assert torch.equal(tok, want_tok), (tok.tolist(), want_tok.tolist())
    big = want_probs >= 2e-38
    assert bool((probs[big] > 0).all()) and bool((probs[want_probs == 0] == 0).all())
    assert bool((probs[~big] <= 4e-38).all())
    rel = (probs.double() - want_probs).abs()[big] / want_probs[big]
    assert float(rel.max()) <= 1e-5, float(rel.max())
    # seq_out: column pos[b] of row b, nothing else
    seq = seq.cpu()
    for b in range(B):
        assert int(seq[b, pos[b]]) == int(tok[b])
        seq[b, pos[b]] = -99
    assert bool((seq == -99).all())


def test_sample_ragged_rows_do_not_see_each_other(K):
    """Row b's token and distribution do not change when the other rows' positions and draw keys do."""
    buf = padded(make_logits(B, V, seed=302), LDL)
    tok, probs = ragged_sample(K, buf, [3, 17, 0, 39], [11, 2, 70000, 5], 9)
    for b in range(B):
        pos, row_id = [8, 1, 30, 2], [0, 1, 2, 3]
        pos[b], row_id[b] = [3, 17, 0, 39][b], [11, 2, 70000, 5][b]
        t2, p2 = ragged_sample(K, buf, pos, row_id, 9)
        assert int(t2[b]) == int(tok[b]) and torch.equal(p2[b], probs[b]), b
    # the key matters: over 64 keys a row draws more than one token
    draws = {int(ragged_sample(K, buf, [3] * B, [r] * B, 9, want_probs=False)[0][0]) for r in range(64)}
    assert len(draws) > 1


def test_sample_ragged_without_keys_at_equal_positions_is_the_scalar_sampler(K):
    buf = padded(make_logits(B, V, seed=303), LDL)
    for T in (0.0, 0.8):
        tok = torch.full((2, B), -7, dtype=torch.int64, device=dev)
        probs = torch.full((2, B, V), -1.0, device=dev)
        seq = torch.full((2, B, LSEQ), -99, dtype=torch.int64, device=dev)
        K.sample(buf, V, T, 20, 0.9, 4, 9, tok[0], seq_out=seq[0], probs_out=probs[0])
        K.sample_ragged(buf, V, T, 20, 0.9, 4, [9] * B, tok[1], seq_out=seq[1], probs_out=probs[1])
        torch.cuda.synchronize()
        assert torch.equal(tok[0], tok[1]) and torch.equal(seq[0], seq[1])
        assert torch.equal(bits(probs[0]), bits(probs[1])), T
