"""gpt2mi_attn_extend and gpt2mi_decode_extend (several rows of a launch in one sequence) against the one-position
entries bit for bit, against an fp64 reference, and for what they must not touch.

Everything above them (DecodeSession.extend, speculate's "the same tokens as the plain loop") rests on one claim: a row
of an extend call has the bits it gets when the rows are fed one position at a time. Shapes are the smallest that show
it: B = 3 sequences, H = 2, a cache of 70 positions (three key ranges of 32, the last partial) and 11 rows in three
runs: across the 32-key range edge, from an empty stream, and up to the last cache slot. A second map leaves a sequence
out."""
import pytest
import torch

from tests.test_generation_gpu import TINY, make_model
from tests.test_kernels_gpu import rel_err

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
SENTINEL_BITS = 0x7FC1  # a bf16 NaN: poisons whatever reads it, and no kernel writes it
WS_SENTINEL = -12288.0
B, H, TCAP, C = 3, 2, 70, 128
MAPS = {
    "three-runs": ([0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2], [30, 31, 32, 33, 0, 1, 2, 66, 67, 68, 69]),
    "one-absent": ([0, 0, 0, 0, 2, 2, 2, 2], [30, 31, 32, 33, 66, 67, 68, 69]),
}


@pytest.fixture(scope="module", autouse=True)
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def firsts(seq, pos):
    """first[r]: the position of the first row of row r's run."""
    return [pos[min(i for i, s in enumerate(seq) if s == seq[r])] for r in range(len(seq))]


@pytest.fixture(scope="module")
def attn_inputs():
    """Random bf16 qkv rows and caches, full to the last position (never modified: every run works on clones)."""
    g = torch.Generator().manual_seed(43)
    qkv = torch.randn(11, 3 * C, generator=g).to(BF16).to(dev)
    kc = torch.randn(B, H, TCAP, 64, generator=g).to(BF16).to(dev)
    vc = torch.randn(B, H, TCAP, 64, generator=g).to(BF16).to(dev)
    return qkv, kc, vc


def run_extend(K, qkv, kc, vc, seq, pos):
    R = len(seq)
    kc, vc = kc.clone(), vc.clone()
    out = torch.full((R, C), -12288.0, dtype=BF16, device=dev)
    ws = torch.full((K.attn_decode_workspace(R, H, TCAP),), WS_SENTINEL, device=dev)
    K.attn_extend(qkv[:R].contiguous(), kc, vc, out, ws, R, B, H, 64, TCAP, seq, pos)
    torch.cuda.synchronize()
    return out, kc, vc, ws


def run_one_by_one(K, qkv, kc, vc, seq, pos):
    """The same rows through gpt2mi_attn_decode_ragged, one position per call, on the row's own sequence (a [1][H][Tcap]
    slice of the caches: a row's bits depend on its own inputs and position only)."""
    R = len(seq)
    kc, vc = kc.clone(), vc.clone()
    out = torch.full((R, C), -12288.0, dtype=BF16, device=dev)
    ws = torch.empty(K.attn_decode_workspace(1, H, TCAP), device=dev)
    for r in range(R):
        K.attn_decode_ragged(qkv[r:r + 1], kc[seq[r]:seq[r] + 1], vc[seq[r]:seq[r] + 1], out[r:r + 1], ws, 1, H, 64,
                             TCAP, [pos[r]])
    torch.cuda.synchronize()
    return out, kc, vc


@pytest.mark.parametrize("name", MAPS)
def test_attn_extend_has_the_bits_of_one_position_at_a_time(K, attn_inputs, name):
    seq, pos = MAPS[name]
    out, kc1, vc1, _ = run_extend(K, *attn_inputs, seq, pos)
    want, kcs, vcs = run_one_by_one(K, *attn_inputs, seq, pos)
    assert torch.equal(bits(out), bits(want))
    assert torch.equal(bits(kc1), bits(kcs)) and torch.equal(bits(vc1), bits(vcs))
    assert not torch.equal(bits(kc1), bits(attn_inputs[1]))  # (the call did write)


def test_attn_extend_with_runs_of_one_is_attn_decode_ragged(K, attn_inputs):
    """The relation the two entries' shared body encodes: the decode entry is the extend entry with first = pos. With
    the identity map (row r is sequence r, every run one row) at positions 0 / 32 / 69 (the first key, a range edge, the
    last and partly filled range) one gpt2mi_attn_extend gives what one gpt2mi_attn_decode_ragged over the same three
    rows gives: out, both caches and the whole sentinel-filled workspace, bit for bit."""
    qkv, kc, vc = attn_inputs
    seq, pos = [0, 1, 2], [0, 32, 69]
    out, kc1, vc1, ws = run_extend(K, qkv, kc, vc, seq, pos)
    kc2, vc2 = kc.clone(), vc.clone()
    want = torch.full((B, C), -12288.0, dtype=BF16, device=dev)
    ws2 = torch.full_like(ws, WS_SENTINEL)
    K.attn_decode_ragged(qkv[:B].contiguous(), kc2, vc2, want, ws2, B, H, 64, TCAP, pos)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))
    assert torch.equal(bits(kc1), bits(kc2)) and torch.equal(bits(vc1), bits(vc2))
    assert torch.equal(bits(ws), bits(ws2))
    assert not torch.equal(bits(kc1), bits(kc)) and bool((ws != WS_SENTINEL).any())  # (the calls did write)


@pytest.mark.parametrize("name", MAPS)
def test_attn_extend_against_fp64(K, attn_inputs, name):
    seq, pos = MAPS[name]
    qkv, kc, vc = attn_inputs
    out, _, _, _ = run_extend(K, qkv, kc, vc, seq, pos)
    first = firsts(seq, pos)
    q, kn, vn = (qkv.view(11, 3, H, 64)[:, i].double() for i in range(3))
    for r, (s, p) in enumerate(zip(seq, pos)):
        run = range(r - (p - first[r]), r + 1)  # the rows of this run up to r: positions first..p
        keys = torch.cat([kc[s, :, :first[r]].double()] + [kn[i][:, None] for i in run], dim=1)
        vals = torch.cat([vc[s, :, :first[r]].double()] + [vn[i][:, None] for i in run], dim=1)
        assert keys.size(1) == p + 1
        att = torch.softmax(torch.einsum("hd,htd->ht", q[r], keys) / 8.0, dim=-1)
        ref = torch.einsum("ht,htd->hd", att, vals).reshape(C)
        err = rel_err(out[r], ref)
        print(f"attn_extend {name} row {r} (seq {s}, pos {p}): rel_err {err:.3e}")
        assert err < 6e-3, (r, s, p, err)  # the scalar kernel's bound (test_decode_kernels_gpu.py): the same arithmetic


@pytest.mark.parametrize("name", MAPS)
def test_attn_extend_reads_in_call_keys_from_qkv_and_writes_one_position_per_row(K, attn_inputs, name):
    """Every present stream holds a NaN sentinel from its run's first position upward: a finite output shows that the
    keys of this call came from qkv and that nothing above pos[r] was read. Afterwards exactly positions first..last
    of each present stream differ, holding the rows' k / v bits; an absent sequence's streams and the workspace slots
    of ranges beyond a row's position are untouched."""
    seq, pos = MAPS[name]
    qkv, kc, vc = attn_inputs
    kc, vc = kc.clone(), vc.clone()
    first = firsts(seq, pos)
    for s, f in set(zip(seq, first)):
        bits(kc)[s, :, f:] = SENTINEL_BITS
        bits(vc)[s, :, f:] = SENTINEL_BITS
    out, kc1, vc1, ws = run_extend(K, qkv, kc, vc, seq, pos)
    R = len(seq)
    assert bool(torch.isfinite(out.float()).all())
    new = qkv.view(11, 3, H, 64)
    for c0, c1, which in ((kc, kc1, 1), (vc, vc1, 2)):
        changed = (bits(c0) != bits(c1)).any(-1)  # [B, H, Tcap]
        want = torch.zeros_like(changed)
        for r, (s, p) in enumerate(zip(seq, pos)):
            want[s, :, p] = True
            assert torch.equal(bits(c1[s, :, p]), bits(new[r, which])), (which, r)
        assert torch.equal(changed, want), which
        for s in set(range(B)) - set(seq):
            assert torch.equal(bits(c1[s]), bits(c0[s])), (which, s)
    nr = (TCAP + 31) // 32
    ml, acc = ws[:R * H * nr * 2].view(R, H, nr, 2), ws[R * H * nr * 2:].view(R, H, nr, 64)
    for r, p in enumerate(pos):
        used = p // 32 + 1
        assert bool((ml[r, :, used:] == WS_SENTINEL).all()) and bool((acc[r, :, used:] == WS_SENTINEL).all()), r
        assert bool((ml[r, :, :used] != WS_SENTINEL).all()), r


# ---- gpt2mi_decode_extend against gpt2mi_decode_step_ragged ------------------------------------------------------------
WIDE = dict(n_layer=2, n_head=12, n_embd=768, vocab_size=50257, n_positions=64)  # GPT-2 124M's widths (Vp = 50432)
CASES = {
    "tiny": (TINY, 3, 70, MAPS["three-runs"]),
    "tiny-one-absent": (TINY, 3, 70, MAPS["one-absent"]),
    "124M-widths": (WIDE, 2, 40, ([0, 0, 0, 0, 0, 0, 1, 1], [29, 30, 31, 32, 33, 34, 31, 32])),
}


@pytest.mark.parametrize("name", CASES)
def test_decode_extend_has_the_bits_of_one_step_per_position(K, name):
    """One gpt2mi_decode_extend over the row map against the same tokens through gpt2mi_decode_step_ragged, one position
    per call, each sequence in a one-row session of its own that starts from the same cache contents: every logits row
    and both caches, bit for bit."""
    cfg, nseq, tcap, (seq, pos) = CASES[name]
    model = make_model(cfg)
    g = torch.Generator().manual_seed(5)
    R, L, nh = len(seq), cfg["n_layer"], cfg["n_head"]
    tok = torch.randint(0, cfg["vocab_size"], (R,), generator=g).to(dev)
    kc0 = torch.randn(L, nseq, nh, tcap, 64, generator=g).to(BF16).to(dev)
    vc0 = torch.randn(L, nseq, nh, tcap, 64, generator=g).to(BF16).to(dev)
    sess = model.decoder(nseq, max_len=tcap)
    sess._ready(True)  # (what a prefill does first: the bf16 weight shadow is current)
    sess.kcache.copy_(kc0), sess.vcache.copy_(vc0)
    scratch, plan = sess._rows_plan()
    K.decode_extend(plan, tok, seq, pos)
    torch.cuda.synchronize()
    got = scratch["logits"][:R].clone()
    assert bool(torch.isfinite(got[:, :cfg["vocab_size"]]).all())
    for s in range(nseq):
        one = model.decoder(1, max_len=tcap)
        one.kcache.copy_(kc0[:, s:s + 1]), one.vcache.copy_(vc0[:, s:s + 1])
        for r in [r for r in range(R) if seq[r] == s]:
            K.decode_step_ragged(one._plan, tok[r:r + 1], [pos[r]])
            assert torch.equal(bits(one.logits[0]), bits(got[r])), (s, r)
        assert torch.equal(bits(one.kcache[:, 0]), bits(sess.kcache[:, s])), s
        assert torch.equal(bits(one.vcache[:, 0]), bits(sess.vcache[:, s])), s
    written = (bits(sess.kcache) != bits(kc0)).any(-1).any(0).any(1)  # [nseq, Tcap]
    want = torch.zeros_like(written)
    for s, p in zip(seq, pos):
        want[s, p] = True
    assert torch.equal(written, want)
