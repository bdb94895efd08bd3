"""The decode kernels (csrc/decode.hip) against fp64 references of the same ops on the same bf16-rounded inputs.

Tolerances are those tests/test_kernels_gpu.py holds the training kernels to for the same output formats (rel_err as
defined there): fp32 outputs at accumulation-order resolution, bf16 outputs at bf16 resolution. Beyond values, each
kernel is checked for what it must NOT touch (sentinel-filled slack / cache positions, compared bitwise) and for
run-to-run bitwise equality."""
import math

import pytest
import torch

from oracle import model_ref
from tests.test_kernels_gpu import rel_err

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
NAN_BITS = 0x7FC1  # a bf16 NaN: a sentinel that poisons whatever reads it
F32_SENTINEL = -12288.0  # exact in bf16 too


@pytest.fixture(scope="module", autouse=True)
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


# ---- skinny GEMM ---------------------------------------------------------------------------------------------------
SHAPES = [(192, 64), (320, 192), (2304, 768), (768, 3072), (1600, 6400), (512, 128)]
MS = (1, 3, 16, 17, 64)
SLACK = 256


def _skinny_inputs(N, Kd):
    g = torch.Generator().manual_seed(N * 7 + Kd)
    A = torch.randn(64, Kd, generator=g).to(BF16).to(dev)
    W = (torch.randn(N, Kd, generator=g) * 0.05).to(BF16).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    resid = torch.randn(64, N, generator=g).to(dev)
    acc = A.double() @ W.double().t()  # fp64 on the bf16-rounded operands
    return A, W, bias, resid, acc


def _run_skinny(K, epi, M, N, Kd, A, W, bias, resid, lda=None, ldc=None):
    """Launch on the first M rows; returns the whole output buffer (M*ldc elements + sentinel slack)."""
    lda, ldc = lda or Kd, ldc or N
    f32 = epi in (K.EPI_F32, K.EPI_RESID)
    out = torch.full((M * ldc + SLACK,), F32_SENTINEL, dtype=torch.float32 if f32 else BF16, device=dev)
    ws = torch.empty(max(K.gemm_skinny_workspace(M, N, Kd), 1), device=dev)
    K.gemm_skinny(epi, M, N, Kd, A, lda, W, Kd, out, ldc, bias=bias, resid=resid if epi == K.EPI_RESID else None,
                  workspace=ws)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N,Kd", SHAPES)
def test_gemm_skinny_against_fp64(K, N, Kd):
    A, W, bias, resid, acc = _skinny_inputs(N, Kd)
    u = acc + bias.double()
    refs = {K.EPI_F32: (u, 1e-6), K.EPI_BF16: (u, 4e-3), K.EPI_RESID: (resid.double() + u, 1e-5),
            K.EPI_GELU: (model_ref.gelu_tanh(u), 4e-3)}
    for M in MS:
        for epi, (ref, tol) in refs.items():
            out = _run_skinny(K, epi, M, N, Kd, A, W, bias, resid)
            err = rel_err(out[:M * N].view(M, N), ref[:M])
            print(f"gemm_skinny N={N} K={Kd} M={M} epi={epi}: rel_err {err:.3e}")
            assert err < tol, (M, epi, err)
            slack = out[M * N:]
            assert bool((slack == F32_SENTINEL).all()), (M, epi, "wrote past M*ldc")


@pytest.mark.parametrize("N,Kd", [(320, 192), (768, 3072), (1600, 6400)])
def test_gemm_skinny_rows_are_independent_and_reproducible(K, N, Kd):
    """Row r of an M = 17 launch has the bits of the M = 1 launch on that row alone (the K split depends on (N, K)
    only, and no row's sum sees another row); two identical launches are bitwise equal."""
    A, W, bias, resid, _ = _skinny_inputs(N, Kd)
    for epi in (K.EPI_F32, K.EPI_BF16, K.EPI_RESID, K.EPI_GELU):
        full = _run_skinny(K, epi, 17, N, Kd, A, W, bias, resid)
        again = _run_skinny(K, epi, 17, N, Kd, A, W, bias, resid)
        assert torch.equal(bits(full), bits(again)), epi
        for r in (0, 5, 16):
            one = _run_skinny(K, epi, 1, N, Kd, A[r:r + 1].contiguous(), W, bias, resid[r:r + 1].contiguous())
            assert torch.equal(bits(one[:N]), bits(full[r * N:(r + 1) * N])), (epi, r)


def test_gemm_skinny_strided_rows(K):
    """The prefill's lm_head reads one row per sequence out of a [B, Tp, C] buffer (lda = Tp * C) and C may be wider than
    N: rows and columns outside the operands are neither read into the result nor written."""
    N, Kd, M, lda, ldc = 320, 192, 5, 3 * 192, 320 + 64
    g = torch.Generator().manual_seed(3)
    buf = torch.randn(M, lda, generator=g).to(BF16).to(dev)
    W = (torch.randn(N, Kd, generator=g) * 0.05).to(BF16).to(dev)
    out = _run_skinny(K, K.EPI_F32, M, N, Kd, buf[:, 2 * Kd:], W, None, None, lda=lda, ldc=ldc)
    ref = buf[:, 2 * Kd:].double() @ W.double().t()
    rows = out[:M * ldc].view(M, ldc)
    assert rel_err(rows[:, :N], ref) < 1e-6
    assert bool((rows[:, N:] == F32_SENTINEL).all()) and bool((out[M * ldc:] == F32_SENTINEL).all())


# ---- kv_store ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 100])
@pytest.mark.parametrize("t0", [0, 7])
def test_kv_store(K, n, t0):
    B, H, Tcap = 2, 3, 128
    C, T_src = 64 * H, (n + 63) // 64 * 64
    g = torch.Generator().manual_seed(n + t0)
    qkv = torch.randn(B * T_src, 3 * C, generator=g).to(BF16).to(dev)
    kc = torch.full((B, H, Tcap, 64), NAN_BITS, dtype=torch.int16, device=dev).view(BF16)
    vc = kc.clone()
    K.kv_store(qkv, kc, vc, B, T_src, n, t0, H, 64, Tcap)
    torch.cuda.synchronize()
    src = qkv.view(B, T_src, 3, H, 64)[:, :n]  # rows >= n are tile padding
    for cache, which in ((kc, 1), (vc, 2)):
        want = torch.full((B, H, Tcap, 64), NAN_BITS, dtype=torch.int16, device=dev)
        want[:, :, t0:t0 + n] = bits(src[:, :, which].permute(0, 2, 1, 3).contiguous())
        assert torch.equal(bits(cache), want), which


# ---- attn_decode ---------------------------------------------------------------------------------------------------
POSITIONS = (0, 1, 63, 64, 65, 255, 256, 1023)
TCAP = 1024


def _attn_case(K, B, H, pos, scale=1.0, seed=0):
    """One launch at `pos` on a cache holding random rows below pos and NaN sentinels from pos on; returns the output,
    the fp64 reference and the caches before / after."""
    C = 64 * H
    g = torch.Generator().manual_seed(seed * 4099 + pos * 31 + B * 7 + H)
    qkv = (torch.randn(B, 3 * C, generator=g) * scale).to(BF16).to(dev)
    caches = []
    for _ in range(2):
        c = torch.full((B, H, TCAP, 64), NAN_BITS, dtype=torch.int16, device=dev).view(BF16)
        if pos:
            c[:, :, :pos] = (torch.randn(B, H, pos, 64, generator=g) * scale).to(BF16).to(dev)
        caches.append(c)
    kc, vc = caches
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.full((B * C + SLACK,), F32_SENTINEL, dtype=BF16, device=dev)
    ws = torch.empty(K.attn_decode_workspace(B, H, TCAP), device=dev)
    K.attn_decode(qkv, kc, vc, out, ws, B, H, 64, TCAP, pos)
    torch.cuda.synchronize()
    q, kn, vn = (qkv.view(B, 3, H, 64)[:, i].double() for i in range(3))
    keys = torch.cat([kc0[:, :, :pos].double(), kn[:, :, None]], dim=2)  # the key / value at pos: the new token's
    vals = torch.cat([vc0[:, :, :pos].double(), vn[:, :, None]], dim=2)
    att = torch.softmax(torch.einsum("bhd,bhtd->bht", q, keys) / 8.0, dim=-1)
    ref = torch.einsum("bht,bhtd->bhd", att, vals).reshape(B, C)
    return out, ref, qkv, (kc0, vc0), (kc, vc)


@pytest.mark.parametrize("B,H", [(1, 2), (1, 5), (3, 2), (3, 5)])
def test_attn_decode_against_fp64(K, B, H):
    C = 64 * H
    for pos in POSITIONS:
        out, ref, qkv, before, after = _attn_case(K, B, H, pos)
        err = rel_err(out[:B * C].view(B, C), ref)
        print(f"attn_decode B={B} H={H} pos={pos}: rel_err {err:.3e}")
        assert err < 6e-3, (pos, err)
        assert bool((out[B * C:] == F32_SENTINEL).all())
        for i, (c0, c1) in enumerate(zip(before, after)):
            new = qkv.view(B, 3, H, 64)[:, 1 + i]
            assert torch.equal(bits(c1[:, :, pos]), bits(new)), (pos, "the new k / v is not at pos")
            assert torch.equal(bits(c1[:, :, :pos]), bits(c0[:, :, :pos])), (pos, "positions < pos changed")
            assert torch.equal(bits(c1[:, :, pos + 1:]), bits(c0[:, :, pos + 1:])), (pos, "positions > pos changed")


def test_attn_decode_large_score_spread(K):
    """q and k scaled so the scores q.k/8 have a standard deviation near 10 (a spread of +-30 over 1024 keys): the key
    ranges' maxima differ by tens, which exercises the rescaling of the cross-range (max, sum, acc) combine."""
    B, H, pos = 2, 2, 1023
    out, ref, qkv, (kc0, _), _ = _attn_case(K, B, H, pos, scale=math.sqrt(10.0), seed=1)
    s = torch.einsum("bhd,bhtd->bht", qkv.view(B, 3, H, 64)[:, 0].double(), kc0[:, :, :pos].double()) / 8.0
    assert float(s.max()) > 25 and float(s.min()) < -25, (float(s.min()), float(s.max()))
    err = rel_err(out[:B * 64 * H].view(B, 64 * H), ref)
    print(f"attn_decode spread [{float(s.min()):.1f}, {float(s.max()):.1f}]: rel_err {err:.3e}")
    assert err < 6e-3, err


def test_attn_decode_is_reproducible(K):
    for pos in (65, 1023):
        a = _attn_case(K, 3, 5, pos)[0]
        b = _attn_case(K, 3, 5, pos)[0]
        assert torch.equal(bits(a), bits(b)), pos


# ---- embed_decode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 191])
def test_embed_decode(K, pos):
    B, C, V, T = 5, 128, 509, 192
    g = torch.Generator().manual_seed(pos)
    wte, wpe = torch.randn(V, C, generator=g).to(dev), torch.randn(T, C, generator=g).to(dev)
    tok = torch.randint(0, V, (B,), generator=g).to(dev)
    x = torch.full((B * C + SLACK,), F32_SENTINEL, device=dev)
    K.embed_decode(tok, wte, wpe, x, B, C, pos)
    torch.cuda.synchronize()
    assert torch.equal(x[:B * C].view(B, C), wte[tok] + wpe[pos])
    assert bool((x[B * C:] == F32_SENTINEL).all())
