"""The fp8 cache kernels (csrc/decode.hip: kv_store_fp8, attn_decode_fp8, attn_extend_fp8) on the MI355X.

The quantiser is held to generation.kv_quantize bit for bit (computed on the CPU, where torch's cast to float8_e4m3fn
rounds to nearest even and keeps subnormals). The attention is held to an fp64 reference computed from the dequantised
cache, the new token's k / v passed through kv_quantize too: the quantisation sits in the reference, so what is left is
the fp32 arithmetic and the bf16 rounding of the output, and the bound is the one tests/test_decode_kernels_gpu.py holds
the bf16 kernel to. Code and scale tensors start out as sentinels (0x7F, e4m3fn's NaN, and NaN scales): anything read
above a row's position poisons the output, anything written outside a call's positions shows bitwise."""
import math

import pytest
import torch

from gpt_2_distributed_amd.generation import kv_dequantize, kv_quantize
from tests.test_kernels_gpu import rel_err
from tests.test_kv_fp8_cpu import constructed_rows

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
CODE_SENTINEL = 0x7F
OUT_SENTINEL = -12288.0
SLACK = 256


@pytest.fixture(scope="module", autouse=True)
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def sentinels(*shape):
    """A code tensor of 0x7F and a scale tensor of NaN (compared through their bits)."""
    return (torch.full((*shape, 64), CODE_SENTINEL, dtype=torch.uint8, device=dev),
            torch.full(shape, float("nan"), device=dev))


def quantize_on_host(x):
    """kv_quantize on the CPU (the reference cast), moved to the device."""
    codes, scale = kv_quantize(x.cpu())
    return codes.to(dev), scale.to(dev)


# ---- kv_store_fp8 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 100])
@pytest.mark.parametrize("t0", [0, 7])
def test_kv_store_fp8_is_kv_quantize(K, n, t0):
    B, H, Tcap = 2, 3, 128
    C, T_src = 64 * H, (n + 63) // 64 * 64
    g = torch.Generator().manual_seed(n + t0)
    qkv = torch.randn(B * T_src, 3 * C, generator=g) * 2.0 ** torch.randint(-6, 7, (B * T_src, 1), generator=g).float()
    rows = qkv.view(B, T_src, 3, H, 64)
    for i, row in enumerate(constructed_rows().values()):  # the edge rows, spread over (b, t, K or V, h)
        rows[i % B, (5 * i) % n, 1 + i % 2, i % H] = row.float()
    qkv = qkv.to(BF16).to(dev)
    (kc, ks), (vc, vs) = sentinels(B, H, Tcap), sentinels(B, H, Tcap)
    K.kv_store_fp8(qkv, kc, vc, ks, vs, B, T_src, n, t0, H, 64, Tcap)
    torch.cuda.synchronize()
    src = qkv.view(B, T_src, 3, H, 64)[:, :n]  # rows >= n are tile padding
    for codes, scale, which in ((kc, ks, 1), (vc, vs, 2)):
        want_c, want_s = sentinels(B, H, Tcap)
        want_c[:, :, t0:t0 + n], want_s[:, :, t0:t0 + n] = quantize_on_host(src[:, :, which].permute(0, 2, 1, 3))
        assert torch.equal(codes, want_c), which
        assert torch.equal(bits(scale), bits(want_s)), which


# ---- attn_decode_fp8 -------------------------------------------------------------------------------------------------
POSITIONS = (0, 1, 63, 64, 65, 255, 1023)
TCAP = 1024


def _attn_case(K, B, H, pos, scale=1.0, seed=0):
    """One launch with every row at `pos` on a cache holding kv_quantize of random rows below pos and sentinels from
    pos on; returns the output, the fp64 reference, (q, the reference's keys), kv_quantize of the new k and v, and the
    cache [kcodes, vcodes, kscales, vscales] before / after."""
    C = 64 * H
    g = torch.Generator().manual_seed(seed * 4099 + pos * 31 + B * 7 + H)
    qkv = (torch.randn(B, 3 * C, generator=g) * scale).to(BF16)
    kv = []
    for _ in range(2):
        codes, scales = sentinels(B, H, TCAP)
        if pos:
            rows = (torch.randn(B, H, pos, 64, generator=g) * scale).to(BF16)
            codes[:, :, :pos], scales[:, :, :pos] = quantize_on_host(rows)
        kv.append((codes, scales))
    before = [kv[0][0], kv[1][0], kv[0][1], kv[1][1]]
    after = [t.clone() for t in before]
    out = torch.full((B * C + SLACK,), OUT_SENTINEL, dtype=BF16, device=dev)
    ws = torch.empty(K.attn_decode_workspace(B, H, TCAP), device=dev)
    K.attn_decode_fp8_ragged(qkv.to(dev), *after, out, ws, B, H, 64, TCAP, [pos] * B)
    torch.cuda.synchronize()
    q, kn, vn = (qkv.view(B, 3, H, 64)[:, i] for i in range(3))
    new = [kv_quantize(kn), kv_quantize(vn)]  # the key / value at pos: the new token's, quantised like the rest
    kc0, vc0, ks0, vs0 = (t.cpu() for t in before)
    keys = torch.cat([kv_dequantize(kc0[:, :, :pos], ks0[:, :, :pos]), kv_dequantize(*new[0])[:, :, None]], dim=2).double()
    vals = torch.cat([kv_dequantize(vc0[:, :, :pos], vs0[:, :, :pos]), kv_dequantize(*new[1])[:, :, None]], dim=2).double()
    att = torch.softmax(torch.einsum("bhd,bhtd->bht", q.double(), keys) / 8.0, dim=-1)
    ref = torch.einsum("bht,bhtd->bhd", att, vals).reshape(B, C).to(dev)
    return out, ref, (q, keys), new, before, after


@pytest.mark.parametrize("B,H", [(1, 2), (3, 5)])
def test_attn_decode_fp8_against_fp64(K, B, H):
    C = 64 * H
    for pos in POSITIONS:
        out, ref, _, new, before, after = _attn_case(K, B, H, pos)
        assert bool(torch.isfinite(out[:B * C].float()).all()), (pos, "a sentinel was read")
        err = rel_err(out[:B * C].view(B, C), ref)
        print(f"attn_decode_fp8 B={B} H={H} pos={pos}: rel_err {err:.3e}")
        assert err < 6e-3, (pos, err)
        assert bool((out[B * C:] == OUT_SENTINEL).all())
        for i in range(2):  # K then V
            c0, s0, c1, s1 = before[i], before[2 + i], after[i], after[2 + i]
            assert torch.equal(c1[:, :, pos], new[i][0].to(dev)), (pos, "the new codes are not kv_quantize's")
            assert torch.equal(bits(s1[:, :, pos]), bits(new[i][1].to(dev))), (pos, "the new scale is not kv_quantize's")
            for lo, hi in ((0, pos), (pos + 1, TCAP)):
                assert torch.equal(c1[:, :, lo:hi], c0[:, :, lo:hi]), (pos, lo, "codes at other positions changed")
                assert torch.equal(bits(s1[:, :, lo:hi]), bits(s0[:, :, lo:hi])), (pos, lo, "scales elsewhere changed")


def test_attn_decode_fp8_large_score_spread(K):
    """As test_attn_decode_large_score_spread: scores q.k/8 spread over +-25, so the key ranges' maxima differ by tens."""
    B, H, pos = 2, 2, 1023
    out, ref, (q, keys), _, _, _ = _attn_case(K, B, H, pos, scale=math.sqrt(10.0), seed=1)
    s = torch.einsum("bhd,bhtd->bht", q.double(), keys) / 8.0
    assert float(s.max()) > 25 and float(s.min()) < -25, (float(s.min()), float(s.max()))
    err = rel_err(out[:B * 64 * H].view(B, 64 * H), ref)
    print(f"attn_decode_fp8 spread [{float(s.min()):.1f}, {float(s.max()):.1f}]: rel_err {err:.3e}")
    assert err < 6e-3, err


def test_attn_decode_fp8_is_reproducible(K):
    for pos in (65, 1023):
        a, b = _attn_case(K, 3, 5, pos), _attn_case(K, 3, 5, pos)
        assert torch.equal(bits(a[0]), bits(b[0])), pos
        for x, y in zip(a[5], b[5]):
            assert torch.equal(bits(x), bits(y)), pos


# ---- attn_extend_fp8 -------------------------------------------------------------------------------------------------
def test_attn_extend_fp8_has_the_bits_of_one_position_at_a_time(K):
    """Runs of 1, 3 and 5 rows in three sequences at unequal positions: one row in a partly filled range, a run from an
    empty stream, a run across the 32-key range edge. Each stream holds quantised rows below its run and sentinels from
    there on, so a key of the call read from the cache (another wave is writing it) would show."""
    B, H, Tcap, C = 3, 2, 70, 128
    seq, pos = [0, 1, 1, 1, 2, 2, 2, 2, 2], [40, 0, 1, 2, 29, 30, 31, 32, 33]
    first = {0: 40, 1: 0, 2: 29}
    R = len(seq)
    g = torch.Generator().manual_seed(47)
    qkv = torch.randn(R, 3 * C, generator=g).to(BF16).to(dev)
    kv = []
    for _ in range(2):
        codes, scales = sentinels(B, H, Tcap)
        for b, n in first.items():
            if n:
                codes[b, :, :n], scales[b, :, :n] = quantize_on_host(torch.randn(H, n, 64, generator=g).to(BF16))
        kv.append((codes, scales))
    start = [kv[0][0], kv[1][0], kv[0][1], kv[1][1]]  # kcodes, vcodes, kscales, vscales: the entries' order

    ext = [t.clone() for t in start]
    out = torch.full((R, C), OUT_SENTINEL, dtype=BF16, device=dev)
    ws = torch.empty(K.attn_decode_workspace(R, H, Tcap), device=dev)
    K.attn_extend_fp8(qkv, *ext, out, ws, R, B, H, 64, Tcap, seq, pos)

    one = [t.clone() for t in start]
    want = torch.full((R, C), OUT_SENTINEL, dtype=BF16, device=dev)
    ws1 = torch.empty(K.attn_decode_workspace(1, H, Tcap), device=dev)
    for r in range(R):  # one position per call, on the row's own sequence
        K.attn_decode_fp8_ragged(qkv[r:r + 1], *(t[seq[r]:seq[r] + 1] for t in one), want[r:r + 1], ws1, 1, H, 64, Tcap,
                                 [pos[r]])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all()) and bool(torch.isfinite(out.float()).all())
    assert torch.equal(bits(out), bits(want))
    for a, b in zip(ext, one):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(ext[0], start[0])  # (the calls did write)
    for b, n in first.items():  # and only their own positions: what lies above a run's last row is still the sentinel
        last = max(p for s, p in zip(seq, pos) if s == b)
        assert bool((ext[0][b, :, last + 1:] == CODE_SENTINEL).all()) and bool(ext[2][b, :, last + 1:].isnan().all())
        assert torch.equal(ext[0][b, :, :n], start[0][b, :, :n])
