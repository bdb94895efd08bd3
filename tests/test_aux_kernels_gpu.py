"""The bandwidth kernels around the step (csrc/aux_ops.hip, the AdamW / norm / cast kernels of csrc/xent_adamw.hip, the
single-matrix transpose of csrc/transpose.hip) against fp64 or bitwise references, at single-element and odd sizes, at
second trips of the grid-stride loops and with every option of the entries. Comparison rules and helpers: see
tests/test_row_kernels_gpu.py."""
import math

import numpy as np
import pytest
import torch

from tests.test_decode_kernels_gpu import BF16, bits
from tests.test_kernels_gpu import rel_err
from tests.test_row_kernels_gpu import (SLACK, U, bf16_ulp_bound, check_elements, dropout_f32, sentinel, sum_bound,
                                        untouched)

pytestmark = pytest.mark.gpu

dev = "cuda"


@pytest.fixture(scope="module", autouse=True)
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


def padded(vals, dtype=None):
    """vals on the device with SLACK sentinel elements behind them; returns (whole buffer, n)."""
    vals = vals.reshape(-1)
    buf = sentinel(vals.numel() + SLACK, dtype or vals.dtype)
    buf[:vals.numel()] = vals.to(dev)
    return buf, vals.numel()


# ---- AdamW and the gradient norm ------------------------------------------------------------------------------------
HYPER = dict(lr=1e-3, wd=0.1, b1=0.9, b2=0.95, eps=1e-8)
ADAMW_BIG = 2048 * 256 * 8 + 12  # one element group past a full trip of 2048 x 256 threads x 8, and the odd-group tail


def adamw_ref64(p, g, m, v, step, grad_scale, lr, wd, b1, b2, eps):
    """The kernel's update (torch/optim/adam.py's decoupled decay) in fp64, hyper-parameters as fp32 passes them."""
    lr, wd, b1, b2, eps, grad_scale = (float(np.float32(t)) for t in (lr, wd, b1, b2, eps, grad_scale))
    gg = g * grad_scale
    m = m + (1 - b1) * (gg - m)
    v = b2 * v + (1 - b2) * gg * gg
    step_size, bc2_sqrt = lr / (1 - b1 ** step), math.sqrt(1 - b2 ** step)
    return p * (1 - lr * wd) - step_size * m / (v.sqrt() / bc2_sqrt + eps), m, v


@pytest.mark.parametrize("with_shadow", [True, False], ids=["p_bf16", "no_p_bf16"])
@pytest.mark.parametrize("n", [4, 8, 12, ADAMW_BIG])
def test_adamw_sizes_and_state(K, n, with_shadow):
    """n = 4: the odd-group tail alone; 8: one thread of the main loop; 12: both; ADAMW_BIG: a second trip of the loop.
    Three steps from non-zero moments with grad_scale = 0.5; m and v held to p's bound."""
    gen = torch.Generator().manual_seed(n)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.01
    m0, v0 = torch.randn(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 1e-4 + 1e-6
    (p, _), (g, _), (m, _), (v, _) = (padded(t) for t in (p0, g0, m0, v0))
    pb = sentinel(n + SLACK, BF16) if with_shadow else None
    part = sentinel(K.norm_partials_size() + SLACK)
    gn = sentinel(1 + SLACK)
    ref = (p0.double(), m0.double(), v0.double())
    for step in (1, 2, 3):
        ref = adamw_ref64(ref[0], g0.double(), ref[1], ref[2], step, 0.5, **HYPER)
        K.adamw(p, g, m, v, pb, n, HYPER["lr"], HYPER["wd"], HYPER["b1"], HYPER["b2"], HYPER["eps"], step, 0.5, part,
                gn)
    torch.cuda.synchronize()
    errs = [rel_err(t[:n].cpu(), r) for t, r in zip((p, m, v), ref)]
    print(f"adamw n={n} shadow={with_shadow}: rel_err p {errs[0]:.3e} m {errs[1]:.3e} v {errs[2]:.3e}")
    assert all(e < 1e-6 for e in errs), errs
    # per element too (one element the loop skipped moves the norm ratio of 4 M elements by less than 1e-6): a step
    # rounds at most 8 times, each on a quantity no larger than |state| + |what the step adds| (for p at most
    # step_size x m / sqrt(v) < 0.01): 3 steps x 8 roundings x 2^-24, taken as 32 x 2^-24 of that scale
    gg = (g0.double() * 0.5).abs()
    scales = (p0.double().abs() + 0.01, m0.double().abs() + gg, v0.double() + gg * gg)
    for name, t, r, scale in zip("pmv", (p, m, v), ref, scales):
        check_elements(name, t[:n], r, 32 * U * scale)
    if with_shadow:
        assert torch.equal(bits(pb[:n]), bits(p[:n].to(BF16))), "p_bf16 is not the rounding of p"
        assert untouched(pb[n:])
    assert torch.equal(bits(g[:n].cpu()), bits(g0)), "the gradient changed"
    assert all(untouched(t[n:]) for t in (p, g, m, v)), "wrote past n"
    want = float((g0.double() * 0.5).norm())
    assert abs(float(gn[0]) - want) <= 1e-5 * want, (float(gn[0]), want)
    assert untouched(gn[1:]) and untouched(part[K.norm_partials_size():])


def test_grad_norm_and_partials_second_trip(K):
    n = ADAMW_BIG
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(5)) * 0.01
    g, _ = padded(g0)
    P = K.norm_partials_size()
    want = float((g0.double() * 0.5).norm())
    part, out = sentinel(P + SLACK), sentinel(1 + SLACK)
    K.grad_norm(g, n, 0.5, part, out)
    torch.cuda.synchronize()
    got = float(out[0])
    print(f"grad_norm n={n}: rel err {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-5 * want
    part2, out2 = sentinel(P + SLACK), sentinel(1 + SLACK)
    K.sumsq_partials(g, n, 0.5, part2)
    K.norm_finalize(part2, P, out2)
    torch.cuda.synchronize()
    assert abs(math.sqrt(float(part2[:P].double().sum())) - want) <= 1e-5 * want
    assert torch.equal(bits(part2), bits(part)) and torch.equal(bits(out2), bits(out))
    assert untouched(part[P:]) and untouched(out[1:])
    # n = 4: one thread holds the whole sum
    K.grad_norm(g, 4, 0.5, part, out)
    torch.cuda.synchronize()
    want4 = float((g0[:4].double() * 0.5).norm())
    assert abs(float(out[0]) - want4) <= 1e-5 * want4


def test_adamw_and_norms_refuse_n_not_multiple_of_4(K):
    n = 6
    bufs = [sentinel(8) for _ in range(4)]
    pb, part, gn = sentinel(8, BF16), sentinel(K.norm_partials_size()), sentinel(1)
    with pytest.raises(K.KernelError):
        K.adamw(*bufs, pb, n, 1e-3, 0.1, 0.9, 0.95, 1e-8, 1, 1.0, part, gn)
    with pytest.raises(K.KernelError):
        K.grad_norm(bufs[1], n, 1.0, part, gn)
    with pytest.raises(K.KernelError):
        K.sumsq_partials(bufs[1], n, 1.0, part)
    torch.cuda.synchronize()
    assert all(untouched(t) for t in (*bufs, pb, part, gn))


# ---- dlogits_accum --------------------------------------------------------------------------------------------------
DLA_CASES = [(2, 8, 5, 509, 512, 509), (1, 4, 4, 130, 136, 130), (3, 6, 1, 700, 768, 704)]


def _dla_inputs(B, Tp, Tv, V, ldd, ldg, dtype):
    gen = torch.Generator().manual_seed(B + Tp + V)
    g = torch.full((B * Tv, ldg), math.nan)  # columns [V, ldg) are not part of the gradient: poison
    g[:, :V] = torch.randn(B * Tv, V, generator=gen)
    dl0 = torch.randn(B * Tp, ldd, generator=gen)
    valid = (torch.arange(B * Tp) % Tp) < Tv
    return g.to(dtype), dl0.to(dtype), valid


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,Tp,Tv,V,ldd,ldg", DLA_CASES)
def test_dlogits_accum_init(K, B, Tp, Tv, V, ldd, ldg, dtype):
    g, _, valid = _dla_inputs(B, Tp, Tv, V, ldd, ldg, dtype)
    dl = sentinel(B * Tp * ldd + SLACK, dtype)
    dl[:B * Tp * ldd] = math.nan  # init: dl is written, not read
    K.dlogits_accum(dl, ldd, g.to(dev), ldg, B, Tp, Tv, V, init=True)
    torch.cuda.synchronize()
    rows = dl[:B * Tp * ldd].view(B * Tp, ldd).cpu()
    assert torch.equal(bits(rows[valid][:, :V]), bits(g[:, :V].contiguous())), "valid rows != g"
    assert bool((bits(rows[valid][:, V:]) == 0).all()), "padding columns are not +0"
    assert bool((bits(rows[~valid]) == 0).all()), "padding rows are not +0"
    assert untouched(dl[B * Tp * ldd:])


@pytest.mark.parametrize("alpha", [None, 0.5])
@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,Tp,Tv,V,ldd,ldg", DLA_CASES)
def test_dlogits_accum_scaled_sum(K, B, Tp, Tv, V, ldd, ldg, dtype, alpha):
    """dl = alpha dl + g, where the compiler may or may not fuse the multiply-add: fp32 within 2^-23 (|alpha dl| + |g|)
    of the fp64 value (one rounding each of product and sum, at most), bf16 within one bf16 ulp."""
    g, dl0, valid = _dla_inputs(B, Tp, Tv, V, ldd, ldg, dtype)
    dl, n = padded(dl0)
    a_dev = None if alpha is None else torch.tensor([alpha], device=dev)
    K.dlogits_accum(dl, ldd, g.to(dev), ldg, B, Tp, Tv, V, alpha_dev=a_dev)
    torch.cuda.synchronize()
    rows = dl[:n].view(B * Tp, ldd).cpu()
    a = 1.0 if alpha is None else alpha
    prod, add = a * dl0[valid][:, :V].double(), g[:, :V].double()
    ref = prod + add
    bound = bf16_ulp_bound(ref) if dtype == BF16 else 2.0 ** -23 * (prod.abs() + add.abs())
    worst = check_elements("dl", rows[valid][:, :V], ref, bound)
    print(f"dlogits_accum {dtype} alpha={alpha} V={V}: err/bound {worst:.3f}")
    assert bool((bits(rows[valid][:, V:]) == 0).all()), "padding columns of valid rows are not +0"
    assert torch.equal(bits(rows[~valid]), bits(dl0[~valid])), "padding rows changed"
    assert untouched(dl[n:])


def test_dlogits_accum_refusals(K):
    dl, g = sentinel(4 * 16, BF16), torch.zeros(4, 16, device=dev)
    with pytest.raises(K.KernelError):
        K.dlogits_accum(dl, 16, g, 16, 1, 4, 4, 16)  # bf16 dlogits, fp32 gradient
    with pytest.raises(K.KernelError):
        K.dlogits_accum(sentinel(4 * 16), 16, g.to(BF16), 16, 1, 4, 4, 16)
    for d in (dl, sentinel(4 * 16)):
        with pytest.raises(K.KernelError):
            K.dlogits_accum(d, 16, g.to(d.dtype), 16, 1, 3, 4, 16)  # Tv > Tp
    torch.cuda.synchronize()
    assert untouched(dl)


# ---- branch_bwd -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,C", [(5, 68), (37, 768), (300, 1600), (1000, 260)])
def test_branch_bwd(K, M, C, dtype, p):
    """C = 68, 260: a part-filled column block; M = 5, 37: part-filled row groups; M = 300, 1000: several row blocks."""
    seed = 0x5EED_0000_0042 + M
    dres = torch.randn(M, C, generator=torch.Generator().manual_seed(M + C))
    want = dropout_f32(dres, seed, p).to(dtype)
    stored = want.double()
    ref = 1.0 + stored.sum(0)
    for with_dbias in (True, False):
        out = sentinel(M * C + SLACK, dtype)
        dbias = sentinel(C + SLACK) if with_dbias else None
        if with_dbias:
            dbias[:C] = 1.0
        K.branch_bwd(dres.to(dev), out, dbias, M, C, p, seed)
        torch.cuda.synchronize()
        assert torch.equal(bits(out[:M * C].view(M, C).cpu()), bits(want)), ("out", with_dbias)
        assert untouched(out[M * C:])
        if with_dbias:
            worst = check_elements("dbias", dbias[:C], ref, sum_bound(M + 1, 1.0 + stored.abs().sum(0), ref))
            assert untouched(dbias[C:])
            print(f"branch_bwd {dtype} M={M} C={C} p={p}: dbias err/bound {worst:.3f}")


def test_branch_bwd_refuses_c_not_multiple_of_4(K):
    for dtype in (BF16, torch.float32):
        out, dbias = sentinel(5 * 66, dtype), sentinel(66)
        with pytest.raises(K.KernelError):
            K.branch_bwd(torch.zeros(5, 66, device=dev), out, dbias, 5, 66)
        torch.cuda.synchronize()
        assert untouched(out) and untouched(dbias)


# ---- casts, scale, transpose -----------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
# +-0, +-inf, NaN, exact ties towards the even neighbour below (1 + 2^-8 -> 1) and above (1 + 3 2^-8 -> 1 + 2^-6), the
# largest finite fp32 (rounds to inf), and values just off a tie. No subnormals: those are the hardware mode's business
SPECIALS = [0.0, -0.0, math.inf, -math.inf, math.nan, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, FLT_MAX, -FLT_MAX,
            1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, -(1 + 2.0 ** -8), 2.0 ** -126]


def _same_or_both_nan(got, want):
    nan = torch.isnan(want.float())
    return bool(torch.equal(torch.isnan(got.float()), nan)) and torch.equal(bits(got[~nan]), bits(want[~nan]))


@pytest.mark.parametrize("n", [1, 7, 2048 * 256 + 3])
def test_cast_f32_bf16(K, n):
    """Bitwise torch's round-to-nearest-even. n = 1 and 7 walk every window of the special values; the large n puts
    them in front of random data and takes the grid-stride loop into a second, part-filled trip."""
    sp = torch.tensor(SPECIALS, dtype=torch.float32)
    if n <= 7:
        inputs = [torch.roll(sp, -s)[:n].clone() for s in range(len(SPECIALS))]
    else:
        x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3
        x[:len(SPECIALS)] = sp
        x[-1] = 1 + 3 * 2.0 ** -8
        inputs = [x]
    for x in inputs:
        y = sentinel(n + SLACK, BF16)
        K.cast_f32_bf16(x.to(dev), y, n)
        torch.cuda.synchronize()
        assert _same_or_both_nan(y[:n].cpu(), x.to(BF16)), x[:8]
        assert untouched(y[n:])


def test_cast_bf16_f32(K):
    n = 4096 * 256 + 3
    x = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 100).to(BF16)
    x[:len(SPECIALS)] = torch.tensor(SPECIALS, dtype=torch.float32).to(BF16)
    x[-1] = -3.0
    y = sentinel(n + SLACK)
    K.cast_bf16_f32(x.to(dev), y, n)
    torch.cuda.synchronize()
    assert _same_or_both_nan(y[:n].cpu(), x.float())
    assert untouched(y[n:])


@pytest.mark.parametrize("s", [0.125, 1.0 / 3.0])
@pytest.mark.parametrize("n", [4, 4096 * 256 * 4 + 4])
def test_scale_f32(K, n, s):
    x0 = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 7
    buf, _ = padded(x0)
    K.scale_(buf[:n], s)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf[:n].cpu()), bits(x0 * torch.tensor(s, dtype=torch.float32)))
    assert untouched(buf[n:])


def test_scale_f32_refuses_n_not_multiple_of_4(K):
    buf = sentinel(8)
    with pytest.raises(K.KernelError):
        K.scale_(buf[:6], 0.5)
    torch.cuda.synchronize()
    assert untouched(buf)


def test_scale_mul(K):
    a0, b0 = torch.tensor(1.0 / 3.0), torch.tensor(-7.3)
    buf = sentinel(12)
    buf[4], buf[8] = a0, b0
    K.scale_mul(buf[4:], buf[8:], buf[0:])
    torch.cuda.synchronize()
    want = sentinel(12, device="cpu")
    want[0], want[4], want[8] = a0 * b0, a0, b0
    assert torch.equal(bits(buf.cpu()), bits(want))


@pytest.mark.parametrize("R,C,ld_src,ld_dst", [(64, 64, 64, 64), (192, 64, 64, 192), (128, 192, 200, 136)])
def test_transpose_bf16(K, R, C, ld_src, ld_dst):
    src = sentinel(R * ld_src + SLACK, BF16, device="cpu")
    src[:R * ld_src].view(R, ld_src)[:, :C] = torch.randn(R, C, generator=torch.Generator().manual_seed(R + C)).to(BF16)
    s = src.to(dev)
    dst = sentinel(C * ld_dst + SLACK, BF16)
    K.transpose_bf16(s, dst, R, C, ld_src, ld_dst)
    torch.cuda.synchronize()
    want = sentinel(C * ld_dst + SLACK, BF16, device="cpu")
    want[:C * ld_dst].view(C, ld_dst)[:, :R] = src[:R * ld_src].view(R, ld_src)[:, :C].t()
    assert torch.equal(bits(dst.cpu()), bits(want)), "transpose, or the padding of dst changed"
    assert torch.equal(bits(s.cpu()), bits(src)), "src changed"


def test_transpose_bf16_refuses_partial_tiles(K):
    src, dst = torch.zeros(96 * 64, dtype=BF16, device=dev), sentinel(96 * 64, BF16)
    with pytest.raises(K.KernelError):
        K.transpose_bf16(src, dst, 96, 64)
    with pytest.raises(K.KernelError):
        K.transpose_bf16(src, dst, 64, 64, ld_src=68)
    torch.cuda.synchronize()
    assert untouched(dst)
