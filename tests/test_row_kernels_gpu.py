"""The row kernels (csrc/norm_embed.hip: LayerNorm, embedding, column sums; csrc/xent_adamw.hip: cross entropy) against
fp64 references of the same operations on the same rounded inputs, at every instantiated width, at part-filled blocks,
at second trips of the grid-stride loops and with every option of the entries.

How results are compared (per element; a norm ratio hides one wrong row or column):
  * a sum of n fp32 addends in any order (db, dbias, dwte, dwpe, column sums, dw's reduction, mean): sum_bound();
  * one rounded fp32 operation on the kernel's own inputs (dropout scaling, embedding sum, bf16 rounding): bitwise
    against the same operation in torch fp32 on the CPU;
  * LayerNorm y, dres, rstd and dw's xhat part, for which no bound exists without fixing an order of operations: at most
    LN_YARDSTICK_FACTOR times the maximum absolute error of torch's own fp32 CPU layer_norm (forward and autograd)
    against the same fp64 reference;
  * cross entropy: the project's figure for the mean loss, 1e-5 max(1, |ref|), per row; dlogits by rel_err as
    tests/test_kernels_gpu.py holds it, and the label column as one element.
What a kernel must not read is poisoned (NaN table rows, NaN padding columns), what it must not write is sentinel-filled
and compared bitwise: a wrong guard shows as a failed comparison."""
import math

import numpy as np
import pytest
import torch

from oracle import dropout_ref
from tests.test_decode_kernels_gpu import BF16, F32_SENTINEL, bits
from tests.test_kernels_gpu import rel_err

pytestmark = pytest.mark.gpu

dev = "cuda"
U = 2.0 ** -24  # unit roundoff of fp32
SLACK = 256
EPS = float(np.float32(1e-5))  # LayerNorm's eps as the C entry receives it


@pytest.fixture(scope="module", autouse=True)
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


# ---- helpers shared with tests/test_aux_kernels_gpu.py (checked on the CPU by tests/test_row_refs_cpu.py) -----------
def sentinel(n, dtype=torch.float32, device=dev):
    """n elements of F32_SENTINEL (fp32 / bf16 / int64 -1): output buffers and the slack behind them."""
    if dtype == torch.int64:
        return torch.full((n,), -1, dtype=dtype, device=device)
    return torch.full((n,), F32_SENTINEL, dtype=dtype, device=device)


def untouched(t):
    return bool((t == F32_SENTINEL).all())


def sum_bound(n, abs_sum, ref):
    """|fp32 sum of n addends in any order - exact sum| <= (n - 1) 2^-24 sum|addend|, plus one rounding of the result
    (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, to first order)."""
    return (n - 1) * U * abs_sum + U * ref.abs()


def inv_keep(p):
    """1 / (1 - p) as the host code forms it, a torch fp32 scalar."""
    one = torch.tensor(1.0, dtype=torch.float32)
    return one / (one - torch.tensor(p, dtype=torch.float32)) if p > 0 else one


def keep_mask(seed, rows, cols, p):
    if p <= 0:
        return torch.ones(rows, cols, dtype=torch.bool)
    return dropout_ref.site_scale(seed, rows, cols, p) != 0


def dropout_f32(x, seed, p):
    """keep ? x * inv_keep : 0 in torch fp32 on the CPU: the bits every dropout site of these kernels stores."""
    if p <= 0:
        return x.clone()
    return torch.where(keep_mask(seed, x.shape[0], x.shape[1], p), x * inv_keep(p), torch.zeros_like(x))


def bf16_ulp_bound(ref):
    """One bf16 ulp as a relative figure, 2^-8 |ref|: between half an ulp and one ulp of ref's binade, so the correct
    rounding of ref always passes and a value two representable steps away never does."""
    return 2.0 ** -8 * ref.abs()


def f32_ulp(ref):
    """The spacing of fp32 numbers at |ref| (fp64 tensor in, normal range)."""
    return torch.exp2(torch.floor(torch.log2(ref.abs())) - 23)


def check_elements(name, out, ref, bound):
    """Every element of out (any dtype) within its own bound of the fp64 ref; returns the largest error / bound."""
    err = (out.double().cpu() - ref).abs()
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    bad = ~(err <= bound)  # (a NaN error is bad)
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert not bool(bad.any()), (name, "first bad element", bad.nonzero()[0].tolist(), "max err", float(err.max()),
                                 "err / bound", worst)
    return worst


def ln_ref64(x, w, b, eps=EPS):
    """fp64 LayerNorm of fp64 x [M, C] (biased variance): y, mean, rstd, xhat."""
    mu = x.mean(1, keepdim=True)
    rstd = (((x - mu) ** 2).mean(1, keepdim=True) + eps).rsqrt()
    xhat = (x - mu) * rstd
    return xhat * w + b, mu[:, 0], rstd[:, 0], xhat


def ln_bwd_ref64(xhat, rstd, w, dy):
    """Closed-form fp64 LayerNorm backward: dx, and the addends of dw and db (their column sums are the gradients)."""
    gw = dy * w
    dx = rstd[:, None] * (gw - gw.mean(1, keepdim=True) - xhat * (gw * xhat).mean(1, keepdim=True))
    return dx, dy * xhat, dy


def xent_ref64(logits, labels, V, ignore_index):
    """fp64 cross entropy over the first V columns of `logits`: lse, loss_rows (0 where ignored, NaN where the label is
    outside [0, V)), dlogits = softmax - onehot (0 rows where ignored, NaN rows for a bad label), mean loss, count."""
    z = logits[:, :V].double()
    lse = torch.logsumexp(z, dim=1)
    ign = labels == ignore_index
    bad = ~ign & ((labels < 0) | (labels >= V))
    safe = labels.clamp(0, V - 1)
    rows = lse - z.gather(1, safe[:, None])[:, 0]
    rows = torch.where(ign, torch.zeros_like(rows), torch.where(bad, torch.full_like(rows, math.nan), rows))
    d = torch.exp(z - lse[:, None])
    d[torch.arange(len(labels)), safe] -= 1.0
    d[ign] = 0.0
    d[bad] = math.nan
    count = int((~ign).sum())
    return lse, rows, d, (rows.sum() / count if count else torch.tensor(math.nan, dtype=torch.float64)), count


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
# every (VEC, NV) instantiation of GPT2MI_ROW_CASES: VEC 1 (C % 128 != 0), VEC 2 (C % 256 == 128), VEC 4
LN_WIDTHS = [64, 192, 1600, 128, 384, 640, 896, 256, 512, 768, 1024, 1280, 1536, 1792, 2048]
FAMILIES = ("spread", "offset")  # 2 randn + 0.5; 100 + 0.1 randn (a one-pass E[x^2] - E[x]^2 variance fails this one)
# The kernel's maximum absolute error may be this many times torch's own fp32 CPU error against the same fp64
# reference, per output tensor. The margin is for summation order (a wave tree against torch's vectorised loop).
# Observed on the MI355X (every case prints its own figures), kernel error / yardstick, largest ratio over all cases:
#   y     1.71  (M = 1, C = 128, spread: 3.5e-7 / 2.1e-7); offset family at M = 37: 0.5 .. 1.6 (C = 1600: 1.5e-4 / 9.4e-5)
#   rstd  1.75  (M = 1, C = 128, offset: 6.1e-7 / 3.5e-7), which is 0.17 of the bound once the 4 ulp floor applies
#   dres  1.11  (M = 37, C = 512, spread: 3.4e-7 / 3.1e-7); offset family 0.07 .. 0.8
#   dw    2.70  (M = 4099, C = 768, spread: 1.9e-4 / 7.1e-5; the summation bound is the larger there); M = 37: <= 1.6
# mean stays below 0.03 of its summation bound, db and dbias_out below 0.5 of theirs (0.5 is one rounding at M = 1).
# Per width at M = 37, offset family (100 + 0.1 randn), kernel error / yardstick (the spread family: y 3.3e-7 .. 6.2e-7
# against 4.3e-7 .. 8.3e-7, dres 2.2e-7 .. 4.0e-7 against 3.0e-7 .. 5.7e-7):
#      C   y                 rstd              dres              dw
#     64   9.4e-5 / 1.2e-4   9.7e-7 / 1.1e-6   3.8e-4 / 1.1e-3   6.1e-4 / 1.1e-3
#    192   1.6e-4 / 1.9e-4   1.0e-6 / 1.2e-6   4.3e-4 / 9.5e-4   9.7e-4 / 8.4e-4
#   1600   1.5e-4 / 9.4e-5   8.6e-7 / 9.6e-7   2.3e-4 / 9.7e-4   1.1e-3 / 8.1e-4
#    128   8.9e-5 / 1.3e-4   9.3e-7 / 7.9e-7   5.3e-4 / 6.9e-4   5.2e-4 / 7.3e-4
#    384   1.4e-4 / 1.4e-4   9.4e-7 / 7.9e-7   3.7e-4 / 7.2e-4   8.9e-4 / 9.1e-4
#    640   1.1e-4 / 1.3e-4   9.0e-7 / 9.4e-7   1.9e-4 / 8.0e-4   9.6e-4 / 1.1e-3
#    896   1.1e-4 / 1.7e-4   8.9e-7 / 9.0e-7   7.8e-5 / 6.2e-4   7.9e-4 / 7.7e-4
#    256   6.2e-5 / 1.3e-4   8.2e-7 / 8.7e-7   1.2e-4 / 9.5e-4   3.4e-4 / 7.6e-4
#    512   1.0e-4 / 1.4e-4   8.2e-7 / 9.1e-7   1.9e-4 / 1.0e-3   1.0e-3 / 1.0e-3
#    768   1.3e-4 / 1.2e-4   6.6e-7 / 5.3e-7   3.8e-4 / 7.4e-4   1.0e-3 / 9.0e-4
#   1024   1.3e-4 / 1.1e-4   9.2e-7 / 7.8e-7   1.9e-4 / 5.6e-4   7.7e-4 / 8.9e-4
#   1280   1.1e-4 / 1.6e-4   5.4e-7 / 1.1e-6   1.2e-4 / 1.0e-3   8.4e-4 / 1.0e-3
#   1536   1.3e-4 / 1.3e-4   7.4e-7 / 1.1e-6   1.6e-4 / 7.1e-4   1.3e-3 / 9.6e-4
#   1792   1.0e-4 / 1.4e-4   9.0e-7 / 1.0e-6   1.1e-4 / 9.3e-4   7.6e-4 / 1.0e-3
#   2048   9.4e-5 / 1.4e-4   7.0e-7 / 1.0e-6   9.4e-5 / 1.3e-3   5.6e-4 / 1.0e-3
LN_YARDSTICK_FACTOR = 8.0


def _ln_inputs(M, C, family, seed=0, f32_dy=False):
    g = torch.Generator().manual_seed(1000 * seed + 7 * M + C + (1 if family == "offset" else 0))
    r = torch.randn(M, C, generator=g)
    x = r * 2 + 0.5 if family == "spread" else r * 0.1 + 100
    w = torch.randn(C, generator=g) * 0.1 + 1
    b = torch.randn(C, generator=g) * 0.1
    dy = torch.randn(M, C, generator=g)
    dy = dy if f32_dy else dy.to(BF16)
    dres0 = torch.randn(M, C, generator=g)
    return x, w, b, dy, dres0


_ln_cache = {}


def _ln_case(M, C, family, f32_dy=False):
    """Inputs, the fp64 reference and the yardstick (torch's fp32 CPU errors) of one case, computed once."""
    key = (M, C, family, f32_dy)
    if key in _ln_cache:
        return _ln_cache[key]
    x, w, b, dy, dres0 = _ln_inputs(M, C, family, f32_dy=f32_dy)
    y64, mu64, rstd64, xhat64 = ln_ref64(x.double(), w.double(), b.double())
    dx64, dw_add, db_add = ln_bwd_ref64(xhat64, rstd64, w.double(), dy.double())
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yt = torch.nn.functional.layer_norm(xr, (C,), wr, br, EPS)
    yt.backward(dy.float())
    rstd_t = torch.rsqrt(x.var(1, unbiased=False) + EPS)
    yard = {"y": float((yt.detach().double() - y64).abs().max()),
            "rstd": float((rstd_t.double() - rstd64).abs().max()),
            "dres": float(((dres0 + xr.grad).double() - (dres0.double() + dx64)).abs().max()),
            "dw": float((wr.grad.double() - dw_add.sum(0)).abs().max())}
    case = dict(x=x, w=w, b=b, dy=dy, dres0=dres0, y=y64, mean=mu64, rstd=rstd64, dres=dres0.double() + dx64, dx=dx64,
                dw_add=dw_add, db_add=db_add, yard=yard, M=M, C=C, family=family)
    _ln_cache[key] = case
    return case


def _ln_forward(K, c, want_bf16=True, want_f32=True):
    M, C = c["M"], c["C"]
    yb = sentinel(M * C + SLACK, BF16) if want_bf16 else None
    yf = sentinel(M * C + SLACK) if want_f32 else None
    mean, rstd = sentinel(M + SLACK), sentinel(M + SLACK)
    K.layernorm_fwd(c["x"].to(dev), c["w"].to(dev), c["b"].to(dev), yb, yf, mean, rstd, M, C, EPS)
    torch.cuda.synchronize()
    return yb, yf, mean, rstd


def _check_ln_forward(c, yb, yf, mean, rstd, tag):
    M, C, yard = c["M"], c["C"], c["yard"]
    F = LN_YARDSTICK_FACTOR
    x64 = c["x"].double()
    r = {}
    if yf is not None:
        r["y"] = check_elements("y_f32", yf[:M * C].view(M, C), c["y"], F * yard["y"])
        assert untouched(yf[M * C:]), "y_f32 written past M*C"
    if yb is not None:
        assert untouched(yb[M * C:]), "y_bf16 written past M*C"
    if yb is not None and yf is not None:
        assert torch.equal(bits(yb[:M * C]), bits(yf[:M * C].to(BF16))), "y_bf16 is not the rounding of y_f32"
    r["mean"] = check_elements("mean", mean[:M], c["mean"],
                               (C - 1) * U * x64.abs().sum(1) / C + U * c["mean"].abs())
    rstd_floor = 4 * f32_ulp(c["rstd"])
    r["rstd"] = check_elements("rstd", rstd[:M], c["rstd"], torch.clamp_min(rstd_floor, F * yard["rstd"]))
    assert untouched(mean[M:]) and untouched(rstd[M:]), "mean / rstd written past M"
    err_y = float((yf[:M * C].view(M, C).double().cpu() - c["y"]).abs().max()) if yf is not None else math.nan
    err_r = float((rstd[:M].double().cpu() - c["rstd"]).abs().max())
    print(f"ln_fwd {tag} M={M} C={C} {c['family']}: y err {err_y:.3e} yardstick {yard['y']:.3e}; rstd err {err_r:.3e} "
          f"yardstick {yard['rstd']:.3e} (4 ulp {float(rstd_floor.max()):.3e}); mean err/bound {r['mean']:.3f}")
    return r


def _ln_backward(K, c, mean, rstd, p_out=0.0, seed_out=0, dres_init=False, want_dw=True, want_out=True, dres_fill=None):
    """Launch on dres = dres0 (or dres_fill), with dw / db / dbias_out pre-filled by _ln_prefill; returns the buffers."""
    M, C = c["M"], c["C"]
    dy = c["dy"].to(dev)
    dres = sentinel(M * C + SLACK)
    dres[:M * C] = (c["dres0"] if dres_fill is None else dres_fill).to(dev).reshape(-1)
    pre = _ln_prefill(C)
    dw, db, dbo = (sentinel(C + SLACK) for _ in range(3))
    for t, v in zip((dw, db, dbo), pre):
        t[:C] = v.to(dev)
    out = sentinel(M * C + SLACK, dy.dtype)
    if not want_dw:
        dw = db = None
    if not want_out:
        out = dbo = None
    K.layernorm_bwd(c["x"].to(dev), c["w"].to(dev), mean, rstd, dy, dres, dw, db, out, dbo, M, C, p_out, seed_out,
                    dres_init)
    torch.cuda.synchronize()
    return dres, dw, db, out, dbo


def _ln_prefill(C):
    g = torch.Generator().manual_seed(C)
    return [torch.randn(C, generator=g) + 3.0 for _ in range(3)]  # non-zero: the entries accumulate (+=)


def _check_ln_backward(c, bufs, tag, p_out=0.0, seed_out=0, dres_ref=None):
    M, C, yard = c["M"], c["C"], c["yard"]
    F = LN_YARDSTICK_FACTOR
    dres, dw, db, out, dbo = bufs
    pre = _ln_prefill(C)
    dres_ref = c["dres"] if dres_ref is None else dres_ref
    r = {"dres": check_elements("dres", dres[:M * C].view(M, C), dres_ref, F * yard["dres"])}
    assert untouched(dres[M * C:]), "dres written past M*C"
    err_dw = math.nan
    if dw is not None:
        ref_dw = pre[0].double() + c["dw_add"].sum(0)
        bound = sum_bound(M + 1, pre[0].double().abs() + c["dw_add"].abs().sum(0), ref_dw)
        r["dw"] = check_elements("dw", dw[:C], ref_dw, torch.clamp_min(bound, F * yard["dw"]))
        err_dw = float((dw[:C].double().cpu() - ref_dw).abs().max())
        ref_db = pre[1].double() + c["db_add"].sum(0)
        r["db"] = check_elements("db", db[:C], ref_db,
                                 sum_bound(M + 1, pre[1].double().abs() + c["db_add"].abs().sum(0), ref_db))
        assert untouched(dw[C:]) and untouched(db[C:]), "dw / db written past C"
    if out is not None:
        mine = dres[:M * C].view(M, C).cpu()  # the kernel's own residual gradient
        want = dropout_f32(mine, seed_out, p_out).to(out.dtype)
        assert torch.equal(bits(out[:M * C].view(M, C).cpu()), bits(want)), "out is not the mask applied to dres"
        assert untouched(out[M * C:]), "out written past M*C"
        stored = out[:M * C].view(M, C).double().cpu()
        ref_dbo = pre[2].double() + stored.sum(0)
        r["dbias_out"] = check_elements("dbias_out", dbo[:C], ref_dbo,
                                        sum_bound(M + 1, pre[2].double().abs() + stored.abs().sum(0), ref_dbo))
        assert untouched(dbo[C:]), "dbias_out written past C"
    err_d = float((dres[:M * C].view(M, C).double().cpu() - dres_ref).abs().max())
    print(f"ln_bwd {tag} M={M} C={C} {c['family']}: dres err {err_d:.3e} yardstick {yard['dres']:.3e}; dw err "
          f"{err_dw:.3e} yardstick {yard['dw']:.3e}; err/bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    return r


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layernorm_every_width(K, C, family):
    """M = 37: nine full blocks of four rows and one block holding a single row."""
    c = _ln_case(37, C, family)
    yb, yf, mean, rstd = _ln_forward(K, c)
    _check_ln_forward(c, yb, yf, mean, rstd, "widths")
    _check_ln_backward(c, _ln_backward(K, c, mean[:37], rstd[:37]), "widths")


@pytest.mark.parametrize("C", [128, 768])
@pytest.mark.parametrize("M", [1, 3])
def test_layernorm_decode_rows(K, M, C):
    for family in FAMILIES:
        c = _ln_case(M, C, family)
        yb, yf, mean, rstd = _ln_forward(K, c)
        _check_ln_forward(c, yb, yf, mean, rstd, "decode")
        _check_ln_backward(c, _ln_backward(K, c, mean[:M], rstd[:M]), "decode")


def test_layernorm_forward_second_trip(K):
    """More rows than 4 x 8192 blocks hold: the forward's grid-stride loop takes a second trip, and ends in a tail."""
    c = _ln_case(4 * 8192 + 7, 64, "offset")
    _check_ln_forward(c, *_ln_forward(K, c), "stride")


@pytest.mark.parametrize("C", [192, 768])
def test_layernorm_backward_second_trip(K, C):
    """M = 4099 > 4 x LN_BWD_MAX_BLOCKS = 2048 rows: three trips of the backward's loop, the last part-filled."""
    c = _ln_case(4099, C, "spread")
    _, _, mean, rstd = _ln_forward(K, c)
    _check_ln_backward(c, _ln_backward(K, c, mean[:4099], rstd[:4099]), "stride")


@pytest.mark.parametrize("C", [256, 1600])
def test_layernorm_single_output_forward(K, C):
    c = _ln_case(37, C, "spread")
    M = 37
    yb, yf, mean, rstd = _ln_forward(K, c)
    yb1, none1, mean1, rstd1 = _ln_forward(K, c, want_f32=False)
    none2, yf2, mean2, rstd2 = _ln_forward(K, c, want_bf16=False)
    assert none1 is None and none2 is None
    _check_ln_forward(c, yb1, None, mean1, rstd1, "bf16 only")
    _check_ln_forward(c, None, yf2, mean2, rstd2, "f32 only")
    assert torch.equal(bits(yb1), bits(yb)) and torch.equal(bits(yf2), bits(yf))
    for a, b in ((mean1, mean), (mean2, mean), (rstd1, rstd), (rstd2, rstd)):
        assert torch.equal(bits(a[:M]), bits(b[:M]))


@pytest.mark.parametrize("C", [256, 1600])
def test_layernorm_backward_fp32_dy(K, C):
    """gpt2mi_layernorm_bwd_f32: fp32 dy and fp32 out, which at p = 0 is dres itself."""
    c = _ln_case(37, C, "spread", f32_dy=True)
    _, _, mean, rstd = _ln_forward(K, c)
    bufs = _ln_backward(K, c, mean[:37], rstd[:37])
    assert bufs[3].dtype == torch.float32
    _check_ln_backward(c, bufs, "fp32 dy")
    assert torch.equal(bits(bufs[3]), bits(bufs[0])), "out != dres at p = 0"


@pytest.mark.parametrize("C", [256, 1600])
def test_layernorm_backward_options(K, C):
    c = _ln_case(37, C, "spread")
    M = 37
    _, _, mean, rstd = _ln_forward(K, c)
    mean, rstd = mean[:M], rstd[:M]
    full = _ln_backward(K, c, mean, rstd)
    _check_ln_backward(c, full, "all outputs")
    # dres_init: dres is written, not read (NaN-filled here): the gradient alone, the bits of an accumulation onto zeros
    init = _ln_backward(K, c, mean, rstd, dres_init=True, dres_fill=torch.full((M, C), math.nan))
    _check_ln_backward(c, init, "dres_init", dres_ref=c["dx"])
    onto_zero = _ln_backward(K, c, mean, rstd, dres_fill=torch.zeros(M, C))
    assert torch.equal(bits(init[0]), bits(onto_zero[0])) and torch.equal(bits(init[3]), bits(onto_zero[3]))
    # NULL parameter gradients / NULL branch outputs: the rest is unchanged (bitwise where no atomics are involved)
    no_dw = _ln_backward(K, c, mean, rstd, want_dw=False)
    assert no_dw[1] is None and no_dw[2] is None
    _check_ln_backward(c, no_dw, "dw = db = NULL")
    no_out = _ln_backward(K, c, mean, rstd, want_out=False)
    assert no_out[3] is None and no_out[4] is None
    _check_ln_backward(c, no_out, "out = dbias_out = NULL")
    for other in (no_dw, no_out):
        assert torch.equal(bits(other[0]), bits(full[0])), "dres changed with a NULL output"
    assert torch.equal(bits(no_dw[3]), bits(full[3])), "out changed with dw = db = NULL"


@pytest.mark.parametrize("M,C", [(201, 256), (37, 1600)])
def test_layernorm_backward_output_dropout(K, M, C):
    """p_out = 0.1: `out` is the site's mask (oracle.dropout_ref) applied to the kernel's own dres, scaled by the host's
    inv_keep, bitwise; dbias_out the column sums of out as stored. M x C >= 50 000 elements for the dropped share."""
    p, seed = 0.1, 0x1234_5678_9ABC
    assert M * C >= 50_000
    for f32_dy in (False, True):
        c = _ln_case(M, C, "spread", f32_dy=f32_dy)
        _, _, mean, rstd = _ln_forward(K, c)
        bufs = _ln_backward(K, c, mean[:M], rstd[:M], p_out=p, seed_out=seed)
        _check_ln_backward(c, bufs, f"p_out={p} f32_dy={f32_dy}", p_out=p, seed_out=seed)
        share = float((bufs[3][:M * C] == 0).float().mean())
        print(f"ln_bwd dropout M={M} C={C}: dropped share {share:.4f}")
        assert abs(share - p) <= 0.01, share


@pytest.mark.parametrize("C", [320, 96, 2304])
def test_layernorm_refuses_other_widths(K, C):
    M = 8
    x, w, b = torch.randn(M, C).to(dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    yb, yf, mean, rstd = sentinel(M * C, BF16), sentinel(M * C), sentinel(M), sentinel(M)
    with pytest.raises(K.KernelError):
        K.layernorm_fwd(x, w, b, yb, yf, mean, rstd, M, C, EPS)
    dres, dw, db, out, dbo = sentinel(M * C), sentinel(C), sentinel(C), sentinel(M * C, BF16), sentinel(C)
    with pytest.raises(K.KernelError):
        K.layernorm_bwd(x, w, torch.zeros(M, device=dev), torch.ones(M, device=dev), x.to(BF16), dres, dw, db, out, dbo,
                        M, C)
    torch.cuda.synchronize()
    assert all(untouched(t) for t in (yb, yf, mean, rstd, dres, dw, db, out, dbo))


# ---- embedding ------------------------------------------------------------------------------------------------------
EMB_T, EMB_V = 24, 61
EMB_POISON = EMB_V - 1  # the wte row the padding entries of idx point at: NaN


def _embed_case(K, B, C, T_valid, p, same_token=False):
    T, V = EMB_T, EMB_V
    seed = 0xABCD_0000_0000 + 97 * B + C
    g = torch.Generator().manual_seed(B * 1000 + C + T_valid)
    idx = torch.randint(0, V - 1, (B, T), generator=g)  # 60 tokens over up to 192 positions: tokens repeat
    if same_token:
        idx[:] = 7
    idx[:, T_valid:] = EMB_POISON
    wte, wpe = torch.randn(V, C, generator=g), torch.randn(T, C, generator=g)
    wte[EMB_POISON] = math.nan
    wpe[T_valid:] = math.nan
    valid = torch.zeros(B, T, dtype=torch.bool)
    valid[:, :T_valid] = True
    valid = valid.reshape(-1)
    # forward: x = drop(wte[idx] + wpe[t]) in fp32, bitwise; exact zeros in the padding rows
    x = sentinel(B * T * C + SLACK)
    K.embed_fwd(idx.to(dev), wte.to(dev), wpe.to(dev), x, B, T, C, p, seed, T_valid=T_valid)
    torch.cuda.synchronize()
    want = dropout_f32((wte[idx] + wpe[None]).reshape(B * T, C), seed, p)
    want[~valid] = 0.0
    assert torch.equal(bits(x[:B * T * C].view(B * T, C).cpu()), bits(want)), "embed_fwd"
    assert untouched(x[B * T * C:]), "x written past B*T*C"
    # backward: dwte[idx] += g, dwpe[t] += sum_b g with g = drop(dres); padding rows of dres are never read (NaN)
    dres = torch.randn(B * T, C, generator=g)
    dres[~valid] = math.nan
    dwte0 = torch.randn(V, C, generator=g) + 2.0
    dwpe0 = torch.randn(T, C, generator=g) - 2.0
    dwte = sentinel(V * C + SLACK)
    dwte[:V * C] = dwte0.to(dev).reshape(-1)
    dwpe = sentinel(T * C + SLACK)
    dwpe[:T_valid * C] = dwpe0[:T_valid].to(dev).reshape(-1)
    K.embed_bwd(idx.to(dev), dres.to(dev), dwte, dwpe, B, T, C, p, seed, T_valid=T_valid)
    torch.cuda.synchronize()
    add = dropout_f32(torch.nan_to_num(dres), seed, p).double()  # the fp32 addends, exact in fp64
    add[~valid] = 0.0
    flat = idx.reshape(-1)
    ref_te = dwte0.double().index_add(0, flat, add)
    abs_te = dwte0.double().abs().index_add(0, flat, add.abs())
    n_te = 1 + torch.bincount(flat[valid], minlength=V).double()[:, None].expand(V, C)
    got_te = dwte[:V * C].view(V, C).cpu()
    w_te = check_elements("dwte", got_te, ref_te, (n_te - 1) * U * abs_te + U * ref_te.abs())
    hit = torch.zeros(V, dtype=torch.bool)
    hit[flat[valid]] = True
    assert torch.equal(bits(got_te[~hit]), bits(dwte0[~hit])), "dwte rows of absent tokens changed"
    ref_pe = dwpe0[:T_valid].double() + add.view(B, T, C)[:, :T_valid].sum(0)
    abs_pe = dwpe0[:T_valid].double().abs() + add.view(B, T, C)[:, :T_valid].abs().sum(0)
    w_pe = check_elements("dwpe", dwpe[:T_valid * C].view(T_valid, C), ref_pe, sum_bound(B + 1, abs_pe, ref_pe))
    assert untouched(dwpe[T_valid * C:]), "dwpe rows from T_valid on changed"
    assert untouched(dwte[V * C:]), "dwte written past V*C"
    return w_te, w_pe


@pytest.mark.parametrize("C", [64, 384, 768])
def test_embedding_batch_tails_padding_and_dropout(K, C):
    """B = 1, 3 (tail loop only), 5 (one group of four and a tail), 8 (two groups): the backward's batch walk."""
    for B in (1, 3, 5, 8):
        for T_valid in (24, 17, 1):
            for p in (0.0, 0.1):
                w_te, w_pe = _embed_case(K, B, C, T_valid, p)
                print(f"embed C={C} B={B} T_valid={T_valid} p={p}: err/bound dwte {w_te:.3f} dwpe {w_pe:.3f}")


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_embedding_one_token_everywhere(K, p):
    """Every position holds token 7: B x T_valid atomic adds land on one dwte row."""
    w_te, w_pe = _embed_case(K, 5, 384, 17, p, same_token=True)
    print(f"embed same token p={p}: err/bound dwte {w_te:.3f} dwpe {w_pe:.3f}")


# ---- column sums ----------------------------------------------------------------------------------------------------
# (M, N, ld, first column of the slice in a buffer of ld columns)
COLSUM_CASES = [(1, 4, 4, 0), (7, 260, 264, 0), (33, 1600, 1608, 0), (515, 768, 2304, 768), (20010, 256, 256, 0)]


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,N,ld,c0", COLSUM_CASES)
def test_colsum_tails_and_strides(K, M, N, ld, c0, dtype):
    g = torch.Generator().manual_seed(M + N)
    buf = torch.full((M, ld), math.nan)  # columns outside the slice poison whatever sums them
    buf[:, c0:c0 + N] = torch.randn(M, N, generator=g) + 0.25
    buf = buf.to(dtype)
    db = sentinel(N + SLACK)
    db[:N] = 1.0
    gd = buf.to(dev)
    K.colsum_bf16(gd.view(-1)[c0:], db, M, N, ld)
    torch.cuda.synchronize()
    a = buf[:, c0:c0 + N].double()
    ref = 1.0 + a.sum(0)
    worst = check_elements("colsum", db[:N], ref, sum_bound(M + 1, 1.0 + a.abs().sum(0), ref))
    assert untouched(db[N:]), "db written past N"
    print(f"colsum {dtype} M={M} N={N} ld={ld} c0={c0}: err/bound {worst:.3f}")


def test_colsum_refuses_unaligned_stride(K):
    db = sentinel(260)
    for g in (torch.zeros(7, 262, dtype=BF16, device=dev), torch.zeros(7, 262, device=dev)):
        with pytest.raises(K.KernelError):
            K.colsum_bf16(g, db, 7, 260, 262)
    torch.cuda.synchronize()
    assert untouched(db)


# ---- cross entropy --------------------------------------------------------------------------------------------------
# (M, V, ld, ldd, dtype): the bf16 two-pass kernel (three trips of its c += 2048 loop; one; M > 4096 for the finalize
# kernel's four-row loop), the register-resident row kernel (GPT-2's vocabulary), the fp32 kernel
XENT_CASES = [(5, 5000, 5008, 5120, BF16), (9, 130, 136, 136, BF16), (4101, 130, 136, 136, BF16),
              (8, 50257, 50304, 50432, BF16), (5, 5000, 5008, 5120, torch.float32)]
XENT_IDS = ["two-pass-5000", "two-pass-130", "two-pass-4101rows", "row-kernel", "f32"]


def _xent_logits(M, V, ld, dtype):
    g = torch.Generator().manual_seed(M * 3 + V)
    logits = torch.full((M, ld), math.nan)  # the padding [V, ld) poisons a kernel that reads it as logits
    logits[:, :V] = torch.randn(M, V, generator=g) * 3
    labels = torch.randint(0, V, (M,), generator=g)
    labels[0], labels[1] = V - 1, 0  # the last valid column / the first
    return logits.to(dtype), labels


def _run_xent(K, logits, labels, M, V, ld, ldd, ignore_index, with_dlogits=True):
    rows, lse = sentinel(M + SLACK), sentinel(M + SLACK)
    dl = sentinel(M * ldd + SLACK, logits.dtype) if with_dlogits else None
    loss_inv = sentinel(2 + SLACK)
    K.xent_fwd(logits.to(dev), ld, labels.to(dev), rows, lse, dl, ldd, M, V, loss_inv[0:], loss_inv[1:],
               ignore_index=ignore_index)
    torch.cuda.synchronize()
    assert untouched(rows[M:]) and untouched(lse[M:]) and untouched(loss_inv[2:]), "wrote past M rows / the two scalars"
    if dl is not None:
        assert untouched(dl[M * ldd:]), "dlogits written past M*ldd"
    return rows[:M].cpu(), lse[:M].cpu(), None if dl is None else dl[:M * ldd].view(M, ldd).cpu(), loss_inv[:2].cpu()


def _check_xent(K, logits, labels, M, V, ld, ldd, ignore_index, tag):
    """Both forms of the call (with dlogits and with dlogits = NULL) against the fp64 reference."""
    lse64, rows64, d64, loss64, count = xent_ref64(logits, labels, V, ignore_index)
    bad = torch.isnan(rows64)
    good = ~bad
    f32 = logits.dtype == torch.float32
    for with_dl in (True, False):
        rows, lse, dl, loss_inv = _run_xent(K, logits, labels, M, V, ld, ldd, ignore_index, with_dl)
        w_lse = check_elements("lse", lse, lse64, 1e-5 * lse64.abs().clamp_min(1.0))
        assert bool(torch.isnan(rows[bad]).all()), "a label outside [0, V) did not poison its row's loss"
        w_rows = check_elements("loss_rows", rows[good], rows64[good], 1e-5 * rows64[good].abs().clamp_min(1.0))
        ign = labels == ignore_index
        assert bool((bits(rows[ign]) == 0).all()), "an ignored row's loss is not +0"
        loss, inv = float(loss_inv[0]), float(loss_inv[1])
        if count == 0 or bool(bad.any()):
            assert math.isnan(loss), loss
        else:
            assert abs(loss - float(loss64)) <= 1e-5 * max(1.0, abs(float(loss64))), (loss, float(loss64))
        if count:
            assert abs(inv - 1.0 / count) <= 2.0 ** -22 / count, (inv, count)
        else:
            assert math.isinf(inv) and inv > 0
        line = f"xent {tag} dlogits={with_dl}: err/bound lse {w_lse:.3f} loss_rows {w_rows:.3f}"
        if dl is not None:
            assert bool(torch.isnan(dl[bad][:, :V]).all()), "a bad label's dlogits row is not NaN"
            assert bool((dl[good][:, V:] == 0).all()), "dlogits columns [V, ldd) are not zero"
            assert not bool(torch.isnan(dl[good]).any()), "NaN outside the bad labels' rows"
            assert bool((bits(dl[ign]) == 0).all()), "an ignored row's dlogits are not +0"
            live = good & ~ign
            err = rel_err(dl[live][:, :V], d64[live])
            assert err < (1e-5 if f32 else 4e-3), err
            # the row's own label column, one element: p - 1 with p = exp(v - lse) <= 1. fp32: the relative error of p
            # is the absolute error of lse (held to 1e-5 max(1, |lse|) above) plus __expf's few ulp. bf16: p is rounded
            # to bf16 before the 1 is subtracted and the difference rounded again: two roundings of values <= 1, 2^-9
            # each
            r = live.nonzero()[:, 0]
            col = labels[r]
            tol = 2e-5 * lse64[r].abs().clamp_min(1.0) + (0.0 if f32 else 2.0 ** -8)
            w_lab = check_elements("dlogits[label]", dl[r, col], d64[r, col], tol)
            line += f"; dlogits rel_err {err:.3e}, label column err/bound {w_lab:.3f}"
        print(line)


@pytest.mark.parametrize("M,V,ld,ldd,dtype", XENT_CASES, ids=XENT_IDS)
def test_xent_shapes_strides_and_ignored_rows(K, M, V, ld, ldd, dtype):
    logits, labels = _xent_logits(M, V, ld, dtype)
    labels[2] = -100
    if M > 4096:  # ignored rows on both sides of the finalize kernel's four-row loop
        labels[100], labels[4095], labels[4096], labels[M - 1] = -100, -100, -100, -100
    _check_xent(K, logits, labels, M, V, ld, ldd, -100, f"{dtype} M={M} V={V} ld={ld} ldd={ldd}")


@pytest.mark.parametrize("M,V,ld,ldd,dtype", XENT_CASES, ids=XENT_IDS)
def test_xent_other_ignore_index(K, M, V, ld, ldd, dtype):
    """ignore_index = 7 is a valid column: rows labelled 7 are ignored, -100 is then a bad label like any other."""
    logits, labels = _xent_logits(M, V, ld, dtype)
    labels[2], labels[M - 1] = 7, 7
    _check_xent(K, logits, labels, M, V, ld, ldd, 7, f"ignore_index=7 {dtype} M={M} V={V}")


@pytest.mark.parametrize("M,V,ld,ldd,dtype", XENT_CASES, ids=XENT_IDS)
def test_xent_every_label_ignored(K, M, V, ld, ldd, dtype):
    logits, labels = _xent_logits(M, V, ld, dtype)
    labels[:] = -100
    _check_xent(K, logits, labels, M, V, ld, ldd, -100, f"all ignored {dtype} M={M} V={V}")


@pytest.mark.parametrize("M,V,ld,ldd,dtype", XENT_CASES, ids=XENT_IDS)
def test_xent_label_in_the_padding_poisons_its_row_only(K, M, V, ld, ldd, dtype):
    """A label of V and one of ld - 1 (inside the row's allocation, so a kernel that reads them as logits reads NaN
    padding of its own row, nothing else): those rows' loss and dlogits are NaN, every other row is within bounds."""
    logits, labels = _xent_logits(M, V, ld, dtype)
    labels[2], labels[3], labels[4] = V, -100, ld - 1
    _check_xent(K, logits, labels, M, V, ld, ldd, -100, f"bad labels {dtype} M={M} V={V}")
