"""The references and bounds that tests/test_row_kernels_gpu.py and tests/test_aux_kernels_gpu.py hold the kernels to,
checked on the CPU against independent formulations: a wrong reference or a vacuous bound would make those tests pass
or fail for the wrong reason."""
import math

import numpy as np
import torch

from oracle import dropout_ref
from tests import test_aux_kernels_gpu as A
from tests import test_row_kernels_gpu as R

BF16 = torch.bfloat16


def test_layernorm_closed_form_backward_matches_fp64_autograd():
    for C, family in ((64, "spread"), (192, "offset"), (768, "spread")):
        x, w, b, dy, _ = R._ln_inputs(9, C, family)
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
        y = torch.nn.functional.layer_norm(xr, (C,), wr, br, R.EPS)
        y.backward(dy.double())
        y64, mu, rstd, xhat = R.ln_ref64(x.double(), w.double(), b.double())
        dx, dw_add, db_add = R.ln_bwd_ref64(xhat, rstd, w.double(), dy.double())
        torch.testing.assert_close(y64, y.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(mu, x.double().mean(1), rtol=1e-14, atol=0)
        torch.testing.assert_close(rstd, 1 / torch.sqrt(x.double().var(1, unbiased=False) + R.EPS), rtol=1e-13, atol=0)
        # (the offset family loses digits to x - mean in fp64 too: 100 / 0.1 x 2^-53)
        torch.testing.assert_close(dx, xr.grad, rtol=1e-9, atol=1e-10)
        torch.testing.assert_close(dw_add.sum(0), wr.grad, rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(db_add.sum(0), br.grad, rtol=1e-12, atol=1e-12)


def test_layernorm_yardstick_tells_one_pass_variance_from_two_pass():
    """The offset family is there to fail a one-pass E[x^2] - E[x]^2 variance: in fp32 it misses the yardstick bound on
    y by orders of magnitude, while a plain two-pass fp32 evaluation of the kernel's formulas stays inside it."""
    c = R._ln_case(37, 768, "offset")
    x, w, b = c["x"], c["w"], c["b"]
    mu = x.mean(1, keepdim=True)
    two_pass = (x - mu) * torch.rsqrt(((x - mu) ** 2).mean(1, keepdim=True) + R.EPS) * w + b
    var1 = ((x * x).mean(1, keepdim=True) - mu * mu).clamp_min(0)
    one_pass = (x - mu) * torch.rsqrt(var1 + R.EPS) * w + b
    bound = R.LN_YARDSTICK_FACTOR * c["yard"]["y"]
    assert float((two_pass.double() - c["y"]).abs().max()) <= bound
    assert float((one_pass.double() - c["y"]).abs().max()) > 100 * bound


def test_dropout_reference_matches_site_scale():
    p, seed, rows, cols = 0.1, 0x1234_5678_9ABC, 97, 260
    ik = R.inv_keep(p)
    assert ik.dtype == torch.float32
    assert float(ik) == float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    assert float(R.inv_keep(0.0)) == 1.0
    scale = dropout_ref.site_scale(seed, rows, cols, p)
    keep = R.keep_mask(seed, rows, cols, p)
    assert torch.equal(keep, scale != 0)
    assert abs(1 - float(keep.float().mean()) - p) < 0.01
    assert bool(R.keep_mask(seed, rows, cols, 0.0).all())
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(0))
    got = R.dropout_f32(x, seed, p)
    assert bool((got[~keep] == 0).all()) and torch.equal(got[keep], (x * ik)[keep])
    # the oracle's multiplier is the same number (float32(1 / (1 - p))), so the two agree to the last bit here
    torch.testing.assert_close(got, x * scale, rtol=2.0 ** -23, atol=0)
    assert torch.equal(R.dropout_f32(x, seed, 0.0), x)


def test_bf16_ulp_bound_brackets_one_step():
    """The correct rounding of ref passes; the representable values two steps away on either side never do."""
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(20000, generator=g, dtype=torch.float64)
    ref = ref * torch.exp2(torch.randint(-20, 20, (20000,), generator=g))
    edges = [1.0, 1 + 2.0 ** -8, 2 - 2.0 ** -9, 1 + 2.0 ** -7 - 2.0 ** -30]
    ref = torch.cat([ref, torch.tensor(edges, dtype=torch.float64)])
    rounded = ref.float().to(BF16)
    bound = R.bf16_ulp_bound(ref)
    assert bool(((rounded.double() - ref).abs() <= bound).all())
    for step in (-2, 2):
        far = (rounded.view(torch.int16) + step).view(BF16)
        assert bool(((far.double() - ref).abs() > bound).all()), step
    # the neighbours themselves, as torch.nextafter would give them in bf16: one step is a spacing of 2^-7 of the binade
    one = (rounded.view(torch.int16) + 1).view(BF16).double() - rounded.double()
    assert bool((one.abs() >= 2.0 ** -8 * rounded.double().abs()).all())


def test_f32_ulp_is_the_spacing_nextafter_gives():
    x = torch.tensor([1.0, 1.5, 2.0, 0.3, 1e-3, 3.9999, 1e4], dtype=torch.float32)
    step = torch.nextafter(x, torch.full_like(x, math.inf)).double() - x.double()
    assert torch.equal(R.f32_ulp(x.double()), step)


def test_sum_bound_holds_for_fp32_sums_in_any_order():
    g = torch.Generator().manual_seed(4)
    a = torch.randn(4099, 16, generator=g) * torch.exp2(torch.randint(-8, 8, (4099, 16), generator=g).float())
    ref, abs_sum = a.double().sum(0), a.double().abs().sum(0)
    bound = R.sum_bound(a.shape[0], abs_sum, ref)
    seq = torch.zeros(16)
    for row in a:  # strictly sequential, the worst order
        seq = seq + row
    for got in (seq, a.sum(0), a.flip(0).sum(0), a[::2].sum(0) + a[1::2].sum(0)):
        assert bool(((got.double() - ref).abs() <= bound).all())
    # and it is not vacuous: a column that lost its largest addend is outside it
    col = a[:, 0].double()
    k = int(col.abs().argmax())
    assert abs(float(col.sum() - col[k]) - float(ref[0])) > float(bound[0])


def test_check_elements_reports_one_bad_element():
    ref = torch.ones(5, 7, dtype=torch.float64)
    out = torch.ones(5, 7)
    assert R.check_elements("x", out, ref, 1e-6) == 0.0
    out[3, 4] += 1e-3
    try:
        R.check_elements("x", out, ref, 1e-6)
    except AssertionError as e:
        assert "[3, 4]" in str(e)
    else:
        raise AssertionError("one element off by 1e-3 passed a bound of 1e-6")
    out[3, 4] = math.nan
    try:
        R.check_elements("x", out, ref, 1e-6)
    except AssertionError:
        pass
    else:
        raise AssertionError("a NaN passed")


def test_xent_reference_matches_fp64_cross_entropy():
    M, V, ld = 9, 130, 136
    logits, labels = R._xent_logits(M, V, ld, BF16)
    labels[2], labels[5] = 7, 7
    for ignore_index in (-100, 7):
        lab = labels.clone()
        if ignore_index == -100:
            lab[3] = -100
        z = logits[:, :V].double().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(z, lab, ignore_index=ignore_index)
        loss.backward()
        lse, rows, d, mean, count = R.xent_ref64(logits, lab, V, ignore_index)
        per_row = torch.nn.functional.cross_entropy(z.detach(), lab, ignore_index=ignore_index, reduction="none")
        torch.testing.assert_close(rows, per_row, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(mean, loss.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(d / count, z.grad, rtol=1e-12, atol=1e-14)
        assert count == int((lab != ignore_index).sum())
    # labels outside [0, V): NaN rows, everything else as before
    lab = labels.clone()
    lab[4], lab[6] = V, ld - 1
    lse2, rows2, d2, mean2, _ = R.xent_ref64(logits, lab, V, -100)
    bad = torch.zeros(M, dtype=torch.bool)
    bad[4] = bad[6] = True
    assert bool(torch.isnan(rows2[bad]).all()) and bool(torch.isnan(d2[bad]).all()) and math.isnan(float(mean2))
    assert not bool(torch.isnan(rows2[~bad]).any()) and not bool(torch.isnan(d2[~bad]).any())
    assert math.isnan(float(R.xent_ref64(logits, torch.full((M,), -100), V, -100)[3]))


def test_adamw_reference_matches_torch_adamw_in_fp64():
    n = 64
    g = torch.Generator().manual_seed(6)
    p0, gr = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64) * 0.01
    h = {k: float(np.float32(v)) for k, v in A.HYPER.items()}
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([param], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    ref = (p0, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
    for step in (1, 2, 3):
        param.grad = gr * 0.5
        opt.step()
        ref = A.adamw_ref64(ref[0], gr, ref[1], ref[2], step, 0.5, **A.HYPER)
    torch.testing.assert_close(ref[0], param.detach(), rtol=1e-12, atol=1e-14)
    st = opt.state[param]
    torch.testing.assert_close(ref[1], st["exp_avg"], rtol=1e-12, atol=1e-16)
    torch.testing.assert_close(ref[2], st["exp_avg_sq"], rtol=1e-12, atol=1e-20)
