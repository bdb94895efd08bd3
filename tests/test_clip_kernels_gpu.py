"""The v16 clipping entries through the C ABI on the MI355X: gpt2mi_sumsq_partials, gpt2mi_clip_coef and
gpt2mi_adamw_clipped against gpt2mi_norm_finalize / gpt2mi_adamw (bitwise) and fp64 torch on the CPU
(clip_grad_norm_ then torch.optim.AdamW)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
HP = dict(lr=1e-3, wd=0.1, b1=0.9, b2=0.95, eps=1e-8)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


def L():
    from gpt_2_distributed_amd import _lib
    return _lib


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _coef(partials, max_norm, want_sumsq=False):
    out = torch.full((3,), -7.0, device=dev)  # sumsq, norm, coef
    L().clip_coef(partials, partials.numel(), max_norm, out[0:1] if want_sumsq else None, out[1:2], out[2:3])
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("n", [1, 5, 2048, 3 * 2048])
def test_clip_coef_matches_norm_finalize_and_torch_formula(n):
    part = torch.rand(n, generator=torch.Generator().manual_seed(n)).to(dev) * (40.0 / n)  # norm^2 ~ 20
    ref = torch.empty(1, device=dev)
    L().norm_finalize(part, n, ref)
    out = _coef(part, 1.5, want_sumsq=True)
    ref = ref.cpu()
    assert out[1].view(torch.int32) == ref[0].view(torch.int32)  # the bits norm_finalize gives
    want = torch.clamp(1.5 / (ref + 1e-6), max=1.0)[0]  # torch's clip_grad_norm_ formula on the fp32 norm
    assert 0 < want < 1
    assert abs(out[2] - want) <= 1e-6 * want
    s = part.double().sum().item()
    assert abs(out[0].item() - s) <= 2.0 ** -23 * s  # the fp32 rounding of the double-precision sum
    # below max_norm: exactly 1
    out = _coef(part, 1e3)
    assert out[2].item() == 1.0 and out[1].view(torch.int32) == ref[0].view(torch.int32)


@pytest.mark.parametrize("n", [1, 2048])
def test_clip_coef_edge_values(n):
    zero = torch.zeros(n, device=dev)
    out = _coef(zero, 1.0)
    assert out[1].item() == 0.0 and out[2].item() == 1.0  # all-zero gradients: 1, not NaN
    nan = zero.clone()
    nan[n // 2] = float("nan")
    out = _coef(nan, 1.0)
    assert math.isnan(out[1].item()) and math.isnan(out[2].item())
    inf = zero.clone()
    inf[n - 1] = float("inf")
    out = _coef(inf, 1.0)
    assert math.isinf(out[1].item()) and out[2].item() == 0.0


def test_sumsq_partials_in_three_slices_with_one_clip_coef():
    n, cuts = 3 * 4096 + 64, [0, 4096, 4160, 3 * 4096 + 64]
    gr = (torch.randn(n, generator=torch.Generator().manual_seed(12)) * 0.01).to(dev)
    P = L().norm_partials_size()
    part = torch.full((3 * P,), float("nan"), device=dev)
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        L().sumsq_partials(gr[a:b], b - a, 1.0, part[i * P:(i + 1) * P])
    out = _coef(part, 0.5)
    norm = gr.double().norm().item()
    assert abs(out[1].item() - norm) < 1e-5 * norm
    assert abs(out[2].item() - 0.5 / (norm + 1e-6)) < 1e-5 * 0.5 / norm
    # the scale is applied before squaring, and one range gives grad_norm's value
    one, ref = torch.empty(P, device=dev), torch.empty(1, device=dev)
    L().sumsq_partials(gr, n, 3.0, one)
    L().grad_norm(gr, n, 3.0, torch.empty(P, device=dev), ref)
    out = _coef(one, 1.0)
    assert out[1].view(torch.int32) == ref.cpu()[0].view(torch.int32)


def _state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01
    m, v = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-4
    return [t.to(dev) for t in (p, gr, m, v)]


@pytest.mark.parametrize("n", [4, 4100, 2048 * 256 * 8 + 12])  # lone tail group; 8-wide body + tail; second sweep + tail
@pytest.mark.parametrize("coef", [1.0, 0.37])
def test_adamw_clipped_is_bitwise_adamw_with_the_scale_folded_in(n, coef):
    """coef_dev = 1: gpt2mi_adamw's bits. coef_dev = 0.37 with grad_scale = 1: gpt2mi_adamw called with
    grad_scale = 0.37."""
    p0, gr, m0, v0 = _state(n, 21)
    P = L().norm_partials_size()
    outs = []
    for clipped in (False, True):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        pb = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        if clipped:
            cd = torch.tensor([coef], dtype=torch.float32, device=dev)
            L().adamw_clipped(p, gr, m, v, pb, n, HP["lr"], HP["wd"], HP["b1"], HP["b2"], HP["eps"], 3, 1.0, cd)
        else:
            L().adamw(p, gr, m, v, pb, n, HP["lr"], HP["wd"], HP["b1"], HP["b2"], HP["eps"], 3, coef,
                      torch.empty(P, device=dev), None)
        outs.append((p, m, v, pb))
    torch.cuda.synchronize()
    for a, b, name in zip(outs[0], outs[1], "p m v shadow".split()):
        assert torch.equal(a, b), name
    assert not torch.equal(outs[1][0], p0)


def test_adamw_clipped_norm_outputs_are_optional_and_post_scale():
    """partials / grad_norm given: the norm of the gradients as the update saw them (grad_scale * coef)."""
    n = 4100
    p, gr, m, v = _state(n, 22)
    part, gn = torch.empty(L().norm_partials_size(), device=dev), torch.empty(1, device=dev)
    cd = torch.tensor([0.25], dtype=torch.float32, device=dev)
    L().adamw_clipped(p, gr, m, v, None, n, HP["lr"], HP["wd"], HP["b1"], HP["b2"], HP["eps"], 1, 2.0, cd, part, gn)
    torch.cuda.synchronize()
    want = 0.5 * gr.double().norm().item()
    assert abs(gn.item() - want) < 1e-5 * want


def test_four_clipped_steps_vs_fp64_torch():
    """Four steps with a different gradient each (norms 0.6, 2.5, 0.9, 4 around max_norm = 1: two steps unclipped, two
    clipped with different coefficients) against fp64 torch on the CPU: clip_grad_norm_ then torch.optim.AdamW. Adam's
    first update is scale invariant, so one step cannot see a wrong coefficient; this sequence, with m and v compared
    directly, does. p within 1e-6 (test_adamw_matches_oracle_and_norm's bound); m and v within twice the error the
    unchanged gpt2mi_adamw shows against fp64 torch without clipping on the same gradients."""
    n, max_norm, targets = 4100, 1.0, [0.6, 2.5, 0.9, 4.0]
    g = torch.Generator().manual_seed(31)
    p0 = torch.randn(n, generator=g)
    grads = []
    for t in targets:
        x = torch.randn(n, generator=g)
        grads.append((x * (t / x.norm())).float())
    P = L().norm_partials_size()

    def reference(clip):
        p = torch.nn.Parameter(p0.double().clone())
        opt = torch.optim.AdamW([p], lr=HP["lr"], weight_decay=HP["wd"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"])
        norms, coefs = [], []
        for gr in grads:
            p.grad = gr.double().clone()
            nrm = torch.nn.utils.clip_grad_norm_([p], max_norm if clip else float("inf"))
            norms.append(nrm.item())
            coefs.append(min(1.0, max_norm / (nrm.item() + 1e-6)))
            opt.step()
        st = opt.state[p]
        return p.detach(), st["exp_avg"], st["exp_avg_sq"], norms, coefs

    def device(clip):
        p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        part, gn, cf = torch.empty(P, device=dev), torch.empty(1, device=dev), torch.empty(1, device=dev)
        norms, coefs = [], []
        for step, gr in enumerate(grads, 1):
            gd = gr.to(dev)
            if clip:
                L().sumsq_partials(gd, n, 1.0, part)
                L().clip_coef(part, P, max_norm, None, gn, cf)
                L().adamw_clipped(p, gd, m, v, None, n, HP["lr"], HP["wd"], HP["b1"], HP["b2"], HP["eps"], step, 1.0, cf)
                coefs.append(cf.item())
            else:
                L().adamw(p, gd, m, v, None, n, HP["lr"], HP["wd"], HP["b1"], HP["b2"], HP["eps"], step, 1.0, part, gn)
            norms.append(gn.item())
        torch.cuda.synchronize()
        return p.cpu(), m.cpu(), v.cpu(), norms, coefs

    rp, rm, rv, rnorms, rcoefs = reference(True)
    up, um, uv, _, _ = reference(False)
    assert sum(c == 1.0 for c in rcoefs) == 2 and len({c for c in rcoefs if c < 1.0}) == 2, rcoefs
    assert rel_err(rm, um) > 1e-2 and rel_err(rv, uv) > 1e-2  # clipping is visible in the moments
    dp, dm, dv, dnorms, dcoefs = device(True)
    bp, bm, bv, _, _ = device(False)
    base_m, base_v = rel_err(bm, um), rel_err(bv, uv)
    e_p, e_m, e_v = rel_err(dp, rp), rel_err(dm, rm), rel_err(dv, rv)
    print(f"clipped vs fp64: p {e_p:.3e} m {e_m:.3e} v {e_v:.3e}; unclipped gpt2mi_adamw vs fp64: p "
          f"{rel_err(bp, up):.3e} m {base_m:.3e} v {base_v:.3e}")
    for a, b in zip(dnorms, rnorms):
        assert abs(a - b) < 1e-5 * b  # the pre-clip norm
    for a, b in zip(dcoefs, rcoefs):
        assert abs(a - b) <= 1e-6 * b
    assert dcoefs[0] == 1.0 and dcoefs[2] == 1.0
    assert e_p < 1e-6
    assert e_m <= 2 * base_m, (e_m, base_m)
    assert e_v <= 2 * base_v, (e_v, base_v)
