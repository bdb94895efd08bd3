"""The v24.8 Muon entries against muon.py's rule in fp64: one batch (half last 128-tiles: 64, 192; unequal tile counts;
the q / k / v row blocks of one matrix; a tall matrix; a zero matrix) through every stage, one launch each."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
LR, WD, MOM, SCALE, SENTINEL = 0.02, 0.01, 0.95, 0.5, 7.0
A_, B_, C_ = 3.4445, -4.7750, 2.0315


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _batch():
    mats, off = [], 64
    for r, c in [(64, 64), (128, 512), (192, 192), (192, 768)]:
        mats.append((off, r, c, c))
        off += r * c + 64
    mats += [(off + i * 128 * 128, 128, 128, 128) for i in range(3)]
    off += 384 * 128 + 64
    mats += [(off, 512, 128, 128), (off + 512 * 128 + 64, 64, 64, 64)]  # the tall one; the zero one (last)
    return mats, off + 512 * 128 + 64 + 64 * 64 + 64


def _run(nesterov):
    from gpt_2_distributed_amd import _lib as K
    from gpt_2_distributed_amd.muon import muon_tables
    mats, total = _batch()
    t = muon_tables(mats, dev)
    g = torch.Generator().manual_seed(5)
    grad, buf = torch.randn(total, generator=g) * 0.01, torch.randn(t["x_numel"], generator=g) * 0.01
    grad[mats[-1][0]:mats[-1][0] + 64 * 64] = 0
    buf[-64 * 64:] = 0
    arena = torch.full((total,), SENTINEL)
    for off, r, c, _ in mats:
        arena[off:off + r * c] = torch.randn(r * c, generator=g)
    inp = dict(grad=grad, buf=buf, arena=arena)
    d = {k: v.to(dev) for k, v in inp.items()}
    x = [torch.empty(t["x_numel"], dtype=torch.bfloat16, device=dev) for _ in range(3)]
    a, b = (torch.empty(t["a_numel"], dtype=torch.bfloat16, device=dev) for _ in range(2))
    shadow = torch.full((total,), SENTINEL, dtype=torch.bfloat16, device=dev)
    K.muon_prepare(d["grad"], d["buf"], t["mats"], t["tiles64"], SCALE, MOM, nesterov,
                   torch.empty(t["p_numel"], device=dev), x[0])
    K.muon_gram(x[0], a, t["mats"], t["sym"])
    K.muon_poly(a, b, t["mats"], t["sym"], B_, C_)
    K.muon_apply(b, x[0], x[1], t["mats"], t["full"], A_)
    out = dict(buf=d["buf"], x0=x[0], A1=a.clone(), B1=b.clone(), X1=x[1].clone())
    src = 1
    for _ in range(4):
        K.muon_gram(x[src], a, t["mats"], t["sym"])
        K.muon_poly(a, b, t["mats"], t["sym"], B_, C_)
        K.muon_apply(b, x[src], x[3 - src], t["mats"], t["full"], A_)
        src = 3 - src
    K.muon_update(d["arena"], shadow, x[src], t["mats"], t["tiles64"], LR, WD)
    torch.cuda.synchronize()
    out.update(O=x[src], arena=d["arena"], shadow=shadow)
    return inp, {k: v.cpu() for k, v in out.items()}, mats, t["mats"].cpu().tolist()


@pytest.fixture(scope="module", params=[True, False], ids=["nesterov", "plain"])
def run(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return (request.param, *_run(request.param))


def _per_matrix(flat, rows, kind):
    # kind 'w': [rows][cols]; 'x': [m][n]; 'a': [m][m]
    for _, r, c, _, xoff, aoff, _, _ in rows:
        m, n = min(r, c), max(r, c)
        o, (h, w) = (aoff, (m, m)) if kind == "a" else (xoff, (r, c) if kind == "w" else (m, n))
        yield flat[o:o + h * w].view(h, w)


def _within_one_rounding(got, want):
    # each element within 2^-9 relative of the fp64 value plus 2^-9 of the row's largest
    got, want = got.double(), want.double()
    slack = 2.0 ** -9 * (want.abs() + want.abs().amax(dim=1, keepdim=True))
    return bool(((got - want).abs() <= slack).all())


def test_prepare(run):
    nesterov, inp, out, mats, rows = run
    for i, ((off, r, c, _), bk, b0, x0) in enumerate(zip(mats, _per_matrix(out["buf"], rows, "w"),
                                                         _per_matrix(inp["buf"], rows, "w"),
                                                         _per_matrix(out["x0"], rows, "x"))):
        gs = inp["grad"][off:off + r * c].view(r, c).double() * SCALE
        bref = MOM * b0.double() + gs
        u = gs + MOM * bref if nesterov else bref  # fp32 elementwise: 1e-6 of the operands (the sum may cancel)
        assert bool(((bk.double() - bref).abs() <= 1e-6 * ((MOM * b0.double()).abs() + gs.abs())).all()), i
        want = u / (u.norm() + 1e-7)
        want = want.T if r > c else want  # the tall matrix comes out transposed
        # one bf16 rounding (half an ulp: 2^-8) of an fp32 value whose norm was summed in fp32 (2^-16) and whose u
        # comes from operands that may cancel (1e-6 of them, as for the buffer; they enter u at most twice)
        ops = 2e-6 * ((MOM * b0.double()).abs() + gs.abs()) / (u.norm() + 1e-7)
        tol = (2.0 ** -8 + 2.0 ** -16) * want.abs() + (ops.T if r > c else ops)
        assert bool(((x0.double() - want).abs() <= tol).all()), i
    assert not out["x0"][-64 * 64:].any() and not out["O"][-64 * 64:].any() and bool(out["O"].float().isfinite().all())


@pytest.mark.parametrize("stage", ["gram", "poly", "apply"])
def test_stage_elementwise_vs_fp64(run, stage):
    _, _, out, _, rows = run
    for i, (x0, a1, b1, x1) in enumerate(zip(*(_per_matrix(out[k], rows, kind) for k, kind in
                                               (("x0", "x"), ("A1", "a"), ("B1", "a"), ("X1", "x"))))):
        x0d, a1d, b1d = x0.double(), a1.double(), b1.double()
        got, want = {"gram": (a1, x0d @ x0d.T), "poly": (b1, B_ * a1d + C_ * (a1d @ a1d)),
                     "apply": (x1, A_ * x0d + b1d @ x0d)}[stage]
        assert _within_one_rounding(got, want), (stage, i, float((got.double() - want).abs().max()))
        if stage != "apply":
            assert torch.equal(got, got.T), (stage, i)


def test_chain_within_twice_the_bf16_rule(run):
    from gpt_2_distributed_amd.muon import newton_schulz_reference
    _, _, out, _, rows = run
    for i, (x0, o) in enumerate(zip(_per_matrix(out["x0"], rows, "x"), _per_matrix(out["O"], rows, "x"))):
        if not x0.any():
            continue
        ref = newton_schulz_reference(x0, dtype=torch.float64)
        e_ref = rel_err(newton_schulz_reference(x0, dtype=torch.bfloat16), ref)
        e = rel_err(o, ref)
        print(f"matrix {i} {tuple(x0.shape)}: E_ref {e_ref:.3e} kernels {e:.3e}")
        assert e <= 2 * e_ref, (i, e, e_ref)


def test_update(run):
    _, inp, out, mats, rows = run
    touched = torch.zeros(inp["arena"].numel(), dtype=torch.bool)
    for i, ((off, r, c, _), o) in enumerate(zip(mats, _per_matrix(out["O"], rows, "x"))):
        o = (o.T if r > c else o).double()
        w0, step = inp["arena"][off:off + r * c].view(r, c).double(), LR * max(1.0, r / c) ** 0.5
        want = w0 * (1 - LR * WD) - step * o
        got = out["arena"][off:off + r * c].view(r, c)
        assert bool(((got.double() - want).abs() <= 1e-6 * (w0.abs() + step * o.abs())).all()), i
        touched[off:off + r * c] = True
    assert torch.equal(out["shadow"][touched], out["arena"][touched].to(torch.bfloat16))
    assert bool((out["arena"][~touched] == SENTINEL).all()) and bool((out["shadow"][~touched] == SENTINEL).all())


def test_two_runs_give_the_same_bits(run):
    nesterov, _, out, _, _ = run
    again = _run(nesterov)[1]
    for k in out:
        assert torch.equal(out[k], again[k]), k
