"""gpt2mi_lm_loss (csrc/lm_loss.hip): the tied lm_head GEMM fused with the cross-entropy reduction, against fp64.

Reference: on the CPU in fp64 from the same bf16 operands, lg = x.double() @ w[:V].double().T,
ref = logsumexp(lg) - lg[label]; computed once per shape and shared (the logits do not depend on the labels, so the
label-placement calls of one shape reuse them).

Tolerance: per row |loss_rows - ref| <= 1e-4 * max(1, |ref|), and the same for lse: the project's fp32 loss gate
(README). The expected error is fp32 accumulation over K <= 1600 plus the exp / log intrinsics, ~1e-6 relative; a
bf16-rounded logit (2^-9 relative) would not pass, and the test makes that a check: the fused kernel's mean absolute
row error against fp64 must not exceed the parent path's (gpt2mi_gemm EPI_BF16 into [M, w_rows], then gpt2mi_xent_fwd).

Inputs: x ~ randn, w ~ 0.05 randn, except: feature 0 of w rises linearly with the column index and three rows of x are
built on it (row 3 = +8 e_0: logits ascending, the max arrives in the last tile and every tile rescales; row 4 = -8 e_0:
descending, the max is in the first tile), row 5 of x is scaled by 30 (a wide exponent range), and rows V..w_rows of w
hold 100.0 (padded columns must be masked, not assumed zero)."""
import functools
import math

import pytest
import torch

from gpt_2_distributed_amd import _lib as K

pytestmark = pytest.mark.gpu
dev = "cuda"

# (M, V, K): one panel, one K tile, V not a multiple of 8 | the real V (392 full 128-column tiles + 81 columns), a
# partial 128-row panel, several vocabulary splits | the 1.5B width, an odd count of 64-deep K tiles
SHAPES = [(64, 509, 64), (192, 50257, 128), (320, 1000, 1600)]
IGN = -100
ROW_ASC, ROW_DESC, ROW_WIDE = 3, 4, 5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def case(M, V, Kd):
    """(x, w on the device, w_rows, fp64 logits [M, V], fp64 lse [M]); never modified by a test."""
    g = torch.Generator().manual_seed(1000 + M + V + Kd)
    w_rows = (V + 127) // 128 * 128
    assert w_rows > V
    x = torch.randn(M, Kd, generator=g)
    w = 0.05 * torch.randn(w_rows, Kd, generator=g)
    w[:V, 0] = torch.linspace(-3.0, 3.0, V)
    x[ROW_ASC] = 0.0
    x[ROW_ASC, 0] = 8.0
    x[ROW_DESC] = 0.0
    x[ROW_DESC, 0] = -8.0
    x[ROW_WIDE] *= 30.0
    w[V:] = 100.0
    x, w = x.bfloat16(), w.bfloat16()
    lg = x.double() @ w[:V].double().T
    d = lg[ROW_ASC, 1:] - lg[ROW_ASC, :-1]
    assert (d >= 0).all() and lg[ROW_ASC, -1] == lg[ROW_ASC].max() and lg[ROW_DESC, 0] == lg[ROW_DESC].max()
    return x.to(dev), w.to(dev), w_rows, lg, torch.logsumexp(lg, dim=1)


def run(M, V, Kd, labels, loss_sum=None, count=None, accumulate=False):
    x, w, w_rows, _, _ = case(M, V, Kd)
    rows = torch.full((M,), 7.0, device=dev)
    lse = torch.full((M,), 7.0, device=dev)
    mean = torch.full((1,), 7.0, device=dev)
    if loss_sum is None:
        loss_sum, count = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    ws = torch.empty(K.lm_loss_workspace(M, V), device=dev)
    K.lm_loss(x, Kd, w, Kd, w_rows, labels.to(dev), M, V, Kd, rows, lse, ws, loss_sum=loss_sum, count=count,
              accumulate=accumulate, loss_mean=mean, ignore_index=IGN)
    return rows, lse, loss_sum, count, mean


def ref_rows(M, V, Kd, labels):
    _, _, _, lg, lse = case(M, V, Kd)
    valid = labels != IGN
    safe = labels.clamp(0, V - 1)
    r = lse - lg.gather(1, safe[:, None])[:, 0]
    return torch.where(valid, r, torch.zeros_like(r)), valid


def label_sets(M, V, seed=5):
    """Label vectors that between them put, on some row: ignore_index (row 0 and the last row), 0, V - 1, and for
    every multiple c of 128 below V both c and c - 1 (every tile or split boundary, whatever the split count); the
    other rows are uniform."""
    need = [0, V - 1] + [v for c in range(128, V, 128) for v in (c, c - 1)]
    g = torch.Generator().manual_seed(seed)
    per = M - 2
    out = []
    for s in range(0, len(need), per):
        lab = torch.randint(0, V, (M,), generator=g)
        chunk = need[s:s + per]
        lab[1:1 + len(chunk)] = torch.tensor(chunk)
        lab[0] = lab[M - 1] = IGN
        out.append(lab)
    return out


def check_rows(M, V, Kd, labels, rows, lse):
    ref, valid = ref_rows(M, V, Kd, labels)
    lse_ref = case(M, V, Kd)[4]
    rows, lse = rows.double().cpu(), lse.double().cpu()
    err = (rows - ref).abs()
    bound = 1e-4 * ref.abs().clamp(min=1.0)
    print(f"(M,V,K)=({M},{V},{Kd}): max loss err {err.max().item():.3e} (bound >= 1e-4), "
          f"max lse err {(lse - lse_ref).abs().max().item():.3e}")
    assert (err <= bound).all(), (err / bound).max()
    assert (rows[~valid] == 0).all()
    assert ((lse - lse_ref).abs() <= 1e-4 * lse_ref.abs().clamp(min=1.0)).all()
    return err[valid].mean().item()


@pytest.mark.parametrize("M,V,Kd", SHAPES)
def test_rows_match_fp64_at_every_label_placement_and_beat_the_bf16_logits_path(M, V, Kd):
    sets = label_sets(M, V)
    for n, labels in enumerate(sets):
        rows, lse, s, c, mean = run(M, V, Kd, labels)
        fused_err = check_rows(M, V, Kd, labels, rows, lse)
        ref, valid = ref_rows(M, V, Kd, labels)
        assert c.item() == valid.sum().item()
        tot = ref.sum().item()
        assert abs(s.item() - tot) <= 1e-4 * max(1.0, abs(tot))
        assert abs(mean.item() - tot / valid.sum().item()) <= 1e-4 * max(1.0, abs(tot) / valid.sum().item())
        if n:
            continue
        # the parent path on the same operands: bf16 logits in HBM, then the cross-entropy kernel
        x, w, w_rows, _, _ = case(M, V, Kd)
        logits = torch.empty(M, w_rows, dtype=torch.bfloat16, device=dev)
        K.gemm(K.FWD, K.EPI_BF16, M, w_rows, Kd, x, Kd, w, Kd, logits, w_rows)
        prow, plse = torch.empty(M, device=dev), torch.empty(M, device=dev)
        ploss, pinv = torch.empty((), device=dev), torch.empty(1, device=dev)
        K.xent_fwd(logits, w_rows, labels.to(dev), prow, plse, None, w_rows, M, V, ploss, pinv, ignore_index=IGN)
        parent_err = (prow.double().cpu() - ref).abs()[valid].mean().item()
        print(f"mean |row error| vs fp64: fused {fused_err:.3e}, bf16-logits path {parent_err:.3e}")
        assert fused_err <= parent_err


@pytest.mark.parametrize("M,V,Kd", SHAPES)
@pytest.mark.parametrize("bad", ["V", "-5"])
def test_a_bad_label_poisons_its_row_and_the_sums_only(M, V, Kd, bad):
    labels = label_sets(M, V)[0]
    good = run(M, V, Kd, labels)
    lab2 = labels.clone()
    lab2[9] = V if bad == "V" else -5  # (w_rows > V: row V of w exists and holds 100.0)
    rows, lse, s, c, mean = run(M, V, Kd, lab2)
    assert math.isnan(rows[9].item()) and math.isnan(s.item()) and math.isnan(mean.item())
    keep = torch.arange(M, device=dev) != 9
    assert torch.equal(rows[keep], good[0][keep]) and torch.equal(lse, good[1])
    assert c.item() == good[3].item()


@pytest.mark.parametrize("M,V,Kd", SHAPES)
def test_all_labels_ignored_gives_what_xent_fwd_gives(M, V, Kd):
    labels = torch.full((M,), IGN, dtype=torch.int64)
    rows, lse, s, c, mean = run(M, V, Kd, labels)
    x, w, w_rows, _, _ = case(M, V, Kd)
    logits = torch.zeros(M, w_rows, dtype=torch.bfloat16, device=dev)
    prow, plse = torch.empty(M, device=dev), torch.empty(M, device=dev)
    ploss, pinv = torch.empty((), device=dev), torch.empty(1, device=dev)
    K.xent_fwd(logits, w_rows, labels.to(dev), prow, plse, None, w_rows, M, V, ploss, pinv, ignore_index=IGN)
    assert torch.equal(mean.reshape(()), ploss) or (math.isnan(mean.item()) and math.isnan(ploss.item()))
    assert s.item() == prow.sum().item() == 0.0
    assert (1.0 / c).item() == pinv.item()  # count 0 <-> inv_count inf
    assert (rows == 0).all()
    check_rows(M, V, Kd, labels, rows, lse)


@pytest.mark.parametrize("M,V,Kd", SHAPES)
def test_two_calls_are_bit_identical(M, V, Kd):
    labels = label_sets(M, V)[0]
    a, b = run(M, V, Kd, labels), run(M, V, Kd, labels)
    for i in (0, 1, 2, 3, 4):
        assert torch.equal(a[i], b[i]), i


@pytest.mark.parametrize("M,V,Kd", SHAPES)
def test_accumulate_adds_this_call_to_the_running_sums(M, V, Kd):
    l1, l2 = label_sets(M, V, seed=5)[0], label_sets(M, V, seed=6)[0]
    l2[10:20] = IGN  # different counts
    a, b = run(M, V, Kd, l1), run(M, V, Kd, l2)
    s, c = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    run(M, V, Kd, l1, loss_sum=s, count=c, accumulate=True)
    r2 = run(M, V, Kd, l2, loss_sum=s, count=c, accumulate=True)
    want = a[2].double().item() + b[2].double().item()
    w32 = torch.tensor(want, dtype=torch.float32)
    ulp = (torch.nextafter(w32.abs(), torch.tensor(float("inf"))) - w32.abs()).item()  # one fp32 ulp at the sum
    assert abs(s.double().item() - want) <= ulp, (s.item(), want)
    assert c.item() == a[3].item() + b[3].item()
    assert torch.equal(r2[4], b[4])  # loss_mean is this call's alone


def test_argument_checks_run_before_any_launch():
    lib = K.load()

    def call(M=64, V=509, Kd=64, w_rows=512, ldx=None, ldw=None):
        return lib.gpt2mi_lm_loss(None, Kd if ldx is None else ldx, None, Kd if ldw is None else ldw, w_rows, None, M, V,
                                  Kd, IGN, None, None, None, None, 0, None, None, None)

    for kw, word in ((dict(M=96), b"M=96"), (dict(Kd=96), b"K=96"), (dict(V=0), b"V=0"), (dict(w_rows=508), b"w_rows"),
                     (dict(M=0), b"M=0"), (dict(ldx=32), b"stride"), (dict(), b"NULL")):
        assert call(**kw) == 22, kw
        assert word in lib.gpt2mi_last_error(), (kw, lib.gpt2mi_last_error())
    assert K.lm_loss_workspace(64, 509) > 0 and lib.gpt2mi_lm_loss_workspace(0, 509) == 0
