"""The deterministic mode's kernels (csrc/deterministic.hip, gpt2mi.h v24.7) through _lib against fp64 torch on the CPU.

Each replaces a kernel that adds the same fp32 terms with float atomics, so each is held to the bound the existing test
of that output uses (tests/test_row_kernels_gpu.py): sum_bound() for db, dbias_out, the column sums and dwte, and
max(sum_bound, LN_YARDSTICK_FACTOR x torch's own fp32 error) for dw. What the mode adds on top: two calls on the same
inputs give the same bits, and what the replaced kernel forms without atomics (dres, out, dwpe) keeps its bits.
Measured on the MI355X, error / bound: column sums <= 0.09; dwte 0.50 with every token once (one rounding), 0.50-0.51 for
the Zipf draw, <= 0.011 for one or two tokens everywhere; dw at M = 2051, C = 768: 2.8e-5 against fp64 (torch's own fp32
error 4.0e-5), 8.4e-5 between the ordered and the atomic kernel."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from tests.test_decode_kernels_gpu import BF16, bits
from tests.test_row_kernels_gpu import (SLACK, U, _check_ln_backward, _ln_backward, _ln_case, _ln_forward,
                                        check_elements, dropout_f32, sentinel, sum_bound, untouched)

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "f32"])


@pytest.fixture(scope="module", autouse=True)
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


def workspace(K, rows, C, N):
    return torch.empty(K.det_workspace_bytes(1, rows, C, N), dtype=torch.uint8, device=dev)


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@DTYPES
@pytest.mark.parametrize("N", [192, 768])
@pytest.mark.parametrize("M", [1, 37, 1000])
def test_colsum_det(K, M, N, dtype):
    """One row, one part-filled chunk, many chunks (8 rows each at these widths); a slice of a wider buffer; entries
    scaled by powers of two over +-12 so that the order of the sum shows in the low bits."""
    g = torch.Generator().manual_seed(M * N)
    ld = N + 8
    buf = torch.full((M, ld), math.nan)
    buf[:, :N] = torch.randn(M, N, generator=g) * torch.exp2(torch.randint(-12, 13, (M, N), generator=g).float())
    buf = buf.to(dtype)
    db0 = torch.randn(N, generator=g) + 3.0
    ws = workspace(K, M, N, N)
    runs = []
    for _ in range(2):
        db = sentinel(N + SLACK)
        db[:N] = db0.to(dev)
        K.colsum_det(buf.to(dev), db, M, N, ld, ws)
        torch.cuda.synchronize()
        runs.append(db)
    a = buf[:, :N].double()
    ref = db0.double() + a.sum(0)
    worst = check_elements("colsum_det", runs[0][:N], ref, sum_bound(M + 1, db0.double().abs() + a.abs().sum(0), ref))
    assert untouched(runs[0][N:]), "db written past N"
    assert torch.equal(bits(runs[0]), bits(runs[1])), "two calls differ"
    print(f"colsum_det M={M} N={N}: err/bound {worst:.3f}")


# (with out, p_out, dres_init); p_out means nothing without out
LN_OPTIONS = [(True, 0.0, False), (True, 0.0, True), (True, 0.1, False), (True, 0.1, True), (False, 0.0, False),
              (False, 0.0, True)]


@DTYPES
@pytest.mark.parametrize("want_out,p_out,dres_init", LN_OPTIONS)
@pytest.mark.parametrize("M", [5, 2051])
@pytest.mark.parametrize("C", [64, 768, 1600])
def test_layernorm_bwd_det(K, C, M, want_out, p_out, dres_init, dtype):
    """The three VEC classes (1600 is X(1, 25)); fewer rows than two blocks' waves, and 512 blocks with a ragged second
    trip. Measured on the MI355X, dw error against the atomic kernel's on the same inputs: see DESIGN.md §13."""
    c = _ln_case(M, C, "spread", f32_dy=dtype == torch.float32)
    _, _, mean, rstd = _ln_forward(K, c)
    seed = 0x1234_5678_9ABC
    kw = dict(p_out=p_out, seed_out=seed, dres_init=dres_init, want_out=want_out,
              dres_fill=torch.full((M, C), math.nan) if dres_init else None)
    det = SimpleNamespace(layernorm_bwd=functools.partial(K.layernorm_bwd_det, workspace=workspace(K, M, C, C)))
    atomic = _ln_backward(K, c, mean[:M], rstd[:M], **kw)
    first, second = (_ln_backward(det, c, mean[:M], rstd[:M], **kw) for _ in range(2))
    _check_ln_backward(c, first, "det", p_out=p_out, seed_out=seed, dres_ref=c["dx"] if dres_init else None)
    assert same_bits(first, second), "two calls differ"
    assert torch.equal(bits(first[0]), bits(atomic[0])), "dres is not layernorm_bwd's"
    assert first[3] is None or torch.equal(bits(first[3]), bits(atomic[3])), "out is not layernorm_bwd's"
    print(f"ln_bwd_det M={M} C={C}: max |dw - atomic dw| {float((first[1][:C] - atomic[1][:C]).abs().max()):.3e}")


EMB_V, EMB_VP = 600, 640
PATTERNS = ["same", "distinct", "zipf", "ends"]


def _tokens(pattern, B, T, T_valid, g):
    n = B * T_valid
    if pattern == "same":  # one run through every chunk and the fix-up
        tok = torch.full((n,), 77)
    elif pattern == "distinct":  # no run crosses a chunk
        tok = torch.randperm(EMB_V, generator=g)[:n]
    elif pattern == "zipf":
        w = 1.0 / torch.arange(1, EMB_V + 1).double() ** 2
        tok = torch.multinomial(w, n, replacement=True, generator=g)
        rank = torch.sort(tok).values
        first = {int(t): i // 32 for i, t in reversed(list(enumerate(rank.tolist())))}
        last = {int(t): i // 32 for i, t in enumerate(rank.tolist())}
        assert max(last[t] - first[t] for t in last) >= 2, "the draw has no token whose run spans three chunks"
    else:
        tok = torch.where(torch.rand(n, generator=g) < 0.5, 0, EMB_V - 1)
    idx = torch.full((B, T), EMB_V - 2)  # padding positions: a token whose row must stay untouched if absent
    idx[:, :T_valid] = tok.view(B, T_valid)
    return idx


@pytest.mark.parametrize("doc", [False, True], ids=["abs", "doc"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,T_valid,C", [(3, 64, 50, 64), (4, 128, 128, 768)])
def test_embed_bwd_det(K, B, T, T_valid, C, p, pattern, doc):
    g = torch.Generator().manual_seed(B * T + C + PATTERNS.index(pattern))
    seed = 0xABCD_0000_0000 + C
    idx = _tokens(pattern, B, T, T_valid, g)
    valid = (torch.arange(T) < T_valid).repeat(B)
    dres = torch.randn(B * T, C, generator=g)
    dres[~valid] = math.nan  # never read
    start = ((torch.arange(T) // 7) * 7).to(torch.int32).repeat(B, 1).contiguous()
    dwte0 = torch.randn(EMB_V, C, generator=g) + 2.0
    dwpe0 = torch.randn(T_valid, C, generator=g) - 2.0
    ws = workspace(K, B * T, C, C)

    def run(det):
        dwte = sentinel(EMB_VP * C)  # the pad rows V..Vp hold the sentinel
        dwte[:EMB_V * C] = dwte0.to(dev).reshape(-1)
        dwpe = sentinel(T * C + SLACK)
        dwpe[:T_valid * C] = dwpe0.to(dev).reshape(-1)
        head = (idx.to(dev), dres.to(dev), dwte, dwpe) + ((start.to(dev),) if doc else ())
        fn = getattr(K, "embed_bwd" + ("_doc" if doc else "") + ("_det" if det else ""))
        fn(*head, B, T, C, p, seed, T_valid=T_valid, **({"workspace": ws} if det else {}))
        torch.cuda.synchronize()
        return dwte, dwpe

    (te, pe), (te2, pe2), (_, pe_atomic) = run(True), run(True), run(False)
    assert torch.equal(bits(te), bits(te2)) and torch.equal(bits(pe), bits(pe2)), "two calls differ"
    assert torch.equal(bits(pe), bits(pe_atomic)), "dwpe is not the existing entry's"
    add = dropout_f32(torch.nan_to_num(dres), seed, p).double()
    add[~valid] = 0.0
    flat = idx.reshape(-1)
    ref = dwte0.double().index_add(0, flat, add)
    mag = dwte0.double().abs().index_add(0, flat, add.abs())
    count = torch.bincount(flat[valid], minlength=EMB_V).double()[:, None]
    got = te[:EMB_V * C].view(EMB_V, C).cpu()
    worst = check_elements("dwte", got, ref, count * U * mag + U * ref.abs())
    assert torch.equal(bits(got[count[:, 0] == 0]), bits(dwte0[count[:, 0] == 0])), "rows of absent tokens changed"
    assert untouched(te[EMB_V * C:]) and untouched(pe[T_valid * C:]), "pad rows of dwte / rows of dwpe past T_valid"
    assert not bool(torch.isnan(pe[:T_valid * C]).any())
    print(f"embed_bwd_det {pattern} doc={doc} B={B} T_valid={T_valid} C={C} p={p}: dwte err/bound {worst:.3f}")
