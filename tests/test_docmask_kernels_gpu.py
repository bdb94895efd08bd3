"""The document-masking kernels on the MI355X: gpt2mi_doc_bounds (csrc/packing.hip) and the ``_doc`` entries of
csrc/attention.hip and csrc/fp32.hip, against gpt_2_distributed_amd/packing.py.

Bounds follow tests/test_attention_edges_gpu.py and come from the reference alone, never from the kernel's result: for
the bf16 kernels 3 x the worst 32-row block error of ``docmask_helpers.doc_bf16_model`` (attn_stress.bf16_model
restated with the document mask) on the same input and tensor, bf16 lse 2^-8 + 1e-4 absolute; for the fp32 kernels
4 x the block error of plain fp32 torch on the CPU, lse 1e-4. Every figure is printed before it is asserted.

The three layouts of a T = 320 row (docmask_helpers.LAYOUTS; row 1 of B = 2 reversed, H = 3) each hit one place the
kernels can go wrong: L1 a length-1 document, boundaries on a 16-query group, a 32-query wave, a 64-key tile and one key
before a 128-query block, and a last block that skips tiles 0-2; L2 a wave whose two 16-query groups lie in different
documents, so a whole group sees no key in a visited tile (the -inf - -inf case of the forward); L3 a boundary inside
a 16-query group.

Measured on the MI355X (ratio = kernel / yardstick on the same case, worst case over layouts and p named):
  test_masked_attention_against_the_reference  bf16 out <= 1.08 (random p=0), dq / dk / dv <= 1.00 (2.5e-3..7.3e-3);
                                               fp32 out <= 1.38, dq <= 1.86 (L3 p=0), dk <= 1.93 (L2 p=0.1), dv <= 1.83
                                               (kernel 2.7e-7..5.5e-7); fp32 lse <= 9.6e-7
  test_scores_of_other_documents_overflow_...  bf16 ratios <= 1.02; fp32 dq 1.56 / 1.26, dk 1.41 / 1.88 (p = 0 / 0.1)
  test_masked_backward_bias_gradient_partials  colsum vs the stored 32-row sums 2.7e-9 / 1.4e-9
  test_one_document_per_row_...                exact: no element differs"""
import pytest
import torch

from gpt_2_distributed_amd import packing as P
from oracle import attn_stress as A
from tests import docmask_helpers as H
from tests.docmask_helpers import EOT, bounds_rows

pytestmark = pytest.mark.gpu

dev = "cuda"
D = 64
LSE_BOUND = {False: 2.0 ** -8 + 1e-4, True: 1e-4}  # by f32
MARGIN = {False: 3.0, True: 4.0}


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


def _act(x, f32):
    return (x.float() if f32 else x.to(torch.bfloat16)).contiguous().to(dev)


def _dev_bounds(b):
    return P.DocBounds(b.start.to(dev).contiguous(), b.end.to(dev).contiguous())


def _run(qkv, dO, B, T, H, p, seed, f32, doc, colsum=None):
    """forward + backward through the bindings -> device tensors out, lse, delta, dqkv (doc None: unmasked entries)."""
    C = H * D
    qd, dod = _act(qkv, f32), _act(A.merge(dO), f32)
    out = torch.empty(B * T, C, dtype=qd.dtype, device=dev)
    lse, delta = torch.empty(B * H, T, device=dev), torch.empty(B * H, T, device=dev)
    dqkv = torch.empty(B * T, 3 * C, dtype=qd.dtype, device=dev)
    L().attn_fwd(qd, out, lse, B, T, H, D, p, seed, doc=doc)
    L().attn_bwd(qd, out, dod, lse, delta, dqkv, B, T, H, D, p, seed, colsum=colsum, doc=doc)
    torch.cuda.synchronize()
    return out, lse, delta, dqkv


def _cpu(out, lse, dqkv, B, T, H):
    got = {"out": A.unmerge(out.cpu().float(), B, T, H), "lse": lse.cpu().view(B, H, T)}
    got["dq"], got["dk"], got["dv"] = A.split(dqkv.cpu().float(), B, T, H)
    return got


def _judge(label, c, got, f32):
    bad = []
    for n in ("out", "lse", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[n]).all()), f"{label}: {n} holds NaN or inf"
        if n == "lse":
            err, bound = float((got[n].double() - c["ref"][n]).abs().max()), LSE_BOUND[f32]
            print(f"DOC {label} lse: worst |d lse| {err:.3e} (model {c['model_err'][n]:.3e}, bound {bound:.3e})")
        else:
            e = A.block_err(got[n], c["ref"][n])
            err, bound = float(e.max()), MARGIN[f32] * c["model_err"][n]
            print(f"DOC {label} {n}: kernel {err:.3e} model {c['model_err'][n]:.3e} ratio "
                  f"{err / c['model_err'][n]:.2f} (worst block {tuple(int(i) for i in (e == e.max()).nonzero()[0])})")
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, f"{label}: (tensor, worst error, bound) {bad}"


# ---- 1. the bounds kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eot", ["end", "begin"])
@pytest.mark.parametrize("T,T_valid", [(64, 64), (192, 150), (1024, 1024)])
def test_doc_bounds_kernel_equals_the_reference(T, T_valid, eot):
    """gpt2mi_doc_bounds gives doc_bounds_reference's integers: B = 3 seeded rows with about one separator in 20 tokens
    (also at position 0, at T_valid - 1 and just past T_valid), and the hand-made rows of the CPU test (no separator,
    one at either end, consecutive, all). Fails if a chunk's scan value, the padding document or a convention is off
    by one anywhere."""
    g = torch.Generator().manual_seed(5 + T)
    idx = torch.randint(0, 20, (3, T), generator=g)
    idx[idx == EOT] = 19
    idx[torch.rand(3, T, generator=g) < 0.05] = EOT
    idx[0, 0] = idx[1, T_valid - 1] = EOT
    idx[2] = 3  # no separator at all
    if T_valid < T:
        idx[:, T_valid] = EOT  # a separator in the padding must not count
    for rows, tv in ((idx, T_valid), (bounds_rows(), None), (bounds_rows(), 11)):
        want = P.doc_bounds_reference(rows, EOT, eot, tv)
        got = P.doc_bounds(rows.to(dev), EOT, eot, tv)
        torch.cuda.synchronize()
        assert got.start.dtype == torch.int32 and got.start.shape == rows.shape
        assert torch.equal(got.start.cpu(), want.start) and torch.equal(got.end.cpu(), want.end)
        on_dev = P.doc_bounds_reference(rows.to(dev), EOT, eot, tv)  # the reference runs on any device
        assert torch.equal(on_dev.start.cpu(), want.start) and torch.equal(on_dev.end.cpu(), want.end)


# ---- 2. forward and backward against the reference ------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", ["L1", "L2", "L3", "random"])
def test_masked_attention_against_the_reference(layout, p, f32):
    """out, lse, dq, dk, dv of the _doc entries against doc_attention_reference per 32-row block, under the kernels' own
    dropout mask restated by dropout_ref (a wrong dropout index is an O(1) error), all finite. `random`: T = 1024,
    B = 1, seeded document lengths of mean about 100. Fails if a tile is skipped that holds a visible key, a boundary
    tile runs unmasked, a masked row's -inf reaches an exponent as -inf - -inf (NaN in out of L2), or the loop bounds of
    a block start past / end before its documents."""
    c = H.case(layout, p, f32)
    B, T, Hh = c["B"], c["T"], c["H"]
    out, lse, _, dqkv = _run(c["qkv"], c["dO"], B, T, Hh, p, c["seed"], f32, _dev_bounds(c["bounds"]))
    _judge(f"{'f32' if f32 else 'bf16'} {layout} p={p}", c, _cpu(out, lse, dqkv, B, T, Hh), f32)


# ---- 3. one document per row is the unmasked kernel -----------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T", [320, 1024])
def test_one_document_per_row_equals_the_unmasked_entries_bit_for_bit(T, p, f32):
    """start = 0, end = T: out, lse, delta and dqkv of the _doc entries equal those of the unmasked entries bit for bit
    (the masked forward starts its running max at a finite value instead of -inf; the first rescale multiplies zeros
    either way)."""
    B, Hh = 2 if T == 320 else 1, 3
    seed = A.SEED_HI if p > 0 else A.SEED_LO
    qkv, dO = A.build("plain", B, T, Hh), A.grad_out(B, T, Hh)
    plain = _run(qkv, dO, B, T, Hh, p, seed, f32, None)
    masked = _run(qkv, dO, B, T, Hh, p, seed, f32, _dev_bounds(H.single_document(B, T)))
    for name, a, b in zip(("out", "lse", "delta", "dqkv"), plain, masked):
        assert bool(torch.isfinite(b.float()).all()), name
        worst = float((a.float() - b.float()).abs().max())
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ, worst {worst:.3e}"


# ---- 4. overflow before masking -------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_scores_of_other_documents_overflow_before_they_are_masked(p, f32):
    """L2 with the first document's keys scaled so that the second document's queries score 100 nats against every
    other one of them (in-document scores stay O(1); docmask_helpers.overflow_qkv says why the signs alternate): the
    backward's recomputed exp2(s - lse) of those pairs is +inf, so a mask applied as a multiply by 0 gives NaN in
    dq / dk / dv. dQ meets them in row 0 (queries 32..79 against tile 0), dK/dV in row 1 (the one-token document at 127
    against the keys of its wave). Everything finite and within the bounds of test 2."""
    c = H.case("L2", p, f32, overflow=True)
    B, T, Hh = c["B"], c["T"], c["H"]
    q, k, _ = (t.float() for t in A.split(c["qkv"], B, T, Hh))
    s = (q @ k.transpose(-2, -1)) / 8.0
    e0 = int(c["bounds"].end[0, 0])
    assert float(s[0, :, e0:int(c["bounds"].end[0, e0]), 0:e0:2].min()) > 89.0   # exp overflows fp32 above 88.7 nats
    assert float(s.masked_fill(~P.doc_mask(c["bounds"])[:, None], 0.0).abs().max()) < 12.0
    out, lse, _, dqkv = _run(c["qkv"], c["dO"], B, T, Hh, p, c["seed"], f32, _dev_bounds(c["bounds"]))
    _judge(f"overflow {'f32' if f32 else 'bf16'} p={p}", c, _cpu(out, lse, dqkv, B, T, Hh), f32)


# ---- 5. the fused bias-gradient partials ----------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_masked_backward_bias_gradient_partials(p):
    """The dqkv_colsum partials of gpt2mi_attn_bwd_doc equal the 32-row column sums of the stored dqkv, and requesting
    them leaves dqkv unchanged (the assertion of test_attention_bwd_fused_bias_grad_partials), on L1."""
    c = H.case("L1", p)
    B, T, Hh = c["B"], c["T"], c["H"]
    C = Hh * D
    doc = _dev_bounds(c["bounds"])
    d1 = _run(c["qkv"], c["dO"], B, T, Hh, p, c["seed"], False, doc)[3]
    cs = torch.full((B * T // 32, 3 * C), float("nan"), device=dev)
    d2 = _run(c["qkv"], c["dO"], B, T, Hh, p, c["seed"], False, doc, colsum=cs)[3]
    assert torch.equal(d1, d2), "dqkv changes when the bias-gradient partials are requested"
    sums = d1.float().view(B * T // 32, 32, 3 * C).sum(1).double()
    cerr = float((cs.double() - sums).norm() / sums.norm())
    print(f"DOC colsum p={p}: rel err {cerr:.3e}")
    assert cerr < 1e-5, cerr


# ---- 6. argument errors ---------------------------------------------------------------------------------------------
def test_doc_entries_reject_bad_arguments():
    """NULL bounds, T = 96 and head_dim = 32 are refused with an error code before any launch, forward and backward,
    both families; the buffers are sized for the next valid shape, so a missing check could not write out of bounds."""
    KernelError = L().KernelError
    B, Hh, T = 1, 1, 128
    good = _dev_bounds(H.single_document(B, T))
    for dtype in (torch.bfloat16, torch.float32):
        qd = torch.zeros(B * T, 3 * Hh * D, dtype=dtype, device=dev)
        out = torch.zeros(B * T, Hh * D, dtype=dtype, device=dev)
        dod = torch.zeros(B * T, Hh * D, dtype=dtype, device=dev)
        dqkv = torch.full_like(qd, 3.0)
        lse, delta = torch.zeros(B * Hh, T, device=dev), torch.zeros(B * Hh, T, device=dev)
        for doc in (P.DocBounds(None, None), P.DocBounds(None, good.end), P.DocBounds(good.start, None)):
            if doc.start is None:
                with pytest.raises(KernelError, match="NULL"):
                    L().attn_fwd(qd, out, lse, B, T, Hh, D, doc=doc)
            with pytest.raises(KernelError, match="NULL"):
                L().attn_bwd(qd, out, dod, lse, delta, dqkv, B, T, Hh, D, doc=doc)
        for Tb, Db in ((96, 64), (128, 32)):
            doc = _dev_bounds(H.single_document(B, Tb))
            with pytest.raises(KernelError):
                L().attn_fwd(qd, out, lse, B, Tb, Hh, Db, doc=doc)
            with pytest.raises(KernelError):
                L().attn_bwd(qd, out, dod, lse, delta, dqkv, B, Tb, Hh, Db, doc=doc)
        with pytest.raises(KernelError, match="int32"):
            L().attn_fwd(qd, out, lse, B, T, Hh, D, doc=P.DocBounds(good.start.long(), good.end))
        torch.cuda.synchronize()
        assert bool((dqkv == 3.0).all()) and bool((out == 0).all()), "a refused call launched"
    idx = torch.zeros(2, 64, dtype=torch.long, device=dev)
    s, e = torch.zeros(2, 64, dtype=torch.int32, device=dev), torch.zeros(2, 64, dtype=torch.int32, device=dev)
    with pytest.raises(KernelError):
        L().doc_bounds(idx, 1, False, s, e, T_valid=65)
    with pytest.raises(KernelError, match="NULL"):
        L().doc_bounds(idx, 1, False, None, e)
    torch.cuda.synchronize()
