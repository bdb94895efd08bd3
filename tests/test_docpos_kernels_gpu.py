"""The embedding kernels with positions per document (csrc/norm_embed.hip: gpt2mi_embed_fwd_doc / gpt2mi_embed_bwd_doc)
by the method of tests/test_row_kernels_gpu.py::_embed_case: fp64 references on the same rounded inputs, the forward
bitwise, every sum within Higham's bound for its own number of addends, NaN in everything a kernel must not read
(``wpe`` from the longest document's length on, the wte row of the padding tokens, the padding rows of ``dres``) and
sentinels behind everything it must not write. ``dwpe`` is also compared bit for bit between two calls."""
import math

import pytest
import torch

from gpt_2_distributed_amd import packing as P
from tests import docmask_helpers as H
from tests import docpos_helpers as D
from tests.test_row_kernels_gpu import (EMB_POISON, EMB_T, EMB_V, SLACK, U, bits, check_elements, dropout_f32, sentinel,
                                        sum_bound, untouched)

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(scope="module", autouse=True)
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


def _inputs(B, C, T, T_valid, rows):
    V = EMB_V
    g = torch.Generator().manual_seed(B * 1000 + C + T_valid)
    bounds = D.padded_bounds(rows, T)
    pos = P.doc_positions(bounds).long()
    Lmax = max(max(r) for r in rows)
    idx = torch.randint(0, V - 1, (B, T), generator=g)
    idx[:, T_valid:] = EMB_POISON
    wte, wpe = torch.randn(V, C, generator=g), torch.randn(T, C, generator=g)
    wte[EMB_POISON] = math.nan
    wpe[Lmax:] = math.nan
    valid = torch.zeros(B, T, dtype=torch.bool)
    valid[:, :T_valid] = True
    dres = torch.randn(B * T, C, generator=g)
    dres[~valid.reshape(-1)] = math.nan
    dwte0 = torch.randn(V, C, generator=g) + 2.0
    dwpe0 = torch.randn(T, C, generator=g) - 2.0
    dwpe0[Lmax:, 0] = -0.0  # an untouched row keeps its bits; one that had 0.0 added would not
    return dict(bounds=bounds, pos=pos, Lmax=Lmax, idx=idx, wte=wte, wpe=wpe, valid=valid.reshape(-1), dres=dres,
                dwte0=dwte0, dwpe0=dwpe0, g=g)


def _backward(K, c, B, C, T, T_valid, p, seed, start, fn=None):
    V = EMB_V
    dwte = sentinel(V * C + SLACK)
    dwte[:V * C] = c["dwte0"].to(dev).reshape(-1)
    dwpe = sentinel(T * C + SLACK)
    dwpe[:T_valid * C] = c["dwpe0"][:T_valid].to(dev).reshape(-1)
    if fn is None:
        K.embed_bwd_doc(c["idx"].to(dev), c["dres"].to(dev), dwte, dwpe, start, B, T, C, p, seed, T_valid=T_valid)
    else:
        fn(c["idx"].to(dev), c["dres"].to(dev), dwte, dwpe, B, T, C, p, seed, T_valid=T_valid)
    torch.cuda.synchronize()
    return dwte, dwpe


def _doc_case(K, B, C, T_valid, p, rows, T=EMB_T, also_plain=False):
    V = EMB_V
    seed = 0xABCD_0000_0000 + 97 * B + C
    c = _inputs(B, C, T, T_valid, rows)
    idx, wte, wpe, valid, pos, Lmax = c["idx"], c["wte"], c["wpe"], c["valid"], c["pos"], c["Lmax"]
    start = c["bounds"].start.to(dev)
    # forward: x = drop(wte[idx] + wpe[pos]) in fp32, bitwise; exact zeros in the padding rows
    x = sentinel(B * T * C + SLACK)
    K.embed_fwd_doc(idx.to(dev), wte.to(dev), wpe.to(dev), x, start, B, T, C, p, seed, T_valid=T_valid)
    torch.cuda.synchronize()
    want = dropout_f32((wte[idx] + wpe[pos]).reshape(B * T, C), seed, p)
    want[~valid] = 0.0
    assert not bool(torch.isnan(want).any())
    assert torch.equal(bits(x[:B * T * C].view(B * T, C).cpu()), bits(want)), "embed_fwd_doc"
    assert untouched(x[B * T * C:]), "x written past B*T*C"
    # backward: dwte[idx] += g, dwpe[p] += the sum of g over the rows at position p, g = drop(dres)
    dwte, dwpe = _backward(K, c, B, C, T, T_valid, p, seed, start)
    add = dropout_f32(torch.nan_to_num(c["dres"]), seed, p).double()  # the fp32 addends, exact in fp64
    add[~valid] = 0.0
    flat = idx.reshape(-1)
    dwte0, dwpe0 = c["dwte0"], c["dwpe0"]
    ref_te = dwte0.double().index_add(0, flat, add)
    abs_te = dwte0.double().abs().index_add(0, flat, add.abs())
    n_te = 1 + torch.bincount(flat[valid], minlength=V).double()[:, None].expand(V, C)
    got_te = dwte[:V * C].view(V, C).cpu()
    w_te = check_elements("dwte", got_te, ref_te, (n_te - 1) * U * abs_te + U * ref_te.abs())
    hit = torch.zeros(V, dtype=torch.bool)
    hit[flat[valid]] = True
    assert torch.equal(bits(got_te[~hit]), bits(dwte0[~hit])), "dwte rows of absent tokens changed"
    pflat = pos.reshape(-1)[valid]
    assert int(pflat.max()) == Lmax - 1
    ref_pe = dwpe0[:T_valid].double().index_add(0, pflat, add[valid])
    abs_pe = dwpe0[:T_valid].double().abs().index_add(0, pflat, add[valid].abs())
    n_pe = torch.bincount(pflat, minlength=T_valid).double()[:, None].expand(T_valid, C)
    got_pe = dwpe[:T_valid * C].view(T_valid, C).cpu()
    w_pe = check_elements("dwpe", got_pe[:Lmax], ref_pe[:Lmax], sum_bound(n_pe[:Lmax] + 1, abs_pe[:Lmax], ref_pe[:Lmax]))
    assert torch.equal(bits(got_pe[Lmax:]), bits(dwpe0[Lmax:T_valid])), "dwpe rows from the longest document on changed"
    assert untouched(dwpe[T_valid * C:]), "dwpe rows from T_valid on changed"
    assert untouched(dwte[V * C:]), "dwte written past V*C"
    # a second call on the same inputs: dwpe bit for bit
    _, again = _backward(K, c, B, C, T, T_valid, p, seed, start)
    assert torch.equal(bits(again.cpu()), bits(dwpe.cpu())), "dwpe differs between two calls"
    if also_plain:  # one document per row: the plain entries compute the same thing
        assert Lmax == T_valid
        xp = sentinel(B * T * C + SLACK)
        K.embed_fwd(idx.to(dev), wte.to(dev), wpe.to(dev), xp, B, T, C, p, seed, T_valid=T_valid)
        torch.cuda.synchronize()
        assert torch.equal(bits(xp.cpu()), bits(x.cpu())), "embed_fwd_doc differs from embed_fwd on one document per row"
        _, plain = _backward(K, c, B, C, T, T_valid, p, seed, None, fn=K.embed_bwd)
        check_elements("dwpe (embed_bwd)", plain[:T_valid * C].view(T_valid, C), ref_pe,
                       sum_bound(n_pe + 1, abs_pe, ref_pe))
    return w_te, w_pe


# (B, first layout): row b of the batch takes layout first + b of docpos_helpers.LAYOUT_NAMES, so every layout is met
# alone (B = 1), the rows of a batch hold unequal document counts, and the walk meets B = 3, 5, 8
BATCHES = [(1, n) for n in D.LAYOUT_NAMES] + [(3, "one"), (3, "tail1"), (5, "ones"), (8, "mixed")]


@pytest.mark.parametrize("C", [64, 384, 768, 1600])
def test_embedding_with_positions_per_document(K, C):
    for B, first in BATCHES:
        for T_valid in (24, 17, 1):
            for p in (0.0, 0.1):
                rows = D.batch_layouts(B, T_valid, first)
                w_te, w_pe = _doc_case(K, B, C, T_valid, p, rows)
                print(f"embed_doc C={C} B={B} from {first} T_valid={T_valid} p={p}: err/bound dwte {w_te:.3f} "
                      f"dwpe {w_pe:.3f}")


@pytest.mark.parametrize("C", [64, 384, 768, 1600])
def test_one_document_per_row_is_the_plain_embedding(K, C):
    for B in (1, 3, 5, 8):
        for T_valid in (24, 17, 1):
            for p in (0.0, 0.1):
                _doc_case(K, B, C, T_valid, p, [(T_valid,)] * B, also_plain=True)


@pytest.mark.parametrize("fill", [EMB_T + 5, -3])
def test_contract_breaking_bounds_stay_in_range(K, fill):
    """start = T + 5 (clamped to t: every token at position 0) and start = -3 (clamped to 0: absolute positions): the
    calls complete and write nothing outside their buffers. Values are not checked."""
    B, C, T, T_valid, V = 3, 384, EMB_T, 17, EMB_V
    c = _inputs(B, C, T, T_valid, [(T_valid,)] * B)
    start = torch.full((B, T), fill, dtype=torch.int32, device=dev)
    x = sentinel(B * T * C + SLACK)
    K.embed_fwd_doc(c["idx"].to(dev), c["wte"].to(dev), c["wpe"].to(dev), x, start, B, T, C, 0.1, 5, T_valid=T_valid)
    dwte, dwpe = _backward(K, c, B, C, T, T_valid, 0.1, 5, start)
    assert untouched(x[B * T * C:]) and untouched(dwte[V * C:]) and untouched(dwpe[T_valid * C:])
    assert not untouched(x[:B * T * C])


def test_a_long_row_of_random_documents(K):
    """B = 2, T = 1024, C = 128, documents of mean length 64, p = 0.1: the second trips of the backward's scan and of
    its list, with the checks of the small cases."""
    T = 1024
    rows = [H.random_lengths(T, 64, seed=21), H.random_lengths(T, 64, seed=22)]
    assert rows[0] != rows[1] and min(len(r) for r in rows) > 4
    w_te, w_pe = _doc_case(K, 2, 128, T, 0.1, rows, T=T)
    print(f"embed_doc T=1024 mean 64: err/bound dwte {w_te:.3f} dwpe {w_pe:.3f}")


def test_every_token_a_document_of_its_own(K):
    """The worst case: B x T addends land on dwpe[0], in bounded time, and pass the bound."""
    T = 1024
    w_te, w_pe = _doc_case(K, 4, 64, T, 0.1, [(1,) * T] * 4, T=T)
    print(f"embed_doc T=1024 all ones: err/bound dwte {w_te:.3f} dwpe {w_pe:.3f}")
