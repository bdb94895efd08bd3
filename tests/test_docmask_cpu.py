"""Document masking on the CPU: the rule of gpt_2_distributed_amd/packing.py (bounds from tokens on both separator
conventions, bounds from document ids, the validator), that the masked reference attention means "each document on its
own", the v24.5 C ABI, and the argument checks of the public surface and of the two command lines. No GPU."""
import os

import pytest
import torch

from gpt_2_distributed_amd import packing as P
from oracle import attn_stress as A
from tests import docmask_helpers as H
from tests.conftest import REPO
from tests.docmask_helpers import EOT, bounds_rows

NEW = ("gpt2mi_doc_bounds", "gpt2mi_attn_fwd_doc", "gpt2mi_attn_bwd_doc", "gpt2mi_attn_fwd_f32_doc",
       "gpt2mi_attn_bwd_f32_doc")


def brute_bounds(idx, eot, T_valid=None):
    """The issue's formulas, position by position."""
    B, T = idx.shape
    tv = T if T_valid is None else T_valid
    start, end = torch.zeros(B, T, dtype=torch.int32), torch.zeros(B, T, dtype=torch.int32)
    for b in range(B):
        sep = [s for s in range(tv) if int(idx[b, s]) == EOT]
        for t in range(T):
            if t >= tv:
                start[b, t], end[b, t] = tv, T
            elif eot == "end":
                start[b, t] = 1 + max([s for s in sep if s < t], default=-1)
                end[b, t] = min(1 + min([s for s in sep if s >= t], default=tv - 1), tv)
            else:
                start[b, t] = max([s for s in sep if s <= t], default=0)
                end[b, t] = min([s for s in sep if s > t], default=tv)
    return start, end


@pytest.mark.parametrize("T_valid", [None, 11])
@pytest.mark.parametrize("eot", ["end", "begin"])
def test_bounds_reference_on_both_conventions(eot, T_valid):
    idx = bounds_rows()
    got = P.doc_bounds_reference(idx, EOT, eot, T_valid)
    want = brute_bounds(idx, eot, T_valid)
    assert got.start.dtype == got.end.dtype == torch.int32 and got.start.is_contiguous() and got.end.is_contiguous()
    assert torch.equal(got.start, want[0]), (got.start, want[0])
    assert torch.equal(got.end, want[1]), (got.end, want[1])
    P.check_bounds(got)  # the reference produces what the validator accepts, padding document included
    if T_valid is not None:
        assert (got.start[:, T_valid:] == T_valid).all() and (got.end[:, T_valid:] == 16).all()
        assert (got.end[:, :T_valid] <= T_valid).all()


def test_bounds_reference_examples():
    idx = torch.tensor([[5, EOT, 1, EOT, EOT, 9]])
    e = P.doc_bounds_reference(idx, EOT, "end")
    assert e.start.tolist() == [[0, 0, 2, 2, 4, 5]] and e.end.tolist() == [[2, 2, 4, 4, 5, 6]]
    b = P.doc_bounds_reference(idx, EOT, "begin")
    assert b.start.tolist() == [[0, 1, 1, 3, 4, 4]] and b.end.tolist() == [[1, 3, 3, 4, 6, 6]]
    with pytest.raises(ValueError):
        P.doc_bounds_reference(idx, EOT, "middle")
    with pytest.raises(ValueError):
        P.doc_bounds_reference(idx, EOT, T_valid=7)
    with pytest.raises(ValueError):
        P.doc_bounds(idx, EOT)  # the kernel form takes device tensors


def test_bounds_from_ids_and_the_validator():
    for eot in ("end", "begin"):
        ref = P.doc_bounds_reference(bounds_rows(), EOT, eot)
        # document ids from the bounds: the start of each position's document
        ids = P.doc_bounds_from_ids(ref.start.long())
        assert torch.equal(ids.start, ref.start) and torch.equal(ids.end, ref.end)
        P.check_bounds(ref)
    with pytest.raises(ValueError, match="contiguous"):
        P.doc_bounds_from_ids(torch.tensor([[0, 0, 1, 0]]))
    with pytest.raises(ValueError):
        P.doc_bounds_from_ids(torch.zeros(4))
    good = H.bounds_from_lengths([(3, 2, 3)])
    P.check_bounds(good)

    def broken(which, t, value):
        s, e = good.start.clone(), good.end.clone()
        (s if which == "start" else e)[0, t] = value
        return P.DocBounds(s, e)
    with pytest.raises(ValueError, match="start"):
        P.check_bounds(broken("start", 1, 2))          # start > t
    with pytest.raises(ValueError, match="end"):
        P.check_bounds(broken("end", 4, 4))            # end <= t
    with pytest.raises(ValueError, match="constant"):
        P.check_bounds(broken("start", 4, 4))          # not constant over [3, 5)
    with pytest.raises(ValueError, match="constant"):
        P.check_bounds(broken("end", 0, 8))            # not constant over [0, 3)
    with pytest.raises(ValueError, match="int32"):
        P.check_bounds(P.DocBounds(good.start.long(), good.end))
    with pytest.raises(ValueError, match="shape"):
        P.check_bounds(P.DocBounds(good.start, good.end[:, :7]))
    with pytest.raises(ValueError):
        P.check_bounds(good.start)


def test_pad_bounds_adds_the_padding_document():
    b = P.pad_bounds(H.bounds_from_lengths([(3, 5), (8,)]), 12)
    assert b.start[:, 8:].tolist() == [[8] * 4] * 2 and b.end[:, 8:].tolist() == [[12] * 4] * 2
    assert b.start[:, :8].tolist() == [[0] * 3 + [3] * 5, [0] * 8]
    P.check_bounds(b)
    same = H.bounds_from_lengths([(8,)])
    assert P.pad_bounds(same, 8).start is same.start


@pytest.mark.parametrize("layout", ["L1", "L2", "L3"])
def test_the_rule_means_each_document_on_its_own(layout):
    """doc_attention_reference on a packed row equals, per document, attn_stress.reference on that document alone
    (fp64, 1e-12), forward and backward; the layouts are the ones the table in the issue lists."""
    B, T, Hh = 2, H.T_LAYOUT, 3
    bounds = H.layout_bounds(layout, B)
    P.check_bounds(bounds)
    lens = H.LAYOUTS[layout]
    starts = [sum(lens[:i]) for i in range(len(lens))]
    assert bounds.start[0].unique().tolist() == starts and sum(lens) == T
    q, k, v = (t.double() for t in A.split(A.build("plain", B, T, Hh), B, T, Hh))
    dO = A.grad_out(B, T, Hh).double()
    out, lse, dq, dk, dv = P.doc_attention_reference(q, k, v, bounds, dO)
    got = {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    for b in range(B):
        s = 0
        for n in (lens if b == 0 else lens[::-1]):
            sl = slice(s, s + n)
            alone = A.reference(q[b:b + 1, :, sl], k[b:b + 1, :, sl], v[b:b + 1, :, sl], dO[b:b + 1, :, sl])
            for name in got:
                g = got[name][b:b + 1, :, sl]
                err = float((g - alone[name]).abs().max())
                assert err <= 1e-12 * max(1.0, float(alone[name].abs().max())), (layout, b, s, name, err)
            s += n


def test_layouts_hit_what_they_are_chosen_for():
    s1 = H.layout_bounds("L1").start[0]
    assert int(H.layout_bounds("L1").end[0, 0]) == 1                      # a length-1 document
    assert {16, 32, 64, 127, 192} <= set(s1.unique().tolist())           # group, wave, tile, block - 1, tile 3
    assert int(s1[256]) == 192                                            # the last query block starts at tile 3
    s2 = H.layout_bounds("L2").start[0]
    assert int(s2[64]) == 32 and int(s2[79]) == 32 and int(s2[80]) == 80 and int(s2[95]) == 80
    s3 = H.layout_bounds("L3").start[0]
    assert int(s3[87]) == 40 and int(s3[88]) == 88 and 88 % 16 != 0


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from gpt_2_distributed_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgpt2mi.so not built")
    return _lib, _lib.load()


def test_abi_minor_counts_the_addition():
    _lib, lib = _lib_or_skip()
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    minor = int(hdr.split("#define GPT2MI_ABI_MINOR")[1].split()[0])
    assert minor == lib.gpt2mi_abi_minor() == _lib.ABI_MINOR and _lib.ABI_MINOR >= 5
    assert int(hdr.split("#define GPT2MI_ABI_VERSION")[1].split()[0]) == 24 == lib.gpt2mi_abi_version()
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(lib, name) and (name + "(") in hdr, name
        assert _lib._SINCE_MINOR[name] == 5


def test_a_v24_4_library_is_refused_by_name(monkeypatch):
    from gpt_2_distributed_amd import _lib

    class Fn:
        def __init__(self, value=0):
            self.value = value

        def __call__(self, *a):
            return self.value

    class Old:  # a ctypes.CDLL stand-in: every symbol up to v24.4, none newer
        def __init__(self, path):
            for name in _lib._SIGS:
                if _lib._SINCE_MINOR.get(name, 0) <= 4:
                    value = {"gpt2mi_abi_version": 24, "gpt2mi_abi_minor": 4}.get(name, 0)
                    setattr(self, name, Fn(value))

    monkeypatch.setattr(_lib.ctypes, "CDLL", Old)
    with pytest.raises(_lib.KernelError, match=r"v24\.4.*rebuild"):
        _lib.open_library("old.so")
    old = _lib.open_library("old.so", min_minor=4)  # an A/B tool may still load it: the new entries stay absent
    assert isinstance(old, Old) and not any(hasattr(old, n) for n in NEW)


# ---- argument checks, no GPU ----------------------------------------------------------------------------------------
TINY = dict(n_layer=1, n_head=2, n_embd=128, vocab_size=509, n_positions=64, resid_pdrop=0.0, attn_pdrop=0.0)


def test_public_surface_checks_bounds_before_anything_runs():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config, _checked_bounds
    m = GPT2(GPT2Config(**TINY))
    idx = torch.zeros(2, 8, dtype=torch.long)
    good = H.bounds_from_lengths([(3, 5), (8,)])
    assert _checked_bounds(None, idx) is None
    assert _checked_bounds(good, idx).start is good.start
    bad = [P.DocBounds(good.start.long(), good.end),                    # dtype
           P.DocBounds(good.start[:, :7], good.end[:, :7]),             # shape
           P.DocBounds(good.start.t().contiguous().t(), good.end),      # not contiguous
           (good.start,), good.start, "end"]                            # not a pair
    for b in bad:
        for call in (lambda: m(idx, doc_bounds=b), lambda: m.score(idx, idx, doc_bounds=b),
                     lambda: m.transformer(idx, doc_bounds=b),
                     lambda: m.transformer.h[0](torch.zeros(2, 8, 128), doc_bounds=b),
                     lambda: m.transformer.h[0].attn(torch.zeros(2, 8, 128), doc_bounds=b)):
            with pytest.raises(ValueError, match="doc_bounds"):
                call()
    if torch.cuda.is_available():  # (a device check needs a second device to name)
        with pytest.raises(ValueError, match="doc_bounds"):
            _checked_bounds(good, idx.cuda())
    # valid bounds reach forward's own refusal of a CPU model: the keyword is accepted
    for call in (lambda: m(idx, doc_bounds=good), lambda: m.score(idx, idx, doc_bounds=good)):
        with pytest.raises(RuntimeError, match="cuda"):
            call()
    with pytest.raises(TypeError):
        m(idx, None, None, good)  # keyword-only in forward
    for kw in (dict(eot="middle"), dict(eot_token_id=-1), dict(eot_token_id=1.5), dict(eot_token_id=True)):
        with pytest.raises(ValueError):
            m.evaluate(iter(()), **kw)


def test_trainer_and_evaluator_parse_the_flags():
    from gpt_2_distributed_amd import evaluate, train_gpt2_distributed as T
    a = T.build_parser().parse_args([])
    assert a.doc_mask is False and a.eot_token_id == 50256 and a.eot_position == "end"
    assert T.doc_mask_from_args(a) == {}
    a = T.build_parser().parse_args(["--doc_mask", "--eot_token_id", "3", "--eot_position", "begin"])
    assert T.doc_mask_from_args(a) == {"eot_token_id": 3, "eot": "begin"}
    with pytest.raises(SystemExit):
        T.doc_mask_from_args(T.build_parser().parse_args(["--doc_mask", "--eot_token_id", "-1"]))
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--eot_position", "middle"])
    base = ["--checkpoint", "c", "--data_dir", "d"]
    e = evaluate.parse_args(base)
    assert e.doc_mask is False and e.eot_token_id == 50256 and e.eot_position == "end"
    e = evaluate.parse_args(base + ["--doc_mask", "--eot_token_id", "3"])
    assert T.doc_mask_from_args(e) == {"eot_token_id": 3, "eot": "end"}
    with pytest.raises(SystemExit):
        evaluate.parse_args(base + ["--eot_position", "middle"])
