"""Per-document positions on the CPU: ``packing.doc_positions`` against a loop over the documents, the v24.6 C ABI, and
the refusals of ``reset_positions`` without bounds by the public surface and the two command lines. No GPU."""
import os

import pytest
import torch

from gpt_2_distributed_amd import packing as P
from tests import docmask_helpers as H
from tests import docpos_helpers as D
from tests.conftest import REPO
from tests.docmask_helpers import EOT, bounds_rows

NEW = ("gpt2mi_embed_fwd_doc", "gpt2mi_embed_bwd_doc")


@pytest.mark.parametrize("eot", ["end", "begin"])
def test_positions_of_token_rows_equal_the_loop(eot):
    bounds = P.doc_bounds_reference(bounds_rows(), EOT, eot)
    pos = P.doc_positions(bounds)
    assert pos.dtype == torch.int32 and pos.shape == bounds.start.shape and pos.is_contiguous()
    assert torch.equal(pos, D.loop_positions(bounds))
    T = pos.shape[1]
    first = bounds.start.long() == torch.arange(T)[None]
    assert bool((pos[first] == 0).all()) and bool((pos[~first] > 0).all())
    assert int(pos[0, T - 1]) == T - 1  # row 0 holds no separator: one document


def test_positions_of_length_layouts_equal_the_loop():
    T = 24
    rows = [D.layout_lengths(n, T, seed=3) for n in D.LAYOUT_NAMES] + [H.random_lengths(T, 5, seed=2)]
    bounds = H.bounds_from_lengths(rows)
    pos = P.doc_positions(bounds)
    assert torch.equal(pos, D.loop_positions(bounds))
    assert pos[0].tolist() == list(range(T)) and pos[1].tolist() == [0] * T
    assert pos[2].tolist() == [0] + list(range(T - 1)) and pos[3].tolist() == list(range(T - 1)) + [0]
    for b, lens in enumerate(rows):
        assert int(pos[b].max()) == max(lens) - 1
    # the engine's padding is a document of its own: positions restart there too (its rows are zeros anyway)
    padded = P.doc_positions(D.padded_bounds([(3, 5), (8,)], 12))
    assert padded[:, 8:].tolist() == [[0, 1, 2, 3]] * 2 and padded[0, :8].tolist() == [0, 1, 2, 0, 1, 2, 3, 4]
    big = P.doc_positions(H.bounds_from_lengths([H.random_lengths(1024, 64, seed=5)]))
    assert torch.equal(big, D.loop_positions(H.bounds_from_lengths([H.random_lengths(1024, 64, seed=5)])))


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_abi_minor_counts_the_addition():
    from gpt_2_distributed_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgpt2mi.so not built")
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    minor = int(hdr.split("#define GPT2MI_ABI_MINOR")[1].split()[0])
    assert minor == lib.gpt2mi_abi_minor() == _lib.ABI_MINOR and _lib.ABI_MINOR >= 6
    assert int(hdr.split("#define GPT2MI_ABI_VERSION")[1].split()[0]) == 24 == lib.gpt2mi_abi_version()
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(lib, name) and (name + "(") in hdr, name
        assert _lib._SINCE_MINOR[name] == 6
        assert len(_lib._SIGS[name]) == len(_lib._SIGS[name[:-4]]) + 1  # the plain entry's arguments plus start
    assert callable(_lib.embed_fwd_doc) and callable(_lib.embed_bwd_doc)


# ---- argument checks, no GPU ----------------------------------------------------------------------------------------
TINY = dict(n_layer=1, n_head=2, n_embd=128, vocab_size=509, n_positions=64, resid_pdrop=0.0, attn_pdrop=0.0)


def test_reset_positions_needs_bounds_before_anything_runs():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    m = GPT2(GPT2Config(**TINY))
    idx = torch.zeros(2, 8, dtype=torch.long)
    good = H.bounds_from_lengths([(3, 5), (8,)])
    for call in (lambda: m(idx, reset_positions=True), lambda: m(idx, labels=idx, reset_positions=True),
                 lambda: m.score(idx, idx, reset_positions=True),
                 lambda: m.score(idx, idx, reduction="none", reset_positions=True),
                 lambda: m.transformer(idx, reset_positions=True),
                 lambda: m.evaluate(iter(()), reset_positions=True),
                 lambda: m.evaluate(iter([(idx, idx)]), reset_positions=True)):
        with pytest.raises(ValueError, match="reset_positions"):
            call()
    # with bounds the keyword is accepted and the call reaches the refusal of a CPU model
    for call in (lambda: m(idx, doc_bounds=good, reset_positions=True),
                 lambda: m.score(idx, idx, doc_bounds=good, reset_positions=True),
                 lambda: m.transformer(idx, doc_bounds=good, reset_positions=True)):
        with pytest.raises(RuntimeError, match="cuda"):
            call()
    # off is the default and needs nothing
    with pytest.raises(RuntimeError, match="cuda"):
        m(idx, reset_positions=False)
    # blocks, attention and MLP have no embedding: no such keyword
    for mod in (m.transformer.h[0], m.transformer.h[0].attn):
        with pytest.raises(TypeError):
            mod(torch.zeros(2, 8, 128), doc_bounds=good, reset_positions=True)
    from gpt_2_distributed_amd.engine import Engine
    with pytest.raises(ValueError, match="reset_positions"):
        Engine._check_reset(None, True)
    assert Engine._check_reset(None, False) is False and Engine._check_reset(good, 1) is True


def test_trainer_and_evaluator_refuse_the_flag_without_doc_mask(capsys):
    from gpt_2_distributed_amd import evaluate, train_gpt2_distributed as T
    a = T.build_parser().parse_args([])
    assert a.reset_positions is False and T.doc_mask_from_args(a) == {}
    a = T.build_parser().parse_args(["--doc_mask", "--eot_token_id", "3", "--reset_positions"])
    assert T.doc_mask_from_args(a) == {"eot_token_id": 3, "eot": "end", "reset_positions": True}
    a = T.build_parser().parse_args(["--doc_mask", "--eot_token_id", "3"])
    assert T.doc_mask_from_args(a) == {"eot_token_id": 3, "eot": "end"}  # off: evaluate() is called as it was
    with pytest.raises(SystemExit) as e:
        T.build_parser().parse_args(["--reset_positions"])
    assert e.value.code == 2 and "--doc_mask" in capsys.readouterr().err
    base = ["--checkpoint", "c", "--data_dir", "d"]
    assert evaluate.parse_args(base).reset_positions is False
    e = evaluate.parse_args(base + ["--doc_mask", "--reset_positions"])
    assert T.doc_mask_from_args(e) == {"eot_token_id": 50256, "eot": "end", "reset_positions": True}
    with pytest.raises(SystemExit) as e:
        evaluate.parse_args(base + ["--reset_positions"])
    assert e.value.code == 2 and "--doc_mask" in capsys.readouterr().err
