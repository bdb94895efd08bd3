"""The eight per-row sampler bindings (sample_ragged ... decode_generate_constrained) without a GPU or a library: which
keywords each takes, and that each reaches the C symbol of its own name with as many arguments as _lib._SIGS types for
it, the arguments it shares with the entry below being equal for equal inputs. _lib._call is replaced by a recorder."""
import ctypes

import pytest
import torch

from gpt_2_distributed_amd import _lib

ENTRIES = ("ragged", "penalized", "logprobs", "constrained")
B, V, LD = 3, 37, 12


class Plan:
    """What the bindings read of a DecodePlan."""
    B = B

    def ref(self):
        return "plan"


def _sample_keywords():
    """Per entry, the keywords it adds with non-neutral values (CPU tensors: _ptr is stubbed)."""
    return (dict(row_id=[5, 6, 7], eos=3, done=torch.zeros(B, dtype=torch.uint8),
                 seq_out=torch.zeros(B, LD, dtype=torch.int64), probs_out=torch.zeros(B, V)),
            dict(repetition=1.2, presence=0.5, frequency=0.25, hist=torch.zeros(B, LD, dtype=torch.int64),
                 hist_row=[2, 1, 0], gen_start=[1, 0, 2], logits_out=torch.zeros(B, V)),
            dict(logprob=torch.zeros(B, LD), top_ids=torch.zeros(B, LD, 2, dtype=torch.int32),
                 top_logprobs=torch.zeros(B, LD, 2), col=[0, 1, 2]),
            dict(logit_bias=torch.zeros(2, V), bias_row=[0, -1, 1], min_p=0.1, min_new_tokens=2, stop=[[1], [2, 3]]))


def _generate_keywords():
    s = _sample_keywords()
    return (dict(row_id=[5, 6, 7], eos=3, seq=torch.zeros(B, LD, dtype=torch.int64), done=s[0]["done"]),
            dict(repetition=1.2, presence=0.5, frequency=0.25, gen_start=[1, 0, 2]),
            {k: s[2][k] for k in ("logprob", "top_ids", "top_logprobs")}, s[3])


HEADS = {"sample": (torch.zeros(B, 40), V, 0.8, 5, 0.9, 11, [4, 5, 6], torch.zeros(B, dtype=torch.int64)),
         "decode_generate": (Plan(), V, 0.8, 5, 0.9, 11, [4, 5, 6], 2, torch.zeros(B, dtype=torch.int64))}


FAMILIES = {"sample": _sample_keywords, "decode_generate": _generate_keywords}


@pytest.fixture
def calls(monkeypatch):
    """The (symbol, arguments) of every _call, with CPU tensors for device ones and no stream."""
    seen = []
    monkeypatch.setattr(_lib, "_call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(_lib, "_ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, "_stream", lambda: "stream")
    return seen


def _plain(a):
    """An argument as a value that compares: a byref as the struct's fields (of a pointer, the address of a temporary
    host array or of a tensor, whether it is set), a host array as its list."""
    if hasattr(a, "_obj"):
        a = a._obj
    if isinstance(a, ctypes.Structure):
        return tuple((name, getattr(a, name) is not None if ctype is ctypes.c_void_p else getattr(a, name))
                     for name, ctype in a._fields_)
    if isinstance(a, ctypes.Array):
        return list(a)
    return a


def _run(calls, family, entry, keywords):
    del calls[:]
    getattr(_lib, f"{family}_{entry}")(*HEADS[family], **keywords)
    (name, args), = calls
    return name, args


@pytest.mark.parametrize("family", FAMILIES)
def test_an_entry_takes_its_keywords_and_those_below_and_no_later_one(calls, family):
    blocks = FAMILIES[family]()
    for level, entry in enumerate(ENTRIES):
        for at, block in enumerate(blocks):
            if at <= level:  # (a block at a time: top_ids goes with logprob)
                _run(calls, family, entry, block)
                continue
            for key, value in block.items():
                with pytest.raises(TypeError, match=f"{family}_{entry}.*{key}"):
                    _run(calls, family, entry, {key: value})
                assert not calls
    with pytest.raises(TypeError):
        _run(calls, family, "constrained", {"no_such_keyword": 1})


def test_the_examples_of_a_keyword_of_a_later_entry(calls):
    s, g = HEADS["sample"], HEADS["decode_generate"]
    with pytest.raises(TypeError):
        _lib.sample_ragged(*s, repetition=1.2)
    with pytest.raises(TypeError):
        _lib.sample_penalized(*s, logprob=torch.zeros(B, LD))
    with pytest.raises(TypeError):
        _lib.sample_logprobs(*s, min_p=0.1)
    with pytest.raises(TypeError):
        _lib.decode_generate_penalized(*g, stop=[[1]])
    with pytest.raises(TypeError):
        _lib.decode_generate_ragged(*g, gen_start=[0] * B)
    with pytest.raises(TypeError):
        _lib.decode_generate_logprobs(*g, col=[0] * B)  # (the loop has no col: step i writes column pos0[b] + i)
    assert not calls


@pytest.mark.parametrize("family", FAMILIES)
def test_each_forwarder_reaches_its_own_symbol_with_the_arity_of_its_signature(calls, family):
    blocks = FAMILIES[family]()
    for level, entry in enumerate(ENTRIES):
        for keywords in ({}, {k: v for block in blocks[:level + 1] for k, v in block.items()}):
            name, args = _run(calls, family, entry, keywords)
            assert name == f"gpt2mi_{family}_{entry}"
            assert len(args) == len(_lib._SIGS[name]), (name, len(args))
            for a, ctype in zip(args, _lib._SIGS[name]):  # a float where the entry takes one, and nowhere else
                assert isinstance(a, float) == (ctype is ctypes.c_float), (name, a, ctype)


@pytest.mark.parametrize("family", FAMILIES)
def test_neighbouring_entries_share_their_prefix_for_equal_inputs(calls, family):
    """The sampler's new arguments go before the stream, the loop's behind it (gpt2mi.h)."""
    blocks = FAMILIES[family]()
    for level in range(len(ENTRIES) - 1):
        for keywords in ({}, {k: v for block in blocks[:level + 1] for k, v in block.items()}):
            below = [_plain(a) for a in _run(calls, family, ENTRIES[level], keywords)[1]]
            above = [_plain(a) for a in _run(calls, family, ENTRIES[level + 1], keywords)[1]]
            assert below[-1] == "stream" or family == "decode_generate"
            shared = below[:-1] if family == "sample" else below
            assert above[:len(shared)] == shared and len(above) > len(below)
            if family == "sample":
                assert above[-1] == "stream"
    # what the full lists are: the tail (pen, logits_out, lp, con) / (repetition, presence, frequency, gen_start, lp, con)
    full = {k: v for block in blocks for k, v in block.items()}
    args = [_plain(a) for a in _run(calls, family, "constrained", full)[1]]
    if family == "sample":
        pen, logits_out, lp, con, stream = args[-5:]
        assert dict(pen)["repetition"] == pytest.approx(1.2) and dict(pen)["hist_rows"] == B
        assert logits_out == full["logits_out"].data_ptr() and stream == "stream"
    else:
        stream, rp, pp, fp, gen_start, lp, con = args[-7:]
        assert (stream, pp, fp, gen_start) == ("stream", 0.5, 0.25, [1, 0, 2]) and rp == pytest.approx(1.2)
    assert dict(lp)["top_n"] == 2 and dict(lp)["ld"] == LD
    assert dict(con)["n_stop"] == 2 and dict(con)["min_new"] == 2 and dict(con)["bias_rows"] == 2


def test_gen_start_of_another_length_is_refused_before_the_call(calls):
    for entry in ENTRIES[1:]:
        with pytest.raises(_lib.KernelError, match="gen_start has 2 entries for B=3 rows"):
            getattr(_lib, f"decode_generate_{entry}")(*HEADS["decode_generate"], gen_start=[0, 0])
        with pytest.raises(_lib.KernelError, match="gen_start must have B=3"):
            getattr(_lib, f"sample_{entry}")(*HEADS["sample"], gen_start=[0, 0])
    assert not calls
