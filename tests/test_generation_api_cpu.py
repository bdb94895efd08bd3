"""The surface of generation that callers and stub sessions rely on, without a GPU: the public signatures, written out
from the commit before the sampling options became one record (``generation.Sampler``), and the record itself: what it
renders for a session, what it re-indexes for a verify call and what its constructor refuses."""
import inspect

import pytest
import torch

from gpt_2_distributed_amd import generation
from gpt_2_distributed_amd.generation import DecodeSession, Sampler
from gpt_2_distributed_amd.model import GPT2

INF = float("inf")
REQ = inspect.Parameter.empty
GENERATE = [("idx", REQ), ("max_new_tokens", REQ), ("temperature", 1.0), ("top_k", None), ("generator", None),
            ("eos_token_id", None), ("top_p", None), ("seed", None), ("prompt_lens", None), ("pad_token_id", None),
            ("draft_tokens", None), ("draft_fn", None), ("repetition_penalty", 1.0), ("presence_penalty", 0.0),
            ("frequency_penalty", 0.0), ("kv_dtype", "bf16"), ("num_samples", 1), ("logprobs", None), ("num_beams", None),
            ("length_penalty", 1.0), ("num_return_sequences", 1), ("logit_bias", None), ("allowed_token_ids", None),
            ("min_p", None), ("min_new_tokens", 0), ("stop", None)]
GENERATE_MANY = [("prompts", REQ), ("max_new_tokens", REQ), ("batch_size", 32), ("temperature", 1.0), ("top_k", None),
                 ("top_p", None), ("seed", 0), ("eos_token_id", None), ("generator", None), ("repetition_penalty", 1.0),
                 ("presence_penalty", 0.0), ("frequency_penalty", 0.0), ("kv_dtype", "bf16"), ("logprobs", None),
                 ("logit_bias", None), ("allowed_token_ids", None), ("min_p", None), ("min_new_tokens", 0), ("stop", None)]
RUN_TAIL = [("temperature", 1.0), ("top_k", None), ("top_p", None), ("seed", 0), ("eos_token_id", None), ("seq", None),
            ("done", None), ("row_id", None), ("repetition_penalty", 1.0), ("presence_penalty", 0.0),
            ("frequency_penalty", 0.0), ("gen_start", None), ("logprobs", None), ("logit_bias", None), ("bias_row", None),
            ("min_p", None), ("min_new_tokens", 0), ("stop", None)]
SIGNATURES = [
    (GPT2.generate, [("self", REQ)] + GENERATE), (GPT2.generate_many, [("self", REQ)] + GENERATE_MANY),
    (generation.generate, [("model", REQ)] + GENERATE), (generation.generate_many, [("model", REQ)] + GENERATE_MANY),
    (DecodeSession.sample, [("self", REQ), ("temperature", 1.0), ("top_k", None), ("top_p", None), ("seed", 0),
                            ("row_id", None), ("repetition_penalty", 1.0), ("presence_penalty", 0.0),
                            ("frequency_penalty", 0.0), ("gen_start", None), ("history", None), ("logprobs", None),
                            ("logit_bias", None), ("bias_row", None), ("min_p", None), ("min_new_tokens", 0),
                            ("stop", None), ("eos_token_id", None), ("done", None)]),
    (DecodeSession.generate, [("self", REQ), ("n", REQ)] + RUN_TAIL),
    (DecodeSession.speculate, [("self", REQ), ("n", REQ), ("k", REQ), ("draft_fn", None)] + RUN_TAIL),
]


@pytest.mark.parametrize("fn, want", SIGNATURES, ids=[fn.__qualname__ for fn, _ in SIGNATURES])
def test_public_signatures_are_the_parent_commits(fn, want):
    assert [(k, p.default) for k, p in inspect.signature(fn).parameters.items()] == want


# ---- the record ------------------------------------------------------------------------------------------------------------
V = 10
PEN_NAMES = {"repetition_penalty", "presence_penalty", "frequency_penalty"}
CON_NAMES = {"min_p", "min_new_tokens", "stop"}
BIAS_NAMES = CON_NAMES | {"logit_bias", "bias_row"}
FAMILIES = {
    "penalties": (dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2), PEN_NAMES),
    "min_p": (dict(min_p=0.1), CON_NAMES),
    "min_new_tokens": (dict(min_new_tokens=2, eos_token_id=5), CON_NAMES),
    "stop": (dict(stop=[[1, 2]], eos_token_id=5), CON_NAMES),
    "bias": (dict(logit_bias=torch.zeros(2, V), bias_row=[0, 1]), BIAS_NAMES),
}
FAMILIES["all"] = ({k: v for kw, _ in FAMILIES.values() for k, v in kw.items()}, PEN_NAMES | BIAS_NAMES)


def test_a_neutral_record_renders_no_keyword():
    for s in (Sampler(), Sampler.of(), Sampler.of(0.8, 20, 0.9, 3, 5, 1.0, 0.0, 0.0, None, 0, None),
              Sampler.of(min_p=0.0, stop=[], vocab_size=V), Sampler.of(logit_bias=torch.zeros(1, V), bias_row=[-1, -1])):
        assert not s.penalised and not s.constrained
        assert s.keywords([3, 4]) == {} and s.blocks([3, 4]) == ({}, {}) and s.blocks([3, 4], seqs=[1, 0, 1]) == ({}, {})


@pytest.mark.parametrize("family", FAMILIES)
def test_a_record_renders_todays_keywords_and_reindexes_by_sequence(family):
    kw, names = FAMILIES[family]
    s = Sampler.of(0.8, 20, 0.9, 3, **kw, vocab_size=V)
    assert s.penalised == bool(names & PEN_NAMES) and s.constrained == bool(names & CON_NAMES)
    out = s.keywords([3, 4])
    assert set(out) == names | {"gen_start"} and out["gen_start"] == [3, 4]
    for k, v in kw.items():
        if k != "eos_token_id":
            assert out[k] is v if isinstance(v, torch.Tensor) else out[k] == v, k
    hist = torch.zeros(2, 8, dtype=torch.int64)
    pen, con = s.blocks([3, 4], s.bias_row, [1, 0, 1], hist)
    assert bool(pen) == s.penalised and bool(con) == s.constrained
    if pen:
        assert pen["gen_start"] == [4, 3, 4] and pen["hist"] is hist and pen["hist_row"] == [1, 0, 1]
        assert (pen["repetition"], pen["presence"], pen["frequency"]) == (1.3, 0.5, 0.2)
    if con:
        assert con["gen_start"] == [4, 3, 4] and con["stop"] == []
        assert (con["min_p"], con["min_new_tokens"]) == (s.min_p, s.min_new_tokens)
        assert con.get("bias_row") == ([1, 0, 1] if "logit_bias" in kw else None)
    assert s.stop == kw.get("stop", [])                       # (the record itself keeps its stop table)


def test_the_driver_form_builds_one_bias_table():
    s = Sampler.of(seed=0, logit_bias={3: -INF, 4: 2.5}, allowed_token_ids=[3, 4, 5], vocab_size=V, rows=3, device="cpu")
    assert s.logit_bias.shape == (1, V) and s.bias_row == [0, 0, 0] and s.constrained
    assert s.logit_bias[0].tolist() == [-INF] * 3 + [-INF, 2.5, 0.0] + [-INF] * 4
    s = Sampler.of(seed=0, logit_bias=torch.ones(3, V), vocab_size=V, rows=3, device="cpu")
    assert s.logit_bias.shape == (3, V) and s.bias_row == [0, 1, 2]
    assert Sampler.of(seed=0, vocab_size=V, rows=3, device="cpu").logit_bias is None


@pytest.mark.parametrize("kw, msg", [
    (dict(temperature=-1.0), "temperature"), (dict(top_p=0.0), "top_p"), (dict(top_p=float("nan")), "top_p"),
    (dict(seed=1.5), "seed must be an int"),
    (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(presence_penalty=INF), "presence_penalty"),
    (dict(frequency_penalty=float("nan")), "frequency_penalty"),
    (dict(min_p=1.5), "min_p"), (dict(min_new_tokens=-1, eos_token_id=5), "min_new_tokens"),
    (dict(min_new_tokens=1), "eos_token_id"), (dict(stop=[[1]]), "eos_token_id"),
    (dict(stop=[[1]] * 9, eos_token_id=5), "at most 8"), (dict(stop=[[]], eos_token_id=5), "1 to 16"),
    (dict(stop=[[10]], eos_token_id=5), "stop tokens"),
    (dict(logit_bias={10: 1.0}), "logit_bias tokens"), (dict(logit_bias={1: INF}), "finite or -inf"),
    (dict(logit_bias=torch.zeros(9), rows=2), "logit_bias must be"),
    (dict(logit_bias=torch.zeros(3, V), rows=2), "logit_bias"), (dict(logit_bias=torch.zeros(2, V), rows=2, per_row=False),
                                                                 "logit_bias"),
    (dict(allowed_token_ids=[], rows=2), "allowed_token_ids"), (dict(allowed_token_ids=[10], rows=2), "allowed_token_ids"),
    (dict(seed=0, eos_token_id=10, rows=2), "eos_token_id 10 not in"),
])
def test_the_constructor_refuses_one_bad_value_of_each_option(kw, msg):
    with pytest.raises(ValueError, match=msg):
        Sampler.of(**{"vocab_size": V, **kw})
