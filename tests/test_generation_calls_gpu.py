"""The C calls generation makes, recorded: every path of ``generate`` / ``generate_many`` runs once on a tiny model with
the sampler bindings wrapped as ``generation`` sees them, and the list of calls must equal
tests/golden/generation_calls.json, which the same recorder and script wrote on the parent of the commit that put the
sampling options into one record. The bitwise suites show that the tokens are unchanged; this one catches a changed
argument that happens to leave the tiny model's tokens alone.

A call is noted as the binding sees it: the entry, its positional arguments by name and every keyword of the entry
tables (``_lib._SAMPLE_OPTIONS`` / ``_GENERATE_OPTIONS``) over its neutral value there, so a neutral keyword written out
and one left out are the same call, as they are the same C call. Scalars and host lists are kept verbatim, a tensor is
``[dtype, shape]``, a plan its rows, None null.

``python tests/test_generation_calls_gpu.py OUT.json [TREE]`` writes the recording of the package under TREE (default:
this repository) to OUT.json: on a checkout of another commit that is how the fixture is regenerated."""
import json
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "generation_calls.json")
CFG = dict(n_layer=1, n_head=1, n_embd=64, vocab_size=96, n_positions=48)
SAMPLE_HEAD = ("logits", "V", "temperature", "top_k", "top_p", "seed", "pos", "tok_out")
GENERATE_HEAD = ("plan", "V", "temperature", "top_k", "top_p", "seed", "pos0", "n", "tok")
ENTRIES = ("ragged", "penalized", "logprobs", "constrained")
PEN = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2)
LOOSE = dict(temperature=0.8, top_k=20, top_p=0.9)
CON = dict(logit_bias={5: 0.5, 7: -float("inf")}, min_p=0.05, min_new_tokens=2, stop=[[3, 4]], eos_token_id=9)


def note(v):
    if isinstance(v, torch.Tensor):
        return [str(v.dtype), list(v.shape)]
    if isinstance(v, (list, tuple, range)):
        return [note(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return {"plan": [int(v.B), int(v.rows)]}  # a DecodePlan


def record(K, calls):
    """Wrap the bindings of module ``K`` (generation's ``_lib``) so that each call is appended to ``calls`` and then made;
    returns the originals by name."""
    import inspect
    kept = {}

    def wrap(name, names, neutral):
        fn = kept[name] = getattr(K, name)

        def recorded(*args, **kw):
            unknown = set(kw) - set(neutral)
            assert len(args) <= len(names) and not unknown, (name, len(args), unknown)
            calls.append([name, {k: note(v) for k, v in {**neutral, **dict(zip(names, args)), **kw}.items()}])
            return fn(*args, **kw)
        setattr(K, name, recorded)

    for level, entry in enumerate(ENTRIES):
        for prefix, head, blocks in (("sample_", SAMPLE_HEAD, K._SAMPLE_OPTIONS),
                                     ("decode_generate_", GENERATE_HEAD, K._GENERATE_OPTIONS)):
            wrap(prefix + entry, head, {k: v for block in blocks[:level + 1] for k, v in block.items()})
    for name in ("decode_extend", "decode_beam_search"):
        params = inspect.signature(getattr(K, name)).parameters
        wrap(name, tuple(params), {k: p.default for k, p in params.items() if p.default is not inspect.Parameter.empty})
    return kept


def script(model):
    """Each path once: B = 3 ragged prompts of 1, 4 and 7 tokens, 5 new tokens; one eos run of 40 crosses EOS_CHUNK."""
    dev = model.arena.device
    S = torch.randint(0, CFG["vocab_size"], (4, 7), generator=torch.Generator().manual_seed(17)).to(dev)
    prompts = [S[0, :1], S[1, :4], S[2, :7]]
    for kw in (dict(temperature=0.0), LOOSE, dict(LOOSE, **PEN), dict(LOOSE, logprobs=2), dict(LOOSE, **CON),
               dict(LOOSE, **PEN, **CON, logprobs=2),
               dict(LOOSE, **PEN, draft_tokens=2, stop=[[3, 4]], eos_token_id=9), dict(LOOSE, num_samples=2)):
        model.generate(prompts, 5, seed=3, **kw)
    model.generate(prompts, 40, temperature=0.0, seed=3, eos_token_id=9)
    model.generate(prompts, 5, num_beams=2)
    model.generate_many(prompts + [S[3, :2]], 5, batch_size=2, seed=3, **LOOSE)


def recording(tree=REPO):
    """The calls of ``script`` with the package under ``tree``, as JSON gives them back."""
    if tree not in sys.path:
        sys.path.insert(0, tree)
    from gpt_2_distributed_amd import generation
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    assert os.path.dirname(os.path.dirname(os.path.abspath(generation.__file__))) == os.path.abspath(tree)
    torch.manual_seed(1234)
    model = GPT2(GPT2Config(**CFG)).to("cuda")
    calls = []
    kept = record(generation.K, calls)
    try:
        script(model)
    finally:
        for name, fn in kept.items():
            setattr(generation.K, name, fn)
    return json.loads(json.dumps(calls))


@pytest.mark.gpu
def test_generation_makes_the_recorded_calls():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    got, want = recording(), json.load(open(FIXTURE))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {i}"
    assert len(got) == len(want)
    names = [c[0] for c in got]
    assert {n.rsplit("_", 1)[1] for n in names if n.startswith("decode_generate_")} == set(ENTRIES)  # every loop,
    assert {"decode_extend", "decode_beam_search", "sample_constrained"} <= set(names)               # verify and beams
    eos_run = [c[1]["n"] for c in got if c[0] == "decode_generate_ragged" and c[1]["eos"] == 9]
    assert eos_run == [32, 8]                                                                        # EOS_CHUNK crossed


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(recording(*sys.argv[2:3]), f, indent=0, allow_nan=True)
        f.write("\n")
