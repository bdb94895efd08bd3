"""Sample from a checkpoint: ``python -m gpt_2_distributed_amd.generate --checkpoint out/step_0001000 --model 124M
--prompt_ids 50256 --max_new_tokens 64 [--temperature T --top_k K --top_p P --sampler {torch,device} --seed S --batch B
--draft_tokens K --repetition_penalty R --presence_penalty P --frequency_penalty F --kv_dtype {bf16,fp8}
--num_samples S --logprobs [N] --num_beams W --length_penalty A --num_return_sequences R --logit_bias T:V,T:V
--min_p M --min_new_tokens N --stop IDS [--stop IDS ...]]``.

Loads ``model.pt`` of a ``save_checkpoint`` directory (train_gpt2_distributed.py) into a GPT2 of the named size, runs
``GPT2.generate`` on ``--batch`` copies of the prompt and prints one JSON list of token ids per sequence (prompt
included). No tokenizer is shipped: prompts and outputs are GPT-2 BPE ids (50256 = <|endoftext|>).

Several prompts: repeat ``--prompt_ids`` or give ``--prompts_file`` (one comma-separated prompt per line). They go
through ``GPT2.generate_many`` (continuous batching on the device sampler, ``--batch`` rows at a time; prompt i draws from
(``--seed``, i, position)) and one JSON list per prompt is printed, in input order.

``--num_samples S`` (S > 1) draws S continuations of every prompt through ``GPT2.generate(num_samples=S)``: each prompt
is run once and its rows share its cache. One JSON object per sample is printed, prompt-major:
``{"prompt": b, "sample": j, "tokens": [...]}`` (the prompt's own padding, if the prompts differ in length, removed).
``--batch`` is not used then; prompts x S <= 64.

``--logprobs [N]`` makes every line a JSON object (``"tokens"`` as above) with ``"logprobs"``, the log-probability of each
new token under the model's own distribution (before penalties, temperature and filters), and ``"cum_logprob"``, their
sum; with N > 0 also ``"top_logprobs"``, per new token the N most likely ``[id, logprob]`` pairs. Without the flag the
lines are what they were.

``--num_beams W`` searches instead of drawing (``GPT2.generate(num_beams=W)``: beam search on the device over the prompt's
shared cache) and prints, prompt-major, one JSON object per returned beam, best first:
``{"prompt": b, "beam": j, "tokens": [...], "score": s, "cum_logprob": c}`` (``tokens``: the prompt and the beam up to and
including its first eos). ``--length_penalty`` enters the final ranking only and ``--num_return_sequences`` (default 1,
at most W) says how many beams of each prompt are printed. The sampler's flags (``--sampler device`` among them) do not
go with it; prompts x W <= 64.

``--logit_bias 50256:-100,198:2.5`` adds a value to a token's logit (``-inf`` bans it), ``--min_p 0.05`` drops the tokens
less than that fraction as likely as the most likely one, ``--min_new_tokens 8`` holds ``--eos_token_id`` back for that
many tokens and ``--stop 198,198`` (repeatable) ends a sequence at the token that completes the given tokens; the last two
need ``--eos_token_id``. They go with either ``--sampler`` (``GPT2.generate``'s keywords), not with ``--num_beams``."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

from .model import GPT2, GPT2Config, MODEL_SIZES


def make_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--checkpoint", required=True, help="a step_XXXXXXX directory written by save_checkpoint")
    p.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES) + ["auto"],
                   help="model size; auto: widths and depth from the checkpoint (n_head = n_embd / 64)")
    p.add_argument("--prompt_ids", action="append", default=None,
                   help="comma-separated token ids (default 50256); may be given several times")
    p.add_argument("--prompts_file", default=None, help="a file with one comma-separated prompt per line")
    p.add_argument("--max_new_tokens", type=int, default=64)
    p.add_argument("--temperature", type=float, default=1.0)
    p.add_argument("--top_k", type=int, default=None)
    p.add_argument("--top_p", type=float, default=None, help="nucleus filter in (0, 1); >= 1 or unset: off")
    p.add_argument("--sampler", default="torch", choices=["torch", "device"],
                   help="torch: sample_next with a torch.Generator seeded by --seed; device: the fused sampling kernel, "
                        "drawing from (--seed, row, position), and the token loop issued from C")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch", type=int, default=1,
                   help="one prompt: the number of copies; several prompts: the rows of generate_many's session")
    p.add_argument("--eos_token_id", type=int, default=None)
    p.add_argument("--draft_tokens", type=int, default=None,
                   help="one prompt, --sampler device: verify up to this many prompt-lookup draft tokens per pass over "
                        "the weights (the same tokens as without; batch * (draft_tokens + 1) <= 64)")
    p.add_argument("--repetition_penalty", type=float, default=1.0,
                   help="HF's rule: the logit of a token of the prompt or the output so far is divided by this "
                        "(multiplied if negative); 1: off")
    p.add_argument("--presence_penalty", type=float, default=0.0,
                   help="subtracted from the logit of every token generated so far (OpenAI / vLLM); 0: off")
    p.add_argument("--frequency_penalty", type=float, default=0.0,
                   help="times the number of times a token was generated so far, subtracted from its logit; 0: off")
    p.add_argument("--kv_dtype", default="bf16", choices=["bf16", "fp8"],
                   help="the key/value cache: bf16, or fp8 (e4m3 codes with a power-of-two scale per 64-wide row, "
                        "0.53 x the bytes)")
    p.add_argument("--num_samples", type=int, default=1,
                   help="continuations per prompt (> 1: one prefill per prompt, its rows share the prompt's cache; "
                        "prompts x num_samples <= 64)")
    p.add_argument("--logprobs", type=int, nargs="?", const=0, default=None, metavar="N",
                   help="print each new token's log-probability and their sum; N > 0 (<= 20): the N most likely tokens "
                        "of each step as well")
    p.add_argument("--num_beams", type=int, default=None,
                   help="beam search with this many beams per prompt (1..20; prompts x num_beams <= 64) instead of "
                        "sampling: the sampler's flags do not go with it")
    p.add_argument("--length_penalty", type=float, default=1.0,
                   help="--num_beams: the final score is cum_logprob / length ** this (1: the mean log-probability)")
    p.add_argument("--num_return_sequences", type=int, default=1, help="--num_beams: beams printed per prompt, best first")
    p.add_argument("--logit_bias", type=parse_logit_bias, default=None, metavar="TOKEN:VALUE,...",
                   help="added to the logits of the named tokens after the penalties (-inf bans a token)")
    p.add_argument("--min_p", type=float, default=None,
                   help="drop every token less than this fraction as likely as the most likely one; 0 or unset: off")
    p.add_argument("--min_new_tokens", type=int, default=0,
                   help="--eos_token_id is held back until a sequence has this many new tokens")
    p.add_argument("--stop", type=parse_stop, action="append", default=None, metavar="IDS",
                   help="comma-separated token ids: a sequence ends at the token that completes them (needs "
                        "--eos_token_id); may be given up to 8 times, 16 tokens each")
    return p


def parse_logit_bias(text: str) -> dict:
    """``"50256:-100,198:2.5"`` as ``{50256: -100.0, 198: 2.5}``."""
    try:
        return {int(t): float(v) for t, v in (item.split(":") for item in text.split(",") if item.strip())}
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected TOKEN:VALUE[,TOKEN:VALUE...] (got {text!r})")


def parse_stop(text: str) -> list:
    """``"198,198"`` as ``[198, 198]``."""
    try:
        return [int(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected comma-separated token ids (got {text!r})")


def parse_args(argv=None):
    return make_parser().parse_args(argv)


def beam_lines(out, prompt_lens):
    """The JSON objects of a ``generate(num_beams=)`` result, prompt-major, a beam cut after its last token."""
    lines = []
    for b, n in enumerate(prompt_lens):
        for j in range(out.tokens.size(1)):
            lines.append({"prompt": b, "beam": j, "tokens": out.tokens[b, j, :n + int(out.lengths[b, j])].tolist(),
                          "score": float(out.scores[b, j]), "cum_logprob": float(out.cum_logprob[b, j])})
    return lines


def with_logprobs(line, out, row: int, first: int, last: int, top_n: int):
    """``line`` (a dict, or a token list, which becomes ``{"tokens": ...}``) with the values of columns [first, last) of
    row ``row`` of a ``generate(..., logprobs=)`` result."""
    line = dict(line) if isinstance(line, dict) else {"tokens": line}
    line["logprobs"] = out.logprobs[row, first:last].tolist()
    line["cum_logprob"] = sum(line["logprobs"])
    if top_n > 0:
        line["top_logprobs"] = [[[i, v] for i, v in zip(ids, vals)] for ids, vals in
                                zip(out.top_ids[row, first:last].tolist(), out.top_logprobs[row, first:last].tolist())]
    return line


def load_model(ckpt_dir: str, size: str) -> GPT2:
    """A GPT2 on cuda:0 with the weights of ``ckpt_dir``/model.pt (as load_checkpoint restores them); the vocabulary
    and context length are read from the checkpoint's embedding tables."""
    sd = torch.load(os.path.join(ckpt_dir, "model.pt"), map_location="cpu", weights_only=True)
    V, C = sd["transformer.wte.weight"].shape
    L = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.h."))
    dims = dict(n_layer=L, n_head=C // 64, n_embd=C) if size == "auto" else dict(MODEL_SIZES[size])
    if (dims["n_embd"], dims["n_layer"]) != (C, L):
        raise ValueError(f"--model {size} is {dims['n_layer']} layers of width {dims['n_embd']}, the checkpoint {L} "
                         f"of width {C}")
    cfg = GPT2Config(vocab_size=V, n_positions=sd["transformer.wpe.weight"].shape[0], **dims)
    model = GPT2(cfg).to("cuda:0")
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(sd[n])
    model.engine().refresh_shadow()
    return model


def main(argv=None) -> int:
    a = parse_args(argv)
    if a.num_beams is not None and a.sampler == "device":
        raise SystemExit("--sampler device draws tokens: it does not go with --num_beams, which searches")
    lines = list(a.prompt_ids or [])
    if a.prompts_file:
        with open(a.prompts_file) as f:
            lines += [line for line in f.read().splitlines() if line.strip()]
    prompts = [[int(t) for t in line.split(",") if t.strip()] for line in lines or ["50256"]]
    if not all(prompts):
        raise SystemExit("an empty prompt (--prompt_ids / --prompts_file)")
    model = load_model(a.checkpoint, a.model)
    pen = dict(repetition_penalty=a.repetition_penalty, presence_penalty=a.presence_penalty,
               frequency_penalty=a.frequency_penalty, kv_dtype=a.kv_dtype)
    if a.logprobs is not None:
        pen["logprobs"] = a.logprobs
    pen.update({k: v for k, v in dict(logit_bias=a.logit_bias, min_p=a.min_p, min_new_tokens=a.min_new_tokens,
                                      stop=a.stop).items() if v})  # (only what was set: as the defaults, nothing)
    if a.num_beams is not None:
        # (only what the user set travels on: generate refuses the sampler's keywords beside num_beams by name)
        default = make_parser().get_default
        given = {k: v for k, v in dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p,
                                       draft_tokens=a.draft_tokens, num_samples=a.num_samples, **pen).items()
                 if v != default(k)}
        out = model.generate([torch.tensor(q, dtype=torch.int64, device="cuda:0") for q in prompts] * a.batch,
                             a.max_new_tokens, eos_token_id=a.eos_token_id, num_beams=a.num_beams,
                             length_penalty=a.length_penalty, num_return_sequences=a.num_return_sequences, **given)
        for line in beam_lines(out, [len(q) for q in prompts] * a.batch):
            print(json.dumps(line))
        return 0
    if a.num_samples > 1:
        if a.draft_tokens is not None and a.sampler != "device":
            raise SystemExit("--draft_tokens compares drafts with the device sampler's draws: --sampler device")
        how = (dict(seed=a.seed, draft_tokens=a.draft_tokens) if a.sampler == "device"
               else dict(generator=torch.Generator(device="cuda:0").manual_seed(a.seed)))
        out = model.generate([torch.tensor(q, dtype=torch.int64, device="cuda:0") for q in prompts], a.max_new_tokens,
                             temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, eos_token_id=a.eos_token_id,
                             num_samples=a.num_samples, **how, **pen)
        res, out = out, (out if a.logprobs is None else out.tokens)
        made = out.size(1) - max(len(q) for q in prompts)
        for r, row in enumerate(out.tolist()):
            b, j = divmod(r, a.num_samples)
            line = {"prompt": b, "sample": j, "tokens": row[:len(prompts[b]) + made]}
            if a.logprobs is not None:
                line = with_logprobs(line, res, r, len(prompts[b]), len(prompts[b]) + made, a.logprobs)
            print(json.dumps(line))
        return 0
    if len(prompts) > 1:
        if a.sampler != "device" and a.temperature != 0:
            raise SystemExit("several prompts are served by generate_many, which draws on the device: --sampler device")
        outs = model.generate_many([torch.tensor(q, dtype=torch.int64, device="cuda:0") for q in prompts],
                                   a.max_new_tokens, batch_size=a.batch, temperature=a.temperature, top_k=a.top_k,
                                   top_p=a.top_p, seed=a.seed, eos_token_id=a.eos_token_id, **pen)
        for q, row in zip(prompts, outs):
            if a.logprobs is None:
                print(json.dumps(row.tolist()))
            else:  # (a tuple of 1-D results: one row)
                one = type(row)(*(t[None] for t in row))
                print(json.dumps(with_logprobs(row.tokens.tolist(), one, 0, len(q), row.tokens.numel(), a.logprobs)))
        return 0
    prompt = prompts[0]
    idx = torch.tensor([prompt] * a.batch, dtype=torch.int64, device="cuda:0")
    if a.draft_tokens is not None and a.sampler != "device":
        raise SystemExit("--draft_tokens compares drafts with the device sampler's draws: --sampler device")
    how = (dict(seed=a.seed, draft_tokens=a.draft_tokens) if a.sampler == "device"
           else dict(generator=torch.Generator(device="cuda:0").manual_seed(a.seed)))
    out = model.generate(idx, a.max_new_tokens, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p,
                         eos_token_id=a.eos_token_id, **how, **pen)
    if a.logprobs is not None:
        for r, row in enumerate(out.tokens.tolist()):
            print(json.dumps(with_logprobs(row, out, r, len(prompt), len(row), a.logprobs)))
        return 0
    for row in out.tolist():
        print(json.dumps(row))
    return 0


if __name__ == "__main__":
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments from device memory (see __init__.py)
    sys.exit(main())
