"""Sample from a checkpoint: ``python -m gpt_2_distributed_amd.generate --checkpoint out/step_0001000 --model 124M
--prompt_ids 50256 --max_new_tokens 64 [--temperature T --top_k K --top_p P --sampler {torch,device} --seed S --batch B
--draft_tokens K --repetition_penalty R --presence_penalty P --frequency_penalty F --kv_dtype {bf16,fp8}
--num_samples S]``.

Loads ``model.pt`` of a ``save_checkpoint`` directory (train_gpt2_distributed.py) into a GPT2 of the named size, runs
``GPT2.generate`` on ``--batch`` copies of the prompt and prints one JSON list of token ids per sequence (prompt
included). No tokenizer is shipped: prompts and outputs are GPT-2 BPE ids (50256 = <|endoftext|>).

Several prompts: repeat ``--prompt_ids`` or give ``--prompts_file`` (one comma-separated prompt per line). They go
through ``GPT2.generate_many`` (continuous batching on the device sampler, ``--batch`` rows at a time; prompt i draws from
(``--seed``, i, position)) and one JSON list per prompt is printed, in input order.

``--num_samples S`` (S > 1) draws S continuations of every prompt through ``GPT2.generate(num_samples=S)``: each prompt
is run once and its rows share its cache. One JSON object per sample is printed, prompt-major:
``{"prompt": b, "sample": j, "tokens": [...]}`` (the prompt's own padding, if the prompts differ in length, removed).
``--batch`` is not used then; prompts x S <= 64."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

from .model import GPT2, GPT2Config, MODEL_SIZES


def parse_args(argv=None):
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
    return p.parse_args(argv)


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
    if a.num_samples > 1:
        if a.draft_tokens is not None and a.sampler != "device":
            raise SystemExit("--draft_tokens compares drafts with the device sampler's draws: --sampler device")
        how = (dict(seed=a.seed, draft_tokens=a.draft_tokens) if a.sampler == "device"
               else dict(generator=torch.Generator(device="cuda:0").manual_seed(a.seed)))
        out = model.generate([torch.tensor(q, dtype=torch.int64, device="cuda:0") for q in prompts], a.max_new_tokens,
                             temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, eos_token_id=a.eos_token_id,
                             num_samples=a.num_samples, **how, **pen)
        made = out.size(1) - max(len(q) for q in prompts)
        for r, row in enumerate(out.tolist()):
            b, j = divmod(r, a.num_samples)
            print(json.dumps({"prompt": b, "sample": j, "tokens": row[:len(prompts[b]) + made]}))
        return 0
    if len(prompts) > 1:
        if a.sampler != "device" and a.temperature != 0:
            raise SystemExit("several prompts are served by generate_many, which draws on the device: --sampler device")
        outs = model.generate_many([torch.tensor(q, dtype=torch.int64, device="cuda:0") for q in prompts],
                                   a.max_new_tokens, batch_size=a.batch, temperature=a.temperature, top_k=a.top_k,
                                   top_p=a.top_p, seed=a.seed, eos_token_id=a.eos_token_id, **pen)
        for row in outs:
            print(json.dumps(row.tolist()))
        return 0
    prompt = prompts[0]
    idx = torch.tensor([prompt] * a.batch, dtype=torch.int64, device="cuda:0")
    if a.draft_tokens is not None and a.sampler != "device":
        raise SystemExit("--draft_tokens compares drafts with the device sampler's draws: --sampler device")
    how = (dict(seed=a.seed, draft_tokens=a.draft_tokens) if a.sampler == "device"
           else dict(generator=torch.Generator(device="cuda:0").manual_seed(a.seed)))
    out = model.generate(idx, a.max_new_tokens, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p,
                         eos_token_id=a.eos_token_id, **how, **pen)
    for row in out.tolist():
        print(json.dumps(row))
    return 0


if __name__ == "__main__":
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments from device memory (see __init__.py)
    sys.exit(main())
