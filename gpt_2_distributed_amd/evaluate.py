"""Evaluate a checkpoint on a token-shard split: ``python -m gpt_2_distributed_amd.evaluate --checkpoint out/step_0001000
--model 124M --data_dir D [--split val] [--batch 8] [--seq_len 1024] [--max_batches N] [--per_token OUT.npy]
[--doc_mask [--eot_token_id 50256] [--eot_position end|begin] [--reset_positions]]``.

Loads ``model.pt`` of a ``save_checkpoint`` directory (as generate.py does), runs ``GPT2.evaluate`` under bf16 autocast
over the split's windows in order (``dataloader.iter_eval_batches``, one rank) and prints one JSON line
``{"loss", "ppl", "tokens", "batches"}``: the token-weighted mean negative log-likelihood and its exponential. With the
trainer's ``--eval_batch`` / ``--eval_steps`` / ``--seq_len`` as ``--batch`` / ``--max_batches`` / ``--seq_len`` the loss
is the ``val_loss`` a one-rank training run printed at that step. ``--per_token`` also saves the fp32 per-token values
[batches * batch, seq_len] (``GPT2.score(reduction="none")``) as a .npy file. ``--doc_mask`` scores every window under
document masking, as the trainer's flag of that name trains (the bounds from the window's own tokens);
``--reset_positions``, valid only with it, also restarts the position embedding at every document, as the trainer's."""
from __future__ import annotations

import json
import os
import pathlib
import sys

import torch

from . import dataloader as gpt2_dataloader
from .generate import load_model
from .model import MODEL_SIZES
from .packing import doc_bounds
from .train_gpt2_distributed import DocMaskParser, add_doc_mask_arguments, doc_mask_from_args


def parse_args(argv=None):
    p = DocMaskParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--checkpoint", required=True, help="a step_XXXXXXX directory written by save_checkpoint")
    p.add_argument("--model", default="124M", choices=sorted(MODEL_SIZES) + ["auto"])
    p.add_argument("--data_dir", required=True)
    p.add_argument("--split", default="val", help="shards whose file name contains this")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--seq_len", type=int, default=gpt2_dataloader.DEFAULT_CONTEXT_LENGTH)
    p.add_argument("--max_batches", type=int, default=None)
    p.add_argument("--per_token", default=None, help="write the per-token losses to this .npy file")
    add_doc_mask_arguments(p)
    return p.parse_args(argv)


def main(argv=None) -> int:
    a = parse_args(argv)
    d = pathlib.Path(a.data_dir)
    paths = gpt2_dataloader.get_shard_paths(d, split=a.split) if d.is_dir() else []
    if not paths:
        raise SystemExit(f"no '{a.split}' shard (*{a.split}*.bin) in {a.data_dir}")
    if a.batch < 1 or a.seq_len < 1:
        raise SystemExit("--batch and --seq_len must be >= 1")
    doc = doc_mask_from_args(a)
    model = load_model(a.checkpoint, a.model)
    if a.seq_len > model.config.n_positions:
        raise SystemExit(f"--seq_len {a.seq_len} > the checkpoint's context length {model.config.n_positions}")
    batches = lambda: gpt2_dataloader.iter_eval_batches(paths, a.seq_len, a.batch, 0, 1, a.max_batches)  # noqa: E731
    with torch.autocast("cuda", dtype=torch.bfloat16):
        res = model.evaluate(batches(), **doc)
        if a.per_token:
            import numpy as np

            def bounds(x):
                return doc_bounds(x, doc["eot_token_id"], doc["eot"]) if doc else None
            reset = doc.get("reset_positions", False)
            rows = [model.score(x, y.to("cuda:0"), reduction="none", doc_bounds=bounds(x), reset_positions=reset).cpu()
                    for x, y in ((x.to("cuda:0"), y) for x, y in batches())]
            np.save(a.per_token, torch.cat(rows).numpy() if rows else np.zeros((0, a.seq_len), dtype=np.float32))
    if not res["tokens"]:
        raise SystemExit(f"the '{a.split}' split holds no full batch of {a.batch} windows of {a.seq_len + 1} tokens")
    n = len(gpt2_dataloader.eval_windows(paths, a.seq_len)) // a.batch
    res["batches"] = n if a.max_batches is None else min(n, max(0, a.max_batches))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments from device memory (see __init__.py)
    sys.exit(main())
