"""The GEMM kernel planner (csrc/gemm_plan.h) against recorded choices (CPU only: the planner is plain host C++).

tests/golden/gemm_plan.json holds, for every GEMM of a step (124M, 1.5B, the smoke model), the edges of each selection
rule and the weight-gradient entries, the launches the library made at ABI v14 (the last version whose entry points
chose their kernels inline), recorded at a CU count of 256. A row is [entry point, arguments, outcomes]: the arguments
without `sched` (gpt2mi_gemm: layout epi M N K lda ldb splits; the weight gradients: M N K lda ldb splits; grouped:
problems K splits), and one outcome [variants, return code, launches] per distinct result, `variants` listing the
sched values (gpt2mi_gemm: sched + 65536 when dbias is given) that gave it. A launch reads
    <pp|g256|g128> <a_t b_t epi map persistent bnd dyn grouped: one digit each> grid splits k_per_split
    reduce <plain|t|grouped> <f32|bf16> splits          colsum
The planner must name exactly that sequence; rows v14 refused, and rows with a schedule low byte retired since
(3, 4, 5, 7, 8: recorded as v14 ran them), must be refused."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gpt_2_distributed_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
RETIRED = (3, 4, 5, 7, 8)


def _cases(rows):
    """(input line of gemm_plan_check, sched, return code, launches) of every recorded call"""
    for entry, args, outcomes in rows:
        if entry == "wgrad_kt":  # M N K lda ldb splits: the leading dimensions do not enter the plan
            args = args[:3] + args[5:]
        elif entry == "wgrad_grouped":
            probs, rest = args[0], args[1:]
            args = [len(probs)] + [x for p in probs for x in p] + rest
        for variants, rc, launches in outcomes:
            for v in variants:
                sched, tail = (v & 0xffff, [v >> 16, v & 0xffff]) if entry == "gemm" else (v, [v])
                yield " ".join([entry] + [str(a) for a in args + tail]), sched, rc, launches


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_planner_reproduces_the_recorded_choices(tmp_path):
    exe = str(tmp_path / "gemm_plan_check")
    # -x c++: plain host C++ (no HIP headers, no device pass)
    out = subprocess.run([HIPCC, "-x", "c++", "-std=c++20", "-O1", "-Wall", "-Werror", f"-I{CSRC}",
                          f"-I{CSRC}/../../include", os.path.join(HERE, "gemm_plan_check.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = json.load(open(os.path.join(HERE, "golden", "gemm_plan.json")))
    lines, want = [], []
    for line, sched, rc, launches in _cases(rows):
        assert rc in (0, 22), line
        retired = line.split()[0] in ("gemm", "wgrad") and (sched & 0xff) in RETIRED
        lines.append(line)
        want.append("refused" if rc == 22 or retired else " | ".join(launches))
    run = subprocess.run([exe, "256"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.splitlines()
    assert len(got) == len(want) > 3000
    wrong = [(l, w, g) for l, w, g in zip(lines, want, got) if w != g]
    assert not wrong, f"{len(wrong)} of {len(want)} rows differ; first: {wrong[:5]}"
    # the table exercises every family, the persistent and work-queue schedules, bounded tiles and every reduction
    seen = " ".join(want)
    for needle in ("pp 00001000", "pp 00201010", "pp 116301", "pp 1172", "pp 11630001",
                   "g256 ", "g128 ", "reduce plain f32", "reduce plain bf16", "reduce t f32", "reduce t bf16",
                   "reduce grouped f32", "colsum", "refused"):
        assert needle in seen, needle
