"""The workload for a kernel trace of gpt2mi_lm_loss alone: 25 launches at M = 8192 and 25 at M = 65536 (C = 768, the
GPT-2 vocabulary), nothing else on the device. Run it under the profiler, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o lm -- python tools/lm_loss_trace.py

and read the two kernels' durations per shape from OUT/lm_kernel_trace.csv (profiles/eval/lm_loss_kernel_trace.json holds
the medians of launches 6-25 of each shape)."""
import sys, os, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_2_distributed_amd import _lib as K
V, VP, C = 50257, 50432, 768
for M in (8192, 65536):
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, C, generator=g).bfloat16().cuda()
    w = (0.02 * torch.randn(VP, C, generator=g)).bfloat16().cuda()
    labels = torch.randint(0, V, (M,), generator=g).cuda()
    rows, lse = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    s, n, mean = (torch.empty(1, device="cuda") for _ in range(3))
    ws = torch.empty(K.lm_loss_workspace(M, V), device="cuda")
    for _ in range(25):
        K.lm_loss(x, C, w, C, VP, labels, M, V, C, rows, lse, ws, loss_sum=s, count=n, loss_mean=mean)
    torch.cuda.synchronize()
