"""optim.Muon on the tiny model (L2 H2 C128 V509) against the CPU rule on the engine's own gradients."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
CFG = dict(n_layer=2, n_head=2, n_embd=128, vocab_size=509, n_positions=64, resid_pdrop=0.0, attn_pdrop=0.0)
HP = dict(lr=0.02, momentum=0.95, weight_decay=0.01, adamw_lr=1e-3)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _model():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    torch.manual_seed(0)
    return GPT2(GPT2Config(**CFG)).to(dev)


def _fwd_bwd(m, s):
    g = torch.Generator().manual_seed(100 + s)
    idx, labels = (torch.randint(0, 509, (2, 64), generator=g).to(dev) for _ in range(2))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, loss = m(idx, labels=labels)
    loss.backward()


def test_three_steps_vs_the_rule_on_the_engines_gradients():
    from gpt_2_distributed_amd.muon import muon_matrices, muon_reference
    m = _model()
    opt = m.fused_muon(**HP)
    owned = muon_matrices(m)
    names = {n for n, *_ in owned}
    w0 = {n: p.detach().cpu().double() for n, p in m.named_parameters()}
    rest = {n: torch.nn.Parameter(w0[n].clone()) for n in w0 if n not in names}
    adam = torch.optim.AdamW(rest.values(), lr=HP["adamw_lr"], betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    # per matrix: (W, buf) under the fp64 and the bf16 rule
    st = {k: [[w0[k[0]][k[1]:k[1] + k[2]].clone(), torch.zeros(k[2], k[3], dtype=torch.float64)] for _ in range(2)]
          for k in owned}
    for s in range(3):
        _fwd_bwd(m, s)
        grads = {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}
        total = torch.sqrt(sum(g.square().sum() for g in grads.values()))
        opt.step()
        opt.zero_grad()
        assert abs(opt.grad_norm.item() - total.item()) < 1e-5 * total.item()
        for n, p in rest.items():
            p.grad = grads[n]
        adam.step()
        for k in owned:
            g = grads[k[0]][k[1]:k[1] + k[2]]
            for pair, dt in zip(st[k], (torch.float64, torch.bfloat16)):
                pair[0], pair[1] = muon_reference(pair[0], g, pair[1], HP["lr"], HP["momentum"],
                                                  weight_decay=HP["weight_decay"], dtype=dt)
    got = {n: p.detach().cpu() for n, p in m.named_parameters()}
    for n, p in rest.items():
        assert rel_err(got[n], p.detach()) < 1e-6, n  # tests/test_kernels_gpu.py::test_adamw_matches_oracle_and_norm
    for k in owned:
        start, (ref, _), (bf, _) = w0[k[0]][k[1]:k[1] + k[2]], *st[k]
        e_ref = rel_err(bf - start, ref - start)  # the three updates: the weights themselves would hide them
        e = rel_err(got[k[0]][k[1]:k[1] + k[2]].double() - start, ref - start)
        print(f"{k}: E_ref {e_ref:.3e} kernels {e:.3e}")
        assert e <= 2 * e_ref, (k, e, e_ref)
    assert torch.equal(m.engine().shadow, m.arena.to(torch.bfloat16))


def test_adamw_part_has_fused_adamws_bits():
    from gpt_2_distributed_amd.muon import muon_matrices
    a, b = _model(), _model()
    oa = a.fused_muon(adamw_lr=1e-3)
    ob = b.configure_optimizers(learning_rate=1e-3)
    _fwd_bwd(a, 0)
    _fwd_bwd(b, 0)
    b.engine().grad.copy_(a.engine().grad)
    oa.step()
    ob.step()
    names = {n for n, *_ in muon_matrices(a)}
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        assert torch.equal(p, pb[n]) != (n in names), n
    assert torch.equal(oa.grad_norm, ob.grad_norm)


def test_state_dict_round_trip_continues_bit_for_bit():
    a, b = _model(), _model()
    oa, ob = a.fused_muon(**HP), b.fused_muon(**HP)
    for s in range(2):
        _fwd_bwd(a, s)
        oa.step()
        oa.zero_grad()
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in oa.state_dict().items()}
    with torch.no_grad():
        b.arena.copy_(a.arena)
    b.engine().refresh_shadow()
    ob.load_state_dict(sd)
    for m, o in ((a, oa), (b, ob)):
        _fwd_bwd(m, 2)
    b.engine().grad.copy_(a.engine().grad)
    oa.step()
    ob.step()
    assert ob.step_count == 3 and torch.equal(a.arena, b.arena) and torch.equal(a.engine().shadow, b.engine().shadow)
    assert torch.equal(oa.momentum_buffer, ob.momentum_buffer) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)


@pytest.mark.parametrize("case, words", [("fsdp", "FSDP"), ("fp32", "fp32"), ("clip", "max_grad_norm")])
def test_refused(case, words, tmp_path):
    import torch.distributed as dist
    from gpt_2_distributed_amd.optim import Muon
    from gpt_2_distributed_amd.parallel import FullyShardedDataParallel
    m = _model()
    if case == "fp32":
        m.precision = "fp32"
    if case == "fsdp":  # the wrapper asks the process group for its world
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        target = FullyShardedDataParallel(m) if case == "fsdp" else m
        with pytest.raises(ValueError, match=words):
            Muon(target, **({"max_grad_norm": 1.0} if case == "clip" else {}))
    finally:
        if case == "fsdp":
            dist.destroy_process_group()
