"""Conditions on the attention stress inputs (oracle/attn_stress.py), on the CPU with the fp64 oracle only.

The GPU tests (tests/test_attention_edges_gpu.py) bound the kernels' per-block error by a multiple of the error of
``attn_stress.bf16_model``. That is only meaningful if the inputs reach the kernel paths they are built for and
if the operation is well conditioned on them, which is what is asserted here: a failure here is a bad input,
never a reason to loosen a kernel tolerance."""
import math

import pytest
import torch

from oracle import attn_stress as A
from oracle import dropout_ref

# every (B, T, H) a stress input is run at on the GPU
FWD_SHAPES = [(1, 320, 3), (1, 1024, 3)]
PARITY = [(kind, shape) for kind in ("step", "falling", "plain") for shape in FWD_SHAPES] + [("stairs", (1, 320, 3))]
REDUCED = [("stairs", (1, 1024, 3)), ("spikes", (1, 1024, 3)), ("cliff", (1, 256, 3))]
DROP_SHAPES = [(2, 192, 3), (1, 1024, 3), (3, 256, 5)]
WELL = 1e-2  # an input is well conditioned for a tensor when the rounding model's own worst block error is below this


def _scores(kind, B, T, H):
    q, k, _ = A.split(A.build(kind, B, T, H), B, T, H)
    return A.scores(q.float(), k.float()).view(B * H, T, T)


def test_rescale_events_on_hand_made_scores():
    """Two heads of T = 128: all-zero scores never rescale after tile 0; a single row whose second tile is 6 nats
    (8.66 log2 units) up moves its 16-query group, and so its wave, exactly once; 5 nats (7.2 units) do not."""
    T = 128
    s = torch.zeros(3, T, T, dtype=torch.float64)
    s[1, 100, 64:] = 6.0
    s[2, 100, 64:] = 5.0
    s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
    events, waves = A.rescale_events(s)
    assert events.tolist() == [0, 1, 0] and waves.tolist() == [0, 1, 0]


@pytest.mark.parametrize("B,T,H", FWD_SHAPES + DROP_SHAPES)
def test_plain_inputs_never_rescale_after_the_first_tile(B, T, H):
    """randn q/k/v at unit scale (all the kernel tests had) leave the forward's rescale branch untaken once the
    accumulator is non-empty: the gap the stress inputs close."""
    events, _ = A.rescale_events(_scores("plain", B, T, H))
    assert int(events.sum()) == 0


@pytest.mark.parametrize("B,T,H", FWD_SHAPES)
def test_stress_inputs_reach_the_rescale_paths(B, T, H):
    for kind in ("step", "stairs", "spikes"):
        events, waves = A.rescale_events(_scores(kind, B, T, H))
        print(f"{kind} T={T}: rescales after tile 0 per head {events.tolist()}, waves with one {waves.tolist()}")
        assert int(waves.min()) >= 2, (kind, waves.tolist())
    events, _ = A.rescale_events(_scores("falling", B, T, H))
    assert int(events.sum()) == 0  # the untaken side with P far below 1: late keys underflow instead


@pytest.mark.parametrize("B,T,H", FWD_SHAPES)
def test_step_rows_past_the_step_still_carry_the_early_keys(B, T, H):
    """A skipped or partial rescale shows only if the tiles accumulated before it still matter: the keys before the
    step must hold between 5 % and 90 % of |out| on the rows past it."""
    q, k, v = (t.double() for t in A.split(A.build("step", B, T, H), B, T, H))
    P = torch.softmax(A.scores(q, k), -1)
    for bh in range(B * H):
        ks = T // 2 + 16 * (bh % 4)
        b, h = divmod(bh, H)
        early = P[b, h, ks:, :ks] @ v[b, h, :ks]
        full = P[b, h, ks:] @ v[b, h]
        share = float(early.norm() / full.norm())
        print(f"step T={T} head {bh}: early keys hold {share:.3f} of |out| past the step")
        assert 0.05 <= share <= 0.90, (bh, share)


def test_cliff_future_keys_overflow_inside_every_diagonal_tile():
    """The backward evaluates exp2(s log2e - lse2) for the future keys of a diagonal tile (32 queries x 32 keys in dK/dV,
    32 x 64 in dQ) before masking them. `stairs` rises between tiles only, so there those keys sit at the row's own
    level; on `cliff` they are more than 128 log2 units above the LSE in every 32 x 32 diagonal tile: +inf in fp32."""
    B, T, H = 1, 256, 3
    q, k, _ = (t.double() for t in A.split(A.build("cliff", B, T, H), B, T, H))
    raw = q @ k.transpose(-2, -1) / 8.0
    x = (raw - torch.logsumexp(A.scores(q, k), -1, keepdim=True)) * A.LOG2E  # [B, H, q, key]
    idx = torch.arange(T)
    same_tile_future = (idx[None, :] > idx[:, None]) & (idx[None, :] // 32 == idx[:, None] // 32)
    worst = x.masked_fill(~same_tile_future, float("-inf")).view(B, H, T // 32, 32, T).amax((-1, -2))
    assert float(worst.min()) > 128.0, worst.min()


def test_keep_mask_is_attn_scale_of_one_head():
    T, p = 128, 0.25
    for seed in (A.SEED_LO, A.SEED_HI):
        full = dropout_ref.attn_scale(seed, 3, T, p) != 0
        for bh in range(3):
            assert torch.equal(A.keep_mask(seed, bh, T, p), full[bh])
        assert torch.equal(A.keep_mask(seed, 2, T, p, q=[5, 100]), full[2][[5, 100]])
    # a non-zero high word changes the mask: the seeds are not one stream
    assert not torch.equal(A.keep_mask(A.SEED_HI, 0, T, p), A.keep_mask(77, 0, T, p))


def test_block_err_sees_one_wrong_wave_and_floors_empty_blocks():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(1, 2, 128, 64, generator=g, dtype=torch.float64)
    ref[0, 1, 96:] *= 1e-30  # a block the input drives to nothing
    x = ref.clone()
    x[0, 0, 32:64] *= 1.01
    x[0, 1, 96:] = 0.0
    e = A.block_err(x, ref)
    assert e.shape == (1, 2, 4)
    assert abs(float(e[0, 0, 1]) - 0.01) < 1e-12 and float(e[0, 0, 0]) == 0.0
    assert float(e[0, 1, 3]) < 1e-20  # floored, not 1.0


def test_bf16_model_is_a_bf16_sized_perturbation_of_the_oracle():
    """On plain inputs the model's global errors are those the existing kernel tolerances were sized against
    (about 2e-3 forward, 2.5-3.1e-3 backward)."""
    c = A.case("plain", 1, 320, 3)
    print("plain (1, 320, 3) model errors:", c["model_err"])
    for n in ("out", "dq", "dk", "dv"):
        assert 5e-4 < c["model_err"][n] < 6e-3, (n, c["model_err"][n])


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind,shape", PARITY)
def test_backward_parity_inputs_are_well_conditioned(kind, shape, p):
    c = A.case(kind, *shape, p, A.SEED_HI if p > 0 else A.SEED_LO)
    print(f"{kind} {shape} p={p}: model worst block errors {c['model_err']}")
    for n in ("out", "dq", "dk", "dv"):
        assert c["model_err"][n] <= WELL, (kind, shape, p, n, c["model_err"][n])
    assert c["model_err"]["lse"] <= 2.0 ** -8


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind,shape", REDUCED + [("spikes", (1, 320, 3)), ("stairs", (1, 320, 3))])
def test_forward_and_dv_are_well_conditioned_where_dq_dk_are_not(kind, shape, p):
    """A near-one-hot softmax makes dP - delta cancel against the bf16 rounding of out, so dq / dk of these inputs
    are not a fair target; out, lse and dv stay well conditioned and are what the GPU tests check there."""
    c = A.case(kind, *shape, p, A.SEED_HI if p > 0 else A.SEED_LO)
    print(f"{kind} {shape} p={p}: model worst block errors {c['model_err']}")
    for n in ("out", "dv"):
        assert c["model_err"][n] <= WELL, (kind, shape, p, n, c["model_err"][n])
    assert c["model_err"]["lse"] <= 2.0 ** -8


@pytest.mark.parametrize("seed", [A.SEED_LO, A.SEED_HI])
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("B,T,H", DROP_SHAPES)
def test_dropout_parity_inputs_are_well_conditioned(B, T, H, p, seed):
    c = A.case("plain", B, T, H, p, seed)
    for n in ("out", "dq", "dk", "dv"):
        assert c["model_err"][n] <= WELL, (B, T, H, p, seed, n, c["model_err"][n])


@pytest.mark.parametrize("kind", ["step", "stairs", "falling", "plain"])
def test_fp32_inputs_are_well_conditioned(kind):
    """The fp32 kernels' yardstick is plain fp32 torch: its own worst block error must be fp32-sized."""
    for p in (0.0, 0.1):
        c = A.case(kind, 1, 320, 3, p, A.SEED_HI if p > 0 else A.SEED_LO, f32=True)
        print(f"{kind} fp32 p={p}: model worst block errors {c['model_err']}")
        for n in ("out", "dq", "dk", "dv"):
            assert c["model_err"][n] <= 1e-5, (kind, p, n, c["model_err"][n])
