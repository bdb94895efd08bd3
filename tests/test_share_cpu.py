"""Rows that share a prompt, without a GPU: the session's group bookkeeping (generation.ShareGroups, pure host logic),
the argument checks of fork and num_samples that need no device, and the register budget of the shared kernels."""
import os
import shutil

import pytest
import torch

from gpt_2_distributed_amd.generation import ShareGroups
from tests.test_kernel_resources import HIPCC, _instantiation, _resources


def state(g):
    return g.group, g.length


def check_invariants(g):
    """What the C entries demand of the two arrays (include/gpt2mi.h, v24), whatever happened before."""
    for b in range(g.B):
        lead = g.group[b]
        assert 0 <= lead <= b and g.group[lead] == lead
        assert g.length[b] == g.length[lead] >= 0
        if len(g.members(b)) == 1:
            assert g.length[b] == 0


def test_fork_into_a_fresh_group():
    g = ShareGroups(6)
    assert state(g) == ([0, 1, 2, 3, 4, 5], [0] * 6) and not g.any
    g.fork(0, [2, 3], 70)
    assert state(g) == ([0, 1, 0, 0, 4, 5], [70, 0, 70, 70, 0, 0]) and g.any
    assert g.members(3) == [0, 2, 3] and g.members(1) == [1]
    g.fork(5, [1], 9)  # a second group whose source is not its lowest row
    assert state(g) == ([0, 1, 0, 0, 4, 1], [70, 9, 70, 70, 0, 9])
    check_invariants(g)


def test_fork_from_a_grouped_row_joins_at_the_groups_length():
    g = ShareGroups(6)
    g.fork(2, [3], 70)
    g.fork(3, [0, 5], 99)  # row 3 has grown to 99 since; the copies agree with row 2 below 70 only
    assert state(g) == ([0, 1, 0, 0, 4, 0], [70, 0, 70, 70, 0, 70])
    check_invariants(g)


def test_a_destination_first_leaves_its_group():
    g = ShareGroups(6)
    g.fork(0, [1, 2], 40)
    g.fork(3, [4, 1], 50)  # row 1 moves over
    assert state(g) == ([0, 1, 0, 1, 1, 5], [40, 50, 40, 50, 50, 0])
    g.fork(5, [0], 7)  # row 0 was a source: row 2 is left alone and its group dissolves
    assert state(g) == ([0, 1, 2, 1, 1, 0], [7, 50, 0, 50, 50, 7])
    g.fork(1, [3], 60)  # a member forked onto again: it leaves and rejoins at the group's length
    assert state(g) == ([0, 1, 2, 1, 1, 0], [7, 50, 0, 50, 50, 7])
    check_invariants(g)


def test_fork_without_sharing_leaves_the_destinations_alone():
    g = ShareGroups(4)
    g.fork(0, [1, 2], 33)
    g.fork(0, [2, 3], 33, share=False)
    assert state(g) == ([0, 0, 2, 3], [33, 33, 0, 0])
    g.fork(0, [1], 33, share=False)
    assert state(g) == ([0, 1, 2, 3], [0, 0, 0, 0])


def test_refill_of_the_source_row_hands_over_to_the_next_lowest():
    g = ShareGroups(5)
    g.fork(0, [2, 3], 70)
    g.leave(0)
    assert state(g) == ([0, 1, 2, 2, 4], [0, 0, 70, 70, 0])
    check_invariants(g)


def test_refill_down_to_one_member_dissolves_the_group():
    g = ShareGroups(5)
    g.fork(0, [2, 3], 70)
    g.leave(2)
    assert state(g) == ([0, 1, 2, 0, 4], [70, 0, 0, 70, 0])
    g.leave(3)
    assert state(g) == ([0, 1, 2, 3, 4], [0] * 5) and not g.any
    g.leave(1)  # a row alone: nothing to do
    assert state(g) == ([0, 1, 2, 3, 4], [0] * 5)


def test_reset_dissolves_every_group():
    g = ShareGroups(6)
    g.fork(0, [1], 10)
    g.fork(2, [3, 4], 20)
    g.clear()
    assert state(g) == ([0, 1, 2, 3, 4, 5], [0] * 6) and not g.any


def test_random_histories_keep_the_invariants():
    gen = torch.Generator().manual_seed(5)
    g = ShareGroups(9)
    for _ in range(300):
        rows = torch.randperm(9, generator=gen).tolist()
        if int(torch.randint(0, 3, (1,), generator=gen)):
            k = int(torch.randint(0, 4, (1,), generator=gen))
            g.fork(rows[0], rows[1:1 + k], int(torch.randint(1, 100, (1,), generator=gen)),
                   share=bool(torch.randint(0, 4, (1,), generator=gen)))
        else:
            g.leave(rows[0])
        check_invariants(g)


def test_num_samples_is_checked_before_anything_else():
    """The refusals need neither a GPU nor a model."""
    from gpt_2_distributed_amd import generation
    idx = torch.zeros(13, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="64"):
        generation.generate(None, idx, 4, num_samples=5)  # 65 rows
    with pytest.raises(ValueError, match="num_samples"):
        generation.generate(None, idx, 4, num_samples=0)


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_shared_kernels_have_no_scratch_and_no_spills():
    """And at least 4 waves per SIMD (up to 128 VGPRs): a wave keeps a range's keys and values across its members beside
    attn_range's state and the next member's q, so it may have half of attn_decode_kernel's 8, and no less."""
    kernels = _resources("decode.hip")
    for fmt in ("KvBf16", "KvFp8"):
        k, v = _instantiation(kernels, "attn_decode_shared_kernel", fmt)
        assert v["ScratchSize [bytes/lane]"] == 0, f"{k}: scratch {v}"
        assert v["VGPRs Spill"] == 0, f"{k}: spills {v}"
        assert v["Occupancy [waves/SIMD]"] >= 4, f"{k}: occupancy {v}"
