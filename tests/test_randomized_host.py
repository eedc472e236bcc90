"""The host side of the domain-randomised plan step (judo_amd/randomized.py): the apportionment of rollout blocks to plants by weight, the assignment's validation and
the plant of every rollout.  Hand-worked cases, no GPU."""

import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(a, M):
    return [a.count(m) for m in range(M)]


@pytest.mark.parametrize("weights,G,counts", [
    ([1, 1, 1], 6, [2, 2, 2]),          # equal weights, G a multiple of M
    ([0.5, 0.3, 0.2], 10, [5, 3, 2]),   # exact quotas (10 * 0.3 is 3.0000000000000004 in fp64: still three)
    ([1, 0, 0], 4, [4, 0, 0]),          # everything on one plant
    ([0, 2, 0], 3, [0, 3, 0]),
    ([1, 1], 3, [2, 1]),                # a tie of the remainders 0.5 / 0.5: the lower index takes the open block
    ([1, 1, 1], 4, [2, 1, 1]),          # quotas 4/3: one open block, three equal remainders
    ([1, 1, 1], 2, [1, 1, 0]),          # G below the number of non-zero weights: the lower indices, one each
    ([3, 1, 1, 0], 2, [1, 1, 0, 0]),    # quotas 1.2, 0.4, 0.4, 0: floor 1 0 0 0, the open block to plant 1 (tie with plant 2)
    ([0.7, 0.2, 0.1], 8, [6, 1, 1]),    # quotas 5.6, 1.6, 0.8: floor 5 1 0, two open blocks to remainders 0.8 (plant 2) and 0.6 (plants 0 / 1 tie: plant 0)
    ([5], 7, [7]),                      # M = 1
])
def test_blocks_from_weights(weights, G, counts):
    from judo_amd.randomized import blocks_from_weights

    a = blocks_from_weights(weights, G)
    assert isinstance(a, list) and all(isinstance(p, int) for p in a)
    assert len(a) == G and _counts(a, len(weights)) == counts
    assert a == sorted(a)  # the blocks of one plant are adjacent, plants in rising order
    assert all(weights[p] > 0 for p in a)  # a zero weight gets no block


def test_blocks_from_weights_refuses_bad_weights():
    from judo_amd.randomized import blocks_from_weights

    for w in ([], [0, 0], [1, -1], [1, float("nan")], [float("inf"), 1]):
        with pytest.raises(ValueError, match="weights"):
            blocks_from_weights(w, 4)
    with pytest.raises(ValueError, match="blocks = 0"):
        blocks_from_weights([1, 1], 0)


def test_assignment_validation():
    from judo_amd.randomized import MAX_PLANT_BLOCKS, check_assignment

    assert check_assignment([2, 0, 1], 3) == [2, 0, 1]
    assert check_assignment(np.array([1, 1, 0, 2, 2, 2]), 3) == [1, 1, 0, 2, 2, 2]  # G > M, repeats
    assert check_assignment([0] * MAX_PLANT_BLOCKS, 1) == [0] * MAX_PLANT_BLOCKS
    with pytest.raises(ValueError, match=r"assignment\[1\] = 3 outside \[0, M = 3\).*block 1"):
        check_assignment([0, 3], 3)
    with pytest.raises(ValueError, match=r"assignment\[0\] = -1"):
        check_assignment([-1, 0], 3)
    with pytest.raises(ValueError, match=r"assignment\[2\] = 1.5"):
        check_assignment([0, 1, 1.5], 3)
    with pytest.raises(ValueError, match="0 blocks"):
        check_assignment([], 3)
    with pytest.raises(ValueError, match=f"{MAX_PLANT_BLOCKS + 1} blocks.*JH_MAX_PLANT_BLOCKS"):
        check_assignment([0] * (MAX_PLANT_BLOCKS + 1), 3)


def test_plant_of_rollout():
    from judo_amd.randomized import plant_of_rollout

    got = plant_of_rollout([2, 0, 1], 12)
    assert got.shape == (12,) and got.dtype.kind == "i"
    assert got.tolist() == [2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 1, 1]
    assert plant_of_rollout([3, 0, 2, 0], 24).tolist() == [3] * 6 + [0] * 6 + [2] * 6 + [0] * 6
    assert plant_of_rollout([2], 5).tolist() == [2] * 5
    with pytest.raises(ValueError, match=r"num_rollouts % blocks != 0"):
        plant_of_rollout([0, 1, 2], 8)


def test_the_block_limit_agrees_with_the_header():
    from judo_amd import _lib
    from judo_amd.randomized import MAX_PLANT_BLOCKS

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    assert int(re.search(r"#define JH_MAX_PLANT_BLOCKS (\d+)", header).group(1)) == _lib.MAX_PLANT_BLOCKS == MAX_PLANT_BLOCKS
    assert MAX_PLANT_BLOCKS % 4 == 0  # (the kernels' table packs four blocks to a word)
    assert "jh_plan_step_randomized" in _lib.EXPORTED_SYMBOLS


def test_fr3_and_spot_are_refused_without_a_device():
    """The constructor's refusals come before any model is made."""
    from judo_amd.config import ControllerConfig
    from judo_amd.randomized import RandomizedController
    from judo_amd.tasks import get_registered_tasks

    tasks = get_registered_tasks()
    with pytest.raises(ValueError, match="fr3_pick has no randomised plan step"):
        t = tasks["fr3_pick"][0]()
        RandomizedController(ControllerConfig(), t, None, [t.desc])
    with pytest.raises(ValueError, match="Spot policy tasks have no randomised plan step"):
        t = tasks["spot_box_push"][0]()
        RandomizedController(ControllerConfig(), t, None, [t.desc])
