"""jh_plan_step_randomized_batch_phases through the C ABI: B domain-randomised fr3_pick plan steps, each in its own phase and with its own table from rollout block to
plant, in one launch of the fr3 kernel on the grid (workgroups of N / G rollouts, G, B) against B calls of jh_plan_step_randomized_phase on the same sub-blocks.

Every comparison is on raw 32-bit words; the single entry is held to jh_plan_step by tests/test_gpu_plan_randomized_fr3.py.  No tolerance appears in this file.  The
controllers are laid out by `Blocks` of tests/test_gpu_plan_ensemble_batch_fr3.py; the plants are D0..D3 of tests/test_fr3_plants_host.py."""

import numpy as np
import pytest

from tests.test_gpu_plan_batch_fr3 import _err, _phase_states
from tests.test_gpu_plan_batch_fr3_models import _models
from tests.test_gpu_plan_ensemble_batch_fr3 import Blocks
from tests.test_gpu_plan_randomized import nominal_rule

pytestmark = pytest.mark.gpu

TABLES = ([2, 0, 1, 2], [0, 0, 3, 1], [3, 3, 3, 3])


def _sets(gpu, B, per_controller):
    """(the launch's set, the B sets of a controller's own M = 4 plants).  Shared: D0..D3; per controller: controller b's plant m is D(b + m) % 4."""
    from judo_amd.device import GpuModelSet

    ms = _models(gpu)
    if not per_controller:
        s = GpuModelSet(list(ms))
        return s, [s] * B
    lists = [[ms[(b + m) % 4] for m in range(4)] for b in range(B)]
    return GpuModelSet([m for plants in lists for m in plants]), [GpuModelSet(plants) for plants in lists]


# ------------------------------------------------------------------------------------------------ 1. three controllers, three tables, three phases
@pytest.mark.parametrize("per_controller", [False, True])
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_three_controllers_with_their_own_tables_and_phases(gpu, opt, per_controller):
    """B = 3, G = 4, N = 12 (Nb = 3: ragged waves), H = 8, K = 4, phases (1, 2, 0).  Only each controller's global rollout 0 is noise-free: the first rollout of a later
    block does not cost what its plant's nominal costs."""
    xs = _phase_states()
    phases = (1, 2, 0)
    bl = Blocks(gpu, 3, 12, 8, 4, seed=111, x0s=[xs[p] for p in phases], phases=phases)
    launch, own = _sets(gpu, 3, per_controller)
    tables = [list(a) for a in TABLES]
    got = bl.rnd_batch(launch, 4, tables, opt)
    bl.rnd_check(own, opt, tables, got, what="set of 12" if per_controller else "shared set")
    assert bl.tickets_at_zero()
    for b in range(3):  # the plants' own single-call costs on controller b's block: what `nominal_rule` reads
        singles = [bl.rnd_single(own[b], opt, b, [p])[0] for p in range(4)]
        nominal_rule(got[0][b], singles, tables[b])
    if per_controller:  # the controller's image stride is read
        on_first = bl.rnd_batch(own[0], 4, tables, opt)
        assert on_first[0][0].tobytes() == got[0][0].tobytes() and all((on_first[0][b] != got[0][b]).any() for b in (1, 2))


# ------------------------------------------------------------------------------------------------ 2. larger launch shapes
@pytest.mark.parametrize("G,N", [(2, 518), (4, 1028)])
def test_launch_shapes_outside_the_full_latency_mode(gpu, G, N):
    """B = 2, H = 4, K = 2.  G = 2, N = 518: 1 036 rollouts, two rows of a wave per rollout, Nb = 259 ragged; G = 4, N = 1 028: 2 056 rollouts, every row its own rollout,
    Nb = 257 ragged -- while a single call of N runs in another mode."""
    xs = _phase_states()
    bl = Blocks(gpu, 2, N, 4, 2, seed=112 + G, x0s=[xs[3], xs[1]], phases=(3, 1))
    launch, own = _sets(gpu, 2, True)
    tables = [[1, 3], [2, 0]] if G == 2 else [[3, 0, 2, 1], [1, 1, 0, 2]]
    bl.rnd_check(own, "cem", tables, bl.rnd_batch(launch, 4, tables, "cem"), what=f"B*N={2 * N}")


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals(gpu):
    import torch

    from judo_amd import _lib
    from judo_amd.device import GpuModel, GpuModelSet

    xs = _phase_states()
    bl = Blocks(gpu, 3, 12, 8, 4, seed=115, x0s=xs[:3], phases=(0, 1, 2))
    launch, own = _sets(gpu, 3, False)
    tables = [list(a) for a in TABLES]
    bufs = bl.outputs()
    bad = [list(a) for a in TABLES]
    bad[1][2] = 4
    assert bl.rnd_raw(launch, 4, bad, bufs) == -1 and "controller 1" in _err() and "block 2" in _err()
    word = bl.host.numpy()[:, bl.o_phase]
    word[1] = 1.5
    assert bl.rnd_raw(launch, 4, tables, bufs) == -1 and "controller 1" in _err() and "phase word" in _err()
    word[1] = 1.0
    assert bl.rnd_raw(launch, 4, tables, bufs, o_phase=bl.nblk) == -1 and "o_phase" in _err()
    leap = GpuModel("leap_cube", gpu)
    assert bl.rnd_raw(GpuModelSet([leap] * 4), 4, tables, bufs) == -3 and "jh_plan_step_randomized_batch plans" in _err()
    # B * G above the table's bytes: B = 5 controllers of G = 64 blocks (the blocks are laid out for 5 controllers; nothing is read before the refusal)
    G = _lib.MAX_PLANT_BLOCKS
    assert 5 * G > _lib.MAX_FLEET_PLANT_BLOCKS
    big = Blocks(gpu, 5, G, 8, 4, seed=116, x0s=[xs[0]] * 5, phases=[0] * 5)
    assert big.rnd_raw(launch, 4, [[0] * G] * 5, big.outputs()) == -1 and "JH_MAX_FLEET_PLANT_BLOCKS" in _err()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == v).all() for t, v in zip(bufs, (-7.0, -7.0, 0.0)))  # nothing ran
    bl.rnd_check(own, "mppi", tables, bl.rnd_batch(launch, 4, tables), what="after the refusals")
