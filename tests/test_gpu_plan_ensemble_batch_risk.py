"""jh_plan_step_ensemble_batch_risk and jh_plan_step_ensemble_batch_phases_risk through the C ABI: B ensemble plan steps in one call, each controller under the risk
record in its own packed block -- counted (`worst`) where the tail word is 0.0, plant-weighted otherwise.

Everything is compared bit for bit, no tolerance anywhere:
  member_costs   those of the unweighted batched entry on the same inputs: the rollout launch is the same call;
  controller b   its costs and output record are jh_plan_step_ensemble_weighted[_phase]'s with its weights and tail, or jh_plan_step_ensemble[_phase]'s with worst[b]
                 where its tail word is 0.0, on its block, noise and plants with buffers of their own;
  all zero       a launch with every tail word 0.0 equals jh_plan_step_ensemble_batch[_phases] in every output;
  the tickets    left at zero, and the completion word at its old value + 1.
B = 3, M = 3, N = 64, H = 8, K = 4 throughout: controller 0 counted with `worst` = 2, controller 1 general weights with tail 0.4, controller 2 one-hot weights with
tail 1.  The blocks live in a pinned host buffer with NaN between them and behind the records; the closed-form models read it in place (blk_dev == blk_host) or have it
uploaded into a device buffer that starts as NaN, the others have it uploaded."""

import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_plan_batch import OPTS, _err
from tests.test_gpu_plan_ensemble_batch import FleetProblems, _plants
from tests.test_gpu_plan_ensemble_batch_fr3 import OPTS as FR3_OPTS  # (the arm's own: `Blocks`' calls use them)
from tests.test_gpu_plan_ensemble_batch_fr3 import Blocks, _sets

pytestmark = pytest.mark.gpu

B, M, N, H, K = 3, 3, 64, 8, 4
PAD_REC = 3  # floats behind a block's risk record, NaN
WORST = [2, 1, 3]
RECORDS = [[0.0, 0.0, 0.0, 0.0], [0.4, 0.2, 0.5, 0.3], [1.0, 0.0, 0.0, 1.0]]  # tail | weights


def _ints(v):
    return (C.c_int * len(v))(*v)


def _floats(v):
    return (C.c_float * len(v))(*[float(x) for x in v])


def _same(x, y, what):
    np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32), err_msg=what)


def _widen(blocks, nblk, records):
    """The (B, stride) blocks with a risk record behind each: a pinned (B, nblk + 1 + M + PAD_REC) buffer, NaN where nothing stands."""
    import torch

    host = torch.full((len(records), nblk + 1 + M + PAD_REC), float("nan"), dtype=torch.float32).pin_memory()
    h = host.numpy()
    h[:, :nblk] = blocks[:, :nblk]
    h[:, nblk : nblk + 1 + M] = np.asarray(records, dtype=np.float32)
    return host


# ------------------------------------------------------------------------------------------------ cartpole, cylinder_push, leap_cube
class RiskFleet(FleetProblems):
    """`FleetProblems` whose blocks carry a risk record each: the pinned host buffer `host`, a device copy under `pr.blocks` (what the base's `call` and `single`
    read: the five sections are the same bytes), and `dev`, the device buffer an uploading call writes."""

    def __init__(self, gpu, task, plants, seed, records=RECORDS):
        import torch

        super().__init__(gpu, task, plants, B, M, N, K, H, seed)
        pr = self.pr
        self.host = _widen(pr.blocks.cpu().numpy(), pr.nblk, records)
        pr.blk_stride = self.host.shape[1]
        pr.blocks = self.host.to(gpu)
        self.dev = torch.full_like(pr.blocks, float("nan"))
        self.o_risk = pr.nblk

    def records(self, records):
        self.host.numpy()[:, self.o_risk : self.o_risk + 1 + M] = np.asarray(records, dtype=np.float32)

    def risk_args(self, opt, worst, member, costs, out, mark, in_place):
        a = self.args(opt, worst, member, costs, out, mark)
        a[3], a[4], a[5] = (self.host if in_place else self.dev).data_ptr(), self.host.data_ptr(), 4 * (self.pr.nblk + 1 + M)
        a.insert(11, self.o_risk)
        return a

    def call_risk(self, opt, worst, in_place, use_mark=False):
        """(member_costs (B, M, N), costs (B, N), nominal | sigma (B, 2 KU)) of one jh_plan_step_ensemble_batch_risk."""
        import torch

        from judo_amd import _lib

        pr = self.pr
        member = torch.full((B, M, N), -7.0, dtype=torch.float32, device=pr.dev)
        costs = torch.full((B, N), -7.0, dtype=torch.float32, device=pr.dev)
        out = torch.zeros((B, pr.out_stride), dtype=torch.float32, device=pr.dev)
        a = self.risk_args(opt, worst, member.data_ptr(), costs.data_ptr(), out.data_ptr(), self.mark.data_ptr() if use_mark else out.data_ptr(), in_place)
        _lib.check(pr.lib.jh_plan_step_ensemble_batch_risk(*a), "jh_plan_step_ensemble_batch_risk")
        _lib.check(pr.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:, 2 * pr.KU :] == 0).all(), "the call wrote between the output records"
        return member.cpu().numpy(), costs.cpu().numpy(), o[:, : 2 * pr.KU].copy()

    def single_weighted(self, opt, b, weights, tail):
        """jh_plan_step_ensemble_weighted of controller b alone: (member_costs (M, N), costs (N,), nominal | sigma (2 KU,))."""
        import torch

        from judo_amd import _lib

        pr = self.pr
        mode, lam, k, tie = OPTS[opt]
        member = torch.full((M, N), -7.0, dtype=torch.float32, device=pr.dev)
        costs = torch.full((N,), -7.0, dtype=torch.float32, device=pr.dev)
        out = torch.zeros(2 * pr.KU, dtype=torch.float32, device=pr.dev)
        scratch = torch.zeros(pr.per_scratch, dtype=torch.float32, device=pr.dev)
        p = pr.blocks.data_ptr() + 4 * b * pr.blk_stride
        st = pr.lib.jh_plan_step_ensemble_weighted(self.sets[b].handle, p, p, 4 * pr.nblk, pr.off[1], pr.off[2], pr.off[3], pr.off[4], pr.noise.data_ptr() + 4 * b * pr.noise_stride, pr.ldn,
                                                   pr.W.data_ptr(), N, pr.H, pr.K, member.data_ptr(), costs.data_ptr(), _floats(weights), tail, mode, lam, k, tie, scratch.data_ptr(),
                                                   out.data_ptr(), out.data_ptr(), None, 0)
        _lib.check(st, "jh_plan_step_ensemble_weighted")
        _lib.check(pr.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        return member.cpu().numpy(), costs.cpu().numpy(), out.cpu().numpy()

    def alone(self, opt, b, worst, record):
        return self.single(opt, b, worst) if record[0] == 0.0 else self.single_weighted(opt, b, record[1:], record[0])


def _fleet_plants(gpu, task, per_controller):
    """M plants that every controller shares, or B * M, controller-major, in which no two controllers have the same list."""
    ps = _plants(gpu, task)
    if not per_controller:
        return list(ps[:M])
    return [ps[(b + m) % len(ps)] for b in range(B) for m in range(M)] if len(ps) < B * M else list(ps[: B * M])


CASES = [(t, True, pc) for t in ("cartpole", "cylinder_push") for pc in (False, True)] + [(t, False, pc) for t in ("cartpole", "cylinder_push", "leap_cube") for pc in (False, True)]


@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
@pytest.mark.parametrize("task,in_place,per_controller", CASES)
def test_mixed_records(gpu, task, in_place, per_controller, opt):
    from judo_amd.ensemble import aggregate_costs_risk_batch_host

    fp = RiskFleet(gpu, task, _fleet_plants(gpu, task, per_controller), seed=71)
    assert fp.set.info()["B"] == (B * M if per_controller else M)
    plain = fp.call(opt, WORST)  # jh_plan_step_ensemble_batch on the same inputs
    old = 0xFFFFFFFE
    fp.mark.numpy().view(np.uint32)[0] = old
    got = fp.call_risk(opt, WORST, in_place, use_mark=True)
    assert int(fp.mark.numpy().view(np.uint32)[0]) == old + 1 and (fp.tickets() == 0).all()
    tag = f"{task} {opt} {'in place' if in_place else 'uploaded'} {'B * M plants' if per_controller else 'M plants'}"
    assert got[0].tobytes() == plain[0].tobytes(), f"{tag}: member costs against the unweighted batched entry's"
    if not in_place:
        assert fp.dev.cpu().numpy()[:, : fp.o_risk + 1 + M].tobytes() == fp.host.numpy()[:, : fp.o_risk + 1 + M].tobytes()  # the records went up with the blocks
    _same(got[1], aggregate_costs_risk_batch_host(got[0], WORST, RECORDS), f"{tag}: costs against the restatement")
    for b in range(B):
        m1, c1, o1 = fp.alone(opt, b, WORST[b], RECORDS[b])
        for name, x, y in (("member costs", got[0][b], m1), ("costs", got[1][b], c1), ("nominal | sigma", got[2][b], o1)):
            _same(x, y, f"{tag} controller {b} record {RECORDS[b]}: {name}")
    assert got[1][2].tobytes() == got[0][2][2].tobytes()  # one-hot, tail 1: the member's row
    assert got[1][1].tobytes() != plain[1][1].tobytes()  # the record matters
    again = fp.call_risk(opt, WORST, in_place)  # by the stream's event, on the same scratch
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)) and (fp.tickets() == 0).all()
    fp.records([[0.0] * (1 + M)] * B)
    zero = fp.call_risk(opt, WORST, in_place)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(zero, plain)), f"{tag}: every tail word 0.0 against jh_plan_step_ensemble_batch"
    assert (fp.tickets() == 0).all()


# ------------------------------------------------------------------------------------------------ fr3_pick
class RiskBlocks(Blocks):
    """`Blocks` with a risk record behind every block's phase word."""

    def __init__(self, dev, seed, x0s, phases, records=RECORDS):
        import torch

        super().__init__(dev, B, N, H, K, seed, x0s, phases)
        self.o_risk = self.nblk
        self.host = _widen(self.host.numpy(), self.nblk, records)
        self.blk_stride = self.host.shape[1]
        self.blocks_dev = torch.full((B * self.blk_stride,), float("nan"), dtype=torch.float32, device=dev)

    def records(self, records):
        self.host.numpy()[:, self.o_risk : self.o_risk + 1 + M] = np.asarray(records, dtype=np.float32)

    def risk_raw(self, set_, worst, bufs, opt="mppi", use_mark=False, o_phase=None, o_risk=None, blk_bytes=None, entry=None):
        mode, lam, k, tie = FR3_OPTS[opt]
        mc, costs, out = bufs
        entry = entry or self.lib.jh_plan_step_ensemble_batch_phases_risk
        offs = [self.o_phase if o_phase is None else o_phase, self.o_risk if o_risk is None else o_risk]
        if entry is self.lib.jh_plan_step_ensemble_batch_risk:
            offs = offs[1:]
        return entry(set_.handle, B, M, self.blocks_dev.data_ptr(), self.host.data_ptr(), 4 * (self.nblk + 1 + M) if blk_bytes is None else blk_bytes, 4 * self.blk_stride, self.off[1],
                     self.off[2], self.off[3], self.off[4], *offs, self.noise.data_ptr(), self.ldn, self.noise_stride, self.W.data_ptr(), self.N, self.H, self.K, mc.data_ptr(),
                     costs.data_ptr(), _ints(worst), mode, lam, k, tie, self.batch_scratch.data_ptr(), out.data_ptr(), self.out_stride, self.mark.data_ptr() if use_mark else out.data_ptr(),
                     None, 0)

    def risk_batch(self, set_, worst, opt, use_mark=False):
        bufs = self.outputs(M)
        o = self._finish(self.risk_raw(set_, worst, bufs, opt, use_mark), "jh_plan_step_ensemble_batch_phases_risk", bufs[2])
        return bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), o

    def single_weighted(self, set_, opt, b, weights, tail):
        import torch

        from judo_amd import _lib

        mode, lam, k, tie = FR3_OPTS[opt]
        mc = torch.full((M, self.N), -7.0, dtype=torch.float32, device=self.dev)
        costs = torch.full((self.N,), -7.0, dtype=torch.float32, device=self.dev)
        out = torch.zeros(self.rec, dtype=torch.float32, device=self.dev)
        scratch = torch.zeros(self.per_scratch, dtype=torch.float32, device=self.dev)
        blk = torch.full((self.nblk,), float("nan"), dtype=torch.float32, device=self.dev)
        st = self.lib.jh_plan_step_ensemble_weighted_phase(set_.handle, blk.data_ptr(), self.host.data_ptr() + 4 * b * self.blk_stride, 4 * self.nblk, self.off[1], self.off[2], self.off[3],
                                                           self.off[4], self.noise.data_ptr() + 4 * b * self.noise_stride, self.ldn, self.W.data_ptr(), self.phases[b], self.N, self.H, self.K,
                                                           mc.data_ptr(), costs.data_ptr(), _floats(weights), tail, mode, lam, k, tie, scratch.data_ptr(), out.data_ptr(), out.data_ptr(), None, 0)
        _lib.check(st, "jh_plan_step_ensemble_weighted_phase")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        return mc.cpu().numpy(), costs.cpu().numpy(), out.cpu().numpy()


def _fr3_blocks(gpu, seed):
    from tests.test_gpu_plan_batch_fr3 import _phase_states

    xs = _phase_states()
    return RiskBlocks(gpu, seed, x0s=[xs[0], xs[2], xs[2]], phases=(0, 2, 2))  # two different phases in one launch


@pytest.mark.parametrize("per_controller", [False, True])
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_fr3_mixed_records_in_two_phases(gpu, opt, per_controller):
    from judo_amd.ensemble import aggregate_costs_risk_batch_host

    bl = _fr3_blocks(gpu, seed=171)
    launch, own = _sets(gpu, B, M, per_controller)
    plain = bl.ens_batch(launch, M, WORST, opt)  # jh_plan_step_ensemble_batch_phases on the same inputs
    old = 0xFFFFFFFE
    bl.mark.numpy().view(np.uint32)[0] = old
    got = bl.risk_batch(launch, WORST, opt, use_mark=True)
    assert int(bl.mark.numpy().view(np.uint32)[0]) == old + 1 and bl.tickets_at_zero()
    tag = f"fr3_pick {opt} {'B * M plants' if per_controller else 'M plants'}"
    assert got[0].tobytes() == plain[0].tobytes(), f"{tag}: member costs against the unweighted batched entry's"
    _same(got[1], aggregate_costs_risk_batch_host(got[0], WORST, RECORDS), f"{tag}: costs against the restatement")
    for b in range(B):
        rec = RECORDS[b]
        alone = bl.ens_single(own[b], opt, b, WORST[b]) if rec[0] == 0.0 else bl.single_weighted(own[b], opt, b, rec[1:], rec[0])
        for name, x, y in zip(("member costs", "costs", "nominal | sigma"), (g[b] for g in got), alone):
            _same(x, y, f"{tag} controller {b} (phase {bl.phases[b]}) record {rec}: {name}")
    assert got[1][1].tobytes() != plain[1][1].tobytes()  # the record matters
    bl.records([[0.0] * (1 + M)] * B)
    zero = bl.risk_batch(launch, WORST, opt)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(zero, plain)), f"{tag}: every tail word 0.0 against jh_plan_step_ensemble_batch_phases"
    assert bl.tickets_at_zero()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(gpu):
    """Every refusal comes before anything is enqueued: the outputs, the ticket words and the mark stay as they were."""
    import torch

    from judo_amd.device import GpuModel, GpuModelSet

    plants = _plants(gpu, "cartpole")
    fp = RiskFleet(gpu, "cartpole", list(plants[:M]), seed=11)
    pr, L = fp.pr, fp.pr.lib
    member = torch.full((B, M, N), -7.0, dtype=torch.float32, device=gpu)
    costs = torch.full((B, N), -7.0, dtype=torch.float32, device=gpu)
    out = torch.zeros((B, pr.out_stride), dtype=torch.float32, device=gpu)
    fp.mark.numpy().view(np.uint32)[0] = 41
    base = fp.risk_args("mppi", WORST, member.data_ptr(), costs.data_ptr(), out.data_ptr(), fp.mark.data_ptr(), in_place=False)
    names = ["set", "B", "M", "blk_dev", "blk_host", "blk_bytes", "blk_stride_bytes", "o_nominal", "o_sigma", "o_tp", "o_lohi", "o_risk", "noise", "ldn", "noise_stride_floats", "W", "N", "H",
             "K", "member_costs", "costs", "worst", "mode", "lambda", "k", "tie_high", "scratch", "out", "out_stride_floats", "out_host_mark", "timing", "stream"]
    assert len(names) == len(base)

    def call(**kw):
        a = list(base)
        for key, v in kw.items():
            a[names.index(key)] = v
        return L.jh_plan_step_ensemble_batch_risk(*a)

    who = "plan_step_ensemble_batch_risk: "
    # what the unweighted batched entry refuses
    for ptr in ("set", "blk_dev", "blk_host", "noise", "W", "member_costs", "costs", "worst", "scratch", "out"):
        assert call(**{ptr: None}) == -1 and who + f"{ptr} is a null pointer" in _err(), ptr
    assert call(B=257, worst=_ints([1] * 257)) == -1 and "B = 257" in _err() and "JH_MAX_ENSEMBLE_FLEET = 256" in _err()
    assert call(B=0) == -1 and "B = 0" in _err()
    four = GpuModelSet(list(plants[:4]))
    assert call(set=four.handle) == -1 and "a set of 4 members" in _err() and "M = 3" in _err() and "B * M = 9" in _err()
    four.close()
    big = GpuModelSet([plants[0]] * 33)
    assert call(set=big.handle, M=33) == -1 and "M = 33" in _err() and "JH_MAX_ENSEMBLE = 32" in _err()
    big.close()
    assert call(N=0) == -1 and "N, H, K must be positive" in _err()
    assert call(ldn=N - 1) == -1 and f"ldn ({N - 1}) < N ({N})" in _err()
    assert call(o_sigma=-1) == -1 and "negative block offset" in _err()
    assert call(blk_bytes=4 * pr.nblk - 4) == -1 and "does not hold" in _err()
    assert call(blk_stride_bytes=4 * pr.nblk - 4) == -1 and "blk_stride_bytes" in _err()
    assert call(noise_stride_floats=pr.KU * pr.ldn - 1) == -1 and "noise_stride_floats" in _err()
    assert call(out_stride_floats=2 * pr.KU - 1) == -1 and "out_stride_floats" in _err()
    assert call(mode=2) == -1 and "mode must be" in _err()
    assert call(mode=0, **{"lambda": 0.0}) == -1 and "temperature" in _err()
    assert call(mode=1, k=0) == -1 and "k = 0" in _err()
    forced = GpuModel("cartpole", gpu)
    forced.set_plan_step_launches(1)
    one = GpuModelSet([forced])
    assert call(set=one.handle, M=1, worst=_ints([1, 1, 1])) == -1 and "one launch is forced" in _err()
    one.close()
    # `worst` of every controller, weighted or not
    assert call(worst=_ints([0, 1, 3])) == -1 and "controller 0" in _err() and "worst = 0" in _err()  # (the counted one)
    assert call(worst=_ints([2, 4, 3])) == -1 and "controller 1" in _err() and "worst = 4" in _err() and "M = 3" in _err()  # (a weighted one)
    # the record's place
    assert call(o_risk=-1) == -1 and who + "negative block offset (o_risk=-1)" in _err()
    assert call(blk_bytes=4 * (pr.nblk + M)) == -1 and f"o_risk = {fp.o_risk}" in _err() and "ends outside a block" in _err()  # (blk_bytes must cover the record)
    assert call(o_risk=fp.o_risk + 1) == -1 and "ends outside a block" in _err()
    sections = {"x0": 0, "nominal": pr.off[1], "sigma": pr.off[2], "task params": pr.off[3], "bounds": pr.off[4]}
    for name, at in sections.items():
        assert call(o_risk=at) == -1 and f"overlaps the block's {name}" in _err(), name
    assert call(o_risk=fp.o_risk - 1) == -1 and "overlaps the block's bounds" in _err()
    # the records, read from the host block
    rec = fp.host.numpy()[:, fp.o_risk : fp.o_risk + 1 + M]
    for bad in (float("nan"), -0.25, 1.5, float("inf")):
        rec[1, 0] = bad
        assert call() == -1 and "controller 1" in _err() and "tail word" in _err(), bad
    rec[1, 0] = 0.4
    for bad in (-0.5, float("nan"), float("inf")):
        rec[1, 2] = bad
        assert call() == -1 and "controller 1" in _err() and "weights[1]" in _err() and "negative or not finite" in _err(), bad
    rec[1, 2] = 0.5
    rec[2, 1:] = 0.0
    assert call() == -1 and "controller 2" in _err() and "weights are all zero" in _err()
    rec[2, 1:] = RECORDS[2][1:]
    rec[0, 1:] = [float("nan"), -1.0, float("inf")]  # behind a tail word of zero nothing is read
    # an fr3 set is the phase entry's, and the phase entry takes no other
    bl = _fr3_blocks(gpu, seed=172)
    launch, _ = _sets(gpu, B, M, False)
    bufs = bl.outputs(M)
    assert bl.risk_raw(launch, WORST, bufs, entry=L.jh_plan_step_ensemble_batch_risk) == -3 and "jh_plan_step_ensemble_batch_phases_risk" in _err()
    assert call(set=launch.handle) == -3 and "jh_plan_step_ensemble_batch_phases_risk" in _err()
    leap = GpuModel("leap_cube", gpu)
    leaps = GpuModelSet([leap] * M)
    assert bl.risk_raw(leaps, WORST, bufs) == -3 and "jh_plan_step_ensemble_batch_risk plans this set" in _err()
    # the phase entry's own
    assert bl.risk_raw(launch, WORST, bufs, o_risk=-1) == -1 and "o_risk=-1" in _err()
    assert bl.risk_raw(launch, WORST, bufs, o_phase=-1) == -1 and "o_phase" in _err()
    assert bl.risk_raw(launch, WORST, bufs, o_risk=bl.o_phase) == -1 and "overlaps the block's phase word" in _err()
    assert bl.risk_raw(launch, WORST, bufs, blk_bytes=4 * (bl.nblk + M)) == -1 and "ends outside a block" in _err()
    bl.host.numpy()[2, bl.o_risk] = 1.25
    assert bl.risk_raw(launch, WORST, bufs) == -1 and "controller 2" in _err() and "tail word" in _err()
    bl.host.numpy()[2, bl.o_risk] = 1.0
    bl.host.numpy()[1, bl.o_phase] = 1.5
    assert bl.risk_raw(launch, WORST, bufs) == -1 and "controller 1" in _err() and "phase word" in _err()
    bl.host.numpy()[1, bl.o_phase] = 2.0
    assert bl.risk_raw(launch, [1, 4, 1], bufs) == -1 and "controller 1" in _err() and "worst = 4" in _err()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == v).all() for t, v in zip(bufs, (-7.0, -7.0, 0.0)))  # nothing ran
    assert (member.cpu().numpy() == -7.0).all() and (costs.cpu().numpy() == -7.0).all() and (out.cpu().numpy() == 0).all()
    assert (fp.tickets() == 0).all() and int(fp.mark.numpy().view(np.uint32)[0]) == 41 and bl.tickets_at_zero()
    assert np.isnan(fp.dev.cpu().numpy()).all()  # not even the upload
    assert call() == 0 and L.jh_download_end() == 0
    torch.cuda.synchronize()
    assert (member.cpu().numpy() != -7.0).all() and int(fp.mark.numpy().view(np.uint32)[0]) == 42 and (fp.tickets() == 0).all()
