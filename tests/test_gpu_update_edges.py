"""The update tail under adversarial costs: jh_update_fused (and, for a subset, jh_update_shard + jh_shard_merge) called directly with synthetic costs,
knots and trace rows, against an fp64 restatement of the reference's rules -- judo/optimizers/mppi.py:76-82 (beta = min cost, w = exp(-(c - beta) / lambda),
nominal = sum w x / sum w), cem.py:88-92 (the k best by reward: mean and population std), ps.py:64-65 (np.argmax of the rewards) and
judo/controller/controller.py:339 (the trace elites: argsort(rewards)[-E:][::-1]) -- with the project's two stated rules (include/judo_amd.h): equal costs
rank the higher global index first where tie_high != 0 and the lower one first otherwise, and a NaN cost counts as +inf.

The arg-best of the tail (wave_best: four DPP row modifiers, v_permlane16_swap, v_permlane32_swap; then the waves, the workgroups and topk_choose's register
and memory forms) is checked where a wrong exchange stage would show: a unique best at every lane of a workgroup and of a ragged last workgroup, at every
workgroup of a 257-workgroup launch, and tied pairs at lane distances 1 .. 32 and across waves and workgroups.  Selections and copied rows are compared bit
for bit; the averages within bounds derived next to each assertion."""

import numpy as np
import pytest

from tests.conftest import bounded

pytestmark = pytest.mark.gpu

U = 2.0**-24  # unit round-off of fp32


def _gamma(n):
    return n * U / (1 - n * U)


class _Problem:
    """Device copies of one problem's knots (N, K, nu) and row-major trace rows (N, row); launches of the update tail on P cost vectors at once
    (one launch per vector on one stream, one synchronisation)."""

    def __init__(self, dev, N, K, nu, row, n_offset=0, seed=0):
        import torch

        rng = np.random.default_rng(seed)
        self.N, self.K, self.nu, self.KU, self.row, self.n_offset, self.dev = N, K, nu, K * nu, row, n_offset, dev
        self.knots = rng.uniform(-2.0, 2.0, (N, K, nu)).astype(np.float32)
        self.trace = rng.standard_normal((N, row)).astype(np.float32)
        self.d_knots = torch.from_numpy(self.knots).to(dev)
        self.d_trace = torch.from_numpy(self.trace).to(dev)

    def _costs(self, costs):
        import torch

        c = np.ascontiguousarray(np.atleast_2d(costs), dtype=np.float32)
        assert c.shape[1] == self.N
        return c, torch.from_numpy(c).to(self.dev)

    def fused(self, costs, mode, lam=0.0, k=0, tie=0, E=0):
        """jh_update_fused on every row of `costs` (P, N): (P, 2 KU + E (2 + row)) = nominal | sigma | E trace records."""
        import torch

        from judo_amd import _lib

        L = _lib.lib()
        c, dc = self._costs(costs)
        KU, row = self.KU, self.row
        n_out = 2 * KU + E * (2 + row)
        out = torch.full((c.shape[0], n_out), 7.0, dtype=torch.float32, device=self.dev)  # (a value no update writes: a skipped store shows)
        scr = torch.zeros(int(L.jh_update_fused_scratch_floats(self.N, self.K, self.nu)), dtype=torch.float32, device=self.dev)
        st = torch.cuda.current_stream().cuda_stream
        for p in range(c.shape[0]):
            o = out[p].data_ptr()
            _lib.check(L.jh_update_fused(dc[p].data_ptr(), self.d_knots.data_ptr(), None, None, 0, None, None, self.N, self.n_offset, self.K, self.nu, mode, lam, k, tie, E,
                                         self.d_trace.data_ptr() if E else None, row if E else 0, 0, scr.data_ptr(), o, o + 4 * KU if mode == 1 else None,
                                         o + 8 * KU if E else None, st), "jh_update_fused")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def shards(self, costs, mode, lam=0.0, k=0, tie=0, E=0, G=1):
        """jh_update_shard on G contiguous shards of every row of `costs`, then jh_shard_merge of the G records: (records (P, G, Lrec), merged (P, n_out))."""
        import torch

        from judo_amd import _lib
        from judo_amd.distributed import shard_rollouts

        L = _lib.lib()
        c, dc = self._costs(costs)
        KU, row = self.KU, self.row
        Lrec = int(L.jh_shard_record_floats(self.K, self.nu, mode, k, E, row if E else 0))
        n_out = 2 * KU + E * (2 + row)
        recs = torch.full((c.shape[0], G, Lrec), 7.0, dtype=torch.float32, device=self.dev)
        out = torch.full((c.shape[0], n_out), 7.0, dtype=torch.float32, device=self.dev)
        scr = torch.zeros(int(L.jh_update_fused_scratch_floats(self.N, self.K, self.nu)), dtype=torch.float32, device=self.dev)
        st = torch.cuda.current_stream().cuda_stream
        for p in range(c.shape[0]):
            for g in range(G):
                sh = shard_rollouts(self.N, G, g)
                _lib.check(L.jh_update_shard(dc[p].data_ptr() + 4 * sh.offset, self.d_knots.data_ptr() + 4 * KU * sh.offset, None, None, 0, None, None, sh.count,
                                             self.n_offset + sh.offset, self.K, self.nu, mode, lam, k, tie, E, self.d_trace.data_ptr() + 4 * row * sh.offset if E else None,
                                             row if E else 0, 0, scr.data_ptr(), recs[p, g].data_ptr(), st), "jh_update_shard")
            o = out[p].data_ptr()
            _lib.check(L.jh_shard_merge(recs[p].data_ptr(), G, self.K, self.nu, mode, lam, k, tie, E, row if E else 0, o, o + 4 * KU if mode == 1 else None, o + 8 * KU if E else None,
                                        st), "jh_shard_merge")
        torch.cuda.synchronize()
        return recs.cpu().numpy(), out.cpu().numpy()

    # ---- the fp64 restatement of the reference's rules
    def order(self, costs, tie_high):
        """Local rollout indices best first: smallest cost (NaN = +inf), equal costs by global index, higher first when tie_high."""
        c = np.where(np.isnan(costs), np.inf, np.asarray(costs, dtype=np.float64))
        gi = np.arange(self.N) + self.n_offset
        return np.lexsort((-gi if tie_high else gi, c))

    def trace_records(self, costs, E):
        """E x [cost, global index (bits), trace row] of the trace elites (ties: higher index first); a rollout without a finite cost, or past the last one: [inf, -1, 0]."""
        rec = np.zeros((E, 2 + self.row), dtype=np.float32)
        rec[:, 0] = np.inf
        rec[:, 1] = np.array(-1, dtype=np.int32).view(np.float32)
        for e, i in enumerate(self.order(costs, 1)[:E]):
            if np.isfinite(costs[i]):
                rec[e, 0] = costs[i]
                rec[e, 1] = np.array(self.n_offset + i, dtype=np.int32).view(np.float32)
                rec[e, 2:] = self.trace[i]
        return rec

    def elite_records(self, costs, k, tie_high):
        """What jh_update_shard writes for the elites: k x [cost (NaN -> inf), global index (bits), knots]; past the last rollout [inf, -1, 0]."""
        rec = np.zeros((k, 2 + self.KU), dtype=np.float32)
        rec[:, 0] = np.inf
        rec[:, 1] = np.array(-1, dtype=np.int32).view(np.float32)
        for e, i in enumerate(self.order(costs, tie_high)[:k]):
            rec[e, 0] = np.inf if np.isnan(costs[i]) else costs[i]
            rec[e, 1] = np.array(self.n_offset + i, dtype=np.int32).view(np.float32)
            rec[e, 2:] = self.knots[i].reshape(-1)
        return rec

    def cem(self, costs, k, tie_high):
        """cem.py:88-92 on the elites of `order`: mean and population std (fp64), and the bounds of the fp32 kernel's (below)."""
        x = self.knots[self.order(costs, tie_high)[:k]].reshape(-1, self.KU).astype(np.float64)
        m, s = x.mean(0), x.std(0)
        n = x.shape[0]
        # mean: a sequential fp32 sum of n terms, one division -> |dm| <= gamma_(n+1) * sum|x| / n.  std: d = x - m^ carries dm, and sum (d_e - dm)^2 = sum d_e^2 + n dm^2
        # (sum d_e = 0), so var^ <= (var + dm^2)(1 + gamma_(n+2)) and sqrt adds one rounding: |ds| <= |dm| + gamma_(n+3) * s
        bm = _gamma(n + 1) * np.abs(x).sum(0) / n
        return m, s, bm, bm + _gamma(n + 3) * s

    def mppi(self, costs, lam, levels):
        """mppi.py:76-82 in fp64 (NaN / inf costs: weight zero) and the error bound of the fp32 kernel, per knot.

        The kernel forms a_i = (c_i - beta_b) * (1 / lambda) in fp32 (beta_b the minimum of the rollout's workgroup; three roundings: the difference, 1 / lambda, the
        product, so |da_i| <= 3u a_i), takes w_i = __expf(-a_i) = v_exp_f32(-a_i * log2 e) (two more relative errors of the argument, the rounded log2 e and the
        product: 2u a_i; and 1 ulp = 2u relative of the result), and the merge scales the workgroup's sums by __expf(-(beta_b - beta) / lambda) with the same errors in
        its own argument.  The two arguments add up to A_i = (c_i - beta) / lambda >= 0, so the weight of rollout i is off by a factor exp(delta_i),
        |delta_i| <= 5u A_i + 4u.  A relative error delta_i in w_i moves sum w x / sum w by sum w_i delta_i (x_i - nominal) / sum w: at most
        sum w_i |delta_i| |x_i - nominal| / sum w.  The sums are fp32 trees / chains (six butterfly levels, the four waves, the chain over the workgroup records, the
        ranks' merge) and each term w x is rounded twice (the product in its workgroup, the rescale in the merge): `levels` roundings in all, at most
        gamma_levels (sum w |x| + |nominal| sum w) / sum w, and the final division one rounding u |nominal|.  fp32 underflow of exp(-A_i) (A_i > 87) loses at most
        N e^-87 max|x| / sum w, and sum w >= 1 (the best rollout's weight)."""
        c = np.asarray(costs, dtype=np.float64)
        fin = np.isfinite(c)
        x = self.knots.reshape(self.N, self.KU).astype(np.float64)
        if not fin.any():
            return np.full(self.KU, np.nan), None
        beta = c[fin].min()
        A = np.where(fin, (np.where(fin, c, beta) - beta) / lam, np.inf)
        w = np.exp(-A)
        S = w.sum()
        nom = (w[:, None] * x).sum(0) / S
        delta = np.where(fin, 5 * U * np.where(fin, A, 0) + 4 * U, 0.0)
        bound = ((w * delta)[:, None] * np.abs(x - nom)).sum(0) / S + _gamma(levels) * ((w[:, None] * np.abs(x)).sum(0) + np.abs(nom) * S) / S + U * np.abs(nom)
        bound += self.N * np.exp(-87.0) * np.abs(x).max() / S
        return nom, bound


def _levels(N, G=1):
    nb = (N + 255) // 256
    return 6 + 2 + nb + 2 + (G + 1 if G > 1 else 0)


def _pattern(name, N, rng, lam=0.0025):
    c = rng.uniform(1.0, 2.0, N)
    if name == "random":
        pass
    elif name == "equal":
        c[:] = 1.5
    elif name == "quantised":  # few distinct values: ties at every elite cut
        c = 1.0 + 0.125 * rng.integers(0, 4, N)
    elif name == "nan_inf":  # NaN and +inf sprinkled in, at both ends as well
        r = rng.random(N)
        c[r < 0.15] = np.nan
        c[(r >= 0.15) & (r < 0.3)] = np.inf
        c[0] = np.nan
        c[-1] = np.inf
    elif name == "all_inf":
        c[:] = np.inf
    elif name == "all_nan":
        c[:] = np.nan
    elif name == "one_weight":  # (c - beta) / lambda >= 200 for all but the best: one non-zero weight in fp32
        c[rng.integers(0, N)] = 1.0 - 200 * lam
    elif name == "best_ragged":  # the best rollout in the ragged last workgroup
        c[N - 1 - rng.integers(0, min(N, (N - 1) % 256 + 1))] = 0.5
    return c.astype(np.float32)


def _check_trace(out, P, costs, E, KU):
    got = out[2 * KU :].reshape(E, 2 + P.row)
    np.testing.assert_array_equal(got.view(np.int32), P.trace_records(costs, E).view(np.int32))


def _check_elites_and_mppi(P, costs, k, E, lam, G):
    N, KU = P.N, P.KU
    # PS (ps.py:64-65: np.argmax of the rewards, the lowest index of equal ones): the winner's knots, bit for bit; the trace records of the same launch
    out = P.fused(costs, 1, 0.0, 1, 0, E)[0]
    win = P.order(costs, 0)[0]
    np.testing.assert_array_equal(out[:KU], P.knots[win].reshape(-1))
    np.testing.assert_array_equal(out[KU : 2 * KU], np.zeros(KU, np.float32))  # one elite: population std 0
    if E:
        _check_trace(out, P, costs, E, KU)
    # CEM (tie_high 1: flip(argsort)): the elite records of the shard form bit for bit, mean / std within the fp32 bounds of _Problem.cem, fused == merged shards
    recs, merged = P.shards(costs, 1, 0.0, k, 1, E, G=1)
    np.testing.assert_array_equal(recs[0, 0, : k * (2 + KU)].reshape(k, 2 + KU).view(np.int32), P.elite_records(costs, k, 1).view(np.int32))
    out = P.fused(costs, 1, 0.0, k, 1, E)[0]
    m, s, bm, bs = P.cem(costs, k, 1)
    assert bounded(f"update edges: CEM mean / bound, N={N} k={k} KU={KU}", (np.abs(out[:KU] - m) / bm).max(), 1.0)
    assert bounded(f"update edges: CEM std / bound, N={N} k={k} KU={KU}", (np.abs(out[KU : 2 * KU] - s) / bs).max(), 1.0)
    np.testing.assert_array_equal(merged[0].view(np.int32), out.view(np.int32))  # one rank: the merge sees the same records in the same order
    if E:
        _check_trace(out, P, costs, E, KU)
    if G > 1:
        _, mg = P.shards(costs, 1, 0.0, k, 1, E, G=G)
        np.testing.assert_array_equal(mg[0].view(np.int32), out.view(np.int32))  # same elites, same order: the same mean and std bits
    # MPPI
    out = P.fused(costs, 0, lam, 0, 0, E)[0]
    nom, bound = P.mppi(costs, lam, _levels(N))
    if bound is None:  # no finite cost: the reference's weights are NaN, so is the kernel's mean
        assert np.isnan(out[:KU]).all()
    else:
        assert bounded(f"update edges: MPPI nominal / derived bound, N={N} KU={KU}", (np.abs(out[:KU] - nom) / bound).max(), 1.0)
    if E:
        _check_trace(out, P, costs, E, KU)
    if G > 1:
        _, mg = P.shards(costs, 0, lam, 0, 0, E, G=G)
        if bound is None:
            assert np.isnan(mg[0, :KU]).all()
        else:
            _, bound_g = P.mppi(costs, lam, _levels(N, G))
            assert bounded(f"update edges: MPPI nominal of {G} merged shards / derived bound, N={N}", (np.abs(mg[0, :KU] - nom) / bound_g).max(), 1.0)
        if E:
            _check_trace(mg[0], P, costs, E, KU)
    return out


# (N, K, nu, k, E, n_offset, G): every N of the issue; k and E 1, 5, 32 (N < k, N < E: empty records); K * nu 1, 16, 512 (512 at small N); topk_choose on both
# sides of its 1 024 register-held candidates (ceil(N / 256) * k: 65 537 x 3 -> 771, x 5 -> 1 285, x 32 -> 8 224; 4 097 x 32 -> 544)
CASES = [
    (1, 1, 1, 5, 5, 0, 1), (1, 4, 4, 32, 32, 3, 1), (3, 32, 16, 5, 32, 0, 1), (63, 1, 1, 5, 5, 0, 3), (64, 4, 4, 32, 5, 0, 1), (65, 32, 16, 1, 1, 7, 2),
    (256, 4, 4, 5, 32, 0, 1), (257, 1, 1, 32, 32, 100, 3), (257, 32, 16, 5, 5, 0, 1), (4097, 4, 4, 32, 32, 0, 2), (4097, 1, 1, 5, 1, 9, 1),
    (65537, 1, 1, 3, 3, 0, 1), (65537, 4, 4, 5, 5, 12345, 4), (65537, 1, 1, 32, 32, 0, 1),
]
PATTERNS = ["random", "equal", "quantised", "nan_inf", "all_inf", "all_nan", "one_weight", "best_ragged"]


@pytest.mark.parametrize("N,K,nu,k,E,n_offset,G", CASES)
def test_update_tail_matches_the_fp64_rules(gpu, N, K, nu, k, E, n_offset, G):
    lam = 0.0025
    P = _Problem(gpu, N, K, nu, row=7, n_offset=n_offset, seed=N + K)
    rng = np.random.default_rng(N * 7 + k)
    for pat in PATTERNS if N * K * nu <= 300_000 else ["random", "quantised", "nan_inf", "one_weight", "best_ragged"]:
        costs = _pattern(pat, N, rng, lam)
        out = _check_elites_and_mppi(P, costs, k, E, lam, G)
        if pat == "one_weight":  # every other weight underflows: the MPPI mean is the best rollout's knots, bit for bit
            np.testing.assert_array_equal(out[: P.KU], P.knots[P.order(costs, 0)[0]].reshape(-1))


def test_a_unique_best_at_every_position(gpu):
    """A unique best cost at each of the 256 positions of a workgroup and each of the 44 of a ragged last workgroup (N = 300), then at one lane of each of the 257
    workgroups of N = 65 537 (topk_choose over 1 285 candidates: its memory form) and of N = 4 097 (its register form): PS returns exactly that rollout, CEM
    has it as elite 0, the trace records as record 0."""
    for N, k in ((300, 5), (4097, 5), (65537, 5)):
        nb = (N + 255) // 256
        positions = np.arange(300) if N == 300 else np.minimum(np.arange(nb) * 256 + (np.arange(nb) * 37) % 256, N - 1)  # (one lane per workgroup, a different one each)
        P = _Problem(gpu, N, 2, 2, row=3, n_offset=11, seed=N)
        rng = np.random.default_rng(N)
        costs = np.tile(rng.uniform(1.0, 2.0, N).astype(np.float32), (len(positions), 1))
        costs[np.arange(len(positions)), positions] = 0.5
        ps = P.fused(costs, 1, 0.0, 1, 0, 3)
        recs, _ = P.shards(costs, 1, 0.0, k, 1, 0)
        for j, p in enumerate(positions):
            np.testing.assert_array_equal(ps[j, : P.KU], P.knots[p].reshape(-1), err_msg=f"PS, N={N}, best at {p}")
            assert ps[j, 2 * P.KU + 1 : 2 * P.KU + 2].view(np.int32)[0] == 11 + p, f"trace record 0, N={N}, best at {p}"
            assert recs[j, 0, 1:2].view(np.int32)[0] == 11 + p, f"CEM elite 0, N={N}, best at {p}"
            np.testing.assert_array_equal(recs[j, 0, : k * (2 + P.KU)].reshape(k, -1).view(np.int32), P.elite_records(costs[j], k, 1).view(np.int32))


def test_tied_pairs_at_every_exchange_distance(gpu):
    """Two equal best costs at lane distances 1, 2, 4, 8, 16, 32 (the six exchange stages of wave_best), 64 and 128 (across waves) and 256 (across workgroups), from
    several first lanes: PS and CEM follow their tie rule for tie_high 0 and 1, the trace records take the higher index first."""
    N = 700
    pairs = [(i, i + d) for d in (1, 2, 4, 8, 16, 32, 64, 128, 256) for i in (0, 3, 30, 63, 101, 255, 300) if i + d < N]
    P = _Problem(gpu, N, 2, 1, row=2, n_offset=0, seed=3)
    rng = np.random.default_rng(4)
    costs = np.tile(rng.uniform(1.0, 2.0, N).astype(np.float32), (len(pairs), 1))
    for j, (a, b) in enumerate(pairs):
        costs[j, [a, b]] = 0.25
    for tie in (0, 1):
        ps = P.fused(costs, 1, 0.0, 1, tie, 2)
        recs, _ = P.shards(costs, 1, 0.0, 3, tie, 0)
        for j, (a, b) in enumerate(pairs):
            first, second = (b, a) if tie else (a, b)
            np.testing.assert_array_equal(ps[j, : P.KU], P.knots[first].reshape(-1), err_msg=f"PS tie_high={tie}, pair {a, b}")
            assert list(ps[j, 2 * P.KU :].reshape(2, -1)[:, 1].view(np.int32)) == [b, a], f"trace records, pair {a, b}"
            assert list(recs[j, 0, : 3 * (2 + P.KU)].reshape(3, -1)[:2, 1].view(np.int32)) == [first, second], f"CEM tie_high={tie}, pair {a, b}"
