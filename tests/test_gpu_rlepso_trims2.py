"""The resident RLEPSO kernel after its second round of trims: tournaments compacted per wave (rl_move_listed), the scan's flag from a_0 instead of NLESS[ORDER[rank]],
block_argmin by value exchange + ballot, no group select where NP is a multiple of the group count (csrc/mbx_rlepso.hpp, csrc/mbx_device.hpp).

GPU (marked gpu): for each geometry the rollout route (mbx_rlepso_rollout: the resident kernel where the geometry has one) must equal the per-generation route
(mbx_rlepso_act_step, which keeps one tournament draw per item) bit for bit over 12 generations -- trajectory records and whole state blocks -- and the C oracle,
replaying the actions the kernels drew, must arrive at the same fes / state / reward / done exactly and the same gbest within smoke()'s 1e-5 rule:
  * NP 100 / D 10, kinds 1, 5, 7, 21: the compiled body, 256 threads: the listed tournaments;
  * NP 77 / D 7 and NP 5 / D 2: the run-time geometry (one coordinate per item at odd D; 77 = 5 x 15 + 2: two particles without a group; one particle per group);
  * NP 128 / D 40, 2 instances: the 1024-thread resident kernel (2560 items; it keeps the per-item tournaments).
The learning probabilities pci are fixed at batch creation (0.05 .. 0.5) and no debug export sets them, so the two ends of the list -- nobody on it, everybody on
it -- are covered on the host: list_model() restates rl_move_listed's index arithmetic (ballot / mbcnt positions, the wave's slice of FL, 64 entries dealt per
step, results written over the entries) and is run with empty, full and random need masks.

CPU: (a) block_argmin restated (lanes fold entries l, l + 64, ..., the wave exchanges values only, the index is the lowest lane of the first 64-entry step that
holds the minimum) against np.argmin and against the (value, index) butterfly it replaces, on inputs with equal minima, signed zeros, infinities and NaNs;
(b) the scan bound rounded up to whole unrolled groups (the experiment switch MBX_FDR_ROUND_BOUND; measured, not shipped: docs/EXPERIMENTS.md) on the swarms of
tests/test_fdr_bound.py: no extra candidate is taken and no flag changes.
"""
import numpy as np
import pytest

import test_fdr_bound as fb
from helpers import problems
from oracle import oracle
from test_fdr_bound import natural_swarms  # noqa: F401  (the module's fixture: pbest tables of oracle rollouts)

NLOG = 50
GENS, CHUNKS = 12, (5, 7)


# ------------------------------------------------------------------------------------------------ GPU: both routes and the oracle
def _table(rows, seed):
    import torch
    rs = np.random.RandomState(seed)
    t = torch.empty(rows, 2, 35, dtype=torch.float32)
    t[:, 0] = torch.from_numpy(rs.uniform(0.05, 0.95, (rows, 35)).astype(np.float32))
    t[:, 1] = 0.2
    return t.cuda().contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize('np_,dim,kinds,per_kind,resident', [(100, 10, (1, 5, 7, 21), 2, True), (77, 7, (1, 5, 7, 21), 2, False), (5, 2, (1, 5, 7, 21), 2, False),
                                                           (128, 40, (1, 7), 1, True)])
def test_rollout_equals_per_generation_and_the_oracle(np_, dim, kinds, per_kind, resident):
    import torch
    from metabox_amd.suite import Batch, Suite
    from metabox_amd._abi import ALGO_RLEPSO
    maxfes = 200 * np_
    logi = maxfes // NLOG
    ps = [problems('bbob', dim)[k] for k in kinds]
    B = len(kinds) * per_kind
    idx = np.arange(B) % len(kinds)
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 5
    suite = Suite(ps)
    a, b = (Batch(suite, ALGO_RLEPSO, idx, seeds, np_, maxfes, logi, NLOG, early_stop=False) for _ in range(2))
    assert a.rollout_is_resident() == resident
    table = _table(maxfes + 2 * np_ + 1, 100 * np_ + dim)
    a.reset(); b.reset()
    acts = []
    for n in CHUNKS:
        st, rw, dn, traj = a.rlepso_rollout(table, n, trajectory=True)
        for g in range(n):
            sb, rb, db = b.act_step(table)
            assert torch.equal(traj['state'][g], sb[:, 0]) and torch.equal(traj['reward'][g], rb) and torch.equal(traj['done'][g], db), (n, g)
        torch.cuda.synchronize()
        for k in range(B):
            sa, sb_ = a.read_state(k), b.read_state(k)
            assert np.array_equal(sa, sb_, equal_nan=True), (n, k, np.flatnonzero(sa != sb_)[:8])
        acts.append(traj['actions'].cpu().numpy())
        last = (traj['state'][n - 1].cpu().numpy(), traj['reward'].cpu().numpy(), traj['done'].cpu().numpy())
    acts = np.concatenate(acts)
    states = [a.read_state(k) for k in range(B)]
    a.close(); b.close()
    cfg = oracle.make_cfg(1, np_, dim, maxfes, logi, NLOG, early_stop=0)
    for k in range(B):
        p = ps[idx[k]]
        o = oracle.RlepsoOracle(p.desc(), p.bias, cfg, seed=int(seeds[k]))
        o.reset()
        for g in range(GENS):
            st, rw, dn = o.step(acts[g, k])
        want = oracle.split_rlepso_state(o.state(), np_, dim, NLOG)['scalars']
        got = oracle.split_rlepso_state(states[k], np_, dim, NLOG)['scalars']
        assert got[oracle.SC_FES] == want[oracle.SC_FES] and got[oracle.SC_GEN] == want[oracle.SC_GEN] == GENS, (k, got[:8], want[:8])
        assert got[oracle.SC_RETURN] == want[oracle.SC_RETURN] and got[oracle.SC_COST_LEN] == want[oracle.SC_COST_LEN], (k, got[:8], want[:8])
        assert abs(got[oracle.SC_GBEST] - want[oracle.SC_GBEST]) <= 1e-5 * abs(want[oracle.SC_GBEST]) + 4e-12, (k, got[0], want[0])
        assert last[0][k] == st and last[1][-1, k] == rw and bool(last[2][-1, k]) == bool(dn), k


# ------------------------------------------------------------------------------------------------ the wave lists of rl_move_listed, on the host
def list_model(np_, dim, threads, need):
    """rl_move_listed's index arithmetic for need[item] (bool: the item consumes a tournament).  -> (result[item]: the item whose tournament the item picks up, or -1
    where it reads none; entries used of FL; wave-steps dealt)."""
    NI = np_ * dim // 2
    IT = -(-NI // threads)
    FL = np.full(np_ * dim, -7, int)                               # NE uint16 entries (mbx_lds.hpp: rl_move_layout)
    result = np.full(NI, -1)
    steps = used = 0
    for w in range(threads // 64):
        base, n = w * 64 * IT, 0
        pos = {}
        for j in range(IT):
            its = w * 64 + np.arange(64) + j * threads
            any_ = np.array([it < NI and need[it] for it in its])
            below = np.cumsum(any_) - any_                         # mbcnt: lanes below with the bit set
            for lane in np.flatnonzero(any_):
                pos[its[lane]] = n + below[lane]
                FL[base + pos[its[lane]]] = its[lane]
            n += int(any_.sum())
        assert n <= 64 * IT and base + 64 * IT <= len(FL)
        for s0 in range(0, n, 64):                                 # 64 entries per step: every lane reads its entry, then writes the result over it
            ent = FL[base + s0:base + min(s0 + 64, n)].copy()
            FL[base + s0:base + min(s0 + 64, n)] = 100000 + ent   # "the ranks of item ent"
            steps += 1
        for it, q in pos.items():
            result[it] = FL[base + q] - 100000
        used = max(used, base + n)
    return result, used, steps


@pytest.mark.parametrize('np_,dim,threads', [(100, 10, 256), (100, 12, 256)])
def test_wave_lists_hand_every_item_its_own_tournament(np_, dim, threads):
    NI = np_ * dim // 2
    rs = np.random.RandomState(NI)
    for name, need in (('empty', np.zeros(NI, bool)), ('full', np.ones(NI, bool)), ('18 %', rs.uniform(size=NI) < 0.18), ('one wave only', np.arange(NI) % threads < 64)):
        res, used, steps = list_model(np_, dim, threads, need)
        assert (res[need] == np.flatnonzero(need)).all() and (res[~need] == -1).all(), name
        assert used <= np_ * dim, name
        if name == 'empty':
            assert steps == 0
        if name == 'full':
            assert -(-NI // 64) <= steps <= (threads // 64) * -(-NI // threads)
        if name == 'one wave only':
            assert steps == -(-NI // threads), 'a list longer than one step: the other waves deal nothing'


# ------------------------------------------------------------------------------------------------ block_argmin, on the host
def argmin_new(a):
    """block_argmin: strict-less fold per lane from +inf, minimum of the 64 lane values, first 64-entry step with an entry equal to it, lowest lane."""
    n = len(a)
    with np.errstate(invalid='ignore'):
        m = np.inf
        for lane in range(64):
            v = np.inf
            for x in a[lane::64]:
                if x < v:
                    v = x
            m = min(m, v)                                          # v is never NaN
        idx = 0
        if m < np.inf:
            for j0 in range(0, n, 64):
                eq = np.flatnonzero(a[j0:j0 + 64] == m)
                if len(eq):
                    idx = j0 + eq[0]
                    break
    return idx, a[idx]


def argmin_old(a):
    """The (value, index) butterfly it replaces (wave_argmin): smallest value, lowest index on ties."""
    n = len(a)
    v, i = np.full(64, np.inf), np.full(64, 0x7fffffff)
    with np.errstate(invalid='ignore'):
        for lane in range(64):
            for j in range(lane, n, 64):
                if a[j] < v[lane]:
                    v[lane], i[lane] = a[j], j
        off = 32
        while off:
            ov, oi = v[np.arange(64) ^ off], i[np.arange(64) ^ off]
            take = (ov < v) | ((ov == v) & (oi < i))
            v, i = np.where(take, ov, v), np.where(take, oi, i)
            off >>= 1
    return (0, a[0]) if i[0] >= n else (int(i[0]), v[0])


def test_block_argmin_is_the_first_minimum_nan_and_ties_included():
    rs = np.random.RandomState(4)
    cases = []
    for n in (1, 5, 63, 64, 65, 100, 128, 129, 200, 256):
        x = rs.uniform(-3., 3., n)
        cases.append(x)
        for _ in range(6):
            y = x.copy()
            k = rs.randint(1, min(n, 9) + 1)
            at = rs.choice(n, k, replace=False)
            y[at] = y.min() - 1.                                   # k equal minima, anywhere: lane l + 64 before lane l + 1 included
            y[rs.choice(n, rs.randint(0, n // 3 + 1), replace=False)] = np.nan
            cases.append(y)
        z = np.round(x)                                            # many ties, signed zeros
        z[rs.choice(n, n // 4, replace=False)] = -0.
        cases.append(z)
        cases.append(np.where(z == z.min(), 0., np.where(rs.uniform(size=n) < 0.5, -0., 0.)) if n > 1 else z)
        cases.append(np.full(n, np.nan)); cases.append(np.full(n, np.inf)); cases.append(np.full(n, -np.inf))
        w = np.full(n, np.inf); w[0] = np.nan
        cases.append(w)
        if n > 70:
            w = rs.uniform(0., 1., n); w[64] = w[5] = -1.          # the minimum in lane 0's second entry and in lane 5's first: index 5, not 64
            cases.append(w)
    for a in cases:
        gi, gv = argmin_new(a)
        oi, ov = argmin_old(a)
        assert gi == oi and (gv == ov or (np.isnan(gv) and np.isnan(ov))) and np.signbit(gv) == np.signbit(ov), (a, gi, oi)
        finite = np.where(np.isnan(a), np.inf, a)
        want = int(np.argmin(finite)) if (finite < np.inf).any() else 0    # NaN never wins; nothing below +inf: index 0
        assert gi == want, (a, gi, want)


# ------------------------------------------------------------------------------------------------ the rounded scan bound, on the host
PLAIN_BOUNDS = fb.wave_bounds


def rounded_bounds(NP_, D_, W, threads):
    """fdr_pass with MBX_FDR_ROUND_BOUND: the wave's bound rounded up to 1 + a whole number of unrolled groups where that stays within the table."""
    bound, wave = PLAIN_BOUNDS(NP_, D_, W, threads)
    UN = 2 if D_ == 40 else 4                                      # MBX_FDR_UNROLL_D40 / MBX_FDR_UNROLL
    up = 1 + -(-(bound - 1) // UN) * UN
    return np.where((bound > 0) & (up <= NP_), up, bound), wave


@pytest.fixture
def rounded(monkeypatch):
    """tests/test_fdr_bound.py's scan model with the rounded bounds in place of fdr_pass's own."""
    monkeypatch.setattr(fb, 'wave_bounds', rounded_bounds)


@pytest.mark.parametrize('np_,dim,threads', [(100, 10, 256), (128, 40, 1024), (77, 7, 256), (5, 2, 256)])
def test_rounding_the_bound_up_changes_nothing_on_crafted_swarms(rounded, np_, dim, threads):
    W = 2 if dim % 2 == 0 else 1
    UN = 2 if dim == 40 else 4
    plain, _ = PLAIN_BOUNDS(np_, dim, W, threads)
    up, _ = fb.wave_bounds(np_, dim, W, threads)
    assert (up >= plain).all() and up.max() <= np_ and ((up - 1) % UN == 0)[(plain > 0) & (plain <= np_ - UN + 1)].all()
    if np_ >= 77:
        assert (up > plain).any()
    for name, f, P in fb.crafted_swarms(np_, dim):
        r = fb.check_swarm(f, P, threads, name)                    # no extra candidate taken, exemplars and flags unchanged
        assert r['margin'] >= 2. ** 8, (name, r['margin'])


def test_rounding_the_bound_up_changes_nothing_on_natural_swarms(rounded, natural_swarms):  # noqa: F811
    extras = 0
    for tag, f, P in natural_swarms:
        r = fb.check_swarm(f, P, 256, tag)
        assert r['margin'] >= 2. ** 8, (tag, r['margin'])
        extras += r['extras']
    assert extras > 100_000
