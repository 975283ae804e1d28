"""The resident RLEPSO kernel after its third instruction budget: the FDR scan of the 256-thread resident geometries walks GR = MBX_FDR_GROUPS unrolled groups per
trip of its main loop from one pair of LDS address registers, and its remainder is straight-line code at constant offsets (csrc/mbx_rlepso.hpp: fdr_exact, GR > 1).
k_rlepso_step (one launch per generation) keeps the indexed loops, so the two routes are two statements of the same scan.

GPU (marked gpu):
  * the resident route (mbx_rlepso_rollout) against per-generation stepping (mbx_rlepso_act_step), np.array_equal on every state block, 6 generations from a reset:
    24 instances, one per BBOB function, at NP 100 / D 10 (bounds 12 .. 99: every trip count of the two passes' eight waves), and 4 instances at NP 100 / D 12
    (600 items: three passes, other bounds and remainders);
  * the crafted swarms of tests/test_fdr_bound.py (equal costs, strictly increasing costs, the worst-case tie at zero distance, copies of the best row, ...) and
    collapsed swarms (a few cost levels on a coarse grid, whole-row copies: tests/test_gpu_rlepso_trims.py) through the resident route at NP 100 / D 10: the velocity of
    every (particle, dimension) item must be the one np.argmin of the reference's rounded quotients produces.

CPU: the trip arithmetic of the new loops alone, restated: for every bound 1 .. 100 each candidate 1 .. bound - 1 is visited exactly once, in ascending order, at the
offsets the code uses, and nothing at or beyond the bound (hence NP) is read -- for the shipped (UN, GR) = (4, 3) and for the other values the switches allow.
"""
import numpy as np
import pytest

from helpers import problems
from oracle import oracle

NP, NLOG = 100, 50
GENS = 6


# ------------------------------------------------------------------------------------------------ CPU: the loops' trip arithmetic
def visits(bound, UN, GR):
    """fdr_exact<.., GR > 1>: the candidates read, in order, as (k, cost-stream index, row index); pc / pr are the two pointers, in candidates from the tables' starts."""
    out = []
    pc = pr = 1                                                    # L.NCS + 1, col + D
    k = 1
    while k + GR * UN <= bound:                                    # main loop: GR groups at constant offsets, ONE advance
        for g in range(GR):
            for u in range(UN):
                out.append((k + g * UN + u, pc + g * UN + u, pr + g * UN + u))
        pc += GR * UN; pr += GR * UN; k += GR * UN
    while k + UN <= bound:                                         # whole groups that are left
        for u in range(UN):
            out.append((k + u, pc + u, pr + u))
        pc += UN; pr += UN; k += UN
    for r in range(UN - 1):                                        # remainder: straight-line code, the pointers stay
        if k + r < bound:
            out.append((k + r, pc + r, pr + r))
    return out


def visits_parent(bound, UN):
    """GR = 1: the indexed loops."""
    out = []
    k = 1
    while k + UN <= bound:
        out += [(k + u, k + u, k + u) for u in range(UN)]
        k += UN
    while k < bound:
        out.append((k, k, k))
        k += 1
    return out


@pytest.mark.parametrize('UN,GR', [(4, 3), (4, 2), (4, 4), (2, 3), (3, 2), (8, 2)])
def test_every_candidate_below_the_bound_is_visited_exactly_once(UN, GR):
    for bound in range(0, NP + 1):                                 # (0: what a wave without a better particle may be handed; 1 .. NP - 1: ranks; NP: never, but harmless)
        v = visits(bound, UN, GR)
        ks = [k for k, _, _ in v]
        assert ks == list(range(1, max(bound, 1))), (bound, ks)
        assert all(c == k and r == k for k, c, r in v), (bound, 'a candidate is read at the wrong offset')
        assert all(max(c, r) < max(bound, 1) for _, c, r in v), (bound, 'read at or beyond the bound')
        assert v == visits_parent(bound, UN), bound
        if bound >= 1:
            rem = (bound - 1) % UN
            main = (bound - 1) // (GR * UN)
            assert len(v) == main * GR * UN + ((bound - 1) // UN - main * GR) * UN + rem and rem <= UN - 1


def test_the_headline_geometry_pays_two_advances_per_twelve_candidates():
    """What the change is for, from the bounds fdr_pass hands out at NP 100 / D 10: pointer advances per workgroup-generation, 107 groups before, 37 trips now."""
    from test_fdr_bound import wave_bounds
    bound, wave = wave_bounds(100, 10, 2, 256)
    per_wave = sorted({(int(w), int(b)) for w, b in zip(wave.ravel(), bound.ravel())})
    assert [b for _, b in per_wave] == [12, 25, 38, 51, 99, 87, 74, 61]
    groups = sum((b - 1) // 4 for _, b in per_wave)
    trips = sum((b - 1) // 12 + ((b - 1) // 4 - 3 * ((b - 1) // 12)) for _, b in per_wave)
    assert (groups, trips) == (107, 37)


# ------------------------------------------------------------------------------------------------ GPU: both routes, state blocks bit for bit
def _table(rows, seed):
    import torch
    rs = np.random.RandomState(seed)
    t = torch.empty(rows, 2, 35, dtype=torch.float32)
    t[:, 0] = torch.from_numpy(rs.uniform(0.05, 0.95, (rows, 35)).astype(np.float32))
    t[:, 1] = 0.2
    return t.cuda().contiguous()


def _both_routes(suite_problems, idx, dim, maxfes, logi, nlog, geometry):
    import torch
    from metabox_amd.suite import Batch, Suite
    from metabox_amd._abi import ALGO_RLEPSO
    B = len(idx)
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 17
    s = Suite(suite_problems)
    a, b = (Batch(s, ALGO_RLEPSO, idx, seeds, NP, maxfes, logi, nlog, early_stop=False) for _ in range(2))
    assert a.rollout_is_resident() and a.launch_info()['fixed_geometry'] == geometry, a.launch_info()
    table = _table(maxfes + 2 * NP + 1, 31 * dim)
    a.reset(); b.reset()
    for n in (1, GENS - 1):                                        # a one-generation launch, then the rest in one
        _, _, _, traj = a.rlepso_rollout(table, n, trajectory=True)
        for g in range(n):
            sb, rb, db = b.act_step(table)
            assert torch.equal(traj['state'][g], sb[:, 0]) and torch.equal(traj['reward'][g], rb) and torch.equal(traj['done'][g], db), (n, g)
        torch.cuda.synchronize()
        for k in range(B):
            sa, sb_ = a.read_state(k), b.read_state(k)
            assert np.array_equal(sa, sb_), (n, k, np.flatnonzero(sa != sb_)[:8])
    gen = [oracle.split_rlepso_state(a.read_state(k), NP, dim, nlog)['scalars'][oracle.SC_GEN] for k in range(B)]
    a.close(); b.close()
    assert gen == [GENS] * B


@pytest.mark.gpu
def test_resident_equals_per_generation_on_the_24_functions():
    ps = [problems('bbob', 10)[f] for f in range(1, 25)]
    _both_routes(ps, np.arange(24), 10, 20000, 400, NLOG, 1)


@pytest.mark.gpu
def test_resident_equals_per_generation_at_d12_three_passes():
    from metabox_amd.problem.protein_docking import Protein_Docking_Dataset
    tr, te = Protein_Docking_Dataset.get_datasets('protein', difficulty='easy')
    ps = [tr.data[0], tr.data[7], te.data[0], te.data[-1]]
    assert all(p.dim == 12 for p in ps) and -(-NP * 6 // 256) == 3
    _both_routes(ps, np.arange(4), 12, 1000, 200, 5, 8)


# ------------------------------------------------------------------------------------------------ GPU: crafted and collapsed swarms, every exemplar np.argmin's
@pytest.mark.gpu
def test_resident_scan_picks_np_argmin_on_crafted_and_collapsed_swarms():
    import torch
    from metabox_amd.suite import Batch, Suite
    from metabox_amd._abi import ALGO_RLEPSO
    from test_fdr_bound import crafted_swarms
    from test_fdr_ties import ACTION, _philox_fdr_weights, decode_agreement, reference_targets, state_block
    from test_gpu_rlepso_trims import collapsed_swarm
    dim, maxfes = 10, 20000
    rs = np.random.RandomState(303)
    cases = [(name, f, P) for name, f, P in crafted_swarms(NP, dim)] + [(f'collapsed_{lv}', *collapsed_swarm(rs, lv)) for lv in (3, 12, 40)]
    names = {n for n, _, _ in cases}
    assert {'swarm_all_equal', 'swarm_zero_distance', 'swarm_increasing', 'collapsed_3'} <= names
    n = len(cases)
    seeds = np.arange(n, dtype=np.uint64) * 7 + 3
    batch = Batch(Suite([problems('bbob', dim)[1]]), ALGO_RLEPSO, np.zeros(n, int), seeds, NP, maxfes, maxfes // NLOG, NLOG)
    assert batch.rollout_is_resident() and batch.launch_info()['fixed_geometry'] == 1
    batch.reset()
    torch.cuda.synchronize()
    template = batch.read_state(0)
    for b, (_, f, P) in enumerate(cases):
        batch.write_state(b, state_block(template, f, P))
    table = torch.zeros(maxfes + 2 * NP + 1, 2, 35, dtype=torch.float32)
    table[:, 0] = torch.from_numpy(ACTION)                          # mu = ACTION, sigma = 0: only the FDR term moves a particle
    batch.rlepso_rollout(table.cuda().contiguous(), 1)
    torch.cuda.synchronize()
    bad = {}
    for b, (name, f, P) in enumerate(cases):
        vel = oracle.split_rlepso_state(batch.read_state(b), NP, dim, NLOG)['vel']
        agree = decode_agreement(vel, f, P, reference_targets(f, P), _philox_fdr_weights(seeds[b], NP, dim))
        if not agree.all():
            bad[name] = bad.get(name, 0) + int((~agree).sum())
    batch.close()
    assert not bad, bad
