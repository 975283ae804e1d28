"""GPU: the run-time-geometry step kernels (LDE, GLEET, RL-PSO, QLPSO, DE, PSO) against the C oracle at the geometries they branch on -- even / odd D (the 2x2
register tile of the matvec against its one-element loop), odd row counts, the align2 padding of the LDS arrays, a padded state stride (NP D odd), particles across the
63 / 64 / 65 wave boundary and at 255 / 256, k_lde_step<256> against <512> -- and at budgets that do not divide: max_fes = 3 NP + 17, five log points.  The comparison
is parity.compare, the one the canonical `*_philox_parity_with_oracle` tests make, plus done / fes / cost_len / curve after every step.  Then every state word of an
instance alone, inside a batch and inside the permuted batch, and the fused routes against one launch per step, at the same shapes.

RLEPSO, whose kernels branch on geometry most, has a sweep of its own (parity.RLEPSO_SHAPES: swarm size, dimension AND group count): the ranking's slices of j
(MBX_NT / NP = 1, 2, 3, ..), the move phase's tables inside Z up to the last rank a byte holds (NP = 256), the 512- and 1024-thread instantiations at D = 2 x waves
and at odd D with NP off a wave boundary, NP % n_group != 0 and n_group = 1, 3, 7; whole episodes of 12 NP + 17 evaluations; then __reinit, planted on both sides, at
the same shapes.  What the oracle alone must show there runs without a GPU too (tests/test_rlepso_edge_conditions.py)."""
import numpy as np
import pytest
import torch

import parity
import policy_exact as pe
from helpers import load, print_ledger

pytestmark = pytest.mark.gpu

ALGOS = ('lde', 'gleet', 'rlpso', 'qlpso', 'de', 'pso')
SHAPES = [(4, 2), (5, 3), (63, 7), (64, 10), (65, 33), (100, 40), (255, 13), (256, 10)]
NLOG = 5
OVER_LONG = (4, 2, 45, 2, 5)               # (NP, D, max_fes, log_interval, n_logpoint): at least three entries too long for every algorithm (tests/test_curve_bound.py)
OVER_LONG_RLEPSO = (5, 2, 45, 2, 5)        # NP = 4 is refused with five groups; nine entries in six slots (tests/test_rlepso_edge_conditions.py)
RLEPSO_SHAPES = sorted(parity.RLEPSO_SHAPES)
MBX_E_UNSUPPORTED = -3


def _problems(D):
    """Nine instances: bbob 1, 3, 10, 15, 17, 21 and one noisy function per noise model."""
    return parity.edge_problems(D)


def _budget(NP):
    max_fes = 3 * NP + 17                    # no multiple of NP: the last generation overshoots
    return max_fes, max_fes // NLOG, NLOG


def _steps(name, NP, max_fes):
    """To the end of the budget: six generations where a step moves the population, or as many as the budget takes (seven at NP = 4); where a step moves one
    particle, max_fes - NP steps: more than NP + 3, so the particle pointer wraps."""
    return max(NP + 3, max_fes - NP) if name in parity.PER_PARTICLE else max(6, -(-(max_fes - NP) // NP))


# NP = 4 makes this budget (29, 5, 5) the over-long one of tests/test_curve_bound.py for the kernels that spend NP evaluations a step: seven entries in six slots
ONE_TOO_LONG = {('lde', 4, 2), ('gleet', 4, 2)}


def _report(name, NP, D, total, ledger):
    what = max(total, key=total.get)
    print(f'geometry-edges | {name:5s} | NP {NP:3d} D {D:2d} | worst deviation / tolerance {total[what]:.3g} ({what})')
    print_ledger(ledger)


@pytest.mark.parametrize('NP,D', SHAPES)
@pytest.mark.parametrize('name', ALGOS)
def test_step_kernel_matches_the_oracle_at_edge_geometries(name, NP, D):
    budget = _budget(NP)

    def fits(want):                          # on the oracle alone, before anything is launched: these budgets stay inside the curve
        longest = max(v['sc']['cost_len'] for rec in want for v in rec['views'])
        assert longest == NLOG + 2 if (name, NP, D) in ONE_TOO_LONG else longest <= NLOG + 1, (name, NP, D, longest)
        assert all(rec['done'][-1] for rec in want), (name, NP, D)
    ledger = []
    total, info, got, _ = parity.hip_vs_oracle(name, _problems(D), NP, D, budget, _steps(name, NP, budget[0]), ledger, oracle_check=fits)
    assert info['fixed_geometry'] == 0, info
    assert all(rec['done'][-1] for rec in got)
    _report(name, NP, D, total, ledger)


def test_lde_sweep_covers_both_workgroup_sizes():
    from metabox_amd.suite import Batch, Suite
    threads = set()
    for NP, D in SHAPES:
        s = Suite(_problems(D))
        b = Batch(s, parity.ALGO['lde'], np.arange(9), parity.seeds_for('lde', 9), NP, *_budget(NP))
        info = b.launch_info()
        assert info['fixed_geometry'] == 0, info
        threads.add(info['threads'])
        b.close(); s.close()
    assert threads == {256, 512}, threads


# ------------------------------------------------------------------------------------------------ RLEPSO: edge swarm sizes and group counts
@pytest.mark.parametrize('NP,D,n_group', RLEPSO_SHAPES)
def test_rlepso_matches_the_oracle_at_edge_swarm_sizes_and_groups(NP, D, n_group):
    """k_rlepso_step with run-time geometry, whole episodes (12 NP + 17 evaluations, five log points) of the nine instances against one oracle each: the ranking's
    slices, the move phase's tables inside Z, the 256 / 512 / 1024-thread instantiations, NP % n_group != 0, n_group = 1, 3, 7."""
    ledger = []
    total, info, got, _ = parity.hip_vs_oracle('rlepso', _problems(D), NP, D, parity.rlepso_edge_budget(NP), parity.RLEPSO_STEPS, ledger,
                                               oracle_check=parity.rlepso_fits_and_ends, n_group=n_group)
    assert info['fixed_geometry'] == 0 and info['threads'] == parity.RLEPSO_SHAPES[(NP, D, n_group)], info
    assert all(rec['done'][-1] for rec in got)
    _report(f'rlepso g{n_group}', NP, D, total, ledger)


def test_rlepso_sweep_covers_the_three_workgroup_sizes():
    from metabox_amd.suite import Batch, Suite
    threads = set()
    for NP, D, n_group in RLEPSO_SHAPES:
        s = Suite(_problems(D))
        b = Batch(s, parity.ALGO['rlepso'], np.arange(9), parity.seeds_for('rlepso', 9), NP, *parity.rlepso_edge_budget(NP), n_group=n_group)
        info = b.launch_info()
        assert info['fixed_geometry'] == 0 and info['threads'] == parity.RLEPSO_SHAPES[(NP, D, n_group)], (NP, D, n_group, info)
        threads.add(info['threads'])
        b.close(); s.close()
    assert threads == {256, 512, 1024}, threads


@pytest.mark.parametrize('NP,D,n_group', RLEPSO_SHAPES)
def test_rlepso_reinit_matches_the_oracle_at_edge_swarm_sizes_and_groups(NP, D, n_group):
    """__reinit at the same shapes.  Twelve generations of random actions do not reach it, so it is planted on both sides: after reset() every other stagnation counter
    of the kernel's own state block is set to 100, the block is written back and handed to the oracle, and the actions put c_mutation = 0.01 into every group.  First,
    on the oracle alone: a noisy instance bills more than NP evaluations in some generation.  Then the comparison of the sweep above, with the __reinit flag and fes exact.
    (Where NP % n_group != 0 the particles without coefficients do not move: the oracle re-evaluates the position whose cost it was handed in the kernel's words, so on
    a noise-free function `new_cost < c_cost` is decided by the last bits of two evaluations of the same point -- a proven near-tie at generation 0 that ends that
    instance's comparison and is printed with the ledger.  The noisy instances, whose costs are redrawn, go through; `compared` insists on one.)"""
    ps = _problems(D)

    def bills(want):
        parity.rlepso_reinit_bills(want, NP, ps)
        assert all(rec['done'][-1] for rec in want) and max(v['sc']['cost_len'] for rec in want for v in rec['views']) <= NLOG + 1
    ledger = []
    total, info, got, want = parity.hip_vs_oracle('rlepso', ps, NP, D, parity.rlepso_edge_budget(NP), parity.RLEPSO_STEPS, ledger, oracle_check=bills, n_group=n_group,
                                                  actions=parity.rlepso_reinit_actions(9, n_group), start=parity.rlepso_stagnant(NP, D))
    assert info['fixed_geometry'] == 0, info
    fired = parity.rlepso_reinit_bills(want, NP, ps)                 # the oracles that started from the kernel's own blocks
    cut = {}                                                        # instance -> the generation at which a proven near-tie ended its comparison
    for _, case, g0, _ in ledger:
        if ' pni' in case or ' done' in case:
            k = int(case.split('#')[1].split()[0])
            cut[k] = min(g0, cut.get(k, g0))
    compared = [(k, g) for k, g in fired if g < cut.get(k, parity.RLEPSO_STEPS)]
    assert compared, (fired, ledger)                                # at least one re-initialising generation of a noisy instance went through the whole comparison
    for k, g in compared:
        assert got[k]['views'][g + 1]['sc']['reinit'] and got[k]['views'][g + 1]['sc']['fes'] == want[k]['views'][g + 1]['sc']['fes'] > got[k]['views'][g]['sc']['fes'] + NP
    _report(f'rlepso g{n_group} reinit', NP, D, total, ledger)


@pytest.mark.parametrize('name', ALGOS)
def test_np256_dim64_is_refused_before_any_launch(name):
    """NE + SC alone is 256 KB at (256, 64)."""
    from metabox_amd._abi import MbxError
    from metabox_amd.suite import Batch, Suite
    s = Suite(_problems(64))
    with pytest.raises(MbxError) as e:
        Batch(s, parity.ALGO[name], np.arange(9), parity.seeds_for(name, 9), 256, *_budget(256))
    msg = str(e.value)
    assert f'mbx error {MBX_E_UNSUPPORTED}:' in msg and 'needs' in msg and 'B of LDS per workgroup' in msg, msg
    s.close()


@pytest.mark.parametrize('name', ALGOS + ('rlepso',))
def test_over_long_curve_keeps_to_its_slots(name):
    """A budget whose reference list outgrows n_logpoint + 1: the kernel reports the oracle's true length and stored entries, and every instance of the batch still
    matches its own oracle -- an append past the slots would land in the first words (a position) of the next instance."""
    NP, D, max_fes, li, nlog = OVER_LONG_RLEPSO if name == 'rlepso' else OVER_LONG

    def outgrows(want):
        assert all(rec['done'][-1] and rec['views'][-1]['sc']['cost_len'] >= nlog + 4 for rec in want), name
    ledger = []
    total, info, got, want = parity.hip_vs_oracle(name, _problems(D), NP, D, (max_fes, li, nlog), 4 * max_fes, ledger, oracle_check=outgrows)
    assert not ledger, ledger                # the whole batch was compared to the end
    for g, w in zip(got, want):
        assert g['views'][-1]['sc']['cost_len'] == w['views'][-1]['sc']['cost_len'] >= nlog + 4
    _report(name, NP, D, total, ledger)


# ------------------------------------------------------------------------------------------------ bit for bit: batch composition
def _run_states(name, ps, slots, NP, steps):
    """The instances `slots` of the nine-instance batch (problem, seed and actions follow the slot) -> their state blocks after `steps` steps."""
    from metabox_amd.suite import Batch, Suite
    s = Suite(list(ps))
    slots = np.asarray(slots)
    b = Batch(s, parity.ALGO[name], slots, parity.seeds_for(name, 9)[slots], NP, *_budget(NP))
    b.reset()
    acts = parity.actions_for(name, steps, 9, NP)
    for g in range(steps):
        b.step(None if acts is None else torch.from_numpy(np.ascontiguousarray(acts[g][slots])).cuda())
    out = np.stack([b.read_state(k) for k in range(len(slots))])
    b.close(); s.close()
    return out


@pytest.mark.parametrize('NP,D', [(63, 7), (65, 33)])
@pytest.mark.parametrize('name', ALGOS + ('rs', 'rlepso'))
def test_state_words_do_not_depend_on_the_batch(name, NP, D):
    """NP D odd: the state stride is padded.  An instance alone, in the nine-instance batch and in that batch permuted: the same words."""
    ps = _problems(D)
    steps = NP + 3 if name in parity.PER_PARTICLE else 6
    full = _run_states(name, ps, np.arange(9), NP, steps)
    perm = np.array([4, 8, 0, 6, 2, 7, 1, 5, 3])
    mixed = _run_states(name, ps, perm, NP, steps)
    assert np.array_equal(mixed, full[perm], equal_nan=True), np.flatnonzero((mixed != full[perm]).any(axis=1))
    for k in (2, 7):                         # a plain and a noisy function
        alone = _run_states(name, ps, [k], NP, steps)
        assert np.array_equal(alone[0], full[k], equal_nan=True), (k, np.flatnonzero(alone[0] != full[k])[:8])
    assert len({row.tobytes() for row in full}) == 9                 # nine different instances


# ------------------------------------------------------------------------------------------------ bit for bit: fused routes against one launch per step
def _twins(name, NP, D, max_fes, li, nlog):
    from metabox_amd.suite import Batch, Suite
    s = Suite(_problems(D))
    seeds = parity.seeds_for(name, 9)
    a = Batch(s, parity.ALGO[name], np.arange(9), seeds, NP, max_fes, li, nlog)
    b = Batch(s, parity.ALGO[name], np.arange(9), seeds, NP, max_fes, li, nlog)
    a.reset(); b.reset()
    return s, a, b


def _same(a, b):
    ra, rb = a.results(), b.results()
    for key in ra:
        assert torch.equal(ra[key], rb[key]), key
    assert torch.equal(a.state, b.state)
    for k in range(a.B):
        sa, sb = a.read_state(k), b.read_state(k)
        assert np.array_equal(sa, sb, equal_nan=True), (k, np.flatnonzero(sa != sb)[:8])


@pytest.mark.parametrize('NP,D', [(63, 7), (5, 3)])
def test_rlpso_fused_rollout_equals_policy_plus_step(NP, D):
    """mbx_rlpso_rollout (actor 2 D -> 32 -> 8 -> 1 inside the step kernel) == mbx_gauss_policy + mbx_step per step."""
    w = torch.from_numpy(pe.seeded_gauss(np.random.RandomState(1000 + 14 * D + 32), 2 * D, 32, 8, 1)).cuda()
    net = (w, 32, 8, 0.01, 0.7)
    max_fes = _budget(NP)[0]
    s, a, b = _twins('rlpso', NP, D, *_budget(NP))
    n = max_fes - NP + 5                     # past the end of the episode
    ret_b = torch.zeros(9, dtype=torch.float64, device='cuda')
    for g in range(n):
        _, r, _ = b.step(b.gauss_policy(*net))
        ret_b += r
    ret_a = torch.zeros(9, dtype=torch.float64, device='cuda')
    for chunk in (1, NP + 3, n - NP - 4):
        _, r, _ = a.rlpso_rollout(*net, chunk)
        ret_a += r
    _same(a, b)
    ret = a.results()['return']
    assert torch.allclose(ret_a, ret, rtol=1e-12, atol=1e-12) and torch.allclose(ret_b, ret, rtol=1e-12, atol=1e-12) and bool((a.results()['fes'] == max_fes).all())
    a.close(); b.close(); s.close()


@pytest.mark.parametrize('NP,D', [(63, 7), (7, 3), (255, 17)])
def test_rlepso_rollout_host_loop_equals_one_act_step_per_generation(NP, D):
    """mbx_rlepso_rollout on its host-loop route (no resident kernel is built for these geometries) in chunks of 1, 5 and the rest past the end of every episode ==
    one mbx_rlepso_act_step per generation on a twin batch, with a seeded actor table (sigma 0.05 .. 0.35): trajectory records, results and every state word."""
    max_fes, li, nlog = parity.rlepso_edge_budget(NP)
    s, a, b = _twins('rlepso', NP, D, max_fes, li, nlog)
    assert not a.rollout_is_resident() and a.launch_info()['fixed_geometry'] == 0
    rows = int(a.lib.mbx_rlepso_policy_table_rows(a._h))
    table = torch.rand(rows, 2, 35, generator=torch.Generator().manual_seed(1000 + 14 * D + NP)).cuda()
    table[:, 1] = 0.05 + 0.3 * table[:, 1]
    table = table.contiguous()
    for chunk in (1, 5, parity.RLEPSO_STEPS - 6 + 3):
        st, rw, dn, traj = a.rlepso_rollout(table, chunk, trajectory=True)
        st, rw, dn = st.clone(), rw.clone(), dn.clone()
        rsum = torch.zeros(9, dtype=torch.float64, device='cuda')
        for g in range(chunk):
            live = (b.done == 0).clone()
            sb, rb, db, acts = b.act_step(table, want_actions=True)
            assert torch.equal(traj['state'][g], sb[:, 0]) and torch.equal(traj['reward'][g], rb) and torch.equal(traj['done'][g], db), g
            assert torch.equal(traj['actions'][g][live], acts[live]), g
            rsum += rb
        assert torch.equal(st[:, 0], sb[:, 0]) and torch.equal(dn, db) and torch.equal(rw, rsum)
        _same(a, b)
    res = a.results()
    assert bool((a.done == 1).all()) and bool((res['steps'] <= 15).all()) and bool((res['fes'] >= max_fes).any()), res       # the last launch went on past every episode's end
    a.close(); b.close(); s.close()


@pytest.mark.parametrize('NP,D', [(63, 7), (5, 3)])
def test_qlpso_fused_rollout_equals_one_step_launches(NP, D):
    """mbx_qlpso_rollout over many steps == the same entry point one step at a time, with the shipped Q-table."""
    q = torch.from_numpy(load('qlpso_policy.npz')['q_table']).cuda()
    max_fes = _budget(NP)[0]
    s, a, b = _twins('qlpso', NP, D, *_budget(NP))
    n = max_fes - NP + 5
    ret_a = torch.zeros(9, dtype=torch.float64, device='cuda')
    for chunk in (1, NP + 3, n - NP - 4):
        _, r, _ = a.qlpso_rollout(q, chunk)
        ret_a += r
    for _ in range(n):
        b.qlpso_rollout(q, 1)
    _same(a, b)
    assert torch.equal(ret_a, a.results()['return']) and bool((a.results()['fes'] == max_fes).all())
    a.close(); b.close(); s.close()


@pytest.mark.parametrize('NP,D', [(63, 7), (5, 3)])
def test_lde_rollout_host_loop_equals_policy_plus_step(NP, D):
    """mbx_lde_rollout on its host-loop route (no resident kernel is built for these geometries) == mbx_lde_policy + mbx_step per generation, with a seeded
    PolicyNet NP + 10 -> 16 -> 2 NP."""
    H = 16
    w = torch.from_numpy(pe.seeded_lstm(np.random.RandomState(2000 + 13 * NP + H), NP + 10, H, 2 * NP)).cuda()
    max_fes = 12 * NP
    s, a, b = _twins('lde', NP, D, max_fes, max_fes // 50, 50)
    assert not a.lde_rollout_is_resident()
    ha, ca = torch.zeros(9, H, device='cuda'), torch.zeros(9, H, device='cuda')
    hb, cb = torch.zeros(9, H, device='cuda'), torch.zeros(9, H, device='cuda')
    for n in (4, 9):                         # the second call ends every episode (generation 11) and goes on past it
        st, rw, dn = a.lde_rollout(w, H, ha, ca, n)
        st, rw, dn = st.clone(), rw.clone(), dn.clone()
        rsum = torch.zeros(9, dtype=torch.float64, device='cuda')
        for g in range(n):
            live = (b.done == 0).clone()
            hprev, cprev = hb.clone(), cb.clone()
            acts = b.lde_policy(w, H, hb, cb).clone()
            hb[~live] = hprev[~live]; cb[~live] = cprev[~live]       # (the per-generation policy kernel also advances finished instances; the rollout leaves them)
            sb, rb, db = b.step(acts)
            rsum += rb
        assert torch.equal(st, sb) and torch.equal(dn, db) and torch.equal(rw, rsum)
        assert torch.equal(ha, hb) and torch.equal(ca, cb)
        _same(a, b)
    assert bool((a.results()['steps'] == 11).all())
    a.close(); b.close(); s.close()
