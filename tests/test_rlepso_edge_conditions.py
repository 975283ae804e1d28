"""What the RLEPSO part of tests/test_gpu_geometry_edges.py needs from the C oracle alone, checked without a GPU: at every (NP, D, n_group) of the sweep the budget
12 NP + 17 with five log points ends every episode in 11 .. 15 generations with a curve of exactly n_logpoint + 1 entries; the planted stagnation counters make
__reinit bill evaluations in a noisy instance; the over-long budget outgrows the slots; and the oracle refuses the group counts whose action slice
actions[g * n_group : g * n_group + 7] (rlepso_optimizer.py:119) would end behind the 7 * n_group action row."""
import numpy as np
import pytest

import parity
from helpers import problems
from oracle import oracle

SHAPES = sorted(parity.RLEPSO_SHAPES)


def _records(NP, D, n_group, actions=None, start=None):
    ps = parity.edge_problems(D)
    seeds = parity.seeds_for('rlepso', len(ps))
    acts = parity.actions_for('rlepso', parity.RLEPSO_STEPS, len(ps), NP, n_group) if actions is None else actions
    return ps, [parity.oracle_record('rlepso', ps[k], NP, D, parity.rlepso_edge_budget(NP), seeds[k], acts[:, k], parity.RLEPSO_STEPS, n_group=n_group, start=start)
                for k in range(len(ps))]


@pytest.mark.parametrize('NP,D,n_group', SHAPES)
def test_the_edge_budget_ends_every_episode_inside_the_curve(NP, D, n_group):
    _, want = _records(NP, D, n_group)
    parity.rlepso_fits_and_ends(want)
    for k, rec in enumerate(want):                    # the comparator accepts the oracle against itself at this shape
        st = parity.compare('rlepso', rec, rec, f'NP{NP} D{D} G{n_group} #{k}', ledger=[])
        assert st and max(st.values()) == 0


@pytest.mark.parametrize('NP,D,n_group', SHAPES)
def test_planted_stagnation_reaches_reinit_in_a_noisy_instance(NP, D, n_group):
    ps, want = _records(NP, D, n_group, actions=parity.rlepso_reinit_actions(9, n_group), start=parity.rlepso_stagnant(NP, D))
    fired = parity.rlepso_reinit_bills(want, NP, ps)
    assert all(rec['done'][-1] for rec in want) and max(v['sc']['cost_len'] for rec in want for v in rec['views']) <= parity.RLEPSO_NLOG + 1
    assert min(g for _, g in fired) == 0              # every other particle carries 100 generations without improvement into the first update
    # the particles beyond n_group * (NP // n_group) keep c_mutation = 0 and are never re-initialised by their own counter: a generation bills at most NP + the planted ones
    planted = len(range(0, n_group * (NP // n_group), 2))
    for k, g in fired:
        if g == 0:
            assert want[k]['views'][1]['sc']['fes'] - NP <= NP + planted


def test_without_the_planted_counters_random_actions_do_not_reinitialise():
    """Why the counters are planted: twelve generations of random actions never reach __reinit (c_mutation <= 0.01, counters <= 12: probability <= 1.44 % per
    particle and generation at the very end only)."""
    NP, D, n_group = 63, 7, 5
    _, want = _records(NP, D, n_group)
    assert sum(v['sc']['reinit'] for rec in want for v in rec['views']) <= 2


def test_over_long_budget_outgrows_the_slots():
    NP, D, max_fes, li, nlog = 5, 2, 45, 2, 5
    ps = parity.edge_problems(D)
    acts = parity.actions_for('rlepso', 4 * max_fes, len(ps), NP)
    for k, p in enumerate(ps):
        rec = parity.oracle_record('rlepso', p, NP, D, (max_fes, li, nlog), parity.seeds_for('rlepso', 9)[k], acts[:, k], 4 * max_fes)
        assert rec['done'][-1] and rec['views'][-1]['sc']['cost_len'] == nlog + 4, (k, rec['views'][-1]['sc'])


@pytest.mark.parametrize('n_group', [0, 8, 16, 17])
def test_oracle_refuses_group_counts_whose_action_slice_is_short(n_group):
    p = problems('bbob', 10)[1]
    with pytest.raises(ValueError, match='n_group'):
        oracle.RlepsoOracle(p.desc(), p.bias, oracle.make_cfg(1, 100, 10, 20000, 400, 50, n_group=n_group), seed=1)


def test_oracle_reads_the_last_action_of_seven_groups_and_nothing_behind_it():
    """n_group = 7: group 6 reads actions 42 .. 48, the whole row.  Changing action 48 changes the step; the row handed over is exactly 49 floats long (the wrapper checks
    the length, so a read behind it would need a longer row)."""
    p = problems('bbob', 10)[3]
    cfg = oracle.make_cfg(1, 100, 10, 20000, 400, 50, n_group=7)
    a = np.random.RandomState(3).uniform(0.2, 1, size=49).astype(np.float32)
    out = []
    for last in (a[48], np.float32(0.05)):
        o = oracle.RlepsoOracle(p.desc(), p.bias, cfg, seed=5)
        o.reset()
        b = a.copy(); b[48] = last
        o.step(b)
        out.append(oracle.split_rlepso_state(o.state(), 100, 10, 50)['vel'].copy())
    assert not np.array_equal(out[0], out[1])
    assert np.array_equal(out[0].reshape(100, 10)[:84], out[1].reshape(100, 10)[:84])      # groups 0 .. 5 (particles 0 .. 83) do not read action 48
    with pytest.raises(AssertionError):
        o.step(a[:48])
