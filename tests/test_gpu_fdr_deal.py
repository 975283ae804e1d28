"""GPU: the FDR pass deals its items from the top of the table (csrc/mbx_rlepso.hpp: fdr_deal_item / fdr_deal_top; tests/test_fdr_deal.py restates the arithmetic):
the partial chunk is the lowest one and sits in the first lanes of pass 0, whole waves of pass 0 are idle where more than 64 slots are (NP 100 / D 12, NP 77 / D 7,
NP 5 / D 2).  Every item must still get the exemplar it got before.

  * the resident route (mbx_rlepso_rollout) against per-generation stepping (mbx_rlepso_act_step), np.array_equal on every state block, 6 generations from a reset: one
    instance per BBOB function at NP 100 / D 10, and 4 instances at NP 100 / D 12 (three passes, off = 168: two idle waves and a partial one);
  * the crafted swarms of tests/test_fdr_bound.py and collapsed swarms (a few cost levels on a coarse grid, whole-row copies) through k_rlepso_step at NP 100 / D 10,
    NP 77 / D 7 and NP 5 / D 2, and through the resident kernel at NP 100 / D 10: the velocity of every (particle, dimension) item must be the one np.argmin of the
    reference's rounded quotients produces.  A collapsed swarm flags more than MBX_FDR_OWN_AT items, so every lane settles its own (fdr_settle_own), which derives
    the lane's item from the deal a second time.
"""
import numpy as np
import pytest

from helpers import problems
from oracle import oracle
from test_fdr_bound import crafted_swarms
from test_fdr_ties import ACTION, NLOG, U_FDR, _philox_fdr_weights, decode_agreement, reference_targets, replay_tape, state_block
from test_gpu_rlepso_trims3 import _both_routes


@pytest.mark.gpu
def test_resident_equals_per_generation_on_the_24_functions():
    ps = [problems('bbob', 10)[f] for f in range(1, 25)]
    _both_routes(ps, np.arange(24), 10, 20000, 400, 50, 1)


@pytest.mark.gpu
def test_resident_equals_per_generation_at_d12_with_idle_waves_in_pass_0():
    from metabox_amd.problem.protein_docking import Protein_Docking_Dataset
    tr, te = Protein_Docking_Dataset.get_datasets('protein', difficulty='easy')
    ps = [tr.data[0], tr.data[7], te.data[0], te.data[-1]]
    assert all(p.dim == 12 for p in ps) and 3 * 256 - 100 * 6 == 168
    _both_routes(ps, np.arange(4), 12, 1000, 200, 5, 8)


def collapsed_swarm(rs, levels, np_, dim):
    """pbest costs from `levels` values, coordinates on a 0.25 grid, a tenth of the rows whole copies of another row (tests/test_gpu_rlepso_trims.py, any geometry)."""
    f = -1000. - 3. * rs.randint(0, levels, np_)
    P = 0.25 * rs.randint(-16, 17, (np_, dim)).astype(np.float64)
    for _ in range(np_ // 10):
        i, j = rs.choice(np_, 2, replace=False)
        f[j], P[j] = f[i], P[i]
    return f, P


@pytest.fixture(scope='module')
def swarms():
    """{(NP, D): [(name, f, P, the reference's exemplars)]}, computed once."""
    out = {}
    for np_, dim in ((100, 10), (77, 7), (5, 2)):
        rs = np.random.RandomState(404 + np_)
        cases = crafted_swarms(np_, dim) + [(f'collapsed_{lv}', *collapsed_swarm(rs, lv, np_, dim)) for lv in (3, 12, 40)]
        out[np_, dim] = [(name, f, P, reference_targets(f, P)) for name, f, P in cases]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('np_,dim,route', [(100, 10, 'per_generation'), (77, 7, 'per_generation'), (5, 2, 'per_generation'), (100, 10, 'resident')])
def test_every_exemplar_is_np_argmins_on_crafted_and_collapsed_swarms(swarms, np_, dim, route):
    import torch
    from metabox_amd.suite import Batch, Suite
    from metabox_amd._abi import ALGO_RLEPSO
    cases = swarms[np_, dim]
    n = len(cases)
    assert {'swarm_all_equal', 'swarm_zero_distance', 'swarm_increasing', 'collapsed_3'} <= {c[0] for c in cases}
    maxfes = 2000 * dim
    seeds = np.arange(n, dtype=np.uint64) * 7 + 3
    batch = Batch(Suite([problems('bbob', dim)[1]]), ALGO_RLEPSO, np.zeros(n, int), seeds, np_, maxfes, maxfes // NLOG, NLOG)
    assert batch.rollout_is_resident() == ((np_, dim) == (100, 10))
    batch.reset()
    torch.cuda.synchronize()
    template = batch.read_state(0)
    for b, (_, f, P, _) in enumerate(cases):
        batch.write_state(b, state_block(template, f, P))
    if route == 'per_generation':                                   # k_rlepso_step, draws from the replay tape
        batch.set_tape(torch.from_numpy(np.tile(replay_tape(np_, dim), (n, 1))).cuda())
        batch.step(torch.from_numpy(np.tile(ACTION, (n, 1))).cuda())
    else:                                                           # k_rlepso_run, Philox draws; mu = ACTION, sigma = 0
        table = torch.zeros(maxfes + 2 * np_ + 1, 2, 35, dtype=torch.float32)
        table[:, 0] = torch.from_numpy(ACTION)
        batch.rlepso_rollout(table.cuda().contiguous(), 1)
    torch.cuda.synchronize()
    bad = {}
    for b, (name, f, P, targets) in enumerate(cases):
        vel = oracle.split_rlepso_state(batch.read_state(b), np_, dim, NLOG)['vel']
        u = U_FDR if route == 'per_generation' else _philox_fdr_weights(seeds[b], np_, dim)
        agree = decode_agreement(vel, f, P, targets, u)
        if not agree.all():
            bad[name] = bad.get(name, 0) + int((~agree).sum())
    batch.close()
    assert not bad, bad
