"""GPU: the FDR scan with one trip count per wave (csrc/mbx_rlepso.hpp: fdr_exact's `bound`) picks the reference's exemplar on every item.

The swarms of tests/test_fdr_bound.py (CRAFTED: equal costs, strictly increasing costs, two cost levels, the best row duplicated, worse-cost rows at zero distance,
cost gaps over 2^40, cost-ties of the best beside long scans, whole-row copies that rl_mark_copies takes out) go through the kernels the way tests/test_fdr_ties.py
observes exemplars: the crafted table is written as the pbest table of a state block, one generation runs with only the FDR term alive, and the new velocity of every
(particle, dimension) item must be, bit for bit, the one np.argmin of the reference's rounded quotients produces (rlepso_optimizer.py:97-109, first index) -- on the
route with one launch per generation (replay tape) and through mbx_rlepso_rollout (the resident kernel where the geometry has one, Philox draws).

Geometries: NP 100 / D 10 (compile-time geometry: 500 items, the second pass runs backwards and leaves its last wave partly empty), the same with
MBX_F_GENERIC_GEOMETRY, NP 77 / D 7 (odd D: one coordinate per item; 539 items: the third pass holds 27 of them in one wave) and NP 5 / D 2, the smallest swarm
mbx_batch_create accepts with five groups.
"""
import numpy as np
import pytest

from helpers import problems
from oracle import oracle
from test_fdr_bound import crafted_swarms
from test_fdr_ties import ACTION, NLOG, U_FDR, _philox_fdr_weights, decode_agreement, reference_targets, replay_tape, state_block


@pytest.fixture(scope='module')
def swarms():
    """{(NP, D): [(name, f, P)]} with the reference's exemplars, computed once."""
    out = {}
    for np_, dim in ((100, 10), (77, 7), (5, 2)):
        out[np_, dim] = [(name, f, P, reference_targets(f, P)) for name, f, P in crafted_swarms(np_, dim)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['per_generation', 'rollout'])
@pytest.mark.parametrize('np_,dim,generic', [(100, 10, False), (100, 10, True), (77, 7, False), (5, 2, False)])
def test_hip_fdr_exemplars_with_a_wave_uniform_scan_bound(swarms, np_, dim, generic, route):
    import torch
    from metabox_amd.suite import Batch, Suite
    from metabox_amd._abi import ALGO_RLEPSO, F_GENERIC_GEOMETRY
    cases = swarms[np_, dim]
    n = len(cases)
    assert 20 <= n <= 30
    maxfes = 2000 * dim
    p = problems('bbob', dim)[1]
    seeds = np.arange(n, dtype=np.uint64) * 7 + 3
    batch = Batch(Suite([p]), ALGO_RLEPSO, np.zeros(n, int), seeds, np_, maxfes, maxfes // NLOG, NLOG, flags=F_GENERIC_GEOMETRY if generic else 0)
    info, resident = batch.launch_info(), batch.rollout_is_resident()
    assert info['fixed_geometry'] == (1 if (np_, dim) == (100, 10) and not generic else 0), info
    assert resident == ((np_, dim) == (100, 10) and not generic)
    batch.reset()
    torch.cuda.synchronize()
    template = batch.read_state(0)
    for b, (_, f, P, _) in enumerate(cases):
        batch.write_state(b, state_block(template, f, P))
    if route == 'per_generation':
        batch.set_tape(torch.from_numpy(np.tile(replay_tape(np_, dim), (n, 1))).cuda())
        batch.step(torch.from_numpy(np.tile(ACTION, (n, 1))).cuda())
    else:
        table = torch.zeros(maxfes + 2 * np_ + 1, 2, 35, dtype=torch.float32)
        table[:, 0] = torch.from_numpy(ACTION)                          # mu = ACTION, sigma = 0
        batch.rlepso_rollout(table.cuda().contiguous(), 1)
    torch.cuda.synchronize()
    bad = {}
    items = 0
    for b, (name, f, P, targets) in enumerate(cases):
        vel = oracle.split_rlepso_state(batch.read_state(b), np_, dim, NLOG)['vel']
        u = U_FDR if route == 'per_generation' else _philox_fdr_weights(seeds[b], np_, dim)
        agree = decode_agreement(vel, f, P, targets, u)
        items += agree.size
        if not agree.all():
            bad[name] = bad.get(name, 0) + int((~agree).sum())
    batch.close()
    print(f'NP {np_} / D {dim}{" generic" if generic else ""}, {route}{" (resident)" if resident and route == "rollout" else ""}: '
          f'{sum(bad.values())} of {items} items moved with an exemplar other than np.argmin\'s')
    assert not bad, bad
