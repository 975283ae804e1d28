"""GPU: the resident RLEPSO kernel after its non-scan trims (cross-lane ranking count, scalar bookkeeping, one-barrier re-initialisation count).

k_rlepso_run<256, 100, 10, 5> carries fes / log_index / cost_len / the return as integers on the scalar unit, ranks the particles by ballots and counts the
re-initialised particles per wave; k_rlepso_step (one launch per generation) keeps the float64 per-lane forms.  Both must stay the same function:

  * bit-identity: 48 instances (the 24 bbob kinds x 2 seeds), 40 generations in resident launches of 1, 7 and 32 against mbx_rlepso_act_step one generation at a
    time -- trajectory records, every state block after every launch, results().  The batch holds an instance that terminates by the stop rule INSIDE a launch (F5:
    it reaches its optimum corner in about 25 generations), two in which __reinit fires inside the 7- and inside the 32-generation launch (F7: seed and horizon chosen
    on the CPU oracle -- the first re-initialisations of an episode come after 50 to 150 generations, so these two instances start from the oracle's state that
    many generations into their episode) and every instance crosses log points (one per four generations).
  * bookkeeping: the same runs without the stop rule against the C oracle, which replays the actions the kernel drew: state (fes / maxFEs), reward and done after
    every generation, and fes / cost_len / steps / return after every launch, exactly.
  * equal costs: collapsed swarms (a few cost levels, whole-row copies) through both routes: the ranking's index tie-break and the FDR scan's copy marking.

The actor table has sigma = 0 (the sampled action is the table's mu, bit for bit), so that the CPU oracle can be run ahead of the GPU to choose the F7 seeds and
their head starts; sampled actions are covered by tests/test_gpu_rlepso.py.
"""
import numpy as np
import pytest

from helpers import problems
from oracle import oracle

NP, D, NLOG, MAXFES, LOGI = 100, 10, 50, 20000, 400
ROWS = MAXFES + 2 * NP + 1
GENS, CHUNKS = 40, (1, 7, 32)
B = 48
F5, F7 = 4, 6                    # instance k runs function 1 + k % 24
# seeds: 104729 k + 11, except the two F7 instances: chosen by _f7_with_reinit() below
SEEDS = np.arange(B, dtype=np.uint64) * 104729 + 11


def mu_table():
    """[ROWS, 35] float32 in [0, 1]: the action of an instance whose fes is r is row r.  The five c_mutation entries (group g reads a[5 g : 5 g + 7]) are 1: the
    re-initialisation probability 1e-4 a[5 g] per_no_improve^2 at its largest."""
    mu = np.random.RandomState(2027).uniform(0., 1., (ROWS, 35)).astype(np.float32)
    mu[:, 0:25:5] = 1.
    return mu


def oracle_run(fid, seed, gens, early_stop, mu, start=None, actions=None):
    """`gens` generations of the C oracle; the action of a generation is mu[fes] (or actions[g]).  -> per-generation records and the final state block."""
    p = problems('bbob', D)[fid]
    cfg = oracle.make_cfg(1, NP, D, MAXFES, LOGI, NLOG, early_stop=int(early_stop))
    o = oracle.RlepsoOracle(p.desc(), p.bias, cfg, seed=int(seed))
    o.reset()
    if start is not None:
        o.set_state(start)
    fes = int(oracle.split_rlepso_state(o.state(), NP, D, NLOG)['scalars'][oracle.SC_FES])
    rec = {'state': [], 'reward': [], 'done': [], 'fes': [], 'cost_len': [], 'return': [], 'fes0': fes}
    for g in range(gens):
        st, rw, dn = o.step(mu[min(fes, ROWS - 1)] if actions is None else actions[g])
        sc = oracle.split_rlepso_state(o.state(), NP, D, NLOG)['scalars']
        fes = int(sc[oracle.SC_FES])
        for k, v in (('state', st), ('reward', rw), ('done', dn), ('fes', fes), ('cost_len', int(sc[oracle.SC_COST_LEN])), ('return', sc[oracle.SC_RETURN])):
            rec[k].append(v)
        if dn:
            break
    return rec, o.state()


def _reinit_generations(rec):
    """0-based generations of a run in which __reinit billed evaluations (fes grew by more than NP)."""
    return np.flatnonzero(np.diff([rec['fes0']] + rec['fes']) != NP)


def _f7_with_reinit(mu, n=2):
    """[(seed, state block)]: the first seeds 1000 + 17 j and, for each, the latest oracle state from which __reinit fires inside the 7-generation launch (behind its
    first generation is not required: any of generations 1 .. 7) and inside the 32-generation launch (generations 8 .. 39) of the GENS that follow."""
    out = []
    for j in range(100):
        seed = 1000 + 17 * j
        at = _reinit_generations(oracle_run(7, seed, 160, True, mu)[0])
        heads = [h for h in range(1, 120) if ((at - h >= 1) & (at - h < 8)).any() and ((at - h >= 8) & (at - h < GENS)).any()]
        if heads:
            rec, head = oracle_run(7, seed, heads[-1], True, mu)
            assert not any(rec['done'])
            out.append((seed, head))
            if len(out) == n:
                return out
    raise AssertionError('no F7 seed re-initialises inside both launches')


@pytest.fixture(scope='module')
def plan():
    """Everything the CPU decides before the GPU runs: the table, the seeds, the F5 head start (computed once, shared, never modified)."""
    mu = mu_table()
    seeds = SEEDS.copy()
    (seeds[F7], h0), (seeds[F7 + 24], h1) = _f7_with_reinit(mu)
    rec, _ = oracle_run(5, seeds[F5], GENS, True, mu)
    assert rec['done'][-1] and 9 < len(rec['done']) < GENS - 1, ('on the oracle the F5 instance must stop inside the 32-generation launch', len(rec['done']))
    return {'mu': mu, 'seeds': seeds, 'heads': {F7: h0, F7 + 24: h1}}


def _batches(plan, early_stop, n=2):
    import torch
    from metabox_amd.suite import Batch, Suite
    from metabox_amd._abi import ALGO_RLEPSO
    ps = [problems('bbob', D)[f] for f in range(1, 25)]
    s = Suite(ps)
    out = [Batch(s, ALGO_RLEPSO, np.arange(B) % 24, plan['seeds'], NP, MAXFES, LOGI, NLOG, early_stop=early_stop) for _ in range(n)]
    table = torch.zeros(ROWS, 2, 35, dtype=torch.float32)
    table[:, 0] = torch.from_numpy(plan['mu'])
    for b in out:
        assert b.rollout_is_resident() and b.launch_info()['lds_bytes'] <= 32768
        b.reset()
    torch.cuda.synchronize()
    for b in out:
        for k, blk in plan['heads'].items():
            b.write_state(k, blk)
    return out, table.cuda().contiguous()


def _same_states(a, b, tag):
    for k in range(B):
        sa, sb = a.read_state(k), b.read_state(k)
        assert np.array_equal(sa, sb, equal_nan=True), (tag, k, np.flatnonzero(sa != sb)[:8])


@pytest.mark.gpu
def test_resident_equals_per_generation_bit_for_bit(plan):
    import torch
    (a, b), table = _batches(plan, True)
    done_at, g0 = {}, 0
    for n in CHUNKS:
        st, rw, dn, traj = a.rlepso_rollout(table, n, trajectory=True)
        st, rw, dn = st.clone(), rw.clone(), dn.clone()
        rsum = torch.zeros(B, dtype=torch.float64, device='cuda')
        for g in range(n):
            live = (b.done == 0).clone()
            sb, rb, db, acts = b.act_step(table, want_actions=True)
            assert torch.equal(traj['state'][g], sb[:, 0]) and torch.equal(traj['reward'][g], rb) and torch.equal(traj['done'][g], db), (n, g)
            assert torch.equal(traj['actions'][g][live], acts[live]), (n, g)
            rsum += rb
            for k in torch.nonzero(db.cpu()).flatten().tolist():
                done_at.setdefault(k, (n, g))
        assert torch.equal(st[:, 0], sb[:, 0]) and torch.equal(dn, db) and torch.equal(rw, rsum), n
        torch.cuda.synchronize()
        _same_states(a, b, n)
        g0 += n
    ra, rb_ = a.results(), b.results()
    for key in ra:
        assert torch.equal(ra[key], rb_[key]), key
    fes, clen = ra['fes'].cpu().numpy(), ra['cost_len'].cpu().numpy()
    a.close(); b.close()
    # what the batch was built to hold
    assert F5 in done_at and done_at[F5][0] == 32 and 0 < done_at[F5][1] < 31, ('F5 must stop inside the 32-generation launch', done_at)
    assert fes[F5] < MAXFES, 'by the stop rule, not by the budget'
    for k, blk in plan['heads'].items():
        fes0 = oracle.split_rlepso_state(blk, NP, D, NLOG)['scalars'][oracle.SC_FES]
        assert k not in done_at and fes[k] > fes0 + NP * GENS, '__reinit must have billed evaluations on F7'
    live = np.array([k not in done_at and k not in plan['heads'] for k in range(B)])
    assert (clen[live] >= 1 + (NP * (GENS + 1)) // LOGI).all(), 'every live instance crossed its log points'


@pytest.mark.gpu
def test_resident_bookkeeping_equals_the_oracle_without_the_stop_rule(plan):
    import torch
    (a,), table = _batches(plan, False, n=1)
    orc_state = [plan['heads'].get(k) for k in range(B)]
    reinit = set()
    for n in CHUNKS:
        _, _, _, traj = a.rlepso_rollout(table, n, trajectory=True)
        torch.cuda.synchronize()
        acts, st, rw, dn = (traj[k].cpu().numpy() for k in ('actions', 'state', 'reward', 'done'))
        res = {k: v.cpu().numpy() for k, v in a.results().items()}
        for k in range(B):
            rec, orc_state[k] = oracle_run(1 + k % 24, plan['seeds'][k], n, False, plan['mu'], start=orc_state[k], actions=acts[:, k])
            for g in range(n):
                assert st[g, k] == rec['state'][g] and rw[g, k] == rec['reward'][g] and bool(dn[g, k]) == bool(rec['done'][g]), (n, k, g)
            sc = oracle.split_rlepso_state(orc_state[k], NP, D, NLOG)['scalars']
            assert res['fes'][k] == sc[oracle.SC_FES] and res['cost_len'][k] == sc[oracle.SC_COST_LEN], (n, k, res['fes'][k], sc[oracle.SC_FES])
            assert res['steps'][k] == sc[oracle.SC_GEN] and res['return'][k] == sc[oracle.SC_RETURN], (n, k)
            if n > 1 and (_reinit_generations(rec) >= 1).any():          # inside a launch, behind its first generation
                reinit.add(k)
    a.close()
    assert F7 in reinit and F7 + 24 in reinit, reinit


def collapsed_swarm(rs, levels):
    """pbest costs from `levels` values, coordinates on a 0.25 grid, a tenth of the rows whole copies of another row (same cost, same position)."""
    f = -1000. - 3. * rs.randint(0, levels, NP)            # below every objective value: no particle improves, the equal costs last
    P = 0.25 * rs.randint(-16, 17, (NP, D)).astype(np.float64)
    for _ in range(NP // 10):
        i, j = rs.choice(NP, 2, replace=False)
        f[j], P[j] = f[i], P[i]
    return f, P


def collapsed_block(template, f, P):
    st = template.copy()
    sp = oracle.split_rlepso_state(st, NP, D, NLOG)
    sp['pos'][:] = P.ravel(); sp['vel'][:] = 0.; sp['pbpos'][:] = P.ravel()
    sp['pbest'][:] = f; sp['ccost'][:] = f; sp['pni'][:] = 0.
    g = int(np.argmin(f))
    sp['gbpos'][:] = P[g]
    sp['scalars'][oracle.SC_GBEST] = f[g]; sp['scalars'][oracle.SC_GBEST_IDX] = g
    return st


@pytest.mark.gpu
def test_equal_cost_swarms_rank_alike_on_both_routes():
    """Where pbest costs are equal the number of strictly better particles is NOT the rank: the resident kernel's contested-slot fallback and k_rlepso_step's
    `<` / `<=` count must order the swarm alike, generation after generation, while the equal costs last."""
    import torch
    from metabox_amd.suite import Batch, Suite
    from metabox_amd._abi import ALGO_RLEPSO
    rs = np.random.RandomState(77)
    n = 24
    swarms = [collapsed_swarm(rs, (3, 12, 40)[k % 3]) for k in range(n)]
    assert all(len(np.unique(f)) < NP for f, _ in swarms)
    s = Suite([problems('bbob', D)[f] for f in (1, 7, 15)])
    seeds = np.arange(n, dtype=np.uint64) * 7 + 3
    a, b = (Batch(s, ALGO_RLEPSO, np.arange(n) % 3, seeds, NP, MAXFES, LOGI, NLOG, early_stop=False) for _ in range(2))      # (gbest < 1e-8 from the start)
    table = torch.zeros(ROWS, 2, 35, dtype=torch.float32)
    table[:, 0] = torch.from_numpy(mu_table())
    table = table.cuda().contiguous()
    a.reset(); b.reset()
    torch.cuda.synchronize()
    template = a.read_state(0)
    for k, (f, P) in enumerate(swarms):
        blk = collapsed_block(template, f, P)
        a.write_state(k, blk); b.write_state(k, blk)
    ties = 0
    for m in (1, 2, 5):
        _, _, _, traj = a.rlepso_rollout(table, m, trajectory=True)
        for g in range(m):
            sb, rb, db = b.act_step(table)
            assert torch.equal(traj['state'][g], sb[:, 0]) and torch.equal(traj['reward'][g], rb) and torch.equal(traj['done'][g], db), (m, g)
        torch.cuda.synchronize()
        for k in range(n):
            sa, sb_ = a.read_state(k), b.read_state(k)
            assert np.array_equal(sa, sb_, equal_nan=True), (m, k, np.flatnonzero(sa != sb_)[:8])
            pb = oracle.split_rlepso_state(sa, NP, D, NLOG)['pbest']
            ties += NP - len(np.unique(pb))
    a.close(); b.close()
    assert ties >= 100, ('the swarms must still hold equal pbest costs while they are compared', ties)
