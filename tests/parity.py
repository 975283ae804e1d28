"""A step kernel against the C oracle under Philox: one comparison per algorithm, shared by the `*_philox_parity_with_oracle` tests (canonical shapes) and by
tests/test_gpu_geometry_edges.py (edge geometries and awkward budgets).  Not a test module.

Both sides are turned into the same record, one per instance:

    feat0            what reset() returned (None for the classic baselines, whose state is fes / max_fes)
    feat[g]          what step g returned, reward[g], done[g]
    views            [view after reset(), view after step 0, ...] or [final view] alone; a view is the split state block plus
                     'sc' = {gbest, fes, cost_len, done, ...} and 'curve' (the n_logpoint + 1 stored entries)

`compare` asserts what the canonical tests always asserted, with their tolerances.  Where BOTH records hold a view per step it also compares done, fes, cost_len and the
stored curve entries after every step, and the positions at the end; an integer-valued output (GLEET's stagnation counters, a QLPSO reward, done) that differs must then be a
near-tie on the oracle's own margin (helpers.prove_tie_arrays, recorded in `ledger`), after which the two sides are different, equally valid trajectories and the comparison of
that instance ends.  Records without per-step views get the strict equality the canonical tests have.  Every float check also reports deviation / tolerance; `compare` returns
the worst ratio per quantity.

RLEPSO ('rlepso') is compared generation by generation, as tests/test_gpu_rlepso.py::_hip_vs_oracle compares it at the canonical shape: gbest, pbest and the positions
after every generation, the stagnation counters exact up to a first proven near-tie; its records always hold a view per step.  Its group count reaches both sides
(`n_group`), and both sides can adopt a planted state after reset() (`start`)."""
import copy

import numpy as np

from helpers import ATOL, RTOL, prove_tie_arrays
from oracle import oracle

ALGO = {'rlepso': 1, 'lde': 2, 'rlpso': 5, 'gleet': 6, 'qlpso': 7, 'de': 8, 'pso': 9, 'rs': 4}
PER_PARTICLE = ('rlpso', 'qlpso')                      # one evaluation per step; the others move the population
SEED = {'rlepso': (7919, 17), 'lde': (104729, 3), 'gleet': (53, 17), 'rlpso': (37, 9), 'qlpso': (71, 2), 'de': (977, 41), 'pso': (977, 41), 'rs': (977, 41)}
ACTION_SEED = {'rlepso': 11, 'lde': 5, 'gleet': 21, 'rlpso': 11, 'qlpso': 31, 'de': 0, 'pso': 0, 'rs': 0}
POSITIONS = {'rlepso': 'pos', 'lde': 'pop', 'gleet': 'pos', 'rlpso': 'pos', 'qlpso': 'pop', 'de': 'X', 'pso': 'X'}
BEST = {'rlepso': 'pbest', 'lde': 'fit', 'gleet': 'pbest', 'rlpso': 'pbest', 'qlpso': 'cost', 'de': 'best', 'pso': 'best'}      # the per-particle cost a step may improve


def seeds_for(name, B):
    m, a = SEED[name]
    return np.arange(B, dtype=np.uint64) * m + a


def actions_for(name, G, B, NP, n_group=5):
    """Random actions from a fixed RandomState, drawn as the canonical parity test of the algorithm draws them."""
    rs = np.random.RandomState(ACTION_SEED[name])
    if name == 'rlepso':
        return rs.uniform(0, 1, size=(G, B, 7 * n_group)).astype(np.float32)
    if name == 'lde':
        return rs.uniform(0, 1, size=(G, B, 2 * NP)).astype(np.float32)
    if name == 'gleet':
        return rs.rand(G, B, NP).astype(np.float32)
    if name == 'rlpso':
        return (rs.rand(G, B) * 1.4 - 0.2).astype(np.float32)
    if name == 'qlpso':
        return rs.randint(0, 4, size=(G, B)).astype(np.int32)
    return None


def split(name, st, NP, D, nlog):
    """One state block (kernel layout) -> view."""
    st = np.array(st, dtype=np.float64)
    if name in ('de', 'pso'):
        if name == 'de':
            v = {'X': st[:NP * D], 'best': st[NP * D:NP * D + NP]}
            off = NP * D + NP
        else:
            v = {'X': st[:NP * D], 'best': st[3 * NP * D:3 * NP * D + NP]}
            off = 3 * NP * D + NP + D
        v['scalars'], v['curve'] = st[off:off + 16], st[off + 16:off + 16 + nlog + 1]
    else:
        f = {'rlepso': oracle.split_rlepso_state, 'lde': oracle.split_lde_state, 'gleet': oracle.split_gleet_state, 'rlpso': oracle.split_rlpso_state,
             'qlpso': oracle.split_qlpso_state}[name]
        v = dict(f(st, NP, D, nlog))
        v['curve'] = v['clog'] if name == 'qlpso' else v.pop('cost')
    sc = v['scalars']
    v['sc'] = {'gbest': sc[oracle.SC_GBEST], 'fes': sc[oracle.SC_FES], 'cost_len': int(sc[oracle.SC_COST_LEN]), 'done': bool(sc[oracle.SC_DONE])}
    if name == 'rlepso':
        v['sc'].update(reinit=bool(sc[oracle.SC_REINIT]))            # __reinit fired in the last update
    if name == 'qlpso':
        v['sc'].update(pointer=int(sc[oracle.SC_QLPSO_POINTER]), diversity=sc[oracle.SC_QLPSO_DIVERSITY])
    return v


def _classic_view(o, name, done):
    r = o.result()
    X, c = o.population()
    best = o.pbest()[1] if name == 'pso' else c
    return {'X': X.ravel().copy(), 'best': best.copy(), 'curve': r['cost'].copy(),
            'sc': {'gbest': r['gbest'], 'fes': r['fes'], 'cost_len': r['cost_len'], 'done': bool(done)}}


def oracle_record(name, p, NP, D, budget, seed, actions, steps, per_step=True, n_group=5, start=None):
    """`steps` steps of one oracle instance (fewer when it terminates).  budget = (max_fes, log_interval, n_logpoint); actions: [G, ...] of this instance or None.
    start (RLEPSO): what the instance adopts after reset() -- a state block, or a function of the oracle's own block."""
    max_fes, li, nlog = budget
    cfg = oracle.make_cfg(ALGO[name], NP, D, max_fes, li, nlog, n_group=n_group)
    rec = {'name': name, 'NP': NP, 'D': D, 'nlog': nlog, 'feat': [], 'reward': [], 'done': [], 'views': []}
    assert start is None or name == 'rlepso', name
    if name in ('de', 'pso'):
        o = oracle.ClassicOracle(p.desc(), p.bias, cfg, seed=int(seed))
        o.reset()
        rec['feat0'] = None
        view = lambda d=False: _classic_view(o, name, d)
    else:
        cls = {'rlepso': oracle.RlepsoOracle, 'lde': oracle.LdeOracle, 'gleet': oracle.GleetOracle, 'rlpso': oracle.RlpsoOracle, 'qlpso': oracle.QlpsoOracle}[name]
        o = cls(p.desc(), p.bias, cfg, seed=int(seed))
        rec['feat0'] = o.reset()
        if start is not None:
            o.set_state(start(o.state()) if callable(start) else start)
        view = lambda d=False: split(name, o.state(), NP, D, nlog)
    if per_step:
        rec['views'].append(view())
    d = False
    for g in range(steps):
        if name in ('de', 'pso'):
            d = o.step()
            f, r = None, 0.
        else:
            f, r, d = o.step(actions[g])
        rec['feat'].append(f); rec['reward'].append(r); rec['done'].append(bool(d))
        if per_step:
            rec['views'].append(view(d))
        if d:
            break
    if not per_step:
        rec['views'].append(view(d))
    rec['reward'], rec['done'] = np.array(rec['reward'], dtype=np.float64), np.array(rec['done'], dtype=bool)
    return rec


def _feat(name, st, b, NP):
    if name == 'gleet':
        return st[b].reshape(NP, 27).copy()
    if name == 'qlpso':
        return int(st[b, 0])
    if name in ('de', 'pso', 'rs'):
        return None
    return st[b].copy()


def hip_records(name, batch, NP, D, nlog, actions, steps, per_step=True, start=None):
    """reset() + `steps` steps of a batch -> one record per instance, each cut at the step that finished it (the kernel leaves a finished instance alone).
    start: a function of an instance's state block after reset(); what it returns is written back and kept as the record's 'start'."""
    import torch
    B = batch.B
    st0 = batch.reset().cpu().numpy().copy()
    recs = [{'name': name, 'NP': NP, 'D': D, 'nlog': nlog, 'feat0': _feat(name, st0, b, NP), 'feat': [], 'reward': [], 'done': [], 'views': []} for b in range(B)]
    if start is not None:
        for b in range(B):
            recs[b]['start'] = start(batch.read_state(b))
            batch.write_state(b, recs[b]['start'])
    live = np.ones(B, bool)
    if per_step:
        for b in range(B):
            recs[b]['views'].append(split(name, batch.read_state(b), NP, D, nlog))
    for g in range(steps):
        if not live.any():
            break
        st, r, d = batch.step(None if actions is None else torch.from_numpy(np.ascontiguousarray(actions[g])).cuda())
        st, r, d = st.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().copy()
        for b in np.nonzero(live)[0]:
            recs[b]['feat'].append(_feat(name, st, b, NP)); recs[b]['reward'].append(r[b]); recs[b]['done'].append(bool(d[b]))
            if per_step:
                recs[b]['views'].append(split(name, batch.read_state(b), NP, D, nlog))
            live[b] = not d[b]
    for b in range(B):
        if not per_step:
            recs[b]['views'].append(split(name, batch.read_state(b), NP, D, nlog))
        recs[b]['reward'], recs[b]['done'] = np.array(recs[b]['reward'], dtype=np.float64), np.array(recs[b]['done'], dtype=bool)
    return recs


def _scalar(x):
    return float(np.ravel(x)[0])


class _Stats(dict):
    def check(self, what, got, want, rtol, atol, ident):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (ident, what, got.shape, want.shape)
        if got.size == 0:
            return
        ratio = np.abs(got - want) / (atol + rtol * np.abs(want))
        ratio = np.where(np.isnan(ratio), np.inf, ratio)               # NaN on either side is a failure
        worst = float(ratio.max())
        self[what] = max(self.get(what, 0.), worst)
        assert worst <= 1, (ident, what, 'deviation / tolerance', worst, 'at', int(np.argmax(ratio)))


def _tie(ledger, ident, g, what, rp, rn, ref, prev, cur, mine):
    """An integer-valued output differs: a near-tie on the oracle's margin, or a failure.  Strict when no ledger is kept."""
    assert ledger is not None, (ident, g, what, 'differs from the oracle', mine, ref)
    same = prove_tie_arrays(np.atleast_1d(rp), np.atleast_1d(rn), np.atleast_1d(ref), np.atleast_1d(prev), np.atleast_1d(cur), np.atleast_1d(mine), ledger, 'hip',
                            f'{ident} {what}', g)
    assert not same


def compare(name, got, want, ident, ledger=None, extras=True):
    """got: the kernel's record, want: the oracle's.  -> {quantity: worst deviation / tolerance}.  extras=False: the canonical tests' own assertions and nothing else."""
    st = _Stats()
    views = len(got['views']) > 1 and len(want['views']) > 1
    per_step = views and extras
    if not per_step:
        ledger = None
    G = min(len(got['done']), len(want['done']))
    # ---- reset
    if name == 'lde':
        st.check('feat0', got['feat0'], want['feat0'], 0., 1e-7, ident)
    elif name == 'gleet':
        st.check('feat0', got['feat0'], want['feat0'], 1e-7, 1e-9, ident)
    elif name == 'rlpso':
        st.check('feat0', got['feat0'], want['feat0'], 1e-12, 1e-13, ident)
    elif name == 'qlpso':
        assert got['feat0'] == want['feat0'], ident
    elif name == 'rlepso':
        assert views, 'RLEPSO is compared generation by generation: both records need a view per step'
        assert _scalar(got['feat0']) == _scalar(want['feat0']), ident                   # NP / max_fes
    # ---- every step
    diverged = False
    for g in range(G):
        where = (ident, g)
        gv, wv = (got['views'][g + 1], want['views'][g + 1]) if per_step else (None, None)
        gp, wp = (got['views'][g], want['views'][g]) if per_step else (None, None)
        if name == 'rlepso':
            # what tests/test_gpu_rlepso.py::_hip_vs_oracle asserts after every generation: gbest within the parity tolerance; the stagnation counters exact up to a
            # first difference that is a proven near-tie of `new_cost < c_cost`, after which the two sides are different trajectories; before it fes exact (below,
            # with done / cost_len / the curve and the __reinit flag), pbest within the tolerance and the positions within 1e-9
            gv, wv, gp, wp = got['views'][g + 1], want['views'][g + 1], got['views'][g], want['views'][g]
            st.check('gbest', gv['sc']['gbest'], wv['sc']['gbest'], RTOL, ATOL, where)
            if not np.array_equal(gv['pni'], wv['pni']):
                _tie(ledger, ident, g, 'pni', wp['ccost'], wv['ccost'], wv['pni'], gp['ccost'], gv['ccost'], gv['pni'])
                diverged = True
            else:
                st.check('pbest', gv['pbest'], wv['pbest'], RTOL, ATOL, where)
                st.check('pos', gv['pos'], wv['pos'], 0., 1e-9, where)
                if got['reward'][g] != want['reward'][g]:                               # +1 / -1 on gbest < pre_gbest
                    _tie(ledger, ident, g, 'reward: gbest < pre_gbest', wp['sc']['gbest'], wv['sc']['gbest'], want['reward'][g], gp['sc']['gbest'], gv['sc']['gbest'],
                         got['reward'][g])
            if diverged:                                                                # (the re-initialisation mask follows the counters: fes and done may differ from here on)
                return st
        elif name == 'lde':
            st.check('feat', got['feat'][g], want['feat'][g], 0., 1e-5, where)
            st.check('reward', got['reward'][g], want['reward'][g], 1e-5, 1e-9, where)
        elif name == 'gleet':
            st.check('feat', got['feat'][g], want['feat'][g], 1e-7, 1e-9, where)
            st.check('reward', got['reward'][g], want['reward'][g], 1e-5, 1e-9, where)
            if per_step and not np.array_equal(gv['pni'], wv['pni']):        # stagnation vs the previous CURRENT cost
                _tie(ledger, ident, g, 'pni', wp['ccost'], wv['ccost'], wv['pni'], gp['ccost'], gv['ccost'], gv['pni'])
                diverged = True
        elif name == 'rlpso':
            st.check('feat', got['feat'][g], want['feat'][g], 1e-9, 1e-11, where)
            st.check('reward', got['reward'][g], want['reward'][g], 1e-5, 1e-9, where)
        elif name == 'qlpso':
            assert got['feat'][g] == want['feat'][g], where                     # the next particle's stored action: no arithmetic behind it
            if got['reward'][g] != want['reward'][g]:
                assert per_step, (where, 'reward', got['reward'][g], want['reward'][g])
                i = wp['sc']['pointer']
                gi, wi = got['reward'][g] in (1, 2), want['reward'][g] in (1, 2)          # f_new < f_old
                if gi != wi:
                    _tie(ledger, ident, g, 'reward: f_new < f_old', wp['cost'][i], wv['cost'][i], wi, gp['cost'][i], gv['cost'][i], gi)
                gd, wd = got['reward'][g] in (0, 2), want['reward'][g] in (0, 2)          # d_new > d_old
                if gd != wd:
                    _tie(ledger, ident, g, 'reward: d_new > d_old', wp['sc']['diversity'], wv['sc']['diversity'], wd, gp['sc']['diversity'], gv['sc']['diversity'], gd)
                diverged = True
        elif views:                                                              # de / pso: best-so-far after every sweep
            st.check('gbest', got['views'][g + 1]['sc']['gbest'], want['views'][g + 1]['sc']['gbest'], 1e-9, 1e-12, where)
        if bool(got['done'][g]) != bool(want['done'][g]) and (per_step or name == 'rlpso'):
            assert per_step, (where, 'done', got['done'][g], want['done'][g])
            assert gv['sc']['fes'] == wv['sc']['fes'], (where, 'done differs with different fes', gv['sc']['fes'], wv['sc']['fes'])
            _tie(ledger, ident, g, 'done: gbest <= 1e-8', 1e-8, wv['sc']['gbest'], want['done'][g], 1e-8, gv['sc']['gbest'], got['done'][g])
            diverged = True
        if diverged:
            return st
        if per_step:                                                             # the bookkeeping log_and_terminate keeps
            assert (gv['sc']['done'], gv['sc']['fes'], gv['sc']['cost_len']) == (wv['sc']['done'], wv['sc']['fes'], wv['sc']['cost_len']), \
                (where, 'done / fes / cost_len', gv['sc'], wv['sc'])
            assert gv['sc']['done'] == bool(got['done'][g]), where
            if name == 'rlepso':                                                 # the state a step returns is fes / max_fes; did __reinit fire
                assert _scalar(got['feat'][g]) == _scalar(want['feat'][g]) and gv['sc']['reinit'] == wv['sc']['reinit'], (where, got['feat'][g], want['feat'][g], gv['sc'], wv['sc'])
            n = min(wv['sc']['cost_len'], got['nlog'] + 1)
            st.check('curve', gv['curve'][:n], wv['curve'][:n], RTOL, ATOL, where)
    if per_step:
        assert len(got['done']) == len(want['done']), (ident, 'one side went on after the other had finished', len(got['done']), len(want['done']))
    # ---- the state at the end
    fin, ref = got['views'][-1], want['views'][-1]
    if name == 'rlepso':                                                         # (pbest, pos: every generation, above)
        assert np.array_equal(fin['pni'], ref['pni']), ident
        st.check('ccost', fin['ccost'], ref['ccost'], RTOL, ATOL, ident)
        st.check('pbpos', fin['pbpos'], ref['pbpos'], 0., 1e-9, ident)
        st.check('vel', fin['vel'], ref['vel'], 0., 1e-9, ident)
    elif name == 'lde':
        st.check('fit', fin['fit'], ref['fit'], RTOL, ATOL, ident)
        st.check('pop', fin['pop'], ref['pop'], 0., 1e-9, ident)
        assert np.array_equal(fin['hsum'][:5], ref['hsum'][:5]), ident                  # (slot 5: the kernel's packed copy of the last histogram)
    elif name == 'gleet':
        st.check('pbest', fin['pbest'], ref['pbest'], RTOL, ATOL, ident)
        assert np.array_equal(fin['pni'], ref['pni']), ident
        st.check('scalars', fin['scalars'][:7], ref['scalars'][:7], RTOL, ATOL, ident)
        st.check('pfeat', fin['pfeat'], ref['pfeat'], 0., 1e-7, ident)
        st.check('gfeat', fin['gfeat'], ref['gfeat'], 0., 1e-7, ident)
    elif name == 'rlpso':
        st.check('pbest', fin['pbest'], ref['pbest'], RTOL, ATOL, ident)
        st.check('scalars', fin['scalars'][:7], ref['scalars'][:7], RTOL, ATOL, ident)
        st.check('pbpos', fin['pbpos'], ref['pbpos'], 0., 1e-9, ident)
    elif name == 'qlpso':
        st.check('cost', fin['cost'], ref['cost'], RTOL, ATOL, ident)
        st.check('pop', fin['pop'], ref['pop'], 0., 1e-9, ident)
        st.check('scalars', fin['scalars'][:7], ref['scalars'][:7], RTOL, ATOL, ident)
        st.check('diversity', fin['sc']['diversity'], ref['sc']['diversity'], 1e-12, 0., ident)
    else:
        st.check('X', fin['X'], ref['X'], 0., 1e-9, ident)
    if per_step:                                                                 # positions and per-particle costs of every algorithm, at the tolerances the canonical tests use
        st.check(POSITIONS[name], fin[POSITIONS[name]], ref[POSITIONS[name]], 0., 1e-9, ident)
        st.check(BEST[name], fin[BEST[name]], ref[BEST[name]], RTOL, ATOL, ident)
    return st


def merge(total, st):
    for k, v in st.items():
        total[k] = max(total.get(k, 0.), v)
    return total


def hip_vs_oracle(name, ps, NP, D, budget, steps, ledger, flags=0, seeds=None, oracle_check=None, n_group=5, actions=None, start=None):
    """One batch (instance k on problem ps[k]) through reset + `steps` steps, a view read after every step, against one oracle per instance.  The oracle runs first, and
    `oracle_check(records)` sees its records before anything is launched.  -> (worst deviation / tolerance per quantity, launch_info, the kernel's records, the oracle's).
    n_group (RLEPSO) reaches the oracle's configuration and the batch's; actions: [steps, B, ...] instead of actions_for's.
    start (RLEPSO): a function of a state block, applied after reset() on both sides -- first on every oracle's own block, which is what `oracle_check` sees; then on the
    kernel's blocks, which are written back and handed to a second set of oracles (set_state), so that the comparison starts from the same words."""
    from metabox_amd.suite import Batch, Suite
    max_fes, li, nlog = budget
    B = len(ps)
    seeds = seeds_for(name, B) if seeds is None else seeds
    actions = actions_for(name, steps, B, NP, n_group) if actions is None else actions
    run = lambda k, st: oracle_record(name, ps[k], NP, D, budget, seeds[k], None if actions is None else actions[:, k], steps, n_group=n_group, start=st)
    want = [run(k, start) for k in range(B)]
    if oracle_check is not None:
        oracle_check(want)
    s = Suite(list(ps))
    batch = Batch(s, ALGO[name], np.arange(B), seeds, NP, max_fes, li, nlog, n_group=n_group, flags=flags)
    info = batch.launch_info()
    got = hip_records(name, batch, NP, D, nlog, actions, steps, start=start)
    batch.close(); s.close()
    if start is not None:
        want = [run(k, got[k]['start']) for k in range(B)]
    total = {}
    for k in range(B):
        merge(total, compare(name, got[k], want[k], f'{name} NP{NP} D{D} f{ps[k].func_id} #{k}', ledger))
    return total, info, got, want


# ------------------------------------------------------------------------------------------------ RLEPSO at the edge swarm sizes and group counts
# Shared by tests/test_gpu_geometry_edges.py (the kernels) and tests/test_rlepso_edge_conditions.py (what the oracle alone must show, without a GPU).
# (NP, D, n_group) -> threads per workgroup the library picks (rlepso_prepare: rl_lds_doubles * 8 > 80 KB and D >= 16 / 32), and what the shape reaches
RLEPSO_SHAPES = {
    (5, 2, 5): 256,          # smallest swarm with five groups; the 2 * kThreads floor of rl_z_doubles
    (7, 3, 5): 256,          # per_group 1, particles 5 and 6 without coefficients, odd D
    (63, 7, 5): 256, (64, 10, 5): 256, (65, 33, 5): 256,        # wave boundary; padded stride; 73 KB, just under the 80 KB switch
    (85, 10, 5): 256,        # ranking: three slices of j with uneven ends
    (129, 10, 5): 256,       # first NP with one ranking slice
    (255, 13, 5): 256, (256, 10, 5): 256,                        # KB holds rank 255; NP = workgroup width
    (256, 16, 5): 512,       # D = 2 x 8 waves exactly: the evaluator's per-wave partials fill T
    (255, 17, 5): 512,       # odd D, NP off the wave boundary
    (130, 32, 5): 1024,      # D = 2 x 16 waves exactly
    (129, 33, 5): 1024,      # odd D
    (100, 10, 1): 256,       # one group
    (100, 10, 7): 256,       # the largest legal group count: the last slice ends at action 48
    (7, 3, 7): 256,          # per_group 1 with seven groups
    (23, 5, 3): 256,         # a remainder of 2 with three groups
}
RLEPSO_NLOG = 5
RLEPSO_STEPS = 16            # 11 .. 15 generations end every episode below


def edge_problems(D):
    """Nine instances: bbob 1, 3, 10, 15, 17, 21 and one noisy function per noise model."""
    from helpers import problems
    return [problems('bbob', D)[f] for f in (1, 3, 10, 15, 17, 21)] + [problems('bbob-noisy', D)[f] for f in (101, 117, 130)]


def rlepso_edge_budget(NP):
    max_fes = 12 * NP + 17                   # no multiple of NP: the last generation overshoots
    return max_fes, max_fes // RLEPSO_NLOG, RLEPSO_NLOG


def rlepso_fits_and_ends(want):
    """On the oracle's records alone: the curve stays inside its n_logpoint + 1 slots and every instance ends."""
    longest = max(v['sc']['cost_len'] for rec in want for v in rec['views'])
    assert longest == RLEPSO_NLOG + 1, longest
    assert all(rec['done'][-1] for rec in want), [len(rec['done']) for rec in want]
    assert all(11 <= len(rec['done']) <= 15 for rec in want), [len(rec['done']) for rec in want]


def rlepso_reinit_actions(B, n_group):
    """Random actions whose a[g * n_group], the first entry of group g's slice, is 1: c_mutation = 0.01 in every group."""
    a = actions_for('rlepso', RLEPSO_STEPS, B, 0, n_group)
    a[:, :, [g * n_group for g in range(n_group)]] = 1.
    return a


def rlepso_stagnant(NP, D):
    """block -> block with every other stagnation counter at 100: with c_mutation = 0.01 such a particle is re-initialised with probability 1 unless it improves first."""
    def start(block):
        block = np.array(block, dtype=np.float64)
        block[3 * NP * D + 2 * NP:3 * NP * D + 3 * NP:2] = 100.
        return block
    return start


def rlepso_reinit_bills(want, NP, ps):
    """On the oracle's records alone: in at least one noisy instance at least one generation bills more than NP evaluations (__reinit fired); -> those (instance, generation)."""
    fired = [(k, g) for k, rec in enumerate(want) if ps[k].noise[0] != 0
             for g in range(len(rec['done'])) if rec['views'][g + 1]['sc']['fes'] - rec['views'][g]['sc']['fes'] > NP]
    assert fired, 'no generation of a noisy instance re-initialises: the planted state does not reach __reinit'
    assert all(want[k]['views'][g + 1]['sc']['reinit'] for k, g in fired)
    return fired


def canonical(name, batch, ps, seeds, NP, D, budget, G, ids, per_step=False):
    """What the canonical `*_philox_parity_with_oracle` tests assert, and nothing more: `batch` (instance k on ps[k]) through reset + G steps against one oracle each."""
    nlog = budget[2]
    actions = actions_for(name, G, batch.B, NP)
    got = hip_records(name, batch, NP, D, nlog, actions, G, per_step=per_step)
    for k in range(batch.B):
        want = oracle_record(name, ps[k], NP, D, budget, seeds[k], None if actions is None else actions[:, k], G, per_step=per_step)
        compare(name, got[k], want, ids[k], extras=False)


def plant(rec, defect):
    """A copy of an oracle record with one defect in its last view (tests/test_parity_comparator.py shows that `compare` rejects each).  None where the record
    offers no place for it (a curve without two different neighbours, a swarm whose costs did not move)."""
    name, bad = rec['name'], copy.deepcopy(rec)
    v, v0 = bad['views'][-1], bad['views'][0]
    if defect == 'coordinate':                       # the last coordinate of one particle, 1e-6 relative
        X = v[POSITIONS[name]].reshape(rec['NP'], rec['D'])
        rows = np.nonzero(np.abs(X[:, -1]) > 1e-2)[0]
        if rows.size == 0:
            return None
        X[rows[-1], -1] *= 1 + 1e-6
    elif defect == 'pbest':                          # the last particle whose best cost moved keeps the value it had after reset()
        key = BEST[name]
        moved = np.nonzero(np.abs(v[key] - v0[key]) > 1e-3 * np.abs(v[key]) + 1e-6)[0]
        if moved.size == 0:
            return None
        v[key][moved[-1]] = v0[key][moved[-1]]
    elif defect == 'cost_len':
        v['sc']['cost_len'] += 1
        if 'scalars' in v:
            v['scalars'][oracle.SC_COST_LEN] += 1
    elif defect == 'curve':                          # one entry replaced by its neighbour
        n = min(v['sc']['cost_len'], rec['nlog'] + 1)
        c = v['curve']
        ks = [k for k in range(n - 1) if abs(c[k] - c[k + 1]) > 1e-3 * abs(c[k]) + 1e-6]
        if not ks:
            return None
        c[ks[-1]] = c[ks[-1] + 1]
    elif defect == 'pni':                            # RLEPSO: the stagnation counter of the particle whose cost moved most, one too high (no near-tie behind it)
        v['pni'][int(np.argmax(np.abs(v['ccost'] - bad['views'][-2]['ccost'])))] += 1
    elif defect == 'reinit':                         # RLEPSO: the __reinit flag of the last update
        v['sc']['reinit'] = not v['sc']['reinit']
    elif defect == 'fes':
        v['sc']['fes'] += 1
    else:
        raise ValueError(defect)
    return bad
