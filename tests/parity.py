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
the worst ratio per quantity."""
import copy

import numpy as np

from helpers import ATOL, RTOL, prove_tie_arrays
from oracle import oracle

ALGO = {'lde': 2, 'rlpso': 5, 'gleet': 6, 'qlpso': 7, 'de': 8, 'pso': 9, 'rs': 4}
PER_PARTICLE = ('rlpso', 'qlpso')                      # one evaluation per step; the others move the population
SEED = {'lde': (104729, 3), 'gleet': (53, 17), 'rlpso': (37, 9), 'qlpso': (71, 2), 'de': (977, 41), 'pso': (977, 41), 'rs': (977, 41)}
ACTION_SEED = {'lde': 5, 'gleet': 21, 'rlpso': 11, 'qlpso': 31, 'de': 0, 'pso': 0, 'rs': 0}
POSITIONS = {'lde': 'pop', 'gleet': 'pos', 'rlpso': 'pos', 'qlpso': 'pop', 'de': 'X', 'pso': 'X'}
BEST = {'lde': 'fit', 'gleet': 'pbest', 'rlpso': 'pbest', 'qlpso': 'cost', 'de': 'best', 'pso': 'best'}      # the per-particle cost a step may improve


def seeds_for(name, B):
    m, a = SEED[name]
    return np.arange(B, dtype=np.uint64) * m + a


def actions_for(name, G, B, NP):
    """Random actions from a fixed RandomState, drawn as the canonical parity test of the algorithm draws them."""
    rs = np.random.RandomState(ACTION_SEED[name])
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
        f = {'lde': oracle.split_lde_state, 'gleet': oracle.split_gleet_state, 'rlpso': oracle.split_rlpso_state, 'qlpso': oracle.split_qlpso_state}[name]
        v = dict(f(st, NP, D, nlog))
        v['curve'] = v['clog'] if name == 'qlpso' else v.pop('cost')
    sc = v['scalars']
    v['sc'] = {'gbest': sc[oracle.SC_GBEST], 'fes': sc[oracle.SC_FES], 'cost_len': int(sc[oracle.SC_COST_LEN]), 'done': bool(sc[oracle.SC_DONE])}
    if name == 'qlpso':
        v['sc'].update(pointer=int(sc[oracle.SC_QLPSO_POINTER]), diversity=sc[oracle.SC_QLPSO_DIVERSITY])
    return v


def _classic_view(o, name, done):
    r = o.result()
    X, c = o.population()
    best = o.pbest()[1] if name == 'pso' else c
    return {'X': X.ravel().copy(), 'best': best.copy(), 'curve': r['cost'].copy(),
            'sc': {'gbest': r['gbest'], 'fes': r['fes'], 'cost_len': r['cost_len'], 'done': bool(done)}}


def oracle_record(name, p, NP, D, budget, seed, actions, steps, per_step=True):
    """`steps` steps of one oracle instance (fewer when it terminates).  budget = (max_fes, log_interval, n_logpoint); actions: [G, ...] of this instance or None."""
    max_fes, li, nlog = budget
    cfg = oracle.make_cfg(ALGO[name], NP, D, max_fes, li, nlog)
    rec = {'name': name, 'NP': NP, 'D': D, 'nlog': nlog, 'feat': [], 'reward': [], 'done': [], 'views': []}
    if name in ('de', 'pso'):
        o = oracle.ClassicOracle(p.desc(), p.bias, cfg, seed=int(seed))
        o.reset()
        rec['feat0'] = None
        view = lambda d=False: _classic_view(o, name, d)
    else:
        cls = {'lde': oracle.LdeOracle, 'gleet': oracle.GleetOracle, 'rlpso': oracle.RlpsoOracle, 'qlpso': oracle.QlpsoOracle}[name]
        o = cls(p.desc(), p.bias, cfg, seed=int(seed))
        rec['feat0'] = o.reset()
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


def hip_records(name, batch, NP, D, nlog, actions, steps, per_step=True):
    """reset() + `steps` steps of a batch -> one record per instance, each cut at the step that finished it (the kernel leaves a finished instance alone)."""
    import torch
    B = batch.B
    st0 = batch.reset().cpu().numpy().copy()
    recs = [{'name': name, 'NP': NP, 'D': D, 'nlog': nlog, 'feat0': _feat(name, st0, b, NP), 'feat': [], 'reward': [], 'done': [], 'views': []} for b in range(B)]
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
    # ---- every step
    diverged = False
    for g in range(G):
        where = (ident, g)
        gv, wv = (got['views'][g + 1], want['views'][g + 1]) if per_step else (None, None)
        gp, wp = (got['views'][g], want['views'][g]) if per_step else (None, None)
        if name == 'lde':
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
            n = min(wv['sc']['cost_len'], got['nlog'] + 1)
            st.check('curve', gv['curve'][:n], wv['curve'][:n], RTOL, ATOL, where)
    if per_step:
        assert len(got['done']) == len(want['done']), (ident, 'one side went on after the other had finished', len(got['done']), len(want['done']))
    # ---- the state at the end
    fin, ref = got['views'][-1], want['views'][-1]
    if name == 'lde':
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


def hip_vs_oracle(name, ps, NP, D, budget, steps, ledger, flags=0, seeds=None, oracle_check=None):
    """One batch (instance k on problem ps[k]) through reset + `steps` steps, a view read after every step, against one oracle per instance.  The oracle runs first, and
    `oracle_check(records)` sees its records before anything is launched.  -> (worst deviation / tolerance per quantity, launch_info, the kernel's records, the oracle's)."""
    from metabox_amd.suite import Batch, Suite
    max_fes, li, nlog = budget
    B = len(ps)
    seeds = seeds_for(name, B) if seeds is None else seeds
    actions = actions_for(name, steps, B, NP)
    want = [oracle_record(name, ps[k], NP, D, budget, seeds[k], None if actions is None else actions[:, k], steps) for k in range(B)]
    if oracle_check is not None:
        oracle_check(want)
    s = Suite(list(ps))
    batch = Batch(s, ALGO[name], np.arange(B), seeds, NP, max_fes, li, nlog, flags=flags)
    info = batch.launch_info()
    got = hip_records(name, batch, NP, D, nlog, actions, steps)
    batch.close(); s.close()
    total = {}
    for k in range(B):
        merge(total, compare(name, got[k], want[k], f'{name} NP{NP} D{D} f{ps[k].func_id} #{k}', ledger))
    return total, info, got, want


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
    else:
        raise ValueError(defect)
    return bad
