"""The DE-DDQN step kernel (k_dq_step / k_dq_reset, csrc/mbx_ddqn.hpp) against an exact one-step host restatement (tests/ddqn_exact.py).

Every check goes through `check_step`: the block after a step must equal, bit for bit, the restatement of the block before it (the trial cost
is read from the appended OM_W entry), reward and done must be equal, an accepted trial must be dq_trial() bit for bit, the exact features must
be bit-equal and the reductions inside their derived bounds, and the five indices must be the Philox draws of (seed, steps, episode).

CPU: the restatement follows the trace-pinned C oracle along natural trajectories and on every planted state (so the bounds are not tighter than
float64 allows: the oracle's worst error / bound is printed per feature group); fourteen deliberately defective restatements are each rejected
by check_step on the planted states; the planted states together take every branch the restatement names (ALL_TAGS).
GPU: the same planted states, written into one Batch per geometry with write_state, four actions per state, three consecutive steps each
restated from its own read-back, on (NP, D) = (5, 2), (8, 3), (33, 7), (100, 10), (129, 10), the largest even NP the library takes at D = 10, and
protein docking (100, 12) on the compile-time-geometry kernel and the run-time-geometry one.
"""
import functools

import numpy as np
import pytest

import ddqn_exact as dx
from ddqn_exact import (SC_COST_LEN, SC_DONE, SC_EPISODE, SC_FES, SC_GBEST, SC_GEN, SC_LOG_INDEX, W, X_CPRE, X_G0, X_GBVIEW, X_GEN,
                        X_GWORST, X_MEDHI, X_MEDLO, X_OMWLEN, X_POINTER, X_PREVIEW)
from helpers import problems
from oracle import oracle

MAXFES, INTERVAL, NLOG = 4000, 800, 5
GEOMS = [(5, 2), (8, 3), (33, 7), (100, 10), (129, 10)]
N_MAIN, N_SPHERE = 248, 8                       # instances of a batch on the main problem / on the sphere (whose optimum a trial can hit)
SENTINEL = 777.
BASE_STEPS = 7


def seed_of(slot):
    """Philox seeds below and above 2^32, so a dropped high word shows."""
    return slot * 7 + 1 if slot % 2 == 0 else (1 << 33) + (slot << 35) + slot


@functools.lru_cache(maxsize=None)
def _probs(D):
    """(main, sphere) problems of a geometry: D = 12 is protein docking (no optimum, no sphere)."""
    if D == 12:
        from test_protein import protein
        return (list(protein()[0].values())[7],)
    ps = problems('bbob', D)
    return ps[15], ps[1]


def _cfg(p, NP):
    return dx.Cfg(NP, p.dim, NLOG, MAXFES, INTERVAL, 1, float(p.lb), float(p.ub), p.opt is not None)


def _optimum(p):
    return None if p.opt is None else p.bias


# ================================================================================================ the comparison
def _where(k, cfg):
    L = cfg.lay
    names = [n for n in L._fields if n != 'n']
    offs = [getattr(L, n) for n in names]
    j = max(i for i, o in enumerate(offs) if o <= k)
    return f'{names[j]}[{k - offs[j]}]'


def _cut(S, cfg):
    """Every stored word as it is, but for the cost list beyond its length (read_state reports it padded with its last value)."""
    C = S.copy()
    P = dx.parts(C, cfg)
    P['clog'][int(P['sc'][SC_COST_LEN]):] = 0.
    return C


def _same_bits(want, got, cfg, label):
    diff = np.nonzero(want.view(np.uint64) != got.view(np.uint64))[0]
    assert len(diff) == 0, (label, [(_where(int(k), cfg), want[k], got[k]) for k in diff[:6]])


class Stats:
    def __init__(self):
        self.worst, self.n = {g: 0. for g in dx.GROUPS}, 0

    def add(self, w):
        self.n += 1
        for g, v in w.items():
            self.worst[g] = max(self.worst[g], v)

    def report(self, who):
        print(f'{who}: {self.n} feature vectors, worst |error| / derived bound: ' + ', '.join(f'{g} {v:.3f}' for g, v in self.worst.items()))


def check_features(feat, block, cfg, stats, label):
    f, tol = dx.dq_features(block, cfg)
    bad, worst = dx.judge_features(feat, f, tol)
    assert not bad, (label, [(k, float(feat[k]), float(f[k]), tol[k]) for k in bad[:6]])
    if stats is not None:
        stats.add(worst)


def check_step(pre, action, post, reward, done, feat, cfg, seed=None, med=True, raw=False, stats=None, label=''):
    """One step of one instance, judged.  -> the tags of the branches it took."""
    P0, P1 = dx.parts(pre, cfg), dx.parts(post, cfg)
    if P0['sc'][SC_DONE] != 0:                  # an instance already done: nothing moves
        _same_bits(dx.canon(pre, cfg, med), dx.canon(post, cfg, med), cfg, label)
        if raw:
            _same_bits(_cut(pre, cfg), _cut(post, cfg), cfg, label)
        assert reward == 0 and done, label
        assert feat is None or np.all(feat == SENTINEL), (label, 'state_out row of a finished instance was written')
        return {'already_done'}
    n1 = int(P1['ex'][X_OMWLEN])
    assert 1 <= n1 <= W, (label, n1)
    tc = P1['omw'][n1 - 1, 5]
    r_next = P1['r'][:5].copy()
    want, rw, dn, tags = dx.dq_step(pre, action, tc, r_next, cfg)
    _same_bits(dx.canon(want, cfg, med), dx.canon(post, cfg, med), cfg, label)
    if raw:
        _same_bits(_cut(want, cfg), _cut(post, cfg), cfg, label)     # the words no reader uses (stale gbest / prebest arrays, window tail) stay untouched too
    assert reward == rw and bool(done) == dn, (label, reward, rw, done, dn)
    p = int(P0['ex'][X_POINTER])
    if tags & {'sel_lt', 'sel_eq'}:
        assert P1['X'][p].tobytes() == dx.dq_trial(pre, action, cfg).tobytes() and P1['cost'][p].tobytes() == np.float64(tc).tobytes(), label
    else:
        assert P1['X'][p].tobytes() == P0['X'][p].tobytes() and P1['cost'][p].tobytes() == P0['cost'][p].tobytes(), label
    if med:
        lo, hi = dx.order_stats(P0['cost'])
        assert P1['ex'][X_MEDLO].tobytes() == lo.tobytes() and P1['ex'][X_MEDHI].tobytes() == hi.tobytes(), (label, 'median cache')
    check_features(feat, post, cfg, stats, label)
    if seed is not None:
        assert np.array_equal(r_next, dx.dq_draws(seed, int(P1['sc'][SC_GEN]), int(P1['sc'][SC_EPISODE]), cfg.NP)), (label, 'draws')
    return tags


# ================================================================================================ planted states
def _fill_window(S, cfg, ops, tcs, rs):
    P = dx.parts(S, cfg)
    n = len(ops)
    P['omw'][:n, 0] = ops
    P['omw'][:n, 1:5] = rs.normal(size=(n, 4)) * 3
    P['omw'][:n, 5] = tcs
    P['ex'][X_OMWLEN] = n


def _fill_rings(S, cfg, gen, rs):
    """Rings as `gen` started sweeps leave them: the slots of the last min(gen, 10) generations hold counts, sums and maxima."""
    P = dx.parts(S, cfg)
    for name in ('ntot', 'nsucc', 'omsum', 'ommax'):
        P[name][:] = 0.
    for g in range(min(gen, dx.GENMAX)):
        s = dx.slot(g, gen)
        for op in range(4):
            nt = rs.randint(1, 30)
            P['ntot'][op, s] = nt
            for m in range(4):
                ns = rs.randint(1, nt + 1)
                vals = rs.uniform(0.01, 40., ns)
                P['nsucc'][op * 4 + m, s], P['omsum'][op * 4 + m, s], P['ommax'][op * 4 + m, s] = ns, vals.sum(), vals.max()
    P['ex'][X_GEN] = gen


def _own_gbest(S, cfg):
    """X_gbest as an array of its own (a copy of the row it viewed), so c_gbest may differ from that row's cost."""
    P = dx.parts(S, cfg)
    if P['ex'][X_GBVIEW] != 0:
        P['gbpos'][:] = P['X'][int(P['ex'][X_G0])]
        P['ex'][X_GBVIEW] = 0.


def _above(tc):
    return tc + abs(tc) + 1.


def plant(fresh, base, cfg, p, rs, sphere=False):
    """-> [(name, action, block, rewrite)]: `rewrite(block, tc)`, where given, is applied once the trial cost of (block, action) is known (the
    problems are noiseless, so the step from the rewritten block evaluates the same trial)."""
    NP = cfg.NP
    out = []

    def add(name, fn, src=base, rewrite=None, actions=range(4)):
        for a in actions:
            S = src.copy()
            fn(S, dx.parts(S, cfg), a)
            out.append((name, a, S, rewrite))

    def others(P):
        """indices that are neither the pointer nor G0, in cost order"""
        skip = {int(P['ex'][X_POINTER]), int(P['ex'][X_G0])}
        return [int(j) for j in np.argsort(P['cost'], kind='stable') if int(j) not in skip]

    if sphere:                                  # the trial IS the optimum: cost 0 <= 1e-8, early stop, cost list appended
        def target(S, P, a):
            free = others(P)
            P['X'][free[0]] = p.opt
            P['r'][:5] = [free[0], free[1], free[1], free[2], free[2]]
        add('target', target)
        add('target_fresh', target, src=fresh)
        return out

    K = NP // 2

    def cache(S, P):
        P['ex'][X_MEDLO], P['ex'][X_MEDHI] = dx.order_stats(P['cost'])

    def move(S, P, frm, to):
        """cache the statistics, then move one cost from below / above them to `to(sorted costs)`"""
        cache(S, P)
        srt = np.sort(P['cost'])
        ranks = [j for j in np.argsort(P['cost'], kind='stable') if int(j) != int(P['ex'][X_G0])]
        i = ranks[0] if frm == 'below' else ranks[-1]
        P['cost'][i] = to(srt)

    # ---- median
    add('fresh', lambda S, P, a: None, src=fresh)                                                    # cache NaN, pointer 0, gen 0 -> 1, both views
    add('med_valid', lambda S, P, a: cache(S, P))
    add('med_cross_up', lambda S, P, a: move(S, P, 'below', lambda s: (s[K] + s[K + 1]) / 2))
    add('med_cross_down', lambda S, P, a: move(S, P, 'above', lambda s: (s[K - 2] + s[K - 1]) / 2))
    add('med_land_lo', lambda S, P, a: move(S, P, 'below', lambda s: s[K] if NP & 1 else s[K - 1]))
    add('med_land_hi', lambda S, P, a: move(S, P, 'above', lambda s: s[K]))
    add('med_below_to_hi', lambda S, P, a: move(S, P, 'below', lambda s: s[K]), actions=(0, 3))
    add('med_above_to_lo', lambda S, P, a: move(S, P, 'above', lambda s: s[K - 1]), actions=(1, 2))

    def bogus(kind):
        def fn(S, P, a):
            lo, hi = dx.order_stats(P['cost'])
            P['ex'][X_MEDLO], P['ex'][X_MEDHI] = {'between': ((lo + hi) / 2 + 1e-9, hi + 1e-9), 'infinite': (-np.inf, np.inf), 'swapped': (hi + 1., lo - 1.)}[kind]
        return fn
    for kind in ('between', 'infinite', 'swapped'):
        add(f'med_bogus_{kind}', bogus(kind), actions=(0, 2) if kind != 'between' else range(4))

    def dups(cached):
        def fn(S, P, a):
            order = [j for j in np.argsort(P['cost'], kind='stable')]
            v = P['cost'][order[K]]
            for j in order[max(K - 2, 0):K + 2]:
                if int(j) != int(P['ex'][X_G0]):
                    P['cost'][j] = v
            if cached:
                cache(S, P)
        return fn
    add('med_dups', dups(False), actions=(0, 1))
    add('med_dups_cached', dups(True), actions=(2, 3))

    def all_equal(S, P, a):
        c = P['sc'][SC_GBEST]
        P['cost'][:] = c
        P['ex'][X_GWORST] = P['ex'][X_CPRE] = c
    add('all_equal', all_equal)
    add('all_equal_fresh', all_equal, src=fresh, actions=(1,))

    # ---- window
    def window(n, where, tied=None):
        def fn(S, P, a):
            other = [o for o in range(4) if o != a]
            ops = np.array([other[k] for k in rs.randint(0, 3, n)], dtype=np.float64)
            for k in where:
                ops[k] = a
            tcs = rs.permutation(n) * 1.5 + 2.
            if tied:
                tcs[list(tied)] = tcs.max() + 1.
            _fill_window(S, cfg, ops, tcs, rs)
        return fn
    add('win49', window(49, (3, 30)))
    add('win50_op_at_0', window(50, (0, 12)))
    add('win50_op_at_49', window(50, (49,)))
    add('win50_op_mid', window(50, (20, 35)))
    add('win50_no_op_unique', window(50, ()))
    add('win50_no_op_tied', window(50, (), tied=(17, 31)))
    add('win50_no_op_tied_ends', window(50, (), tied=(0, 49)), actions=(0, 3))

    # ---- rings
    def sweep(gen, pointer=0):
        def fn(S, P, a):
            _fill_rings(S, cfg, gen, rs)
            P['ex'][X_POINTER] = pointer
            P['ex'][X_CPRE] = P['sc'][SC_GBEST] + 3.25          # c_prebest is the initial best and never refreshed (:135)
        return fn
    for gen in (1, 9, 10, 23):
        add(f'ring_gen_{gen}_to_{gen + 1}', sweep(gen))
    add('ring_gen_23_inside', sweep(23, pointer=min(3, NP - 2)))

    def holes(S, P, a):
        _fill_rings(S, cfg, 5, rs)
        P['ex'][X_POINTER] = 2
        s = dx.slot(2, 5)
        P['ntot'][1, s] = 0.
        for name in ('nsucc', 'omsum', 'ommax'):
            P[name][4:8, s] = 0.                # an operator never chosen in that sweep
        s = dx.slot(0, 5)
        P['ntot'][a, s] = 6.
        for name in ('nsucc', 'omsum', 'ommax'):
            P[name][a * 4:a * 4 + 4, s] = 0.    # the chosen operator has not succeeded in the open sweep: its next success is the first maximum
            P[name][8:12, dx.slot(1, 5)] = 0.   # chosen, never successful
    add('ring_holes', holes)

    # ---- views
    def own_gbest_sweep(S, P, a):
        _fill_rings(S, cfg, 3, rs)
        P['ex'][X_POINTER] = 0
        P['ex'][X_GBVIEW], P['ex'][X_PREVIEW] = 0., 1.
        P['gbpos'][:] = np.clip(P['X'][int(P['ex'][X_G0])] + 0.125, cfg.lb, cfg.ub)
        P['prepos'][:] = P['X'][int(P['ex'][X_G0])] * 0.5
    add('view_sweep_own_gbest', own_gbest_sweep)

    def at_g0(S, P, a):
        _own_gbest(S, cfg)
        P['ex'][X_PREVIEW] = 1.
        P['ex'][X_POINTER] = P['ex'][X_G0]

    def accept(S, tc):
        P = dx.parts(S, cfg)
        P['cost'][int(P['ex'][X_POINTER])] = _above(tc)
        P['ex'][X_GWORST] = max(P['ex'][X_GWORST], _above(tc))
    add('view_prebest_follows_g0', at_g0, rewrite=accept)

    def before_new_best(S, P, a):
        P['ex'][X_POINTER] = (int(P['ex'][X_G0]) + 1) % NP
        if P['ex'][X_POINTER] != 0:
            P['ex'][X_GEN] = 1                  # inside the first sweep

    def new_best(S, tc):
        P = dx.parts(S, cfg)
        h = _above(tc)
        P['cost'][int(P['ex'][X_G0])] = P['sc'][SC_GBEST] = P['ex'][X_CPRE] = h
        P['cost'][int(P['ex'][X_POINTER])] = h + 1.
        P['ex'][X_GWORST] = max(P['ex'][X_GWORST], h + 1.)
    add('view_new_best_breaks_gbview', before_new_best, src=fresh, rewrite=new_best)

    def last_pointer(S, P, a):
        P['ex'][X_POINTER] = NP - 1
    add('pointer_last', last_pointer)

    # ---- exact ties
    def off_g0(S, P, a):
        if P['ex'][X_POINTER] == P['ex'][X_G0]:
            P['ex'][X_POINTER] = (int(P['ex'][X_G0]) + 1) % NP

    def tie(parent, gbest):
        def fn(S, tc):
            P = dx.parts(S, cfg)
            if parent:
                P['cost'][int(P['ex'][X_POINTER])] = tc
            if gbest:
                _own_gbest(S, cfg)
                P['sc'][SC_GBEST] = tc
        return fn
    add('tie_parent', off_g0, rewrite=tie(True, False))
    add('tie_gbest', off_g0, rewrite=tie(False, True))
    add('tie_parent_and_gbest', off_g0, rewrite=tie(True, True))

    def tie_gworst(S, tc):
        dx.parts(S, cfg)['ex'][X_GWORST] = tc
    add('tie_gworst', off_g0, rewrite=tie_gworst, actions=(0, 2))

    def below_gworst(S, tc):
        dx.parts(S, cfg)['ex'][X_GWORST] = np.nextafter(tc, -np.inf)
    add('above_gworst', off_g0, rewrite=below_gworst, actions=(1, 3))

    # ---- termination
    def last_fe(S, P, a):
        P['sc'][SC_FES] = MAXFES - 1
        P['sc'][SC_LOG_INDEX] = P['sc'][SC_COST_LEN] = NLOG
        P['clog'][:NLOG] = P['sc'][SC_GBEST] + np.arange(NLOG, 0, -1)
    add('last_evaluation', last_fe)

    def log_cross(S, P, a):
        P['sc'][SC_LOG_INDEX] = P['sc'][SC_COST_LEN] = 2
        P['clog'][1] = P['sc'][SC_GBEST] + 1.
        P['sc'][SC_FES] = 2 * INTERVAL - 1
    add('log_point', log_cross)

    def finished(S, P, a):
        P['sc'][SC_DONE] = 1.
    add('already_done', finished)

    # ---- clipping
    def clip(face):
        def fn(S, P, a):
            free = others(P)[:3]              # NP = 5 leaves three rows besides the pointer and G0
            hi, lo = (cfg.ub, cfg.lb) if face == 'hi' else (cfg.lb, cfg.ub)
            for j, v in zip(free, (hi, hi, lo)):
                P['X'][j] = v
            P['r'][:5] = [free[0], free[1], free[2], free[1], free[2]]
        return fn
    add('clip_hi', clip('hi'))
    add('clip_lo', clip('lo'))
    return out


# ================================================================================================ engines
class OracleEngine:
    """The C oracle behind the interface the GPU engine has: slots with fixed seeds, blocks in, per-step records out."""
    med = False

    def __init__(self, NP, D):
        self.ps = _probs(D)
        self.NP, self.D = NP, D
        self.cfgs = [_cfg(p, NP) for p in self.ps]
        self.ocfg = oracle.make_cfg(3, NP, D, MAXFES, INTERVAL, NLOG)
        self.main = list(range(N_MAIN))
        self.sphere = list(range(N_MAIN, N_MAIN + N_SPHERE)) if len(self.ps) > 1 else []

    def _new(self, slot):
        p = self.ps[0 if slot < N_MAIN else 1]
        return oracle.DqOracle(p.desc(), _optimum(p), self.ocfg, seed=seed_of(slot))

    def bases(self, slots):
        """-> {slot: (fresh block, its features, block after BASE_STEPS natural steps)}"""
        out = {}
        for s in slots:
            o = self._new(s)
            f0 = o.reset()
            fresh = o.state()
            for g in range(BASE_STEPS):
                o.step(g % 4)
            out[s] = (fresh, f0, o.state())
        return out

    def run(self, items, nsteps):
        """items: [(slot, block, action)] -> per item a list of (pre, action, post, reward, done, feat)"""
        out = []
        for slot, block, a in items:
            o = self._new(slot)
            o.set_state(block)
            pre, rec = block, []
            for k in range(nsteps):
                was_done = dx.parts(pre, _cfg(self.ps[0], self.NP))['sc'][SC_DONE] != 0
                f, r, d = o.step((a + k) % 4)
                post = o.state()
                rec.append((pre, (a + k) % 4, post, r, d, None if was_done else f))
                pre = post
            out.append(rec)
        return out

    def close(self):
        pass


class GpuEngine:
    """One Batch per geometry: N_MAIN instances on the main problem, N_SPHERE on the sphere; planted blocks go in with write_state."""
    med = True

    def __init__(self, NP, D):
        import torch
        from metabox_amd._abi import ALGO_DEDDQN
        from metabox_amd.suite import Batch, Suite
        self.torch = torch
        self.ps = _probs(D)
        self.NP, self.D = NP, D
        self.cfgs = [_cfg(p, NP) for p in self.ps]
        self.suite = Suite(list(self.ps))
        n_sph = N_SPHERE if len(self.ps) > 1 else 0
        self.B = N_MAIN + n_sph
        pidx = np.array([0] * N_MAIN + [1] * n_sph)
        seeds = np.array([seed_of(s) for s in range(self.B)], dtype=np.uint64)
        self.b = Batch(self.suite, ALGO_DEDDQN, pidx, seeds, NP, MAXFES, INTERVAL, NLOG)
        self.main = list(range(N_MAIN))
        self.sphere = list(range(N_MAIN, self.B))
        self._reset_done = False

    def _step(self, actions):
        t = self.torch
        self.b.state.fill_(SENTINEL)
        st, r, d = self.b.step(t.from_numpy(np.ascontiguousarray(actions, dtype=np.int32)).cuda())
        return st.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().astype(bool)

    def bases(self, slots):
        f0 = self.b.reset().cpu().numpy().copy()
        fresh = {s: self.b.read_state(s) for s in slots}
        for g in range(BASE_STEPS):
            self._step(np.full(self.B, g % 4))
        return {s: (fresh[s], f0[s], self.b.read_state(s)) for s in slots}

    def run(self, items, nsteps):
        acts = np.zeros(self.B, dtype=np.int64)
        for slot, block, a in items:
            self.b.write_state(slot, block)
            acts[slot] = a
        pre = {slot: block for slot, block, a in items}
        out = [[] for _ in items]
        for k in range(nsteps):
            st, r, d = self._step((acts + k) % 4)
            for i, (slot, block, a) in enumerate(items):
                post = self.b.read_state(slot)
                out[i].append((pre[slot], (a + k) % 4, post, float(r[slot]), bool(d[slot]), st[slot]))
                pre[slot] = post
        return out

    def close(self):
        self.b.close()
        self.suite.close()


def run_planted(eng, nsteps=3, stats=None, collect=None):
    """Plant every case into `eng`, run, judge every step.  -> (tags seen, {case name: tags}, number of steps judged).  collect: a list that
    receives (name, slot, cfg, first-step record) for callers that judge the records once more."""
    NP, D = eng.NP, eng.D
    rs = np.random.RandomState(100 * NP + D)
    slots = [eng.main[0], eng.main[1]] + eng.sphere[:1]
    bases = eng.bases(slots)
    for s in slots:                             # reset itself: the fresh block's features and draws
        cfg = eng.cfgs[0 if s < N_MAIN else 1]
        fresh, f0, _ = bases[s]
        P = dx.parts(fresh, cfg)
        check_features(f0, fresh, cfg, stats, ('reset', NP, D, s))
        assert np.array_equal(P['r'][:5], dx.dq_draws(seed_of(s), 0, int(P['sc'][SC_EPISODE]), NP)) and P['sc'][SC_GEN] == 0
        assert P['ex'][X_POINTER] == 0 and P['ex'][X_GEN] == 0 and P['ex'][X_GBVIEW] == 1 and P['ex'][X_PREVIEW] == 1
        assert P['sc'][SC_GBEST] == P['cost'].min() == P['cost'][int(P['ex'][X_G0])] and P['ex'][X_GWORST] == P['cost'].max()
        assert int(P['ex'][X_G0]) == int(np.argmin(P['cost'])) and P['sc'][SC_FES] == NP
    cases = plant(bases[slots[0]][0], bases[slots[0]][2], eng.cfgs[0], eng.ps[0], rs)
    cases += plant(bases[slots[1]][0], bases[slots[1]][2], eng.cfgs[0], eng.ps[0], rs)[::3]      # a second seed (above 2^32), a third of the cases
    n_main = len(cases)
    if eng.sphere:
        s = eng.sphere[0]
        cases += plant(bases[s][0], bases[s][2], eng.cfgs[1], eng.ps[1], rs, sphere=True)
    assert n_main <= len(eng.main) and len(cases) - n_main <= len(eng.sphere), (n_main, len(cases))
    placed = []
    for i, (name, a, S, rw) in enumerate(cases):
        slot = eng.main[i] if i < n_main else eng.sphere[i - n_main]
        placed.append([name, slot, a, S, rw, eng.cfgs[0 if i < n_main else 1]])
    for name, slot, a, S, rw, cfg in placed:
        dx.validate(S, cfg, a)
    learn = [c for c in placed if c[4] is not None]                 # learn the trial cost, rewrite, validate again
    for c, rec in zip(learn, eng.run([(c[1], c[3], c[2]) for c in learn], 1)):
        post = dx.parts(rec[0][2], c[5])
        tc = post['omw'][int(post['ex'][X_OMWLEN]) - 1, 5]
        c[4](c[3], tc)
        dx.validate(c[3], c[5], c[2])
    seen, by_case, n = set(), {}, 0
    for c, recs in zip(placed, eng.run([(c[1], c[3], c[2]) for c in placed], nsteps)):
        name, slot, a, S, rw, cfg = c
        for k, (pre, act, post, r, d, feat) in enumerate(recs):
            tags = check_step(pre, act, post, r, d, feat, cfg, seed=seed_of(slot), med=eng.med, raw=eng.med, stats=stats, label=(name, NP, D, slot, act, k))
            seen |= tags
            n += 1
            if k == 0:
                by_case.setdefault(name, set()).update(tags)
                if collect is not None:
                    collect.append((name, slot, cfg, (pre, act, post, r, d, feat)))
    return seen, by_case, n


# ================================================================================================ CPU
CPU_GEOMS = GEOMS + [(256, 10), (100, 12)]


@functools.lru_cache(maxsize=None)
def _oracle_planted(NP, D):
    st, rec = Stats(), []
    seen, by_case, n = run_planted(OracleEngine(NP, D), stats=st, collect=rec)
    return seen, by_case, n, st, rec


@pytest.mark.parametrize('which', ['bbob', 'bbob-noisy', 'protein'])
def test_restatement_follows_the_oracle_along_trajectories(which):
    """300 natural steps (three population sweeps at NP = 100: rings, window eviction, prebest re-binding), every step restated from the
    oracle's own block and compared with its next block, reward, done and 99 features."""
    if which == 'protein':
        p, NP = _probs(12)[0], 100
    elif which == 'bbob':
        p, NP = problems('bbob', 10)[15], 100
    else:
        ps = problems('bbob-noisy', 10)
        p, NP = ps[sorted(ps)[6]], 100
    cfg = dx.Cfg(NP, p.dim, NLOG, 360, 72, 1, float(p.lb), float(p.ub), _optimum(p) is not None)
    seed = (1 << 40) + 12345
    o = oracle.DqOracle(p.desc(), _optimum(p), oracle.make_cfg(3, NP, p.dim, 360, 72, NLOG), seed=seed)
    st, seen = Stats(), set()
    f0 = o.reset()
    pre = o.state()
    check_features(f0, pre, cfg, st, (which, 'reset'))
    acts = np.random.RandomState(3).randint(0, 4, 300)
    for g in range(300):
        f, r, d = o.step(int(acts[g]))
        post = o.state()
        was_done = dx.parts(pre, cfg)['sc'][SC_DONE] != 0
        seen |= check_step(pre, int(acts[g]), post, r, d, None if was_done else f, cfg, seed=seed, med=False, stats=st, label=(which, g))
        pre = post
    assert dx.parts(pre, cfg)['sc'][SC_DONE] == 1 and {'done_budget', 'already_done', 'ring_open_fresh', 'win_evict_same'} <= seen
    st.report(f'oracle trajectory {which}')


@pytest.mark.parametrize('NP,D', CPU_GEOMS)
def test_oracle_stays_inside_every_bound_on_the_planted_states(NP, D):
    seen, by_case, n, st, _ = _oracle_planted(NP, D)
    st.report(f'oracle planted NP={NP} D={D} ({n} steps, {len(by_case)} cases)')


def test_planted_states_take_every_branch():
    """The branch ledger: over the planted cases of all geometries every tag the restatement can emit is taken (first steps alone)."""
    seen = set()
    for NP, D in CPU_GEOMS:
        for tags in _oracle_planted(NP, D)[1].values():
            seen |= tags
    assert seen == dx.ALL_TAGS, (sorted(dx.ALL_TAGS - seen), sorted(seen - dx.ALL_TAGS))
    for NP, D in ((100, 10), (33, 7)):          # one even and one odd geometry take every branch on their own, but for the other parity's median tag
        own = set().union(*_oracle_planted(NP, D)[1].values())
        assert dx.ALL_TAGS - own == {'med_odd' if NP % 2 == 0 else 'med_even'}, (NP, D, sorted(dx.ALL_TAGS - own))


def _defective_record(defect, rec, cfg, seed):
    """What a kernel with `defect` would have left behind for the first-step record `rec` of a planted case."""
    pre, act, post, r, d, feat = rec
    P0, P1 = dx.parts(pre, cfg), dx.parts(post, cfg)
    if P0['sc'][SC_DONE] != 0:
        return rec
    tc = P1['omw'][int(P1['ex'][X_OMWLEN]) - 1, 5]
    steps = int(P0['sc'][SC_GEN]) + 1
    r_next = dx.dq_draws(seed, steps, int(P0['sc'][SC_EPISODE]), cfg.NP, defect=defect)
    bad, rw, dn, _ = dx.dq_step(pre, act, tc, r_next, cfg, defect=defect)
    stale = dx.resolve(pre, cfg)[0 if P0['ex'][X_POINTER] == 0 else 1]
    src = bad
    if defect == 10:                            # features of a block whose pointer still indexes the population
        src = bad.copy()
        dx.parts(src, cfg)['ex'][X_POINTER] %= cfg.NP
    f, _ = dx.dq_features(src, cfg, defect=defect, stale_prebest=stale)
    return pre, act, bad, rw, dn, f.astype(np.float64)


DEFECT_GEOMS = ((100, 10), (33, 7))


def test_check_step_accepts_the_restatement_itself():
    """The records the defect test mutates, built with defect = 0, pass check_step as a kernel's read-back would (median cache included)."""
    for NP, D in DEFECT_GEOMS:
        for name, slot, cfg, rec in _oracle_planted(NP, D)[4]:
            check_step(*_defective_record(0, rec, cfg, seed_of(slot)), cfg, seed=seed_of(slot), med=True, raw=True, label=(name, 'no defect'))


@pytest.mark.parametrize('defect', sorted(dx.DEFECTS))
def test_check_step_rejects_a_planted_defect(defect):
    """Each defect, planted into the restatement, is rejected by check_step -- the comparison the GPU tests use -- on planted cases of
    NP = 100, D = 10 and of NP = 33, D = 7 (the search stops at the third rejecting record of a geometry)."""
    rejected = {}
    for NP, D in DEFECT_GEOMS:
        if defect == 1 and NP & 1:
            continue
        hits = rejected.setdefault(NP, [])
        for name, slot, cfg, rec in _oracle_planted(NP, D)[4]:
            try:
                check_step(*_defective_record(defect, rec, cfg, seed_of(slot)), cfg, seed=seed_of(slot), med=True, raw=True, label=name)
            except AssertionError:
                hits.append(name)
                if len(hits) == 3:
                    break
    print(f'defect {defect} ({dx.DEFECTS[defect]}): first rejected by {rejected}')
    assert all(rejected.values()), (dx.DEFECTS[defect], rejected)


# ================================================================================================ GPU
def _largest_even_np(D=10):
    from metabox_amd._abi import ALGO_DEDDQN
    from metabox_amd.suite import Batch, Suite
    s = Suite([_probs(D)[0]])
    try:
        for NP in range(256, 129, -2):
            try:
                Batch(s, ALGO_DEDDQN, [0], [1], NP, MAXFES, INTERVAL, NLOG).close()
                return NP
            except Exception:
                continue
    finally:
        s.close()
    raise AssertionError('no even NP in (129, 256] is accepted at D = 10')


def _gpu_planted(NP, D, want_fixed=None):
    from test_bbob_exact import Checker
    import bbob_exact as be
    eng = GpuEngine(NP, D)
    try:
        if want_fixed is not None:
            assert (eng.b.launch_info()['fixed_geometry'] != 0) == want_fixed
        st, rec = Stats(), []
        seen, by_case, n = run_planted(eng, stats=st, collect=rec)
        st.report(f'MI355X planted NP={NP} D={D} ({n} steps, {len(by_case)} cases)')
        missing = dx.ALL_TAGS - seen - {'med_odd' if NP % 2 == 0 else 'med_even'} - (set() if eng.sphere else {'done_target', 'final_append'})
        assert not missing, sorted(missing)
        if D != 12:                             # the trial cost against mbx_eval of the host trial row, both held to the extended-precision allowance
            chk = Checker(f'k_dq_step trial cost NP={NP} D={D}')
            for k, p in enumerate(eng.ps):
                rows = [(dx.dq_trial(pre, act, cfg), dx.parts(post, cfg)) for name, slot, cfg, (pre, act, post, r, d, f) in rec
                        if (slot >= N_MAIN) == (k == 1) and dx.parts(pre, cfg)['sc'][SC_DONE] == 0]
                X = np.stack([t for t, _ in rows])
                tc = np.array([P['omw'][int(P['ex'][X_OMWLEN]) - 1, 5] for _, P in rows])
                chk(p, X, tc)
                allow, _, _ = be.allowance(p, X)
                ev = eng.suite.eval(k, X, noisy=False) - p.bias
                assert np.all(np.abs(ev - tc) <= 2 * allow), (NP, D, k, float(np.max(np.abs(ev - tc) / allow)))
            chk.report()
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('NP,D', GEOMS)
def test_hip_step_kernel_is_the_restatement_on_planted_states(NP, D):
    _gpu_planted(NP, D, want_fixed=False)


@pytest.mark.gpu
def test_hip_step_kernel_is_the_restatement_at_the_largest_even_np():
    NP = _largest_even_np()
    print(f'largest even NP accepted at D = 10: {NP}')
    _gpu_planted(NP, 10, want_fixed=False)


@pytest.mark.gpu
@pytest.mark.parametrize('generic', ['0', '1'])
def test_hip_step_kernel_is_the_restatement_on_protein_docking(generic, monkeypatch):
    monkeypatch.setenv('MBX_GENERIC_GEOMETRY', generic)
    _gpu_planted(100, 12, want_fixed=generic == '0')


@pytest.mark.gpu
def test_hip_draws_follow_the_philox_route_and_the_tape():
    """Indices R on a noisy problem (whose noise draws use other sites), seeds below and above 2^32, two resets; then the tape route."""
    import torch
    from metabox_amd._abi import ALGO_DEDDQN
    from metabox_amd.suite import Batch, Suite
    ps = problems('bbob-noisy', 7)
    p = ps[sorted(ps)[4]]
    assert p.noise[0] != 0
    NP, D = 33, 7
    cfg = _cfg(p, NP)
    seeds = np.array([5, (1 << 32) + 5, (1 << 63) + 11, 0xFFFFFFFF], dtype=np.uint64)
    s = Suite([p])
    b = Batch(s, ALGO_DEDDQN, np.zeros(len(seeds), dtype=np.int64), seeds, NP, MAXFES, INTERVAL, NLOG)
    episodes = []
    for rep in range(2):
        b.reset()
        for g in range(4):
            for k, seed in enumerate(seeds):
                P = dx.parts(b.read_state(k), cfg)
                assert P['sc'][SC_GEN] == g
                assert np.array_equal(P['r'][:5], dx.dq_draws(int(seed), g, int(P['sc'][SC_EPISODE]), NP)), (rep, g, k)
            if g == 0:
                episodes.append(int(P['sc'][SC_EPISODE]))
            b.step(torch.full((len(seeds),), g % 4, dtype=torch.int32, device='cuda'))
    assert episodes[1] == episodes[0] + 1
    # tape: r comes from the tape words (and the noise from its words), step restated as everywhere else
    fd = [oracle.DqTapeFeeder(int(k) + 3, NP, D, p.noise[0]) for k in range(len(seeds))]
    tape = torch.from_numpy(np.stack([f.reset_tape() for f in fd])).cuda()
    b.set_tape(tape)
    f0 = b.reset().cpu().numpy().copy()
    for k in range(len(seeds)):
        blk = b.read_state(k)
        assert np.array_equal(dx.parts(blk, cfg)['r'][:5], tape[k, :5].cpu().numpy())
        check_features(f0[k], blk, cfg, None, ('tape reset', k))
    for g in range(3):
        pre = [b.read_state(k) for k in range(len(seeds))]
        tape = torch.from_numpy(np.stack([f.step_tape() for f in fd])).cuda()
        b.set_tape(tape)
        st, r, d = b.step(torch.full((len(seeds),), (g + 1) % 4, dtype=torch.int32, device='cuda'))
        st, r, d = st.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
        for k in range(len(seeds)):
            post = b.read_state(k)
            check_step(pre[k], (g + 1) % 4, post, float(r[k]), bool(d[k]), st[k], cfg, seed=None, med=True, raw=True, label=('tape', g, k))
            assert np.array_equal(dx.parts(post, cfg)['r'][:5], tape[k, :5].cpu().numpy()), (g, k)
    b.set_tape(None)
    b.close()
    s.close()
