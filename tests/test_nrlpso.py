"""NRLPSO (src/optimizer/nrlpso_optimizer.py, src/agent/nrlpso_agent.py): a numpy restatement of init_population / update lives here and is
pinned to the reference's recorded episodes (tests/golden/nrlpso_traces*.npz, tools/gen_golden.py nrlpso) bit for bit; its cached variant --
distance matrix with row / column refresh, ef_old reused -- is the design of the cached step kernel and equals the from-scratch form on every
step; the HIP kernels (metabox_amd/csrc/mbx_nrlpso.hpp) are then held against the reference by tape replay and against the restatement, fed the
kernel's own costs, on the Philox route: everything but costs to the bit.

The fixture's budgets (1500 FEs) do not reach the early stop at gbest <= 1e-8; the generator asserts that no episode ends before maxFEs."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import close, load, print_ledger, problems, prove_tie_arrays
from oracle import oracle

FILES = [load('nrlpso_traces.npz')] + [load(f'nrlpso_traces_{n}.npz') for n in (1, 2, 3)]
POL = load('nrlpso_policy.npz')
Q = POL['q_table']
CASES = [str(c) for c in FILES[0]['cases']]
ALGO_NRLPSO, NP0, K, NSC = 19, 100, 5, 16
F_RECOMPUTE = 8
SC_POINTER, SC_G0, SC_ALIAS, SC_RW, SC_W = 10, 11, 12, 13, 14
SITE_LDE_ELEM, SITE_POLICY, SITE_NR_PART, SITE_NR_ELEM, SITE_NR_MUT, SITE_NR_INIT = 12, 15, 48, 49, 50, 53


def TR(key):
    for f in FILES:
        if key in f.files:
            return f[key]
    raise KeyError(key)


def has(key):
    return any(key in f.files for f in FILES)


# ------------------------------------------------------------------------------------------------ layout (include/mbx_layout.h section 16)
def state_off(NP, D, nlog):
    o, out = 0, {}
    for name, n in (('pop', NP * D), ('vel', NP * D), ('pbpos', NP * D), ('snap', NP * D), ('cost', NP), ('pbcost', NP), ('stag', NP), ('sstate', NP),
                    ('pnidx', K * NP), ('gnidx', 8), ('gbpos', D), ('diag', 8), ('scalars', NSC), ('curve', nlog + 1)):
        out[name] = (o, n)
        o += n
    out['end'] = o
    return out


def split(block, NP, D, nlog):
    return {k: block[v[0]:v[0] + v[1]] for k, v in state_off(NP, D, nlog).items() if k != 'end'}


def tape_stride(NP, D):
    return NP * D + 4 * NP + 16


T_RAND, T_IDX, T_NOISE, T_CHOICE, T_VEC = 0, 2, 4, 13, 14


# ------------------------------------------------------------------------------------------------ numpy's legacy stream in the reference's draw order
class NrFeeder:
    """init_population: rand(NP, D), the evaluation's noise, rand() (r_w), randint(0, 4, NP).  Per step: (agent) the uniform of np.random.choice when
    policy-driven; rand(), rand(); randint(0, k) of get_p_b / get_p_a as the action and the sign of cs call them; action 3: two rand(D); the
    evaluation's noise; a mutating step: rand(D), noise, rand(D), noise."""

    def __init__(self, seed, NP, D, noise_kind, policy):
        self.rs = np.random.RandomState(seed)
        self.NP, self.D, self.noise, self.policy = NP, D, noise_kind, policy

    def _noise(self, n):
        rows, rs = np.zeros((3, n)), self.rs
        if self.noise == 1:
            rows[0] = rs.randn(n) if n > 1 else rs.randn()
        elif self.noise == 2:
            rows[0] = rs.rand(n) if n > 1 else rs.rand()
            rows[1] = rs.rand(n) if n > 1 else rs.rand()
        elif self.noise == 3:
            rows[0] = rs.rand(n) if n > 1 else rs.rand()
            rows[1] = rs.randn(n) if n > 1 else rs.randn()
            rows[2] = rs.randn(n) if n > 1 else rs.randn()
        return rows

    def reset_tape(self):
        NP, D = self.NP, self.D
        t = np.zeros(tape_stride(NP, D))
        t[:NP * D] = self.rs.rand(NP, D).ravel()
        t[NP * D:NP * D + 3 * NP] = self._noise(NP).ravel()
        t[NP * D + 4 * NP] = self.rs.rand()
        t[NP * D + 3 * NP:NP * D + 4 * NP] = self.rs.randint(low=0, high=4, size=NP)
        return t

    def choice_uniform(self):
        return float(self.rs.random_sample(1)[0]) if self.policy else 0.

    def step_tape(self, action, csneg, mutated, choice_u=0.):
        D, rs = self.D, self.rs
        t = np.zeros(tape_stride(self.NP, D))
        t[T_RAND], t[T_RAND + 1] = rs.rand(), rs.rand()
        if action == 3:
            t[T_IDX], t[T_IDX + 1] = rs.randint(0, K), rs.randint(0, K)
            t[T_VEC:T_VEC + D] = rs.rand(D)
            t[T_VEC + D:T_VEC + 2 * D] = rs.rand(D)
        elif (action == 0 and not csneg) or (action == 1 and csneg):
            t[T_IDX] = rs.randint(0, K)
        elif action in (0, 1):
            t[T_IDX + 1] = rs.randint(0, K)
        noise = np.zeros((3, 3))
        noise[:, 0] = self._noise(1)[:, 0]
        if mutated:
            t[T_VEC + 2 * D:T_VEC + 3 * D] = rs.rand(D)
            noise[:, 1] = self._noise(1)[:, 0]
            t[T_VEC + 3 * D:T_VEC + 4 * D] = rs.rand(D)
            noise[:, 2] = self._noise(1)[:, 0]
        t[T_NOISE:T_NOISE + 9] = noise.ravel()
        t[T_CHOICE] = choice_u
        return t


def choose(q_row, u):
    """np.random.choice(4, p = softmax(q_row)) for the uniform u (numpy: searchsorted(cumsum(p) / cumsum(p)[-1], u, 'right'))."""
    e = np.exp(q_row)
    cdf = np.cumsum(e / e.sum())
    return int(np.searchsorted(cdf / cdf[-1], u, side='right'))


# ------------------------------------------------------------------------------------------------ the restatement
class Nr:
    """nrlpso_optimizer.py:30-296 in numpy, costs supplied by the caller.  cached = True: update_distance keeps the NP x NP matrix, rewrites one row
    and one column per changed particle and re-sums the row means; the ef_old of a step is what the last update_distance left unless a mutation
    replaced a row since (the cached step kernel's design)."""

    def __init__(self, NP, D, lb, ub, max_fes, log_interval, nlog, early_stop=True, cached=False):
        self.NP, self.D, self.lb, self.ub, self.max_fes, self.log_interval, self.nlog = NP, D, lb, ub, max_fes, log_interval, nlog
        self.early_stop, self.cached = early_stop, cached

    def reset(self, tape, cost):
        NP, D = self.NP, self.D
        self.pop = tape[:NP * D].reshape(NP, D) * (self.ub - self.lb) + self.lb
        self.vmax = -(-0.1 * (self.ub - self.lb))
        self.vel = np.zeros((NP, D))
        self.cost = np.array(cost, dtype=np.float64)
        self.pbpos, self.pbcost = self.pop.copy(), self.cost.copy()
        self.g0 = int(np.argmin(self.cost))
        self.gbest, self.alias, self.gb = self.cost[self.g0], True, self.pop[self.g0].copy()
        self.stag = np.zeros(NP)
        self.fes, self.log_index, self.curve, self.done = NP, 1, [self.gbest], False
        self.r_w, self.w = tape[NP * D + 4 * NP], 0.
        self.sstate = tape[NP * D + 3 * NP:NP * D + 4 * NP].astype(np.int64)
        self.pointer = 0
        self.snap, self.pnidx, self.gnidx = self.pop.copy(), np.zeros((NP, K), dtype=np.int64), np.zeros(K, dtype=np.int64)
        self.dm, self.fresh = None, False
        self.diag = {}
        return int(self.sstate[0])

    def gpos(self):
        return self.pop[self.g0] if self.alias else self.gb

    def refresh(self, r):
        if self.cached and self.dm is not None:
            row = np.sqrt(np.sum((self.pop - self.pop[r]) ** 2, -1))
            self.dm[r, :] = row
            self.dm[:, r] = row
        self.fresh = False

    def update_distance(self):
        if not self.cached:
            d = np.sqrt(np.sum((self.pop[None, :] - self.pop[:, None]) ** 2, -1))
        else:
            if self.dm is None:
                self.dm = np.sqrt(np.sum((self.pop[None, :] - self.pop[:, None]) ** 2, -1))
            d = self.dm
        self.dist = np.sum(d, -1) / (self.NP - 1)
        self.dmin, self.dmax = np.min(self.dist), np.max(self.dist)
        self.fresh = True

    def cal_ef(self, i, reuse=False):
        if not (self.cached and reuse and self.fresh):
            self.update_distance()
        with np.errstate(invalid='ignore', divide='ignore'):
            return (self.dist[i] - self.dmin) / (self.dmax - self.dmin)

    def construct(self):
        NP = self.NP
        m = np.sqrt(np.sum((self.pbpos[None, :] - self.pop[:, None]) ** 2, axis=-1))
        m[np.arange(NP), np.arange(NP)] = np.inf
        self.pnidx = np.argsort(m, -1, kind='stable')[:, :K]
        g = np.sqrt(np.sum((self.gpos()[None, :] - self.pop) ** 2, axis=-1))
        self.gnidx = np.argsort(g, -1, kind='stable')[:K]
        self.snap = self.pop.copy()

    def step(self, action, t, ev):
        """t: the step's tape; ev(k, x): the cost of evaluation k (0 the move, 1 / 2 the mutations) of position x."""
        NP, D, p = self.NP, self.D, self.pointer
        if p == 0:
            self.construct()
            self.r_w = 4 * self.r_w * (1 - self.r_w)
            q = self.fes / self.max_fes
            self.w = 0.6 - (q * self.r_w * 0.4 + 0.33 * (1 - 0.4) * q)
        r1, r2, ib, ia = t[T_RAND], t[T_RAND + 1], int(t[T_IDX]), int(t[T_IDX + 1])
        pb, g, x, v, w = self.pbpos[p], self.gpos(), self.pop[p], self.vel[p], self.w
        with np.errstate(invalid='ignore', divide='ignore'):
            cs = np.sum(pb * g) / (np.sqrt(np.sum(pb ** 2)) * np.sqrt(np.sum(g ** 2)))
        pbn, gbn = self.snap[self.pnidx[p][ib]], self.snap[self.gnidx[ia]]
        if action == 0:
            nv = w * v + 2.2 * r1 * (pb - x) + 1.8 * r2 * (gbn - x) if cs < 0 else w * v + 2.2 * r1 * (pbn - x)
        elif action == 1:
            nv = w * v + 2.1 * r1 * (pbn - x) + 1.8 * r2 * (g - x) if cs < 0 else w * v + 1.8 * r2 * (gbn - x)
        elif action == 2:
            nv = w * v + 2 * r1 * (pb - x) + 2 * r2 * (g - x) if cs < 0 else w * v + 2 * r2 * (g - x)
        elif action == 3:
            nv = w * v + 1.8 * t[T_VEC:T_VEC + D] * (pbn - x) + 2.2 * t[T_VEC + D:T_VEC + 2 * D] * (gbn - x)
        else:
            nv = v
        self.vel[p] = np.clip(nv, -self.vmax, self.vmax)
        ef_old = self.cal_ef(p, reuse=True)
        self.pop[p] = np.clip(self.pop[p] + self.vel[p], self.lb, self.ub)
        self.refresh(p)
        ef_new = self.cal_ef(p)
        f_old, f_new = self.cost[p], ev(0, self.pop[p])
        c1, c2 = f_new < f_old, ef_new > ef_old
        reward = (2 if c2 else 1) if c1 else (0 if c2 else -2)
        self.cost[p] = f_new
        if f_new < self.pbcost[p]:
            self.pbpos[p] = self.pop[p]
            self.stag[p] = 0
        else:
            self.stag[p] += 1
        mutated, pm, gm = bool(self.stag[p] >= 2), 0., 0.
        if mutated:
            nb = self.snap[self.pnidx[p]]
            order = np.argsort(np.sqrt(np.sum((self.pbpos[p][None, :] - nb) ** 2, axis=-1)), kind='stable')
            P3 = self.pbpos[p] + t[T_VEC + 2 * D:T_VEC + 3 * D] * (nb[order[0]] - nb[order[-1]])
            pm = ev(1, P3)
            if pm < self.pbcost[p]:
                self.pbpos[p], self.pbcost[p] = P3, pm
            else:
                q = self.pnidx[p][order[-1]]
                self.pop[q], self.cost[q] = P3, pm
                self.refresh(q)
            nb = self.snap[self.gnidx]
            order = np.argsort(np.sqrt(np.sum((self.gpos()[None, :] - nb) ** 2, axis=-1)), kind='stable')
            P3 = self.gpos() + t[T_VEC + 3 * D:T_VEC + 4 * D] * (nb[order[0]] - nb[order[-1]])
            gm = ev(2, P3)
            if gm < self.gbest:
                self.gb, self.gbest, self.alias = P3, gm, False
            else:
                q = self.gnidx[order[-1]]
                self.pop[q], self.cost[q] = P3, gm
                self.refresh(q)
            self.fes += 2
        self.fes += 1
        if f_new < self.gbest:
            self.gbest, self.alias, self.g0 = f_new, True, p
        self.sstate[p] = action
        self.pointer = (p + 1) % NP
        if self.fes >= self.log_index * self.log_interval:
            self.log_index += 1
            self.curve.append(self.gbest)
        self.done = bool(self.fes >= self.max_fes or (self.early_stop and self.gbest <= 1e-8))
        if self.done:
            if len(self.curve) >= self.nlog + 1:
                self.curve[-1] = self.gbest
            else:
                self.curve.append(self.gbest)
        self.diag = dict(cs=cs, ef_old=ef_old, ef_new=ef_new, mutated=mutated, fnew=f_new, pm=pm, gm=gm)
        return int(self.sstate[self.pointer]), reward, self.done

    def exact(self):
        """Everything that is reproducible to the bit, as one dict of arrays."""
        return dict(pop=self.pop.copy(), vel=self.vel.copy(), pbpos=self.pbpos.copy(), stag=self.stag.copy(), pnidx=np.asarray(self.pnidx, dtype=np.float64).ravel(),
                    gnidx=np.asarray(self.gnidx, dtype=np.float64), gbpos=self.gpos().copy(), alias=float(self.alias), g0=float(self.g0) if self.alias else -1.,
                    w=self.w, r_w=self.r_w, fes=float(self.fes), pointer=float(self.pointer), sstate=self.sstate.astype(np.float64), snap=self.snap.copy())


def _setup(case):
    suite, dim, fid, seed, mode = case.split('/')
    p = problems(suite, int(dim))[int(fid)]
    keys = [(case, int(seed))] + ([(case + '/second', int(seed) + 1)] if has(f'{case}/second/actions') else [])
    return p, int(dim), p.noise[0], mode == 'policy', int(TR(f'{case}/max_fes')), keys


def _new(p, D, max_fes, cached=False, NP=NP0, nlog=50):
    return Nr(NP, D, p.lb, p.ub, max_fes, max_fes // nlog, nlog, cached=cached)


def _snap_check(key, g, got, where):
    """`got`: dict as Nr.exact() gives it; against the reference's snapshot after step g."""
    s = lambda k: TR(f'{key}/snap{g}/{k}')          # noqa: E731
    al = int(s('alias'))
    pairs = (('pop', s('pop')), ('vel', s('vel')), ('pbpos', s('pbpos')), ('stag', s('stag')), ('pnidx', s('pnidx').astype(np.float64).ravel()),
             ('gnidx', s('gnidx').astype(np.float64)), ('gbpos', s('gbpos')), ('alias', float(al >= 0)), ('g0', float(al)), ('w', float(s('w'))), ('r_w', float(s('r_w'))))
    for name, want in pairs:
        assert np.array_equal(np.asarray(got[name]).reshape(np.shape(want)), want), (where, key, g, name)


@functools.lru_cache(maxsize=None)
def chain(case, cached=False):
    """The restatement over the fixture episode(s) of `case`, fed the feeder's tapes and the REFERENCE's recorded costs."""
    p, D, nk, policy, max_fes, keys = _setup(case)
    out = {}
    for key, seed in keys:
        fd = NrFeeder(seed, NP0, D, nk, policy)
        nr = _new(p, D, max_fes, cached)
        t0 = fd.reset_tape()
        s = nr.reset(t0, TR(f'{key}/cost0'))
        assert np.array_equal(nr.sstate, TR(f'{key}/sstate0')) and s == TR(f'{key}/states')[0], key
        acts, csneg, mut = TR(f'{key}/actions'), TR(f'{key}/csneg'), TR(f'{key}/mutated')
        ref = {k: TR(f'{key}/{k}') for k in ('fnew', 'pmcost', 'gmcost', 'reward', 'states', 'done', 'gbest', 'fes', 'ef_old', 'ef_new')}
        snaps, rows = set(int(v) for v in TR(f'{key}/snap_steps')), []
        for g, a in enumerate(acts):
            u = fd.choice_uniform()
            if policy:
                assert choose(Q[s], u) == a, (key, g)
            t = fd.step_tape(int(a), bool(csneg[g]), bool(mut[g]), u)
            s, r, d = nr.step(int(a), t, lambda k, x: (ref['fnew'][g], ref['pmcost'][g], ref['gmcost'][g])[k])
            dg = nr.diag
            assert (dg['cs'] < 0) == csneg[g] and dg['mutated'] == mut[g], (key, g, 'the tape was drawn for another branch')
            assert dg['ef_old'] == ref['ef_old'][g] and dg['ef_new'] == ref['ef_new'][g], (key, g, 'ef')
            assert (s, r, d) == (ref['states'][g + 1], ref['reward'][g], ref['done'][g]) and nr.gbest == ref['gbest'][g] and nr.fes == ref['fes'][g], (key, g)
            if g + 1 in snaps:
                _snap_check(key, g + 1, nr.exact(), 'restatement')
                assert np.array_equal(nr.cost, TR(f'{key}/snap{g + 1}/cost')) and np.array_equal(nr.pbcost, TR(f'{key}/snap{g + 1}/pbcost')), (key, g)
            rows.append((t, dict(dg), dict(dist=nr.dist.copy(), dmin=nr.dmin, dmax=nr.dmax)))
        assert np.array_equal(nr.curve, TR(f'{key}/cost')) and fd.rs.rand() == TR(f'{key}/next_rand'), (key, 'curve / stream position')
        out[key] = (t0, rows, nr)
    return out


# ------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize('case', CASES)
def test_feeder_ends_at_the_recorded_stream_position(case):
    p, D, nk, policy, max_fes, keys = _setup(case)
    for key, seed in keys:
        fd = NrFeeder(seed, NP0, D, nk, policy)
        fd.reset_tape()
        for a, c, m in zip(TR(f'{key}/actions'), TR(f'{key}/csneg'), TR(f'{key}/mutated')):
            fd.step_tape(int(a), bool(c), bool(m), fd.choice_uniform())
        assert fd.rs.rand() == TR(f'{key}/next_rand'), key


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(case):
    """Every recorded per-step quantity and every snapshot, bit for bit (the assertions live in chain())."""
    for key, (t0, rows, nr) in chain(case).items():
        assert len(rows) == len(TR(f'{key}/actions')) and nr.done


def test_cached_restatement_equals_the_from_scratch_one():
    """Distance matrix with row / column refresh and ef_old reused == update_distance from scratch, on every step of the F129 episode (285 mutating
    steps) and of a quiet one: ef_old, ef_new, the row means, d_min and d_max to the bit."""
    for case in [c for c in CASES if '/129/' in c or '/10/3/' in c]:
        a, b = chain(case), chain(case, True)
        for key in a:
            for g, ((_, da, xa), (_, db, xb)) in enumerate(zip(a[key][1], b[key][1])):
                assert da['ef_old'] == db['ef_old'] and da['ef_new'] == db['ef_new'], (key, g)
                assert np.array_equal(xa['dist'], xb['dist']) and xa['dmin'] == xb['dmin'] and xa['dmax'] == xb['dmax'], (key, g)
            ea, eb = a[key][2].exact(), b[key][2].exact()
            assert all(np.array_equal(ea[k], eb[k]) for k in ea), key


def test_fixture_covers_the_quirks():
    cat = lambda k: np.concatenate([TR(f'{c}/{k}') for c in CASES])          # noqa: E731
    pm, gm, act, neg = cat('pm_take'), cat('gm_take'), cat('actions'), cat('csneg')
    assert (pm == 1).any() and (pm == 0).any() and (gm == 1).any() and (gm == 0).any()        # both outcomes of both mutations
    assert cat('moved_alias').any() and (cat('alias') == -1).any() and (cat('alias') >= 0).any()   # the view follows its row; gbest an array of its own
    assert cat('stale').any()                                                                      # a mutation used sweep-start copies that had gone stale
    assert (cat('ef_old') == cat('ef_new')).any()
    for a in range(4):
        assert neg[act == a].any() and (~neg[act == a]).any(), a
    assert any(TR(f'{c}/fes')[-1] > TR(f'{c}/max_fes') for c in CASES)                        # fes passes maxFEs
    assert any((np.diff(TR(f'{c}/fes')) == 3).any() and len(TR(f'{c}/cost')) == 51 for c in CASES)   # one append per step although fes jumps by 3
    again = False
    for c in CASES:                                                                                # the count is not reset by a mutation
        m = np.nonzero(TR(f'{c}/mutated'))[0]
        again = again or bool(np.isin(m + NP0, m).any())
    assert again
    assert any('/30/' in c and TR(f'{c}/mutated').any() for c in CASES) and any(has(f'{c}/second/actions') for c in CASES)
    assert not any(TR(f'{c}/fes')[-1] < TR(f'{c}/max_fes') for c in CASES)                    # the early stop is not reached at these budgets


def _agent(max_learning_step=6000, device='cpu'):
    from metabox_amd.agent import NRLPSO_Agent
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', device, '--max_learning_step', str(max_learning_step)])
    cfg.agent_save_dir = None
    cfg.save_interval = 10 ** 9
    return NRLPSO_Agent(cfg), cfg


def test_td_update_replays_the_recorded_training_episode():
    agent, cfg = _agent(int(POL['train/max_ls']))
    agent.load_exported_weights({'q_table': POL['train/q_before']}, learn_steps=int(POL['train/ls0']))
    for s, a, r, s2 in zip(POL['train/state'], POL['train/action'], POL['train/reward'], POL['train/next_state']):
        agent.td_update(int(s), np.array([int(a)]), int(r), int(s2))
    assert np.array_equal(agent.q_table, POL['train/q_after']) and agent.learn_steps == int(POL['train/ls0']) + len(POL['train/state'])
    assert cfg.gamma == 0.8 and (cfg.n_states, cfg.n_actions) == (4, 4)
    assert np.array_equal(_agent()[0].load_exported_weights(POL).q_table, Q)


def test_abi_geometry_of_nrlpso():
    from metabox_amd import _abi
    lib = _abi.load_lib()
    assert _abi.ALGO_NRLPSO == ALGO_NRLPSO and _abi.F_NRLPSO_RECOMPUTE == F_RECOMPUTE
    for np_, D in ((100, 10), (100, 30), (8, 2), (9, 7), (128, 40)):
        cfg = oracle.make_cfg(ALGO_NRLPSO, np_, D, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(cfg)) == 1 and lib.mbx_action_dim(C.byref(cfg)) == 1
        assert lib.mbx_tape_stride(C.byref(cfg)) == tape_stride(np_, D) >= T_VEC + 4 * D
    for np_, D in ((7, 10), (129, 10), (100, 41)):
        bad = oracle.make_cfg(ALGO_NRLPSO, np_, D, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(bad)) < 0 and lib.mbx_action_dim(C.byref(bad)) < 0 and lib.mbx_tape_stride(C.byref(bad)) < 0, (np_, D)
    for algo in (12, 14, 17):
        bad = oracle.make_cfg(algo, 100, 10, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(bad)) < 0 and lib.mbx_tape_stride(C.byref(bad)) < 0
    assert state_off(100, 10, 50)['end'] == 4 * 1000 + 4 * 100 + 500 + 8 + 10 + 8 + 16 + 51
    assert 'mbx_nrlpso_rollout' in _abi.EXPORTED_SYMBOLS and len(_abi.EXPORTED_SYMBOLS) == 45 and hasattr(lib, 'mbx_nrlpso_rollout')


def test_registered_by_name():
    from metabox_amd import agent, optimizer, tester
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10'])
    opt = tester._lookup(tester._optimizers, 'NRLPSO_Optimizer')(cfg)
    assert isinstance(opt, optimizer.NRLPSO_Optimizer) and (cfg.NP, cfg.k) == (100, 5) and hasattr(agent, 'NRLPSO_Agent') and hasattr(opt, 'make_batch')


# ------------------------------------------------------------------------------------------------ GPU helpers
EP0 = 0          # the Philox episode word of a fresh batch's first reset (the counter starts at -1)


def _u53(a, b):
    return ((a >> 5) * 67108864.0 + (b >> 6)) * (1.0 / 9007199254740992.0)


def philox_reset_tape(seed, episode, NP, D):
    """What the Philox route of k_nrlpso_reset draws (noise excepted), as a reset tape."""
    t = np.zeros(tape_stride(NP, D))
    for e in range(NP * D):
        w = oracle.philox(seed, e, SITE_LDE_ELEM, 0, episode)
        t[e] = _u53(w[0], w[1])
    for i in range(NP):
        t[NP * D + 3 * NP + i] = (oracle.philox(seed, i, SITE_NR_INIT, 0, episode)[0] * 4) >> 32
    w = oracle.philox(seed, NP, SITE_NR_INIT, 0, episode)
    t[NP * D + 4 * NP] = _u53(w[0], w[1])
    return t


def philox_step_tape(seed, step, episode, NP, D):
    """... and of a step of k_nrlpso_step (every slot, whether the step reads it or not)."""
    t = np.zeros(tape_stride(NP, D))
    w, v = oracle.philox(seed, 0, SITE_NR_PART, step, episode), oracle.philox(seed, 1, SITE_NR_PART, step, episode)
    t[T_RAND], t[T_RAND + 1], t[T_IDX], t[T_IDX + 1] = _u53(w[0], w[1]), _u53(w[2], w[3]), (v[0] * K) >> 32, (v[1] * K) >> 32
    for d in range(D):
        e, m = oracle.philox(seed, d, SITE_NR_ELEM, step, episode), oracle.philox(seed, d, SITE_NR_MUT, step, episode)
        t[T_VEC + d], t[T_VEC + D + d] = _u53(e[0], e[1]), _u53(e[2], e[3])
        t[T_VEC + 2 * D + d], t[T_VEC + 3 * D + d] = _u53(m[0], m[1]), _u53(m[2], m[3])
    w = oracle.philox(seed, 0, SITE_POLICY, step, episode)
    t[T_CHOICE] = _u53(w[0], w[1])
    return t


def from_block(block, NP, D, nlog):
    s = split(block, NP, D, nlog)
    sc, dg = s['scalars'], s['diag']
    alias = sc[SC_ALIAS] != 0
    return dict(pop=s['pop'].reshape(NP, D), vel=s['vel'].reshape(NP, D), pbpos=s['pbpos'].reshape(NP, D), stag=s['stag'], pnidx=s['pnidx'], gnidx=s['gnidx'][:K],
                gbpos=s['gbpos'], alias=float(alias), g0=sc[SC_G0] if alias else -1., w=sc[SC_W], r_w=sc[SC_RW], fes=sc[1], pointer=sc[SC_POINTER], sstate=s['sstate'],
                snap=s['snap'].reshape(NP, D), cost=s['cost'], pbcost=s['pbcost'], gbest=sc[0], done=bool(sc[4]), gen=int(sc[6]), ret=sc[5], episode=int(sc[7]),
                curve=s['curve'][:int(sc[3])], cs=dg[0], ef_old=dg[1], ef_new=dg[2], mutated=bool(dg[3]), fnew=dg[4], pm=dg[5], gm=dg[6], action=int(dg[7]))


def same_exact(got, want):
    for k, v in want.items():
        if not np.array_equal(np.asarray(got[k], dtype=np.float64).reshape(np.shape(v)), np.asarray(v, dtype=np.float64), equal_nan=True):
            return k
    return None


def _batch(ps, idx, seeds, NP, max_fes, nlog=50, flags=0):
    from metabox_amd.suite import Batch, Suite
    return Batch(Suite(ps), ALGO_NRLPSO, idx, seeds, NP, max_fes, max(max_fes // nlog, 1), nlog, flags=flags)


# ------------------------------------------------------------------------------------------------ GPU: tape replay of the fixture
def _near_tie(ref_other, ref_new, got_other, got_new, ledger, who, case, g):
    try:
        return not prove_tie_arrays(np.array([ref_other]), np.array([ref_new]), np.array([0.]), np.array([got_other]), np.array([got_new]), np.array([1.]),
                                    ledger, who, case, g)
    except AssertionError:
        return False


def _replay(b, key, seed, D, nk, policy, ledger):
    """-> number of steps compared.  Everything but costs exact at every step and snapshot.  Where a step differs, what no cost of that step decides must still
    be exact and every decision that came out differently (reward bit, stagnation, gbest, either mutation's branch) must be a proven near tie; the episode
    is not compared further after that."""
    import torch
    nlog = 50
    fd = NrFeeder(seed, NP0, D, nk, policy)
    b.set_tape(torch.from_numpy(fd.reset_tape()[None]).cuda())
    s = int(b.reset()[0, 0].item())
    got = from_block(b.read_state(0), NP0, D, nlog)
    assert s == TR(f'{key}/states')[0] and np.array_equal(got['sstate'], TR(f'{key}/sstate0')) and close(got['cost'], TR(f'{key}/cost0')), key
    acts, csneg, mut = TR(f'{key}/actions'), TR(f'{key}/csneg'), TR(f'{key}/mutated')
    ref = {k: TR(f'{key}/{k}') for k in ('fnew', 'pmcost', 'gmcost', 'reward', 'states', 'done', 'gbest', 'fes', 'ef_old', 'ef_new')}
    snaps = set(int(v) for v in TR(f'{key}/snap_steps'))
    q_dev = torch.from_numpy(Q).cuda()
    tape_dev = torch.empty(1, b.tape_stride, dtype=torch.float64, device='cuda')
    for g, a in enumerate(acts):
        prev = got
        tape_dev.copy_(torch.from_numpy(fd.step_tape(int(a), bool(csneg[g]), bool(mut[g]), fd.choice_uniform())[None]))
        b.set_tape(tape_dev)
        if policy:
            st, r, d, la = b.nrlpso_rollout(q_dev, 1)
        else:
            st, r, d = b.step(torch.tensor([int(a)], dtype=torch.int32, device='cuda'))
        out = (int(st[0, 0].item()), r[0].item(), bool(d[0].item()))
        got = from_block(b.read_state(0), NP0, D, nlog)
        exact = (got['action'] == a and (got['cs'] < 0) == csneg[g] and got['mutated'] == mut[g] and got['ef_old'] == ref['ef_old'][g] and
                 got['ef_new'] == ref['ef_new'][g] and out == (ref['states'][g + 1], ref['reward'][g], ref['done'][g]) and got['fes'] == ref['fes'][g])
        if exact and g + 1 in snaps:
            exact = same_exact(got, {k: v for k, v in _ref_snap(key, g + 1).items()}) is None
        if not exact:
            p = int(prev['pointer'])
            assert g + 1 > min(snaps), (key, g, 'diverged before the first snapshot')
            # the state before this step was exact, so whatever does not hang on a cost of this step must still be: only a cost-driven decision may differ
            assert (got['action'] == a and (got['cs'] < 0) == csneg[g] and got['ef_old'] == ref['ef_old'][g] and got['ef_new'] == ref['ef_new'][g]), \
                (key, g, 'a quantity that no cost decides differs', {k: got[k] for k in ('action', 'cs', 'ef_old', 'ef_new')})
            # the step's decisions: name, the reference's outcome (None where the fixture cannot tell), the kernel's, the other operand, the two new costs
            gb_k = got['gm'] if got['mutated'] and got['gm'] < prev['gbest'] else prev['gbest']
            dec = [('f_new < f_old', bool(ref['reward'][g] > 0), bool(got['fnew'] < prev['cost'][p]), prev['cost'][p], ref['fnew'][g], got['fnew']),
                   ('f_new < pbest_cost', (not mut[g]) if prev['stag'][p] >= 1 else None, bool(got['fnew'] < prev['pbcost'][p]), prev['pbcost'][p], ref['fnew'][g], got['fnew']),
                   ('f_new < gbest_cost', bool(ref['gbest'][g] == ref['fnew'][g]), bool(got['gbest'] == got['fnew']), gb_k, ref['fnew'][g], got['fnew'])]
            if mut[g] and got['mutated']:
                dec += [('mutation < pbest_cost', bool(TR(f'{key}/pm_take')[g] == 1), bool(got['pm'] < prev['pbcost'][p]), prev['pbcost'][p], ref['pmcost'][g], got['pm']),
                        ('mutation < gbest_cost', bool(TR(f'{key}/gm_take')[g] == 1), bool(got['gm'] < prev['gbest']), prev['gbest'], ref['gmcost'][g], got['gm'])]
            differing = [d for d in dec if d[1] is not None and d[1] != d[2]]
            unknown = [d for d in dec if d[1] is None]
            tie = lambda d: _near_tie(d[3], d[4], d[3], d[5], ledger, f'hip: {d[0]}', key, g)          # noqa: E731
            assert differing or unknown, (key, g, 'the step differs from the reference although every decision of it agrees', out)
            assert all(tie(d) for d in differing) and (differing or any(tie(d) for d in unknown)), \
                (key, g, 'a decision differs from the reference and is no near tie', [d[0] for d in differing or unknown], {k: got[k] for k in ('fnew', 'pm', 'gm', 'fes')}, out)
            return g
        assert close(got['fnew'], ref['fnew'][g]) and close(got['gbest'], ref['gbest'][g]), (key, g, got['fnew'], ref['fnew'][g])
        if mut[g]:
            assert close(got['pm'], ref['pmcost'][g]) and close(got['gm'], ref['gmcost'][g]), (key, g)
        if g + 1 in snaps:
            assert close(got['cost'], TR(f'{key}/snap{g + 1}/cost')) and close(got['pbcost'], TR(f'{key}/snap{g + 1}/pbcost')), (key, g)
    assert close(got['curve'], TR(f'{key}/cost')) and len(got['curve']) == len(TR(f'{key}/cost')), key
    return len(acts)


def _ref_snap(key, g):
    s = lambda k: TR(f'{key}/snap{g}/{k}')          # noqa: E731
    al = int(s('alias'))
    return dict(pop=s('pop'), vel=s('vel'), pbpos=s('pbpos'), stag=s('stag'), pnidx=s('pnidx').astype(np.float64).ravel(), gnidx=s('gnidx').astype(np.float64),
                gbpos=s('gbpos'), alias=float(al >= 0), g0=float(al), w=float(s('w')), r_w=float(s('r_w')))


LEDGER, ENDED_EARLY = [], []


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_nrlpso_tape_replay_matches_the_reference(case):
    p, D, nk, policy, max_fes, keys = _setup(case)
    b = _batch([p], [0], [0], NP0, max_fes)
    assert (b.state_dim, b.action_dim, b.tape_stride) == (1, 1, tape_stride(NP0, D))
    for key, seed in keys:
        n = _replay(b, key, seed, D, nk, policy, LEDGER)
        if n < len(TR(f'{key}/actions')):
            ENDED_EARLY.append(key)
            break
    b.close()
    print_ledger(LEDGER)
    assert len(ENDED_EARLY) <= 1, ENDED_EARLY


# ------------------------------------------------------------------------------------------------ GPU: the restatement on the kernel's own costs
def _philox_walk(b, nr, seed, NP, D, nlog, steps, rs, where, q=None):
    """Reset and `steps` Philox steps of instance 0 of `b` beside the restatement `nr`, fed the kernel's own costs, then three steps with a planted mutation:
    exact state after every step."""
    import torch
    state = b.reset()
    torch.cuda.synchronize()
    got = from_block(b.read_state(0), NP, D, nlog)
    assert got['episode'] == EP0
    s = nr.reset(philox_reset_tape(seed, EP0, NP, D), got['cost'])
    assert same_exact(got, nr.exact()) is None and int(state[0, 0].item()) == s, (where, 'reset', same_exact(got, nr.exact()))
    seen = dict(mutated=0, neg=0, pos=0, planted=0)
    off = state_off(NP, D, nlog)
    for g in range(steps + 3):
        if g >= steps:
            # Whether a particle stagnates twice within three sweeps is up to the function and the seed (NP = 9 / D = 33 does not), so the mutation is
            # also planted, in the kernel's block and in the restatement alike: the particle whose turn it is has failed before and holds an unbeatable
            # pbest cost -- its turn mutates, the pbest half replaces a live row (:219-221) and the gbest half takes whichever branch its cost decides.
            pt = nr.pointer
            block = b.read_state(0)
            block[off['stag'][0] + pt], block[off['pbcost'][0] + pt] = 5., -1e300
            b.write_state(0, block)
            nr.stag[pt], nr.pbcost[pt] = 5., -1e300
            seen['planted'] += 1
        a = int(rs.randint(0, 4))
        st, r, d = b.step(torch.tensor([a] * b.B, dtype=torch.int32, device='cuda'))
        out = (int(st[0, 0].item()), r[0].item(), bool(d[0].item()))
        got = from_block(b.read_state(0), NP, D, nlog)
        want = nr.step(a, philox_step_tape(seed, g + 1, EP0, NP, D), lambda k, x: (got['fnew'], got['pm'], got['gm'])[k])
        bad = same_exact(got, nr.exact())
        dg = nr.diag
        assert bad is None, (where, g, a, bad)
        assert out == want and got['mutated'] == dg['mutated'] and got['gbest'] == nr.gbest, (where, g, out, want)
        for k in ('cs', 'ef_old', 'ef_new'):
            assert got[k] == dg[k] or (np.isnan(got[k]) and np.isnan(dg[k])), (where, g, k, got[k], dg[k])
        assert np.array_equal(got['cost'], nr.cost) and np.array_equal(got['pbcost'], nr.pbcost) and np.array_equal(got['curve'], nr.curve), (where, g)
        assert g < steps or dg['mutated'], (where, g, 'the planted step did not mutate')
        seen['mutated'] += dg['mutated']; seen['neg' if dg['cs'] < 0 else 'pos'] += 1
        if d:
            break
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize('D', [2, 7, 8, 10, 33, 40])
@pytest.mark.parametrize('NP', [9, 100, 128])
def test_hip_nrlpso_against_the_restatement_on_its_own_costs(NP, D):
    """Both branches of the pairwise sum (D below / from 8), its tails of eight, and both forms at every shape: the batch's default (cached wherever the
    matrix fits beside the resident arrays: NP 9 and 100 at every D here, NP 128 at D 2 and 7) and MBX_F_NRLPSO_RECOMPUTE; 3 sweeps on a bbob and a
    bbob-noisy function, then three turns with a planted mutation.  Positions, ef, neighbour lists and counters exact."""
    total = dict(mutated=0, neg=0, pos=0, planted=0)
    for flags in (0, F_RECOMPUTE):
        for suite, fid in (('bbob', 15), ('bbob-noisy', 118)):
            p = problems(suite, D)[fid]
            seed, max_fes, nlog = 1000 * NP + D, 40 * NP, 10
            b = _batch([p], [0], [seed], NP, max_fes, nlog, flags=flags)
            nr = Nr(NP, D, p.lb, p.ub, max_fes, max_fes // nlog, nlog)
            seen = _philox_walk(b, nr, seed, NP, D, nlog, 3 * NP, np.random.RandomState(NP + D), (suite, NP, D, flags))
            for k in total:
                total[k] += seen[k]
            b.close()
    print(f'NP {NP} D {D}:', total)
    assert total['mutated'] >= total['planted'] == 12 and total['neg'] + total['pos'] == 4 * (3 * NP + 3)


@pytest.mark.gpu
def test_hip_nrlpso_philox_route_equals_the_rebuilt_tape():
    """A batch stepped from Philox and one stepped from tapes rebuilt on the host with oracle.philox and the documented sites leave the same blocks."""
    import torch
    p = problems('bbob', 10)[21]
    seed, steps = 77, 130
    a, b = _batch([p], [0], [seed], NP0, 1500), _batch([p], [0], [seed], NP0, 1500)
    q = torch.from_numpy(Q).cuda()
    b.set_tape(torch.from_numpy(philox_reset_tape(seed, EP0, NP0, 10)[None]).cuda())
    a.reset(); b.reset()
    assert torch.equal(a.state, b.state) and np.array_equal(a.read_state(0), b.read_state(0))
    for g in range(steps):
        b.set_tape(torch.from_numpy(philox_step_tape(seed, g + 1, EP0, NP0, 10)[None]).cuda())
        a.nrlpso_rollout(q, 1); b.nrlpso_rollout(q, 1)
        torch.cuda.synchronize()
    assert np.array_equal(a.read_state(0), b.read_state(0)) and torch.equal(a.state, b.state)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ GPU: routes
@pytest.mark.gpu
def test_hip_nrlpso_routes_are_bit_identical():
    """n one-step launches == chunks (1, 7, 60, 140) == mbx_step fed the recorded actions == MBX_F_NRLPSO_RECOMPUTE, state blocks bit for bit, on a mixed
    batch whose mutating instances reach maxFEs early and stay frozen; a sub-batch gives the same results."""
    import torch
    ps = problems('bbob-noisy', 10)
    fids = (101, 105, 118, 129)
    idx = np.arange(12) % 4
    seeds = np.arange(12, dtype=np.uint64) * 13 + 3
    n, max_fes = 310, 400          # 50 log points of 8 FEs: the curve holds every append (a budget that is no multiple of the interval would overrun it)
    q = torch.from_numpy(Q).cuda()
    mk = lambda flags=0, sel=slice(None): _batch([ps[f] for f in fids], idx[sel], seeds[sel], NP0, max_fes, flags=flags)      # noqa: E731
    one = mk()
    one.reset()
    acts, dones = [], []
    for g in range(n):
        _, _, d, _, traj = one.nrlpso_rollout(q, 1, trajectory=True)
        acts.append(traj['actions'][0].clone()); dones.append(d.clone())
    steps_alive = torch.stack(dones).to(torch.int32).sum(0)
    assert bool(one.done.all()) and int(steps_alive.min()) < int(steps_alive.max()), 'the batch should hold instances that finish at different steps'
    ref_state, ref_res = one.state.clone(), one.results()
    blocks = [one.read_state(i) for i in range(12)]

    def same(b, who):
        torch.cuda.synchronize()
        for i in range(b.B):
            assert np.array_equal(b.read_state(i), blocks[i]), (who, i)
        res = b.results()
        for k in ref_res:
            assert torch.equal(res[k], ref_res[k]), (who, k)
    for flags, who in ((0, 'chunks'), (F_RECOMPUTE, 'recompute')):
        b = mk(flags)
        assert b.flags & F_RECOMPUTE == flags
        b.reset()
        left, ret, k = n, torch.zeros(12, dtype=torch.float64, device='cuda'), 0
        while left > 0:
            c = min((1, 7, 60, 140)[k % 4], left)
            _, r, _, _ = b.nrlpso_rollout(q, c)
            ret += r
            left -= c; k += 1
        same(b, who)
        assert torch.equal(ret, ref_res['return']) and torch.equal(b.state, ref_state)
        b.close()
    b = mk()
    b.reset()
    for g in range(n):
        b.step(torch.where(acts[g] < 0, torch.zeros_like(acts[g]), acts[g]).contiguous())
    same(b, 'mbx_step')
    b.close()
    half = mk(sel=slice(0, 6))
    half.reset()
    half.nrlpso_rollout(q, n)
    res = half.results()
    for k in ref_res:
        assert torch.equal(res[k], ref_res[k][:6]), ('split', k)
    half.close(); one.close()


@pytest.mark.gpu
def test_hip_nrlpso_unmoved_aliased_gbest_row():
    """The moving particle is the aliased gbest row with zero velocity, cs >= 0 and action 2: it does not move, its re-evaluation through the step
    route equals the reset route's cost bit for bit, the reward is -2 and the stagnation count rises by one."""
    import torch
    for suite, fid, D in (('bbob', 15, 10), ('bbob', 21, 10), ('bbob', 8, 30)):
        p = problems(suite, D)[fid]
        b = _batch([p], [0], [5], NP0, 1500)
        b.reset()
        torch.cuda.synchronize()
        block = b.read_state(0)
        off = state_off(NP0, D, 50)
        g0 = int(block[off['scalars'][0] + SC_G0])
        block[off['scalars'][0] + SC_POINTER] = g0
        b.write_state(0, block)
        before = from_block(block, NP0, D, 50)
        assert before['alias'] == 1 and not before['vel'].any()
        _, r, _ = b.step(torch.tensor([2], dtype=torch.int32, device='cuda'))
        got = from_block(b.read_state(0), NP0, D, 50)
        assert got['cs'] >= 0 and np.array_equal(got['pop'], before['pop']) and not got['vel'].any(), (fid, D)
        assert got['fnew'] == before['cost'][g0] and got['cost'][g0] == before['cost'][g0], (fid, D, got['fnew'], before['cost'][g0])
        assert r[0].item() == -2 and got['stag'][g0] == 1 and got['ef_old'] == got['ef_new'] and got['pointer'] == (g0 + 1) % NP0
        b.close()


@pytest.mark.gpu
def test_hip_nrlpso_in_kernel_choice_is_numpys_rule():
    """4 states x a grid of u (interior points on every row; on the all-zero row, whose probabilities are exact, also the cumulative edges and their
    neighbours) through a taped one-step rollout: the action the kernel takes is searchsorted(cumsum(p) / cumsum(p)[-1], u, 'right')."""
    import torch
    table = np.array([[0., 0., 0., 0.], Q[1], Q[2], [1.5, -2., 0.3, 0.]])
    grid = {s: list(np.linspace(0.003, 0.997, 41)) for s in range(4)}
    for e in (0.25, 0.5, 0.75):
        grid[0] += [e, np.nextafter(e, 0), np.nextafter(e, 1)]
    grid[0] += [0., np.nextafter(1., 0)]
    rows = []
    for s in range(4):
        ex = np.exp(table[s]); cdf = np.cumsum(ex / ex.sum()); cdf = cdf / cdf[-1]
        rows += [(s, u) for u in grid[s] if s == 0 or np.abs(cdf - u).min() > 1e-9]
    B = len(rows)
    p = problems('bbob', 10)[1]
    b = _batch([p], [0] * B, list(range(B)), NP0, 1500)
    rs = np.random.RandomState(2)
    t = np.zeros((B, b.tape_stride))
    t[:, :NP0 * 10] = rs.rand(B, NP0 * 10)
    t[:, NP0 * 10 + 4 * NP0] = 0.3
    t[:, NP0 * 10 + 3 * NP0] = [s for s, _ in rows]
    b.set_tape(torch.from_numpy(t).cuda())
    st = b.reset()
    assert np.array_equal(st[:, 0].cpu().numpy(), [s for s, _ in rows])
    t = np.zeros((B, b.tape_stride))
    t[:, T_RAND:T_RAND + 2] = rs.rand(B, 2)
    t[:, T_CHOICE] = [u for _, u in rows]
    b.set_tape(torch.from_numpy(t).cuda())
    _, _, _, acts = b.nrlpso_rollout(torch.from_numpy(table).cuda(), 1)
    want = [choose(table[s], u) for s, u in rows]
    assert np.array_equal(acts.cpu().numpy(), want), [(r, int(a), w) for r, a, w in zip(rows, acts.cpu().numpy(), want) if a != w][:5]
    assert set(want) == {0, 1, 2, 3}
    b.close()


@pytest.mark.gpu
def test_nrlpso_in_the_harness(tmp_path):
    """NRLPSO_Agent.rollout_batch through the Tester and the B = 1 protocol view on two problems at maxFEs 400."""
    from metabox_amd.agent import NRLPSO_Agent
    from metabox_amd.agent.utils import save_class
    from metabox_amd.config import get_config
    from metabox_amd.environment import BatchedPBO_Env, PBO_Env
    from metabox_amd.optimizer import NRLPSO_Optimizer
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda'])
    cfg.agent_save_dir = None
    cfg.maxFEs, cfg.log_interval = 400, 8
    agent = NRLPSO_Agent(copy.deepcopy(cfg)).load_exported_weights(POL)
    pb = [problems('bbob', 10)[f] for f in (1, 16)]
    env = BatchedPBO_Env(pb, NRLPSO_Optimizer(copy.deepcopy(cfg)), np.arange(32) % 2, np.arange(32, dtype=np.uint64) + 5)
    out = agent.rollout_batch(env)
    assert bool((out['fes'] >= 400).all()) and bool((out['fes'] <= 402).all()) and int(out['steps'].max()) <= 300 and bool((out['cost_len'] == 51).all())
    assert bool((out['cost'][:, 1:] <= out['cost'][:, :-1]).all())
    env.close()
    for f in pb:
        np.random.seed(4)
        opt = NRLPSO_Optimizer(copy.deepcopy(cfg))
        info = agent.to('cuda').rollout_episode(PBO_Env(f, opt))
        assert 400 <= info['fes'] <= 402 and len(info['cost']) == 51 and info['cost'][0] >= info['cost'][-1]
    load_dir = str(tmp_path / 'models') + '/'
    save_class(load_dir, 'NRLPSO_Agent', agent)
    tcfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda', '--log_dir', str(tmp_path / 'out'), '--agent_load_dir', load_dir, '--test_runs', '2',
                       '--test', '--agent_for_cp', 'NRLPSO_Agent', '--l_optimizer_for_cp', 'NRLPSO_Optimizer'])
    tcfg.maxFEs, tcfg.log_interval = 400, 8
    t = Tester(tcfg)
    assert 'NRLPSO_Optimizer' not in t.skipped
    res = t.test()
    for prob, rows in res['cost'].items():
        assert len(rows['NRLPSO_Agent']) == 2 and all(len(r) == 51 and r[0] >= r[-1] for r in rows['NRLPSO_Agent']), prob
        assert all(400 <= v <= 402 for v in res['fes'][prob]['NRLPSO_Agent']), prob
    learner, _ = _agent(3, 'cuda')
    learner._NRLPSO_Agent__config.maxFEs, learner._NRLPSO_Agent__config.log_interval = 400, 8
    np.random.seed(2)
    done, info = learner.train_episode(PBO_Env(pb[1], NRLPSO_Optimizer(copy.deepcopy(cfg))))
    assert done and info['learn_steps'] == 3 and learner.learn_steps == 3
