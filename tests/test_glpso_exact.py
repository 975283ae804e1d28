"""GL-PSO's kernels (metabox_amd/csrc/mbx_glpso.hpp) against the exact restatement of tests/glpso_exact.py, away from the geometry of the recorded episodes.

CPU (no GPU needed):
  * the restatement, driven by GlpsoTapeFeeder with the reference's float64 costs, reproduces every recorded quantity of the eleven fixture episodes at every
    generation (a first divergence must be a proven near-tie) -- this ties the restatement to the reference, not to the kernel;
  * the judge has teeth: a stand-in kernel (the restatement with bbob_exact.float64_eval costs) passes `judge` on every planted state below, and each entry of
    glpso_exact.DEFECTS, applied to the stand-in, is rejected by at least one planted state, named in WITNESS;
  * the undecided cap: on the walk inputs of the GPU sweep the stand-in leaves at most 1 decision in 1000 undecided per (shape, problem), none on the planted states.
    Counted apart and printed, not under the cap: an undecided selection whose candidate is, to 4 ulp a coordinate, the row's own exemplar, pbest_position or
    gbest_position (the holder of gbest breeds r x + (1 - r) x every generation; the comparison is between two evaluations of one point).  Measured, stand-in and
    device alike: 25 of 360 decisions at (4, 2), 14 of 360 at (5, 3), at most 6 per shape from NP = 63 up; undecided otherwise: 0 (docs/EXPERIMENTS.md).
GPU: the same planted states and walks through set_tape / read_state / write_state / reset / step, `judge` applied after every launch to the kernel's own previous
block; and the Philox route against the rebuilt tape at three edge shapes.

Planted states (PLANTED; each at (100, 10) and (5, 3), on bbob 15):
  counters     counters at 6, 7, 8 and exemplar costs no candidate can beat: 7 -> 8 fires, 6 -> 7 does not; then once more
  tournament   draws with the row itself, a row replaced in the same launch, a row that won selection in this launch, ten equal indices, indices 0 and NP - 1,
               two drawn rows with bit-equal exemplar_cost (the first drawn wins)
  ties         every particle at rest (V = 0, exemplar = X), k = i, r = 1.0, mutation off, rows 0 and NP - 1 on the best row: launch 1 takes everything from 1e300
               (gbest argmin among three equal rows), launch 2 re-evaluates the same rows (every `<` is c < c: all lose, counters + 1), launch 3 the same with
               pbest_position / gbest_position / gbest_idx planted elsewhere (an `<=` would overwrite them) and rows 0 / NP - 1 drawing each other (equal pbest:
               the crossover branch is the uniform one)
  bounds       X at ub with V > 0, at lb with V < 0, a step landing exactly on ub / lb (no bounce), velocity clamps, |v| exactly vmax where such a draw exists
  mutation     mt in {0, 0.01, nextafter(0.01, 0)}, mu in {0, 1 - 2^-53}, every candidate forced to win so that it is visible
  frozen       the budget 6 NP + 17 to its end (the last generation overshoots), then a launch on the finished instance: frozen, done = 1, reward = 0
  resets       reset, a generation, counters planted (one at 8), reset again (episode + 1), rebind to another problem, reset (episode word restarts): counters
               carried, tournament fired at reset, selection unconditional against costs no candidate can beat
"""
import numpy as np
import pytest

import glpso_exact as gx
import parity
from helpers import print_ledger, problems, prove_tie_arrays
from test_glpso import ALGO_GLPSO, CASES, TR, GlpsoTapeFeeder, _episodes, _fired, philox_tape
from test_glpso import split_state as split_state_glpso

SHAPES = [(4, 2), (5, 3), (63, 7), (64, 10), (65, 33), (100, 12), (100, 40), (255, 13), (256, 10)]      # (100, 12): the docking instance
MUST_RUN = SHAPES                                # all nine fit the LDS of one workgroup (measured; docs/EXPERIMENTS.md)
PLANT_SHAPES = [(100, 10), (5, 3)]
NLOG = 5
MBX_E_UNSUPPORTED = -3
EVENTS = {'tournament', 'mutation', 'bounce_ub', 'bounce_lb', 'vclamp', 'gbest_moved'}


# ------------------------------------------------------------------------------------------------ runners: the stand-in and the device
class StandIn:
    """B instances of the restatement with float64 costs (and, optionally, one defect): the interface of `Device`."""

    def __init__(self, cfgs, pidx, defect=None):
        self.all, self.defect = cfgs, defect
        self.B = len(pidx)
        c = cfgs[0]
        self.blocks = [np.zeros(gx.state_doubles(c.NP, c.D, c.n_logpoint)) for _ in pidx]
        self.rebind(pidx)

    def rebind(self, pidx):
        self.cfgs = [self.all[k] for k in pidx]
        for b in self.blocks:
            gx.split_state(b, self.cfgs[0].D, self.cfgs[0].n_logpoint, self.cfgs[0].NP)['scalars'][gx.SC_EPISODE] = -1.

    def read(self, k):
        return self.blocks[k].copy()

    def write(self, k, block):
        self.blocks[k] = np.array(block, dtype=np.float64)

    def _run(self, fn, tapes):
        was_done = [gx.outputs(b, c)[2] for b, c in zip(self.blocks, self.cfgs)]
        self.blocks = [fn(b, t, c, defect=self.defect) for b, t, c in zip(self.blocks, tapes, self.cfgs)]
        return was_done

    def reset(self, tapes):
        self._run(gx.restate_reset, tapes)
        return [(gx.outputs(b, c)[0], 0., 0) for b, c in zip(self.blocks, self.cfgs)]

    def step(self, tapes):
        self._run(gx.restate_generation, tapes)
        return [gx.outputs(b, c) for b, c in zip(self.blocks, self.cfgs)]

    def close(self):
        pass


class Device:
    """B instances of one Batch, driven through set_tape / read_state / write_state / reset / step."""

    def __init__(self, cfgs, pidx, seeds=None):
        from metabox_amd.suite import Batch, Suite
        self.all = cfgs
        c = cfgs[0]
        self.suite = Suite([q.problem for q in cfgs])
        self.B = len(pidx)
        seeds = np.arange(self.B, dtype=np.uint64) * 131 + 7 if seeds is None else seeds
        self.seeds = seeds
        self.batch = Batch(self.suite, ALGO_GLPSO, np.asarray(pidx, dtype=np.int32), seeds, c.NP, c.max_fes, c.log_interval, c.n_logpoint)
        assert self.batch.tape_stride == gx.tape_stride(c.NP, c.D)
        self.cfgs = [cfgs[k] for k in pidx]

    def rebind(self, pidx):
        self.batch.rebind(np.asarray(pidx, dtype=np.int32), self.seeds)
        self.cfgs = [self.all[k] for k in pidx]

    def read(self, k):
        return self.batch.read_state(k)

    def write(self, k, block):
        self.batch.write_state(k, block)

    def _tape(self, tapes):
        import torch
        self.batch.set_tape(torch.from_numpy(np.ascontiguousarray(np.stack(tapes))).cuda())

    def reset(self, tapes):
        import torch
        self._tape(tapes)
        st = self.batch.reset()
        torch.cuda.synchronize()
        st = st.cpu().numpy()
        return [(st[k, 0], 0., 0) for k in range(self.B)]

    def step(self, tapes):
        import torch
        self._tape(tapes)
        st, rw, dn = self.batch.step(None)
        torch.cuda.synchronize()
        st, rw, dn = st.cpu().numpy(), rw.cpu().numpy(), dn.cpu().numpy()
        return [(st[k, 0], rw[k], dn[k]) for k in range(self.B)]

    def close(self):
        self.batch.close(); self.suite.close()


class Session:
    """Launches on a runner, every one judged against the runner's own previous blocks.  per[k]: the merged report of instance k."""

    def __init__(self, run):
        self.run = run
        self.per = [gx.Report() for _ in range(run.B)]
        self.launches = 0

    def launch(self, tapes, reset=False, known=None):
        run = self.run
        before = [run.read(k) for k in range(run.B)]
        outs = run.reset(tapes) if reset else run.step(tapes)
        for k in range(run.B):
            try:
                rep = gx.judge(before[k], tapes[k], run.read(k), run.cfgs[k], reset, outs[k], known)
            except gx.Rejected as e:
                raise gx.Rejected(f'launch {self.launches} ({"reset" if reset else "generation"}), instance {k}', *e.args) from None
            self.per[k].merge(rep)
        self.launches += 1

    def total(self):
        out = gx.Report()
        for r in self.per:
            out.merge(r)
        return out


# ------------------------------------------------------------------------------------------------ the planted states
def _cfg(NP, D, short=False, fid=15):
    """short: the sweep's budget 6 NP + 17 (reset + three generations, the last overshooting); otherwise 20 NP with log points every 4 NP: the first generation's
    fes + NP = 3 NP is below the first log point, fes + 2 NP = 4 NP is on it."""
    max_fes = 6 * NP + 17 if short else 20 * NP
    return gx.Cfg(problems('bbob', D)[fid], NP, max_fes, max_fes // NLOG, NLOG)


def _rtape(rs, cfg, reset=False):
    return gx.random_tape(rs, cfg.NP, cfg.D, cfg.noise_kind, reset)


def _tview(tape, cfg, reset=False):
    return gx.split_tape(tape, cfg.NP, cfg.D, reset)              # views: writing through them writes the tape


def _base(S, rs, gens=2):
    cfg = S.run.cfgs[0]
    S.launch([_rtape(rs, cfg, True)], reset=True)
    for _ in range(gens):
        S.launch([_rtape(rs, cfg)])


def _edit(S, fn):
    cfg = S.run.cfgs[0]
    blk = S.run.read(0)
    fn(gx.split_state(blk, cfg.D, cfg.n_logpoint, cfg.NP))
    S.run.write(0, blk)


def plant_counters(S, rs):
    cfg = S.run.cfgs[0]
    NP = cfg.NP
    _base(S, rs)

    def f(s):
        s['stag'][:] = np.array([6., 7., 8.])[np.arange(NP) % 3]
        s['excost'][:] = -1e6 - np.arange(NP)                      # no candidate beats these: every row loses, decidedly
    _edit(S, f)
    S.launch([_rtape(rs, cfg)])
    S.launch([_rtape(rs, cfg)])


def plant_tournament(S, rs):
    cfg = S.run.cfgs[0]
    NP = cfg.NP
    r0, r1, r2, r3, rl = 0, 1, 2, NP - 2, NP - 1
    _base(S, rs)

    def f(s):
        s['stag'][:] = 0.
        s['stag'][[r0, r1, r2, r3, rl]] = 8.
        s['excost'][[r0, r1, r2, r3, rl]] = [-10., -20., -5., 1e300, -20.]       # r3 wins its selection (counter -> 0); r1 and rl hold bit-equal costs
    _edit(S, f)
    tape = _rtape(rs, cfg)
    tour = _tview(tape, cfg)['tour']
    tour[r0] = r3                                                  # ten equal indices, of a row that won selection in this launch
    tour[r2] = r2; tour[r2, [0, 2]] = r0                           # the row itself; a row being replaced in this launch (lower cost: chosen)
    tour[r1] = r0; tour[r1, 0] = rl; tour[r1, 2] = r1              # indices NP - 1 and 0; rl and r1 tie: rl, drawn first, wins (the last of the equal ones is r1)
    tour[rl] = rl; tour[rl, 0] = r1; tour[rl, 2:4] = [0, NP - 1]   # the same tie the other way round: r1 drawn first
    S.launch([tape])


def plant_ties(S, rs):
    import bbob_exact as be
    cfg = S.run.cfgs[0]
    NP, D = cfg.NP, cfg.D
    assert cfg.noise_kind == 0
    S.launch([_rtape(rs, cfg, True)], reset=True)
    X = gx.split_state(S.run.read(0), D, cfg.n_logpoint, NP)['X'].reshape(NP, D).copy()
    best = int(np.argmin(be.float64_eval(cfg.problem, X)))
    X[0] = X[best]; X[NP - 1] = X[best]                            # three equal rows hold the minimum: the first is row 0, the last row NP - 1

    def rest(s):
        s['X'][:] = X.ravel(); s['pbpos'][:] = X.ravel(); s['exemplar'][:] = X.ravel()
        s['V'][:] = 0.
        s['pbest'][:] = 1e300; s['excost'][:] = 1e300; s['stag'][:] = 0.
        s['scalars'][gx.SC_GBEST] = 1e300
    _edit(S, rest)

    def tape_ki(cu):
        tape = _rtape(rs, cfg)
        t = _tview(tape, cfg)
        t['cidx'][:] = np.arange(NP)[:, None]
        t['cu'][:] = cu
        t['mt'][:] = 1.
        return tape, t
    S.launch([tape_ki(1.0)[0]])                                    # everything improves from 1e300; the candidate is pbest_position bit for bit
    s = gx.split_state(S.run.read(0), D, cfg.n_logpoint, NP)
    assert gx.same(s['exemplar'], X.ravel()) or S.run.__class__ is StandIn and S.run.defect, 'launch 1 did not take the candidates (= the positions)'
    lose = {i: False for i in range(NP)}
    S.launch([tape_ki(1.0)[0]], known={'pbest': lose, 'sel': lose})            # c < c: nothing improves, every counter + 1
    other = rs.uniform(cfg.lb, cfg.ub, size=(NP, D))
    other[NP - 1] = other[0]

    def elsewhere(s):
        s['pbpos'][:] = other.ravel()
        s['gbpos'][:] = rs.uniform(cfg.lb, cfg.ub, size=D)
        s['scalars'][gx.SC_GBEST_IDX] = 1.
        s['excost'][[0, NP - 1]] = 1e300                           # rows 0 and NP - 1 take their candidates: the uniform branch is visible
    _edit(S, elsewhere)
    tape, t = tape_ki(0.5)
    t['cidx'][0] = NP - 1; t['cidx'][NP - 1] = 0                   # equal pbest, equal pbest_position: pbest[k] < pbest[i] is false
    S.launch([tape], known={'pbest': lose})


def _landing_r():
    """r with fl(c1 r) in {1 - 2^-53, 1}: with x = ub - 1, exemplar = ub, V = 0 the step is that number and x + v rounds to ub exactly."""
    return 1. / gx.C1


def _exact_one_r():
    """r with fl(c1 r) == 1.0 exactly, within a few ulp of 1 / c1, or None."""
    r = 1. / gx.C1
    for cand in (r, np.nextafter(r, 0.), np.nextafter(r, 1.), np.nextafter(np.nextafter(r, 0.), 0.), np.nextafter(np.nextafter(r, 1.), 1.)):
        if gx.C1 * cand == 1.:
            return float(cand)
    return None


def plant_bounds(S, rs):
    cfg = S.run.cfgs[0]
    NP, D = cfg.NP, cfg.D
    lb, ub = cfg.lb, cfg.ub
    vmax = gx.RHO * (ub - lb)
    _base(S, rs)
    one = _exact_one_r()
    tape = _rtape(rs, cfg)
    r = _tview(tape, cfg)['rand']

    def f(s):
        X, V, E = s['X'].reshape(NP, D), s['V'].reshape(NP, D), s['exemplar'].reshape(NP, D)
        X[0], V[0], E[0] = ub, 1., ub                              # at ub, moving out: bounce, v = -0.5 (w V)
        X[1], V[1], E[1] = lb, -1., lb
        X[2], V[2], E[2] = ub - 1., 0., ub                         # lands exactly on ub: nx > ub is false
        X[3], V[3], E[3] = lb + 1., 0., lb
        X[4], V[4] = 0., 0.                                        # c1 r (ex - x) = +-7.48: clamped to +-vmax
        E[4] = np.where(np.arange(D) % 2 == 0, ub, lb)
        if one is not None:
            E[4, 0] = vmax                                         # fl(c1 r) = 1 exactly: v = vmax without the clamp
    _edit(S, f)
    r[2] = r[3] = _landing_r()
    r[4] = 1.
    if one is not None:
        r[4, 0] = one
    s = gx.split_state(S.run.read(0), D, cfg.n_logpoint, NP)
    nx, nv, ev = gx.move(s['X'].reshape(NP, D), s['V'].reshape(NP, D), s['exemplar'].reshape(NP, D), r, cfg)
    assert np.all(nx[2] == ub) and np.all(nv[2] > 0.9) and np.all(nx[3] == lb) and np.all(nv[3] < -0.9), 'the landing rows do not land on the bounds'
    assert np.all(nv[0] == -0.5 * (gx.W * 1.)) and np.all(nv[1] == -0.5 * (gx.W * -1.)) and np.all(np.abs(nv[4]) == vmax) and all(ev.values())
    S.launch([tape])


def plant_mutation(S, rs):
    cfg = S.run.cfgs[0]
    _base(S, rs)
    _edit(S, lambda s: s['excost'].__setitem__(slice(None), 1e300))
    tape = _rtape(rs, cfg)
    t = _tview(tape, cfg)
    e = np.arange(cfg.NP * cfg.D).reshape(cfg.NP, cfg.D)
    t['mt'][:] = np.array([0., 0.01, np.nextafter(0.01, 0.)])[e % 3]
    t['mu'][:] = np.array([0., 1. - 2. ** -53])[(e // 3) % 2]
    S.launch([tape])


def plant_frozen(S, rs):
    cfg = S.run.cfgs[0]
    S.launch([_rtape(rs, cfg, True)], reset=True)
    gens = -(-(cfg.max_fes - 2 * cfg.NP) // (2 * cfg.NP))           # 3 at NP = 100, 4 at NP = 5
    for _ in range(gens):
        S.launch([_rtape(rs, cfg)])
    blk = gx.split_state(S.run.read(0), cfg.D, cfg.n_logpoint, cfg.NP)
    assert blk['scalars'][gx.SC_DONE] == 1. and blk['scalars'][gx.SC_FES] == 2 * cfg.NP * (gens + 1) > cfg.max_fes or getattr(S.run, 'defect', None)
    S.launch([_rtape(rs, cfg)])
    assert 'frozen' in S.total()['events'] or getattr(S.run, 'defect', None)


def plant_resets(S, rs):
    cfg = S.run.cfgs[0]
    NP = cfg.NP
    S.launch([_rtape(rs, cfg, True)], reset=True)
    S.launch([_rtape(rs, cfg)])

    def f(s):
        s['stag'][:] = np.arange(NP) % 5
        s['stag'][0], s['stag'][1] = 8., 7.
        s['excost'][:] = -1e6 - np.arange(NP)                      # a reset that selected with < would keep these
    _edit(S, f)
    S.launch([_rtape(rs, cfg, True)], reset=True)                  # the same batch again: episode + 1, row 0's carried counter fires the tournament
    assert 'tournament' in S.total()['events'] or getattr(S.run, 'defect', None)
    S.launch([_rtape(rs, cfg)])
    _edit(S, f)
    S.run.rebind([1])                                              # another problem on the same batch: the counters stay, the episode word restarts
    cfg = S.run.cfgs[0]
    S.launch([_rtape(rs, cfg, True)], reset=True)
    S.launch([_rtape(rs, cfg)])


PLANTED = {'counters': plant_counters, 'tournament': plant_tournament, 'ties': plant_ties, 'bounds': plant_bounds, 'mutation': plant_mutation, 'frozen': plant_frozen,
           'resets': plant_resets}

# defect -> the planted states that must reject it (at both shapes unless a shape is given)
WITNESS = {
    'pb_le': ['ties'], 'gb_le': ['ties'], 'sel_le': ['ties'], 'stag_ge': ['counters'], 'tour_last': ['tournament'], 'tour_live': ['tournament'],
    'tour_cost': ['counters', 'tournament'], 'tour_zero': ['counters', 'tournament'], 'reset_zero_stag': ['resets'], 'reset_lt': ['resets'],
    'cross_current': ['counters'], 'cross_reversed': ['mutation'], 'cross_le': ['ties'], 'mut_le': ['mutation'], 'bounce_after_clip': ['bounds'], 'bounce_ge': ['bounds'],
    'log_2np': ['counters'], 'gb_excost': ['counters'], 'gb_last': ['ties'], 'row_last': ['tournament'],
}


def _planted_cfgs(name, NP, D):
    if name == 'resets':
        return [_cfg(NP, D), _cfg(NP, D, fid=3)]
    return [_cfg(NP, D, short=(name == 'frozen'))]


def _run_planted(name, NP, D, make):
    """One planted state on a runner made by `make(cfgs, pidx)` -> the session."""
    run = make(_planted_cfgs(name, NP, D), [0])
    S = Session(run)
    try:
        PLANTED[name](S, np.random.RandomState(7000 + 10 * NP + D))
    finally:
        run.close()
    return S


# ------------------------------------------------------------------------------------------------ CPU: the restatement reproduces the reference
@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference_episodes(case):
    """Whole fixture episodes on the restatement with the reference's float64 objective: gbest, fes, pbest, exemplar_cost, the counters at every generation, the cost
    curve and the end of the episode.  A first divergence of a decision must be a proven near-tie; before it, the costs agree to a few ulp."""
    dim, seed, eps = _episodes(case)
    max_fes = int(TR[f'{case}/max_fes'])
    rs = np.random.RandomState(seed)
    ledger, diverged = [], False
    blk = np.zeros(gx.state_doubles(100, dim, 50))
    for p, nk, key in eps:
        cfg = gx.Cfg(p, 100, max_fes, max_fes // 50, 50, protein=case.startswith('protein'))
        assert cfg.noise_kind == nk
        costs = gx.reference_costs(cfg)
        fd = GlpsoTapeFeeder(seed, dim, nk, rs)
        want = {k: TR[f'{key}/{k}'] for k in ('gbest', 'fes', 'pbest', 'exemplar_cost', 'stag')}
        G = len(want['gbest']) - 1
        carried = gx.split_state(blk, dim, 50)['stag'].copy()
        blk = gx.restate_reset(blk, fd.reset_tape(), cfg, costs)
        fd.commit(_fired(want['stag'][0]))
        prev = gx.split_state(blk, dim, 50)
        assert np.array_equal(prev['stag'], carried)               # init_population leaves the counters alone
        for g in range(G + 1):
            if g > 0:
                blk = gx.restate_generation(blk, fd.step_tape(), cfg, costs)
                fd.commit(_fired(want['stag'][g]))
            st = gx.split_state(blk, dim, 50)
            sc = st['scalars']
            assert sc[gx.SC_FES] == want['fes'][g], (case, key, g)
            if not diverged and g > 0:
                ok = prove_tie_arrays(want['exemplar_cost'][g - 1], want['exemplar_cost'][g], want['stag'][g], prev['excost'], st['excost'], st['stag'], ledger,
                                      'restatement', key, g)
                ref_i = (want['pbest'][g] != want['pbest'][g - 1]).astype(np.float64)
                cur_i = (st['pbest'] != prev['pbest']).astype(np.float64)
                ok = prove_tie_arrays(want['pbest'][g - 1], want['pbest'][g], ref_i, prev['pbest'], st['pbest'], cur_i, ledger, 'restatement', key, g) and ok
                diverged = not ok
            tol = dict(rtol=1e-5, atol=8 * 4.6e-13) if diverged else dict(rtol=1e-9, atol=8 * 4.6e-13)
            if not diverged:
                assert np.array_equal(st['stag'], want['stag'][g]), (case, key, g)
            for name, got, ref in (('gbest', sc[gx.SC_GBEST], want['gbest'][g]), ('pbest', st['pbest'], want['pbest'][g]), ('excost', st['excost'], want['exemplar_cost'][g])):
                assert np.all(np.abs(got - ref) <= tol['atol'] + tol['rtol'] * np.abs(ref)), (case, key, g, name)
            prev = {k: v.copy() for k, v in st.items()}
        assert sc[gx.SC_DONE] == 1., (case, key)
    n = int(sc[gx.SC_COST_LEN])
    ref_cost = TR[f'{case}/cost']
    assert n == len(ref_cost) and np.all(np.abs(st['cost'][:n] - ref_cost) <= 8 * 4.6e-13 + (1e-5 if diverged else 1e-9) * np.abs(ref_cost)), (case, n)
    print_ledger(ledger)


def test_split_state_agrees_with_the_layout_of_test_glpso():
    for NP, D in ((100, 10), (5, 3), (65, 33)):
        blk = np.arange(gx.state_doubles(NP, D, 50), dtype=np.float64)
        a, b = gx.split_state(blk, D, 50, NP), split_state_glpso(blk, D, 50, NP)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        assert a['cost'][-1] == blk[-1]


# ------------------------------------------------------------------------------------------------ CPU: the judge has teeth
@pytest.mark.parametrize('NP,D', PLANT_SHAPES)
def test_stand_in_passes_every_planted_state(NP, D):
    for name in PLANTED:
        S = _run_planted(name, NP, D, StandIn)
        rep = S.total()
        assert rep['undecided'] == [] and rep['ambiguous'] == 0, (name, rep['undecided'][:8], rep['ambiguous'])
        print(f'planted {name:10s} NP {NP:3d} D {D:2d}: {S.launches} launches, {rep["decisions"]} decisions (+ {rep["self_ties"]} self-ties), worst cost error / allowance {rep["worst"]:.3g}, '
              f'events {sorted(rep["events"])}')


def _rejected_by(defect, NP, D):
    out = {}
    for name in PLANTED:
        try:
            _run_planted(name, NP, D, lambda cfgs, pidx: StandIn(cfgs, pidx, defect))
        except gx.Rejected as e:
            out[name] = e.args
    return out


@pytest.mark.parametrize('defect', sorted(gx.DEFECTS))
def test_every_defect_is_rejected_by_its_planted_state(defect):
    for NP, D in PLANT_SHAPES:
        hit = _rejected_by(defect, NP, D)
        print(f'{defect:18s} NP {NP:3d} D {D:2d}: rejected by {sorted(hit)}')
        for name in WITNESS[defect]:
            assert name in hit, (defect, NP, D, name, 'did not reject; rejected by', sorted(hit))
            print(f'    {name}: {str(hit[name])[:200]}')


def test_the_merged_bounce_is_the_same_function():
    """`where(a | b, v * -0.5, v)` for the two `where`s of :127-128: x + v cannot exceed ub and fall below lb at once, so no state tells them apart."""
    assert set(gx.EQUIVALENT) == {'bounce_merged'}
    for NP, D in PLANT_SHAPES:
        assert _rejected_by('bounce_merged', NP, D) == {}


# ------------------------------------------------------------------------------------------------ the walks (CPU stand-in and device)
def _walk_cfgs(NP, D):
    max_fes = 6 * NP + 17
    if D == 12:
        from test_protein import protein
        byid, tr, _, _ = protein()
        return [gx.Cfg(byid[k], NP, max_fes, max_fes // NLOG, NLOG, protein=True) for k in tr[:2]]      # two docking instances: their allowance costs 0.25 s a call
    return [gx.Cfg(p, NP, max_fes, max_fes // NLOG, NLOG) for p in parity.edge_problems(D)]


def _walk(NP, D, make):
    """The nine instances in one batch created in permuted order: counters planted before the reset (0 .. 9, so that tournaments fire inside three generations), the
    reset, then generations to the end of the budget (the last one overshoots it) and one launch past it.  -> (session, cfgs in batch order)."""
    cfgs = _walk_cfgs(NP, D)
    rs = np.random.RandomState(1000 * NP + D)
    perm = rs.permutation(len(cfgs))
    run = make(cfgs, perm)
    S = Session(run)
    try:
        for k in range(run.B):
            blk = run.read(k)
            gx.split_state(blk, D, NLOG, NP)['stag'][:] = rs.randint(0, 10, NP)
            run.write(k, blk)
        S.launch([_rtape(rs, c, True) for c in run.cfgs], reset=True)
        gens = -(-(cfgs[0].max_fes - 2 * NP) // (2 * NP))          # three generations end an episode (8 NP >= 6 NP + 17) from NP = 9 up; five at NP = 4, four at NP = 5
        for _ in range(gens + 1):                                  # the last launch finds every instance frozen
            S.launch([_rtape(rs, c) for c in run.cfgs])
        for k in range(run.B):
            sc = gx.split_state(run.read(k), D, NLOG, NP)['scalars']
            assert sc[gx.SC_DONE] == 1. and sc[gx.SC_FES] <= 2 * NP * (gens + 1) and sc[gx.SC_COST_LEN] <= NLOG + 1, (k, sc[:8])
            assert 'frozen' in S.per[k]['events']
    finally:
        run.close()
    return S, run.cfgs


def _walk_report(S, cfgs, NP, D, who):
    events = set()
    for rep, c in zip(S.per, cfgs):
        und = len(rep['undecided'])
        name = str(c.problem)
        print(f'{who} walk NP {NP:3d} D {D:2d} {name[:28]:28s}: undecided {und} of {rep["decisions"]} decisions (+ {rep["self_ties"]} candidates that are a point the row bred before), ambiguous rows {rep["ambiguous"]}, '
              f'worst cost error / allowance {rep["worst"]:.3g}')
        assert und * 1000 <= rep['decisions'], (NP, D, name, und, rep['decisions'], rep['undecided'][:8])
        events |= rep['events']
    return events


@pytest.mark.parametrize('NP,D', SHAPES)
def test_stand_in_walks_stay_under_the_undecided_cap(NP, D):
    S, cfgs = _walk(NP, D, StandIn)
    _walk_report(S, cfgs, NP, D, 'stand-in')


def test_stand_in_walks_see_every_event():
    seen = set()
    for NP, D in [(4, 2), (63, 7)]:
        S, cfgs = _walk(NP, D, StandIn)
        seen |= S.total()['events']
    assert EVENTS <= seen, EVENTS - seen


# ------------------------------------------------------------------------------------------------ GPU
_seen_on_device = {}


@pytest.mark.gpu
@pytest.mark.parametrize('NP,D', SHAPES)
def test_hip_glpso_edge_geometries_against_the_exact_restatement(NP, D):
    from metabox_amd._abi import MbxError
    try:
        S, cfgs = _walk(NP, D, Device)
    except MbxError as e:
        assert f'mbx error {MBX_E_UNSUPPORTED}:' in str(e) and 'LDS' in str(e), str(e)
        assert (NP, D) not in MUST_RUN, ('refused', NP, D, str(e))
        return
    _seen_on_device[(NP, D)] = _walk_report(S, cfgs, NP, D, 'device') | S.total()['events']


@pytest.mark.gpu
def test_hip_glpso_edge_sweep_saw_every_event():
    """Over the shapes that ran: a tournament, a mutation, a bounce at each bound, a velocity clamp, a gbest improvement that moved gbest_position."""
    if set(_seen_on_device) != set(MUST_RUN):                       # run alone: redo the sweep
        for NP, D in MUST_RUN:
            if (NP, D) not in _seen_on_device:
                _seen_on_device[(NP, D)] = _walk(NP, D, Device)[0].total()['events']
    assert set(_seen_on_device) == set(MUST_RUN)
    seen = set().union(*_seen_on_device.values())
    assert EVENTS <= seen, EVENTS - seen


@pytest.mark.gpu
@pytest.mark.parametrize('NP,D', PLANT_SHAPES)
@pytest.mark.parametrize('name', sorted(PLANTED))
def test_hip_glpso_planted_states(name, NP, D):
    S = _run_planted(name, NP, D, Device)
    rep = S.total()
    print(f'device planted {name:10s} NP {NP:3d} D {D:2d}: {S.launches} launches, {rep["decisions"]} decisions, undecided {len(rep["undecided"])} (+ {rep["self_ties"]}), '
          f'worst cost error / allowance {rep["worst"]:.3g}')
    assert rep['undecided'] == [] and rep['ambiguous'] == 0, (name, rep['undecided'][:8], rep['ambiguous'])


@pytest.mark.gpu
@pytest.mark.parametrize('NP,D', [(5, 3), (65, 33), (256, 10)])
def test_hip_glpso_philox_equals_tape_at_edge_shapes(NP, D):
    """The Philox route against the tape rebuilt on the host from oracle.philox (test_glpso.philox_tape), reset + six generations, on the noiseless and the
    uniform-noise instance: every state word and the results.  (The normal-noise kinds stay out: the host cannot rebuild the device's log / cos.)"""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = {**problems('bbob', D), **problems('bbob-noisy', D)}
    ids = [15, 102]
    s = Suite([ps[i] for i in ids])
    seeds = np.array([123456789012345, 987654321], dtype=np.uint64)
    a = Batch(s, ALGO_GLPSO, np.arange(2), seeds, NP, 2000 * D, 40 * D, 50)
    t = Batch(s, ALGO_GLPSO, np.arange(2), seeds, NP, 2000 * D, 40 * D, 50)
    for g in range(7):
        tape = np.stack([philox_tape(int(seeds[k]), D, ps[ids[k]].noise[0], g, NP=NP) for k in range(2)])
        t.set_tape(torch.from_numpy(tape).cuda())
        if g == 0:
            a.reset(); t.reset()
        else:
            a.step(None); t.step(None)
        torch.cuda.synchronize()
        for k in range(2):
            sa, st = a.read_state(k), t.read_state(k)
            assert np.array_equal(sa, st), (ids[k], g, int(np.argmax(sa != st)))
    ra, rt = a.results(), t.results()
    for key in ('cost', 'fes', 'cost_len'):
        assert torch.equal(ra[key], rt[key]), key
    a.close(); t.close(); s.close()
