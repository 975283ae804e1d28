"""DEAP_CMAES generations against the extended-precision restatement of deap.cma.Strategy (tests/cmaes_exact.py).

CPU: the C oracle on every planted state (cmaes_exact's docstring lists what is judged) and on 20-generation episodes at D = 2, 10 and 40,
with the eigendecomposition checks on its B and diagD; a plain float64 strategy passes on the planted set while each deliberate defect is
rejected.  GPU: k_cmaes_generation on the same planted states at D in {2, 3, 10, 31, 40} x NP in {4, 5, 50, 51, 256 where the LDS admits
it}, at the largest D the library admits for NP = 4, 50 and 256 (D + 1 refused), on a finished instance, and on natural episodes judged
generation by generation from the kernel's own previous state.
"""
import time

import numpy as np
import pytest

import bbob_exact as be
import cmaes_exact as ce
from helpers import problems
from oracle import oracle

ALGO = 10
NLOG = 50
MAXFES = 10 ** 7
LOGI = 400
FUNCS = (1, 2, 8, 10, 11, 12, 15, 21)


def _probs(D):
    ps = problems('bbob', D)
    return {f: ps[f] for f in FUNCS + (7,)}


def _rot(rs, D):
    Q, Rm = np.linalg.qr(rs.normal(size=(D, D)))
    return Q * np.sign(np.diag(Rm))[None, :]


def _spectral(D, lam, rs):
    """C = Q diag(lam) Q^T (longdouble, then rounded, mirrored to exact symmetry), B = Q with ascending lam, diagD = sqrt(lam)."""
    lam = np.sort(np.asarray(lam, dtype=np.float64))
    Q = _rot(rs, D)
    C = (Q.astype(be.LD) * lam.astype(be.LD)[None, :]) @ Q.T.astype(be.LD)
    C = np.triu(C.astype(np.float64))
    C = C + np.triu(C, 1).T
    return C, Q, np.sqrt(lam)


def _step_cell_centroid(p, rs):
    """A point whose Step-Ellipsoid z_hat = M1 (x - shift) has every component at +-1 (the middle of a step cell), inside the box."""
    d = p.desc()
    D = p.dim
    M = np.asarray(d['m1'], dtype=np.float64).reshape(D, D)
    sh = np.asarray(d['dshift'], dtype=np.float64)
    best = None
    for _ in range(400):
        z = rs.choice([-1., 1.], size=D)
        x = (be._solve(M.astype(be.LD), z[None])[0] + sh.astype(be.LD)).astype(np.float64)
        m = np.max(np.abs(x))
        if best is None or m < best[0]:
            best = (m, x)
        if m < 4.5:
            break
    return best[1]


def planted(D, NP, light=False):
    """[(name, problem, state block, seed)] of one geometry (cmaes_exact's layout).  light: the reset state and three spectra only."""
    rs = np.random.RandomState(1000 * D + NP)
    ps = _probs(D)
    ub = 5.0
    I = np.eye(D)
    sc_base = dict(gbest=1e3, fes=1000., log_index=1, cost_len=1, gen=7, episode=2, sigma=0.5, updates=10)
    cases = []
    fi = iter(FUNCS * 8)

    def add(name, cen, C, B, dD, ps_=None, pc=None, f=None, **kw):
        sc = dict(sc_base)
        sc.update(kw)
        st = ce.join(D, NLOG, cen, C, B, dD, np.zeros(D) if ps_ is None else ps_, np.zeros(D) if pc is None else pc, ce.scalars(**sc),
                     [sc['gbest']] if sc['cost_len'] else None)
        cases.append((name, ps[f if f is not None else next(fi)], st, 17 + len(cases)))

    add('reset', np.full(D, ub), I, I, np.ones(D), gbest=np.inf, fes=0., log_index=0, cost_len=0, gen=0, episode=1, updates=0)
    spectra = {'cond1': np.ones(D), 'cond1e3': np.logspace(-3, 0, D), 'cond1e8': np.logspace(-8, 0, D), 'cond1e12': np.logspace(-12, 0, D),
               'cond1e14': np.logspace(-14, 0, D)}
    spectra['half_equal'] = np.where(np.arange(D) < D // 2, 0.3, np.logspace(-2, 0, D))
    spectra['all_equal'] = np.full(D, 2.5)
    tiny = np.logspace(-4, 0, D)
    tiny[0] = 0.5 * be.U
    spectra['tiny'] = tiny
    keep = ('cond1e3', 'cond1e12', 'tiny') if light else tuple(spectra)
    for name in keep:
        C, B, dD = _spectral(D, spectra[name], rs)
        add(name, rs.uniform(-2, 2, D), C, B, dD, ps_=rs.normal(size=D) * 0.3, pc=rs.normal(size=D) * 0.1)
    if light:
        return cases
    C, B, dD = _spectral(D, np.logspace(-3, 0, D), rs)
    cen = rs.uniform(-2, 2, D)
    chiN = np.sqrt(D) * (1. - 1. / (4. * D) + 1. / (21. * D * D))
    v = rs.normal(size=D)
    v /= np.linalg.norm(v)
    add('hsig1', cen, C, B, dD, ps_=np.zeros(D), pc=rs.normal(size=D) * 0.1, updates=10)
    add('hsig0', cen, C, B, dD, ps_=40 * chiN * v, pc=rs.normal(size=D) * 0.1, updates=10)
    add('count0', cen, C, B, dD, ps_=v * 0.5, updates=0)
    add('count1', cen, C, B, dD, ps_=v * 0.5, updates=1)
    add('count10000', cen, C, B, dD, ps_=v * 0.5, updates=10000)
    add('sigma1e-8', cen, C, B, dD, sigma=1e-8)
    add('sigma1e3', cen, C, B, dD, sigma=1e3)
    add('near_xopt', ps[1].opt + rs.normal(size=D) * 1e-5, I, I, np.ones(D), f=1, sigma=1e-5, gbest=1e-3)
    add('far_outside', np.full(D, 40.), C, B, dD, f=8)
    add('ties', _step_cell_centroid(ps[7], rs), I, I, np.ones(D), f=7, sigma=1e-7)
    # hsig at its edge: ps_before = a v with |ps_after| exactly at the threshold (in longdouble), v along this generation's own step
    name, p, st, seed = next(c for c in cases if c[0] == 'hsig1')
    out = ce.restate(p.desc(), st, seed + 1000, NP, D, MAXFES, LOGI, NLOG)
    if out['decided']:
        P = out['ps'].v                                                          # ps_after for ps_before = 0
        s = ce.split(st, D)
        prm = out['params']
        cs = prm['cs'].v
        den = np.sqrt(1 - (1 - cs) ** (2 * (s['sc'][ce.SC_UPDATES] + 1)))
        thr = be.LD('1.4') + be.LD(2) / (D + 1)
        target = thr * prm['chiN'].v * den
        nP = np.sqrt((P * P).sum())
        a = (target - nP) / (1 - cs)
        ps_b = (a * P / nP).astype(np.float64)
        st2 = st.copy()
        st2[D + 2 * D * D + D:D + 2 * D * D + 2 * D] = ps_b
        cases.append(('hsig_edge', p, st2, seed + 1000))
    return cases


def _oracle_gen(p, st, seed, NP, D, max_fes=MAXFES):
    o = oracle.ClassicOracle(p.desc(), p.bias, oracle.make_cfg(ALGO, NP, D, max_fes, LOGI, NLOG), seed=int(seed))
    o.reset()
    o.set_cma_state(st)
    assert np.array_equal(o.cma_state(), st)
    o.step()
    X, c = o.population()
    return o.cma_state(), X, c


def _judge_case(label, p, st0, st1, seed, NP, D, led, worst, X=None, cost=None):
    out = ce.judge(p.desc(), st0, st1, seed, NP, D, MAXFES, LOGI, NLOG, led, X=X, cost=cost, label=label)
    s = ce.split(st1, D)
    ce.eigen_check(s['C'], s['B'], s['diagD'], label=label, worst=worst)
    return out


def _report(led, worst, extra=''):
    print('\n' + led.summary())
    print('  eigen checks, worst fraction of the budget: ' + ', '.join(f'{k} {v:.3g}' for k, v in sorted(worst.items())) + extra)


# ------------------------------------------------------------------------------------------------ CPU
CPU_GEOMS = [(10, 50, False), (3, 5, False), (2, 4, False), (40, 51, False), (31, 50, True), (10, 51, True), (2, 256, True)]


def test_oracle_state_accessors_round_trip():
    p = _probs(10)[1]
    o = oracle.ClassicOracle(p.desc(), p.bias, oracle.make_cfg(ALGO, 50, 10, 20000, 400, 50), seed=3)
    o.reset()
    for _ in range(3):
        o.step()
    st = o.cma_state()
    s = ce.split(st, 10)
    assert s['sc'][ce.SC_FES] == 150 and s['sc'][ce.SC_GEN] == 3 and s['sc'][ce.SC_UPDATES] == 3 and s['sc'][ce.SC_COST_LEN] == 1
    assert s['sc'][ce.SC_SIGMA] == o.result()['sigma'] and s['sc'][ce.SC_GBEST] == o.result()['gbest']
    o2 = oracle.ClassicOracle(p.desc(), p.bias, oracle.make_cfg(ALGO, 50, 10, 20000, 400, 50), seed=3)
    o2.reset()
    o2.set_cma_state(st)
    assert np.array_equal(o2.cma_state(), st)
    o.step()
    o2.step()
    assert np.array_equal(o.cma_state(), o2.cma_state())


def test_restatement_against_the_oracle_on_planted_states():
    t0 = time.time()
    led, worst = ce.Ledger(), {}
    seen = set()
    for D, NP, light in CPU_GEOMS:
        for name, p, st, seed in planted(D, NP, light):
            st1, X, c = _oracle_gen(p, st, seed, NP, D)
            out = _judge_case(f'oracle D={D} NP={NP} {name} {p}', p, st, st1, seed, NP, D, led, worst, X, c)
            if name == 'ties':
                assert out['decided'] and out['ties'] == NP, (D, NP, out['ties'])
                s1 = ce.split(st1, D)
                w = out['params']['w'].v
                want = (w[:, None] * X[:NP // 2].astype(be.LD)).sum(0)          # candidates 0 ... mu-1, index order
                assert np.all(np.abs(s1['centroid'] - want) <= out['centroid'].e), name
            if out.get('hsig') is not None:
                seen.add((name, out['hsig']))
    assert ('hsig0', 0) in seen and ('hsig1', 1) in seen, seen
    _report(led, worst, f'  ({time.time() - t0:.1f} s)')


def test_oracle_done_instance_is_left_alone():
    D, NP = 10, 50
    name, p, st, seed = planted(D, NP, light=True)[1]
    st = st.copy()
    st[ce.state_doubles(D, NLOG) - NLOG - 1 - ce.NSCALAR + ce.SC_DONE] = 1.
    o = oracle.ClassicOracle(p.desc(), p.bias, oracle.make_cfg(ALGO, NP, D, MAXFES, LOGI, NLOG), seed=seed)
    o.reset()
    o.set_cma_state(st)
    assert o.step() is True
    assert np.array_equal(o.cma_state(), st)


@pytest.mark.parametrize('D,funcs', [(2, (1, 8, 15, 21)), (10, (1, 2, 10, 12)), (40, (1, 11))])
def test_restatement_against_oracle_episodes(D, funcs):
    led, worst = ce.Ledger(), {}
    NP = 50
    conds = []
    for f in funcs:
        p = _probs(D)[f]
        cfg = oracle.make_cfg(ALGO, NP, D, MAXFES, LOGI, NLOG)
        o = oracle.ClassicOracle(p.desc(), p.bias, cfg, seed=f + 5)
        o.reset()
        for g in range(20):
            st0 = o.cma_state()
            if o.step():
                break
            X, c = o.population()
            st1 = o.cma_state()
            _judge_case(f'oracle episode D={D} {p} g={g}', p, st0, st1, f + 5, NP, D, led, worst, X, c)
            conds.append(np.linalg.cond(ce.split(st1, D)['C']))
    _report(led, worst, f'; largest cond(C) {max(conds):.3g}')


def test_eigen_budget_calibrated_on_jacobi_and_lapack():
    """p(D) holds with room for the oracle's Jacobi (its Python twin, operation for operation) and numpy.linalg.eigh on the planted spectra,
    made slightly asymmetric the way the kernel's C is."""
    worst = {}
    for D in (2, 3, 10, 31):
        rs = np.random.RandomState(D)
        for lam in (np.logspace(-14, 0, D), np.full(D, 2.5), np.where(np.arange(D) < D // 2, 0.3, np.logspace(-2, 0, D)), np.logspace(-3, 3, D)):
            C, _, _ = _spectral(D, lam, rs)
            C = C * (1 + be.U * rs.choice([-1., 0., 1.], size=C.shape))     # not bit-symmetric
            for B, dD in (ce.jacobi_eigh(C)[::-1], np.linalg.eigh(C)[::-1]):
                with np.errstate(invalid='ignore'):
                    dD = np.sqrt(dD)
                ce.eigen_check(C, B, dD, label=f'D={D}', worst=worst)
    print('\nworst fraction of the p(D) budget:', worst)
    assert max(worst.values()) <= 1 / 3, worst


@pytest.mark.parametrize('defect', (None,) + ce.DEFECTS)
def test_checker_rejects_a_defective_strategy(defect):
    led, worst = ce.Ledger(), {}
    failures = []
    for D, NP in ((10, 50), (3, 5)):
        for name, p, st, seed in planted(D, NP):
            st1, X, c = ce.strategy64(p.desc(), st, seed, NP, D, MAXFES, LOGI, NLOG, defect=defect)
            try:
                _judge_case(f'{defect} D={D} {name}', p, st, st1, seed, NP, D, led, worst, X, c)
            except AssertionError as e:
                failures.append((D, name, str(e)[:160]))
                if defect is None:
                    raise
    if defect is not None:
        assert failures, f'defect {defect} passed every planted case'
        print(f'\n{defect}: rejected on {len(failures)} cases, first {failures[0]}')


# ------------------------------------------------------------------------------------------------ GPU
def _suite(ps):
    from metabox_amd.suite import Suite
    return Suite(ps)


def _run_planted(D, NP, cases, led, worst):
    import torch
    from metabox_amd.suite import Batch
    s = _suite([p for _, p, _, _ in cases])
    seeds = np.array([seed for *_, seed in cases], dtype=np.uint64)
    b = Batch(s, ALGO, np.arange(len(cases)), seeds, NP, MAXFES, LOGI, NLOG)
    b.reset()
    for k, (_, _, st, _) in enumerate(cases):
        b.write_state(k, st)
    _, rew, done = b.step(None)
    torch.cuda.synchronize()
    for k, (name, p, st, seed) in enumerate(cases):
        _judge_case(f'kernel D={D} NP={NP} {name} {p}', p, st, b.read_state(k), seed, NP, D, led, worst)
    assert np.all(rew.cpu().numpy() == 0)
    b.close()
    s.close()


def _admits(D, NP):
    from metabox_amd import _abi
    from metabox_amd.suite import Batch
    p = problems('bbob', D)[1]
    s = _suite([p])
    try:
        Batch(s, ALGO, np.arange(1), np.ones(1, dtype=np.uint64), NP, MAXFES, LOGI, NLOG).close()
        return True
    except _abi.MbxError as e:
        assert 'mbx error -3' in str(e), str(e)
        return False
    finally:
        s.close()


@pytest.mark.gpu
def test_kernel_planted_states_every_geometry():
    t0 = time.time()
    led, worst = ce.Ledger(), {}
    run = []
    for D in (2, 3, 10, 31, 40):
        for NP in (4, 5, 50, 51, 256):
            if NP == 256 and not _admits(D, NP):
                continue
            run.append((D, NP))
            _run_planted(D, NP, planted(D, NP, light=D > 10 and NP not in (5, 50)), led, worst)
    assert (10, 256) in run
    _report(led, worst, f'  geometries {run} ({time.time() - t0:.1f} s)')


@pytest.mark.gpu
def test_kernel_largest_admitted_dimension():
    """The largest D the library admits at NP = 4, 50, 256 (probed on the device: the LDS limit is the device's), one generation there on
    planted states; D + 1 is refused with MBX_E_UNSUPPORTED."""
    led, worst = ce.Ledger(), {}
    limits = {}
    for NP in (4, 50, 256):
        lo, hi = 2, 64
        assert _admits(lo, NP)
        if _admits(hi, NP):
            limits[NP] = hi
        else:
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if _admits(mid, NP):
                    lo = mid
                else:
                    hi = mid
            limits[NP] = lo
            assert not _admits(lo + 1, NP)
        _run_planted(limits[NP], NP, planted(limits[NP], NP, light=True), led, worst)
    print('\nlargest D admitted per NP:', limits)
    assert limits[50] < 50 and limits[4] > limits[50] > limits[256] >= 10, limits
    _report(led, worst)


@pytest.mark.gpu
def test_kernel_done_instance_is_left_alone():
    import torch
    from metabox_amd.suite import Batch
    D, NP = 10, 50
    cases = planted(D, NP, light=True)
    s = _suite([p for _, p, _, _ in cases])
    b = Batch(s, ALGO, np.arange(len(cases)), np.arange(len(cases), dtype=np.uint64) + 3, NP, MAXFES, LOGI, NLOG)
    b.reset()
    sts = []
    for k, (_, _, st, _) in enumerate(cases):
        st = st.copy()
        if k % 2 == 0:
            st[ce.state_doubles(D, NLOG) - NLOG - 1 - ce.NSCALAR + ce.SC_DONE] = 1.
        b.write_state(k, st)
        sts.append(b.read_state(k))                      # as read back: the cost curve comes padded with its last value
    _, rew, done = b.step(None)
    torch.cuda.synchronize()
    rew, done = rew.cpu().numpy(), done.cpu().numpy()
    for k in range(len(cases)):
        if k % 2 == 0:
            assert np.array_equal(b.read_state(k), sts[k]) and rew[k] == 0 and done[k] == 1, k
        else:
            assert not np.array_equal(b.read_state(k), sts[k]) and done[k] == 0, k
    b.close()


@pytest.mark.gpu
def test_kernel_natural_episodes():
    import torch
    from metabox_amd.suite import Batch
    t0 = time.time()
    led, worst = ce.Ledger(), {}
    cond = 0.
    for D, funcs, G in ((10, FUNCS, 30), (2, (1, 8, 15, 21), 30), (40, (1, 11, 15), 8)):
        ps = [_probs(D)[f] for f in funcs]
        s = _suite(ps)
        seeds = np.arange(len(ps), dtype=np.uint64) * 31 + 7
        NP = 50
        b = Batch(s, ALGO, np.arange(len(ps)), seeds, NP, MAXFES, LOGI, NLOG)
        b.reset()
        torch.cuda.synchronize()
        prev = [b.read_state(k) for k in range(len(ps))]
        for g in range(G):
            b.step(None)
            torch.cuda.synchronize()
            for k, p in enumerate(ps):
                cur = b.read_state(k)
                if prev[k][ce.state_doubles(D, NLOG) - NLOG - 1 - ce.NSCALAR + ce.SC_DONE] != 0:
                    assert np.array_equal(cur, prev[k])
                    continue
                _judge_case(f'kernel episode D={D} {p} g={g}', p, prev[k], cur, int(seeds[k]), NP, D, led, worst)
                cond = max(cond, float(np.linalg.cond(ce.split(cur, D)['C'])))
                prev[k] = cur
        b.close()
        s.close()
    _report(led, worst, f'; largest cond(C) {cond:.3g} ({time.time() - t0:.1f} s)')
