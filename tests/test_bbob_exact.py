"""BBOB / noisy-BBOB objectives against an extended-precision reference (tests/bbob_exact.py) on the kernel routes that evaluate them.

CPU: the restatement reproduces the reference's own outputs (bbob_kat.npz, bbob_noise.npz); the allowance is calibrated on the C oracle over all 54
functions at D in {2, 3, 5, 7, 10, 16, 17, 30, 31, 40, 64} on adversarial candidates (xopt and ulps around it, the 1e-8 threshold, the box faces,
z = 0 components, Step-Ellipsoid edges, Gallagher peaks); float64 evaluations with one deliberate defect each are rejected; the generator's edge
candidates are where it says.  GPU: mbx_eval (block form) at every D and at row counts around the block sizes, with and without noise draws; RLEPSO
planted swarms through the per-generation and resident kernels of every geometry (all 24 per-kind bodies); LDE, GLEET, RL-PSO, QLPSO, DE and PSO
on natural episodes; the block form against a planted swarm on the same candidates.
"""
import functools
import time

import numpy as np
import pytest

import bbob_exact as be
from helpers import load, problems
from oracle import oracle

DIMS = (2, 3, 5, 7, 10, 16, 17, 30, 31, 40, 64)
NLOG = 5


def _ps(suite, D):
    ps = problems(suite, D)
    return [ps[i] for i in sorted(ps)]


@functools.lru_cache(maxsize=None)
def _adv(suite, D):
    rs = np.random.RandomState(1000 + D + (0 if suite == 'bbob' else 7))
    return [be.adversarial(p, rs) for p in _ps(suite, D)]


def _ratio(allow, namb, ex, got):
    r = np.abs(np.asarray(got, dtype=be.LD) - ex).astype(np.float64) / allow
    return r, namb > 0


# ------------------------------------------------------------------------------------------------ CPU
def test_restatement_is_the_reference_kat():
    """Every value of bbob_kat.npz (the reference's numpy, float64) lies within the allowance of exact()."""
    kat = load('bbob_kat.npz')
    worst, n = 0., 0
    for suite in ('bbob', 'bbob-noisy'):
        for D in (10, 30, 40):
            X = kat[f'x/{D}']
            for p in _ps(suite, D):
                allow, namb, ex = be.allowance(p, X)
                r, amb = _ratio(allow, namb, ex, kat[f'f/{suite}/{D}/{p.func_id}'].astype(be.LD) - be.LD(p.bias))
                assert np.all(r <= 1), (suite, D, p.func_id, r.max())
                worst, n = max(worst, float(r[~amb].max(initial=0))), n + len(r)
    print(f'reference KAT: {n} values, worst error / allowance {worst:.3f}')


def test_restatement_is_the_reference_noise():
    """bbob_noise.npz with the fixture's own draws: the noisy reference values within the allowance of exact(draws=...)."""
    nz = load('bbob_noise.npz')
    worst, namb_tot, n = 0., 0, 0
    for D in (10, 30):
        X = nz[f'x/{D}']
        for p in _ps('bbob-noisy', D):
            for seed in (0, 1):
                draws = oracle.NumpyTapeFeeder(seed, len(X), D, p.noise[0])._noise_rows().reshape(3, -1)
                allow, namb, ex = be.allowance(p, X, draws)
                r, amb = _ratio(allow, namb, ex, nz[f'f/{D}/{p.func_id}/{seed}'].astype(be.LD) - be.LD(p.bias))
                assert np.all(r <= 1), (D, p.func_id, seed, r.max())
                worst, namb_tot, n = max(worst, float(r[~amb].max(initial=0))), namb_tot + int(amb.sum()), n + len(r)
            xo = np.stack([p.opt, p.opt + 1e-7])
            draws = oracle.NumpyTapeFeeder(5, 2, D, p.noise[0])._noise_rows().reshape(3, -1)
            allow, namb, ex = be.allowance(p, xo, draws)
            r, _ = _ratio(allow, namb, ex, nz[f'fopt/{D}/{p.func_id}'].astype(be.LD) - be.LD(p.bias))
            assert np.all(r <= 1), (D, p.func_id, 'xopt', r)
    print(f'reference noise: {n} values, worst error / allowance {worst:.3f}, {namb_tot} on the 1e-8 threshold')


def test_allowance_calibrated_on_the_oracle():
    """The C oracle on the adversarial set of all 54 functions at every D: within half of the allowance for every kind (non-ambiguous
    candidates); ambiguous ones within the allowance."""
    t0 = time.time()
    worst, med, n, namb_tot = {}, [], 0, 0
    for suite in ('bbob', 'bbob-noisy'):
        for D in DIMS:
            for p, X in zip(_ps(suite, D), _adv(suite, D)):
                allow, namb, ex = be.allowance(p, X)
                got = oracle.evaluate(p.desc(), X).astype(be.LD) - be.LD(p.bias)
                r, amb = _ratio(allow, namb, ex, got)
                assert np.all(r <= 1), (suite, D, p.func_id, r.max())
                worst[p.kind] = max(worst.get(p.kind, 0.), float(r[~amb].max(initial=0)))
                c = np.abs(ex.astype(np.float64))
                ok = c > 0
                med.extend(allow[ok] / np.spacing(c[ok]))
                n, namb_tot = n + len(X), namb_tot + int(amb.sum())
    for kind in sorted(worst):
        print(f'  kind {kind:2d}: oracle worst error / allowance {worst[kind]:.3f}')
    print(f'oracle: {n} candidates ({namb_tot} ambiguous), median allowance {np.median(med):.0f} ulp of the cost, {time.time() - t0:.0f} s')
    assert max(worst.values()) <= 0.5, worst


def test_noise_models_calibrated_on_the_oracle():
    """oracle.apply_noise with random draws on the noisy suite's adversarial sets (costs near the 1e-8 threshold included)."""
    rs = np.random.RandomState(5)
    worst, namb_tot = 0., 0
    for D in (2, 10, 31):
        for p, X in zip(_ps('bbob-noisy', D), _adv('bbob-noisy', D)):
            m = len(X)
            draws = np.stack([rs.uniform(0, 1, m), rs.uniform(0, 1, m) if p.noise[0] != 1 else rs.normal(size=m), rs.normal(size=m)])
            if p.noise[0] == 1:
                draws[0] = rs.normal(size=m)
            ftrue = oracle.evaluate(p.desc(), X)
            got = oracle.apply_noise(p.desc(), p.bias, ftrue, draws).astype(be.LD) - be.LD(p.bias)
            allow, namb, ex = be.allowance(p, X, draws)
            r, amb = _ratio(allow, namb, ex, got)
            assert np.all(r <= 1), (D, p.func_id, r.max())
            worst, namb_tot = max(worst, float(r[~amb].max(initial=0))), namb_tot + int(amb.sum())
    print(f'noise models: worst error / allowance {worst:.3f}, {namb_tot} ambiguous at the threshold')
    assert worst <= 0.5
    assert namb_tot > 0


STAGES = {
    'maps32': [k for k in range(1, 25) if k not in (5, 20)],
    'acc32': [k for k in range(1, 25) if k not in (5, 20)],
    'trans': [2, 3, 4, 6, 10, 11, 15, 16, 21, 22],
    'osz32': [2, 3, 4, 6, 10, 11, 15, 16, 21, 22],
}


@pytest.mark.parametrize('defect', sorted(STAGES))
def test_checker_rejects_a_defective_float64_evaluation(defect):
    """The same formula in float64 is inside the allowance; with one defect it is rejected on at least one candidate of every kind that has the
    affected stage (maps / shift in float32, exp off by 1 + 2^-40, a float32 matvec accumulator, the T_osz constants in float32)."""
    caught = set()
    for D in (10, 17):
        for p, X in zip(_ps('bbob', D), _adv('bbob', D)):
            allow, namb, ex = be.allowance(p, X)
            ok, _ = _ratio(allow, namb, ex, be.float64_eval(p, X))
            assert np.all(ok <= 1), (p.func_id, D, ok.max())
            r, amb = _ratio(allow, namb, ex, be.float64_eval(p, X, defect=defect))
            if np.any(r[~amb] > 1):
                caught.add(p.kind)
    missed = sorted(set(STAGES[defect]) - caught)
    print(f'defect {defect}: rejected on kinds {sorted(caught)}')
    assert not missed, (defect, missed)


def test_generator_edges_are_where_it_says():
    """Step-Ellipsoid candidates lie within 64 ulp (of 0.5) of their edge in exact arithmetic; the F7 / F113-F115 sets and the threshold rays
    give ambiguous candidates; xopt itself costs exactly 0 (up to the longdouble rounding of the maps)."""
    rs = np.random.RandomState(3)
    n7, amb7, ambt = 0, 0, 0
    for D in (5, 10, 30):
        for p in _ps('bbob', D) + _ps('bbob-noisy', D):
            if p.kind == 7:
                X, comp, tgt = be.step_edge_points(p, rs)
                d = p.desc()
                M = np.asarray(d['m1'], dtype=np.float64).reshape(D, D).astype(be.LD)
                zh = (X.astype(be.LD) - np.asarray(d['dshift']).astype(be.LD)) @ M.T
                dist = np.abs(zh[np.arange(len(X)), comp] - tgt)
                assert np.all(dist <= 64 * 2.0 ** -53), dist.astype(np.float64)
                _, namb, _ = be.allowance(p, X)
                n7, amb7 = n7 + len(X), amb7 + int((namb > 0).sum())
            if p.func_id in (1, 101):
                X = be.threshold_rays(p, rs)
                ex = be.exact(p, X)
                assert np.all(np.abs(ex.astype(np.float64) - 1e-8) <= 1e-8 * 1e-4), ex
                draws = np.stack([np.full(len(X), 0.5)] * 3)
                _, namb, _ = be.allowance(p, X, draws)
                ambt += int((namb > 0).sum())
            e0 = be.exact(p, p.opt[None])[0]
            assert abs(float(e0)) <= 1e-13, (p.func_id, float(e0))
    print(f'step-ellipsoid edges: {n7} candidates, {amb7} ambiguous; threshold rays: {ambt} ambiguous')
    assert amb7 > 0 and ambt > 0


# ------------------------------------------------------------------------------------------------ GPU
class Checker:
    """Stored (position, cost) pairs against the exact cost; remembers what it has judged (keyed by problem and position bits)."""

    def __init__(self, label):
        self.label, self.worst, self.n, self.n_amb, self._seen = label, 0., 0, 0, {}
        self.ulps = []

    def __call__(self, p, X, f, draws=None):
        X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
        f = np.asarray(f, dtype=np.float64).ravel()
        if draws is not None:                           # each row has its own draws: judged as they come, not cached
            keys = list(range(len(X)))
            allow, namb, ex = be.allowance(p, X, draws)
            seen = {k: (ex[k], allow[k], namb[k]) for k in keys}
        else:
            keys = [(str(p), p.func_id, x.tobytes()) for x in X]
            new = [k for k, key in enumerate(keys) if key not in self._seen]
            if new:
                allow, namb, ex = be.allowance(p, X[new])
                for t, k in enumerate(new):
                    self._seen[keys[k]] = (ex[t], allow[t], namb[t])
            seen = self._seen
        for k, key in enumerate(keys):
            ex, allow, namb = seen[key]
            r = float(abs(be.LD(f[k]) - ex) / be.LD(allow))
            assert r <= 1., (self.label, str(p), p.func_id, k, X[k].tolist(), f[k], float(ex), allow, int(namb))
            if namb:
                self.n_amb += 1
            else:
                self.worst = max(self.worst, r)
            if ex != 0:
                self.ulps.append(allow / np.spacing(abs(float(ex))))
        self.n += len(X)

    def report(self):
        med = f', median allowance {np.median(self.ulps):.0f} ulp' if self.ulps else ''
        print(f'{self.label}: {self.n} (position, cost) pairs, worst error / allowance {self.worst:.3f}, {self.n_amb} ambiguous{med}')


class NoiseFree:
    """A noisy problem with the noise model switched off (desc()['noise_kind'] = none): the algorithm routes evaluate its core."""

    def __init__(self, p):
        self.p, self.dim, self.bias, self.lb, self.ub, self.opt, self.func_id, self.kind = p, p.dim, p.bias, p.lb, p.ub, p.opt, p.func_id, p.kind
        self.noise = (0, 0., 0.)

    def desc(self):
        d = dict(self.p.desc())
        d['noise_kind'] = 0
        return d

    def __str__(self):
        return f'{self.p}-noise-free'


def _suite(ps):
    from metabox_amd.suite import Suite
    return Suite(ps)


@pytest.mark.gpu
def test_mbx_eval_block_form_within_allowance():
    """Both suites at every D on the adversarial set (noisy=False), the row counts 1 ... 257 spread over the problems (D = 64 halves the rows per
    block), and the noisy path with known draws."""
    t0 = time.time()
    chk, chkn = Checker('mbx_eval (noise-free core)'), Checker('mbx_eval (noise draws)')
    counts = (1, 2, 3, 63, 64, 65, 127, 128, 129, 257)
    rs = np.random.RandomState(11)
    for suite in ('bbob', 'bbob-noisy'):
        for D in DIMS:
            ps = _ps(suite, D)
            s = _suite(ps)
            for k, (p, X) in enumerate(zip(ps, _adv(suite, D))):
                m = counts[(k + D) % len(counts)]
                Xm = np.concatenate([X, rs.uniform(-5, 5, size=(max(0, m - len(X)), D))])[:m] if m < len(X) or m > len(X) else X
                chk(p, X, s.eval(k, X, noisy=False) - p.bias)
                chk(p, Xm, s.eval(k, Xm, noisy=False) - p.bias)
                if suite == 'bbob-noisy':
                    draws = oracle.NumpyTapeFeeder(D + k, len(X), D, p.noise[0])._noise_rows().reshape(3, -1)
                    chkn(p, X, s.eval(k, X, noisy=True, noise_draws=draws) - p.bias, draws)
            s.close()
    chk.report(); chkn.report()
    print(f'mbx_eval: {time.time() - t0:.0f} s')


def _inbox(X):
    return X[np.all(np.abs(X) <= 5., 1)]


def _plant(b, k, NP, D, X):
    """Plant X [m <= NP] (inside the box) as instance k's swarm: velocity 0, pbest = the positions, stagnation counters 0."""
    m = len(X)
    P = np.concatenate([X, np.repeat(X[:1], NP - m, 0)]) if m < NP else X[:NP]
    st = b.read_state(k)
    lay = oracle.split_rlepso_state(st, NP, D, NLOG)
    lay['pos'][:] = P.ravel(); lay['pbpos'][:] = P.ravel(); lay['vel'][:] = 0.; lay['pni'][:] = 0.
    b.write_state(k, st)
    return P


def _planted_batch(ps, NP, flags=0):
    from metabox_amd._abi import ALGO_RLEPSO
    from metabox_amd.suite import Batch
    s = _suite(ps)
    B = len(ps)
    b = Batch(s, ALGO_RLEPSO, np.arange(B), np.arange(B, dtype=np.uint64) + 3, NP, 100000, 20000, NLOG, flags=flags)
    b.reset()
    return s, b


def _read_planted(chk, b, ps, planted, NP, D):
    for k, p in enumerate(ps):
        out = oracle.split_rlepso_state(b.read_state(k), NP, D, NLOG)
        assert np.array_equal(out['pos'], planted[k].ravel()) and out['scalars'][oracle.SC_REINIT] == 0, (k, str(p))
        chk(p, planted[k], out['ccost'])


def _rlepso_sets(D, NP, suite='bbob'):
    ps = [p if p.noise[0] == 0 else NoiseFree(p) for p in _ps(suite, D)]
    rs = np.random.RandomState(D)
    Xs = []
    for p, X in zip(ps, _adv(suite, D)):
        X = _inbox(X)
        Xs.append(np.concatenate([X, rs.uniform(-5, 5, size=(max(0, NP - len(X)), D))])[:NP])
    return ps, Xs


@pytest.mark.gpu
@pytest.mark.parametrize('D,NP,geom,flags', [(10, 100, 1, 0), (30, 100, 7, 0), (40, 128, 2, 0), (10, 100, 0, 'generic'), (5, 100, 0, 0),
                                             (7, 100, 0, 0)])
def test_rlepso_per_generation_planted(D, NP, geom, flags):
    """mbx_rlepso step (one launch per generation) with the all-zero action on planted swarms of every function (noisy ones noise-free)."""
    import torch
    from metabox_amd import _abi
    fl = _abi.F_GENERIC_GEOMETRY if flags == 'generic' else 0
    chk = Checker(f'rlepso per generation D{D} NP{NP} geometry {geom}')
    for suite in ('bbob', 'bbob-noisy'):
        ps, Xs = _rlepso_sets(D, NP, suite)
        s, b = _planted_batch(ps, NP, fl)
        assert b.launch_info()['fixed_geometry'] == geom
        planted = [_plant(b, k, NP, D, X) for k, X in enumerate(Xs)]
        b.step(torch.zeros(b.B, 35, dtype=torch.float32, device='cuda'))
        _read_planted(chk, b, ps, planted, NP, D)
        b.close(); s.close()
    chk.report()


@pytest.mark.gpu
@pytest.mark.parametrize('D,NP,geom,fast', [(10, 100, 1, False), (10, 100, 1, True), (30, 100, 7, False), (40, 128, 2, False), (40, 128, 2, True),
                                            (40, 100, 10, False)])
def test_rlepso_resident_planted(D, NP, geom, fast):
    """k_rlepso_run on every geometry (and both FDR_FAST forms) with a policy table of zeros, on batches holding all 24 kinds: every per-kind
    body evaluates its planted swarm."""
    import torch
    from metabox_amd import _abi
    chk = Checker(f'rlepso resident D{D} NP{NP} geometry {geom}{" fdr-fast" if fast else ""}')
    ps, Xs = _rlepso_sets(D, NP)
    s, b = _planted_batch(ps, NP, _abi.F_FDR_FAST if fast else 0)
    assert b.launch_info()['fixed_geometry'] == geom and b.rollout_is_resident()
    assert bool(b.flags & _abi.F_FDR_FAST) == fast
    planted = [_plant(b, k, NP, D, X) for k, X in enumerate(Xs)]
    rows = int(b.lib.mbx_rlepso_policy_table_rows(b._h))
    table = torch.zeros(rows, 2, 35, dtype=torch.float32, device='cuda')
    b.rlepso_rollout(table, 1)
    _read_planted(chk, b, ps, planted, NP, D)
    b.close(); s.close()
    chk.report()


@pytest.mark.gpu
def test_block_form_and_planted_swarm_agree_within_allowance():
    """The same candidates through mbx_eval and a planted RLEPSO swarm (geometries 1 and 7): both within the allowance; the largest
    disagreement in ulps is printed, not asserted."""
    import torch
    chk, ulps = Checker('cross-route'), 0.
    for D, NP in ((10, 100), (30, 100)):
        ps, Xs = _rlepso_sets(D, NP)
        s, b = _planted_batch(ps, NP)
        planted = [_plant(b, k, NP, D, X) for k, X in enumerate(Xs)]
        b.step(torch.zeros(b.B, 35, dtype=torch.float32, device='cuda'))
        for k, p in enumerate(ps):
            fw = oracle.split_rlepso_state(b.read_state(k), NP, D, NLOG)['ccost'].copy()
            fb = s.eval(k, planted[k], noisy=False) - p.bias
            chk(p, planted[k], fw); chk(p, planted[k], fb)
            ulps = max(ulps, float((np.abs(fw - fb) / np.spacing(np.maximum(np.abs(fb), 1e-300))).max()))
        b.close(); s.close()
    print(f'block form vs planted swarm: largest disagreement {ulps:.0f} ulp')
    chk.report()


def _pairs(algo, st, NP, D):
    from metabox_amd import _abi
    if algo == _abi.ALGO_LDE:
        t = oracle.split_lde_state(st, NP, D, NLOG); return [(t['pop'], t['fit'])]
    if algo == _abi.ALGO_GLEET:
        t = oracle.split_gleet_state(st, NP, D, NLOG); return [(t['pos'], t['ccost']), (t['pbpos'], t['pbest'])]
    if algo == _abi.ALGO_RLPSO:
        t = oracle.split_rlpso_state(st, NP, D, NLOG); return [(t['pos'], t['ccost']), (t['pbpos'], t['pbest'])]
    if algo == _abi.ALGO_QLPSO:
        t = oracle.split_qlpso_state(st, NP, D, NLOG); return [(t['pop'], t['cost'])]
    if algo == _abi.ALGO_DE:
        return [(st[:NP * D], st[NP * D:NP * D + NP])]
    if algo == _abi.ALGO_PSO:
        return [(st[2 * NP * D:3 * NP * D], st[3 * NP * D:3 * NP * D + NP])]
    return []


@pytest.mark.gpu
@pytest.mark.parametrize('name,D,NP,geom,generic', [('lde', 10, 50, 9, False), ('lde', 30, 50, 3, False), ('lde', 30, 100, 6, False),
                                                    ('lde', 10, 50, 0, True), ('gleet', 10, 100, 5, False), ('gleet', 10, 100, 0, True),
                                                    ('rlpso', 10, 100, 0, False), ('qlpso', 10, 100, 0, False), ('de', 10, 50, 0, False),
                                                    ('pso', 10, 50, 0, False)] +
                         # edge geometries (tests/test_gpu_geometry_edges.py): NP D odd at 63 x 7 and 65 x 33, more than one wave, the widest rows
                         [(name, D, NP, 0, False) for name in ('lde', 'gleet', 'rlpso', 'qlpso', 'de', 'pso') for NP, D in ((63, 7), (65, 33), (100, 40))])
def test_other_optimizers_natural_episodes(name, D, NP, geom, generic):
    """Every stored (position, cost) pair after the reset and after each of five generations, on all 24 kinds plus the noisy suite's
    functions with the noise switched off."""
    import torch
    from metabox_amd import _abi
    from metabox_amd.suite import Batch
    algo = {'lde': _abi.ALGO_LDE, 'gleet': _abi.ALGO_GLEET, 'rlpso': _abi.ALGO_RLPSO, 'qlpso': _abi.ALGO_QLPSO, 'de': _abi.ALGO_DE,
            'pso': _abi.ALGO_PSO}[name]
    ps = _ps('bbob', D) + [NoiseFree(p) for p in _ps('bbob-noisy', D)]
    s = _suite(ps)
    B = len(ps)
    b = Batch(s, algo, np.arange(B), np.arange(B, dtype=np.uint64) * 5 + 2, NP, 100000, 20000, NLOG,
              flags=_abi.F_GENERIC_GEOMETRY if generic else 0)
    assert b.launch_info()['fixed_geometry'] == geom, b.launch_info()
    chk = Checker(f'{name} D{D} NP{NP} geometry {geom}')
    rs = np.random.RandomState(4)
    b.reset()
    for g in range(6):
        for k in range(B):
            for X, f in _pairs(algo, b.read_state(k), NP, D):
                chk(ps[k], X.reshape(NP, D), f)
        if g == 5:
            break
        if b.action_dim == 0:
            a = None
        elif algo == _abi.ALGO_QLPSO:
            a = torch.from_numpy(rs.randint(0, 4, size=(B, b.action_dim)).astype(np.int32)).cuda()
        else:
            a = torch.from_numpy(rs.uniform(0, 1, size=(B, b.action_dim)).astype(np.float32)).cuda()
        b.step(a)
    chk.report()
    b.close(); s.close()
