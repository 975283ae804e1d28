"""One generation of DEAP_CMAES (deap.cma.Strategy driven by algorithms.eaGenerateUpdate(ngen = 1), src/optimizer/deap_cmaes.py) in
extended precision, and how far a correct float64 kernel may be from it.

The generation is restated from the published deap 1.3.3 equations (cma.Strategy.computeParams / generate / update), not from the oracle
or the kernel, on the `R` arithmetic of tests/bbob_exact.py: every quantity is a longdouble value v with a bound e on |float64 - v| that
holds for ANY float64 evaluation of the same formula (any summation order, with or without fma).  Inputs: a state block in the kernel's
layout (include/mbx_layout.h §10: centroid, C, B, diagD, ps, pc, sigma, update_count, gen, episode) and the instance's Philox seed.  The
stored float64 values are exact inputs.

Derivation of the allowance, stage by stage (u = 2^-53; `Exact` charges its own rules, bbob_exact's docstring):
  * computeParams (lambda_ = NP, mu = NP // 2): w_i = log(mu + 0.5) - log(i), normalised; the two logs are the device's m_log (2 ulp,
    charged 4 u); every sum is a gamma_{n-1} sum; mueff = 1 / sum w^2, cc, cs, ccov1, ccovmu = min(.., 1 - ccov1), damps, chiN with each
    operation rounded once.  The decimal 1.3 and 1.4 are exact reals charged their float64 rounding.
  * generate: arz[i][d] = sqrt(-2 log(1 - ua)) cos(2 pi ub) of Philox(seed, i D + d, MBX_SITE_ELEM_A, gen, episode); 1 - ua is exact
    (ua is a multiple of 2^-53 in [0, 1)), log and cos carry the device library's tested error, 2 pi is charged |fl(2 pi) - 2 pi| ub.
    x_i = centroid + sigma * sum_k arz[i][k] (B[d][k] diagD[k]): one rounded product per term and a D-term dot (gamma_D), then a product and
    a sum.  The kernel's candidate therefore lies within x.e of the exact x; bbob_exact evaluates the cost at an R position, so the cost's
    allowance covers the objective's own roundings AND the displacement of its argument (first order).
  * ranking: deap sorts the population by fitness, best first and stable.  The top mu positions are DECIDED when, for every rank r < mu, the
    cost interval [v - e, v + e] of rank r lies strictly below that of every later candidate; candidates whose exact costs are equal and
    whose evaluation is not ambiguous (a Step-Ellipsoid plateau: the same floored z~ gives bit-identical float64 costs) are an exact tie and
    keep index order.  An undecided generation is counted and its update is not judged (its positions and costs still are).
  * update, with c_diff = centroid_new - centroid_old, each op charged as above:
      ps = (1 - cs) ps + sqrt(cs (2 - cs) mueff) / sigma . B ((1 / diagD) o B^T c_diff)
      hsig = |ps| / sqrt(1 - (1 - cs)^(2 (update_count + 1))) / chiN < 1.4 + 2 / (D + 1)   (m_pow: 3 + |y ln x| ulp).  A decision quantity
          within its bound of the threshold is AMBIGUOUS: pc and C are judged against the branch whose pc the kernel stored, and counted.
      pc = (1 - cc) pc + hsig sqrt(cc (2 - cc) mueff) / sigma . c_diff
      C  = keep C + ccov1 pc pc^T + ccovmu sum_i w_i a_i a_i^T / sigma^2,  a_i = x_(i) - centroid_old,
           keep = 1 - ccov1 - ccovmu + (1 - hsig) ccov1 cc (2 - cc)
      sigma *= exp((|ps| / chiN - 1) cs / damps)   (m_exp: 2 ulp)
  * bookkeeping: gbest = min(previous, min cost) (HallOfFame(1)); its allowance is the largest cost allowance among the candidates that can
    be the minimum.  fes += NP, update_count += 1, gen += 1, then the wrapper's logging and stopping rule (deap_cmaes.py:48-64): a gbest
    within its allowance of the 1e-8 stop threshold makes `done` ambiguous.

Eigendecomposition (`eigen_check`): deap sets diagD, B = eigh(C), sorted ascending, diagD = diagD ** 0.5.  Eigenvectors of clustered
eigenvalues are not unique, so the stored B and diagD are judged against the stored C (which the update check has judged): orthogonality
max |B^T B - I| <= p(D) u, residual max |C B - B diag(diagD^2)| <= p(D) u ||C||_F, ascending diagD, and diagD^2 against the eigenvalues of
(C + C^T) / 2 at 40 digits (mpmath.eigsy) with Weyl's bound p(D) u ||C||_F + ||C - C^T||_F / 2 + 3 u |lambda|.  C is not bit-symmetric:
the kernel builds C[a][c] and C[c][a] as w pa pc and w pc pa.  p(D) = 8 D + 64: cyclic Jacobi's backward error is O(sweeps D u ||C||)
and LAPACK's O(D u ||C||); calibrated on the oracle's Jacobi and numpy.linalg.eigh on the planted spectra (condition up to 1e14, clustered
and repeated eigenvalues), where the worst is below p(D) / 3.  A NaN in diagD (sqrt of a negative computed eigenvalue; deap produces it
too) is allowed only where the 40-digit eigenvalue lies within the budget of zero.

`strategy64` is the same generation in plain float64 numpy, optionally with one deliberate defect (the teeth, tests/test_cmaes_exact.py).
"""
import numpy as np

import bbob_exact as be
from bbob_exact import LD, U, R, gamma, _f

EX = be.Exact()
SITE_ELEM_A = 0                 # MBX_SITE_ELEM_A
NSCALAR = 16
SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_RETURN, SC_GEN, SC_EPISODE = range(8)
SC_SIGMA, SC_UPDATES = 10, 11


# ================================================================================================ state block (include/mbx_layout.h §10)
def state_doubles(D, nlog):
    return 4 * D + 2 * D * D + NSCALAR + nlog + 1


def split(st, D):
    st = np.asarray(st, dtype=np.float64)
    o = {'centroid': st[0:D], 'C': st[D:D + D * D].reshape(D, D), 'B': st[D + D * D:D + 2 * D * D].reshape(D, D)}
    b = D + 2 * D * D
    o['diagD'], o['ps'], o['pc'] = st[b:b + D], st[b + D:b + 2 * D], st[b + 2 * D:b + 3 * D]
    o['sc'] = st[b + 3 * D:b + 3 * D + NSCALAR]
    o['cost'] = st[b + 3 * D + NSCALAR:]
    return o


def join(D, nlog, centroid, C, B, diagD, ps, pc, sc=None, cost=None):
    st = np.zeros(state_doubles(D, nlog))
    st[0:D] = centroid
    st[D:D + D * D] = np.asarray(C).ravel()
    st[D + D * D:D + 2 * D * D] = np.asarray(B).ravel()
    b = D + 2 * D * D
    st[b:b + D], st[b + D:b + 2 * D], st[b + 2 * D:b + 3 * D] = diagD, ps, pc
    if sc is not None:
        st[b + 3 * D:b + 3 * D + NSCALAR] = sc
    if cost is not None:
        st[b + 3 * D + NSCALAR:b + 3 * D + NSCALAR + len(cost)] = cost
    return st


def scalars(gbest=np.inf, fes=0., log_index=0, cost_len=0, done=0, gen=0, episode=1, sigma=0.5, updates=0):
    sc = np.zeros(NSCALAR)
    sc[SC_GBEST], sc[SC_FES], sc[SC_LOG_INDEX], sc[SC_COST_LEN], sc[SC_DONE] = gbest, fes, log_index, cost_len, done
    sc[SC_GEN], sc[SC_EPISODE], sc[SC_SIGMA], sc[SC_UPDATES] = gen, episode, sigma, updates
    return sc


# ================================================================================================ R helpers
def _sum(x, axis):
    return EX.sum(x, axis=axis)


def _lit(s):
    return EX.lit(s)


def _min(a, b):
    """min of two R scalars (ccovmu's clamp): the value of the smaller, the larger bound (1-Lipschitz)."""
    return R(min(a.v, b.v), max(float(a.e), float(b.e)))


def params(D, NP):
    """computeParams defaults for lambda_ = NP (R scalars, w an R [mu])."""
    mu = NP // 2
    lg = EX.log(R(np.arange(1, mu + 1, dtype=np.float64)))
    w = EX.log(R(mu + 0.5)) - lg
    w = w / _sum(w, 0)
    mueff = R(1.) / _sum(w * w, 0)
    Df = float(D)
    cc = R(4.) / R(Df + 4.)
    cs = (mueff + 2.) / ((mueff + Df) + 3.)
    d13 = R(Df) + _lit('1.3')
    ccov1 = R(2.) / (d13 * d13 + mueff)
    ccovmu = R(2.) * ((mueff - 2.) + R(1.) / mueff) / (R((Df + 2.) ** 2) + mueff)
    ccovmu = _min(ccovmu, R(1.) - ccov1)
    sq = EX.sqrt((mueff - 1.) / R(Df + 1.)) - 1.
    damps = (R(1.) + R(2.) * EX.maximum(0., sq)) + cs
    chiN = EX.sqrt(R(Df)) * ((R(1.) - R(1.) / R(4. * Df)) + R(1.) / (R(21. * Df) * Df))
    return dict(mu=mu, w=w, mueff=mueff, cc=cc, cs=cs, ccov1=ccov1, ccovmu=ccovmu, damps=damps, chiN=chiN)


def _u53(a, b):
    return ((a >> 5) * 67108864.0 + (b >> 6)) * (1.0 / 9007199254740992.0)


def uniforms(seed, gen, episode, NP, D):
    """(ua, ub) [NP, D] float64 of Philox(seed, i D + d, MBX_SITE_ELEM_A, gen, episode)."""
    from oracle import oracle
    ua, ub = np.empty((NP, D)), np.empty((NP, D))
    for e in range(NP * D):
        w = oracle.philox(int(seed), e, SITE_ELEM_A, int(gen), int(episode))
        ua.flat[e], ub.flat[e] = _u53(w[0], w[1]), _u53(w[2], w[3])
    return ua, ub


def normals(ua, ub):
    """The first Box-Muller normal, sqrt(-2 log(1 - ua)) cos(2 pi ub), as R."""
    L = EX.log(R(1. - ua))                                        # 1 - ua is exact
    r = EX.sqrt(R(-2. * L.v, 2. * L.e))                          # the doubling is exact
    return r * EX.cos(be._two_pi(EX) * R(ub))


def positions(st, arz, sigma):
    """x = centroid + sigma * arz . (B * diagD)^T  -> R [NP, D]."""
    BD = R(st['B']) * R(st['diagD'])[None, :]                    # BD[d][k] = B[d][k] diagD[k]
    a = arz.v[:, None, :] * BD.v[None, :, :]                      # [NP, D(d), D(k)]
    aa = np.abs(_f(arz.v))[:, None, :]
    ba = np.abs(_f(BD.v))[None, :, :]
    D = arz.v.shape[1]
    s = R(a.sum(-1), (arz.e[:, None, :] * ba + aa * BD.e[None] + arz.e[:, None, :] * BD.e[None]).sum(-1) + gamma(D) * (aa * ba).sum(-1))
    return R(st['centroid'])[None, :] + R(sigma) * s


# ================================================================================================ the generation
def restate(desc, st_before, seed, NP, D, max_fes, log_interval, nlog, early_stop=True):
    """One generation from the state block st_before.  -> dict:
    'X' (R positions), 'cost' (R), 'cost_amb' (per candidate), 'decided' (bool), and when decided: 'centroid', 'ps', 'pc' (dict of
    hsig branch -> R), 'C' (dict), 'sigma' (R), 'hsig' (0, 1 or None when ambiguous); always: 'gbest' (value, allowance), 'done' (0, 1 or
    None), 'fes', 'gen', 'updates'."""
    s = split(st_before, D)
    sc = s['sc']
    out = {}
    gen, episode = int(sc[SC_GEN]) + 1, int(sc[SC_EPISODE])
    sigma0, upd = float(sc[SC_SIGMA]), int(sc[SC_UPDATES])
    p = params(D, NP)
    mu = p['mu']
    ua, ub = uniforms(seed, gen, episode, NP, D)
    arz = normals(ua, ub)
    X = positions(s, arz, sigma0)
    cost, amb = be._eval(desc, X)
    out.update(X=X, cost=cost, cost_amb=np.asarray(amb), params=p)
    # ranking: best first, stable
    v, e = cost.v, cost.e
    order = np.argsort(v, kind='stable')
    lo, hi = v - e.astype(LD), v + e.astype(LD)
    decided = bool(np.all(np.isfinite(e)))
    tie = np.zeros(NP, dtype=bool)
    for r in range(min(mu, NP - 1)):
        a = order[r]
        for q in order[r + 1:]:
            if v[q] == v[a] and amb[q] == 0 and amb[a] == 0:
                tie[a] = tie[q] = True
                continue
            if not hi[a] < lo[q]:
                decided = False
                break
        if not decided:
            break
    out['decided'], out['order'], out['ties'] = decided, order, int(tie.sum())
    # gbest (HallOfFame(1)) and the bookkeeping
    gprev = float(sc[SC_GBEST])
    mhi = np.min(hi)
    cand = lo <= mhi
    gex = min(LD(gprev), np.min(v))
    gal = float(np.max(e[cand])) if np.min(lo) <= LD(gprev) else 0.
    out['gbest'] = (gex, gal)
    fes = float(sc[SC_FES]) + NP
    done_fes = fes >= max_fes
    stop = early_stop                                             # the BBOB problems have an optimum: the 1e-8 rule applies
    th = LD(1e-8)
    if done_fes or not stop:
        done = int(done_fes)
    elif abs(gex - th) <= LD(gal):
        done = None
    else:
        done = int(gex <= th)
    out.update(done=done, fes=fes, gen=gen, updates=upd + 1, log_index=int(sc[SC_LOG_INDEX]), cost_len=int(sc[SC_COST_LEN]),
               cost_curve=s['cost'].copy(), log_interval=log_interval, nlog=nlog, max_fes=max_fes)
    if not decided:
        return out
    w, cc, cs, mueff = p['w'], p['cc'], p['cs'], p['mueff']
    sel = order[:mu]
    Xs = X[sel]
    old = R(s['centroid'])
    cen = _sum(w[:, None] * Xs, 0)
    cd = cen - old
    B = R(s['B'])
    t = _sum(B * cd[:, None], 0)                                  # B^T c_diff
    t1 = t / R(s['diagD'])
    y = _sum(B * t1[None, :], 1)                                  # B t1
    sig = R(sigma0)
    kps = EX.sqrt(cs * (R(2.) - cs) * mueff) / sig
    ps = (R(1.) - cs) * R(s['ps']) + kps * y
    nps = EX.sqrt(_sum(ps * ps, 0))
    den = EX.sqrt(R(1.) - EX.pow(R(1.) - cs, R(2. * (upd + 1.))))
    q = nps / den / p['chiN']
    thr = _lit('1.4') + R(2.) / R(D + 1.)
    if abs(q.v - thr.v) <= LD(float(q.e) + float(thr.e)):
        hsigs, hs = (0, 1), None
    else:
        hs = int(q.v < thr.v)
        hsigs = (hs,)
    kpc0 = EX.sqrt(cc * (R(2.) - cc) * mueff) / sig
    A = Xs - old[None, :]                                         # a_i [mu, D]
    wa = w[:, None] * A
    rk = _sum(wa[:, :, None] * A[:, None, :], 0)                  # sum_i w_i a_i a_i^T
    s2 = sig * sig
    pcs, Cs = {}, {}
    for h in hsigs:
        kpc = kpc0 * R(float(h))
        pc = (R(1.) - cc) * R(s['pc']) + kpc * cd
        keep = ((R(1.) - p['ccov1']) - p['ccovmu']) + R(1. - h) * p['ccov1'] * cc * (R(2.) - cc)
        C = (keep * R(s['C']) + p['ccov1'] * (pc[:, None] * pc[None, :])) + p['ccovmu'] * rk / s2
        pcs[h], Cs[h] = pc, C
    sigma = sig * EX.exp((nps / p['chiN'] - 1.) * cs / p['damps'])
    out.update(centroid=cen, ps=ps, pc=pcs, C=Cs, sigma=sigma, hsig=hs, hsig_q=(q, thr))
    return out


def _log(out, gbest, done):
    """The wrapper's logging (log_and_terminate) from the kernel's own gbest and done: -> (log_index, cost_len, cost curve)."""
    li, cl, cc = out['log_index'], out['cost_len'], out['cost_curve'].copy()
    if out['fes'] >= li * out['log_interval']:
        li += 1
        cc[cl] = gbest
        cl += 1
    if done:
        if cl >= out['nlog'] + 1:
            cc[cl - 1] = gbest
        else:
            cc[cl] = gbest
            cl += 1
    return li, cl, cc


def _ratio(got, r):
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got.astype(LD) - r.v).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err == 0, 0., err / r.e)


def _ulps(r):
    return r.e / np.maximum(np.spacing(np.abs(_f(r.v))), np.finfo(np.float64).tiny)


class Ledger:
    """Worst error / allowance ratios, ambiguous counts and allowances in ulp over many judged generations."""

    def __init__(self):
        self.worst = {}
        self.ulps = {}
        self.n = dict(generations=0, undecided=0, hsig_ambiguous=0, done_ambiguous=0, cost_ambiguous=0, ties=0)

    def add(self, name, ratio, r=None):
        ratio = np.asarray(ratio, dtype=np.float64)
        if ratio.size:
            self.worst[name] = max(self.worst.get(name, 0.), float(np.max(ratio)))
        if r is not None:
            self.ulps.setdefault(name, []).append(np.ravel(_ulps(r)))

    def summary(self):
        med = {k: float(np.median(np.concatenate(v))) for k, v in self.ulps.items()}
        lines = [f'generations judged {self.n}']
        lines += [f'  {k:9s} worst ratio {self.worst.get(k, 0.):.3g}' + (f'   median allowance {med[k]:.3g} ulp' if k in med else '')
                  for k in sorted(self.worst)]
        return '\n'.join(lines)


def judge(desc, st_before, st_after, seed, NP, D, max_fes, log_interval, nlog, ledger, X=None, cost=None, label=''):
    """Assert that st_after is a correct float64 generation from st_before (and, if given, that the candidates X / costs are within their
    allowance).  Returns the restatement (restate's dict)."""
    out = restate(desc, st_before, seed, NP, D, max_fes, log_interval, nlog)
    a = split(st_after, D)
    sc = a['sc']
    ledger.n['generations'] += 1
    ledger.n['cost_ambiguous'] += int(np.sum(out['cost_amb'] > 0))
    ledger.n['ties'] += out['ties']
    if X is not None:
        rx = _ratio(X, out['X'])
        ledger.add('position', rx, out['X'])
        assert np.all(rx <= 1), (label, 'candidate positions', float(np.max(rx)))
    if cost is not None:
        rc = _ratio(cost, out['cost'])
        ledger.add('cost', rc, out['cost'])
        assert np.all(rc <= 1), (label, 'candidate costs', float(np.max(rc)))
    gex, gal = out['gbest']
    gr = abs(LD(sc[SC_GBEST]) - gex)
    assert gr <= LD(gal) or (gr == 0), (label, 'gbest', sc[SC_GBEST], gex, gal)
    ledger.add('gbest', [float(gr) / gal if gal > 0 else 0.])
    assert sc[SC_FES] == out['fes'] and sc[SC_GEN] == out['gen'] and sc[SC_UPDATES] == out['updates'], (label, 'bookkeeping', sc[:12])
    if out['done'] is None:
        ledger.n['done_ambiguous'] += 1
    else:
        assert sc[SC_DONE] == out['done'], (label, 'done', sc[SC_DONE], out['done'], gex)
    li, cl, cc = _log(out, sc[SC_GBEST], sc[SC_DONE] != 0)
    assert sc[SC_LOG_INDEX] == li and sc[SC_COST_LEN] == cl and np.array_equal(a['cost'][:cl], cc[:cl]), (label, 'log', sc[:4], li, cl)
    if not out['decided']:
        ledger.n['undecided'] += 1
        return out
    for name, got in (('centroid', a['centroid']), ('ps', a['ps'])):
        r = _ratio(got, out[name])
        ledger.add(name, r, out[name])
        assert np.all(r <= 1), (label, name, float(np.max(r)), np.argmax(r))
    rs = _ratio(sc[SC_SIGMA], out['sigma'])
    ledger.add('sigma', rs, out['sigma'])
    assert rs <= 1, (label, 'sigma', sc[SC_SIGMA], out['sigma'].v, out['sigma'].e)
    # hsig: the branch whose pc the kernel stored (the only one, unless ambiguous)
    fits = {h: _ratio(a['pc'], out['pc'][h]) for h in out['pc']}
    ok = [h for h, r in fits.items() if np.all(r <= 1)]
    if out['hsig'] is None:
        ledger.n['hsig_ambiguous'] += 1
    assert ok, (label, 'pc', {h: float(np.max(r)) for h, r in fits.items()}, out['hsig'])
    h = ok[0]
    ledger.add('pc', fits[h], out['pc'][h])
    rC = _ratio(a['C'], out['C'][h])
    ledger.add('C', rC, out['C'][h])
    assert np.all(rC <= 1), (label, 'C', float(np.max(rC)), np.unravel_index(np.argmax(rC), rC.shape))
    out['hsig_taken'] = h
    return out


# ================================================================================================ eigendecomposition
def p_of(D):
    return 8 * D + 64


def eigen_check(C, B, diagD, label='', worst=None):
    """Stored B, diagD against the stored C (see the module docstring).  worst: a dict updated with the largest ratio of each check."""
    import mpmath
    C, B, dD = (np.asarray(a, dtype=np.float64) for a in (C, B, diagD))
    D = C.shape[0]
    nC = float(np.sqrt((C.astype(LD) ** 2).sum()))
    asym = float(np.sqrt(((C.astype(LD) - C.T.astype(LD)) ** 2).sum())) / 2
    budget = p_of(D) * U * nC
    Bl = B.astype(LD)
    orth = float(np.max(np.abs(Bl.T @ Bl - np.eye(D, dtype=LD))))
    lam = dD.astype(LD) ** 2
    fin = np.isfinite(dD)
    res = (C.astype(LD) @ Bl - Bl * lam[None, :])[:, fin]
    resid = float(np.max(np.abs(res))) if res.size else 0.
    mpmath.mp.dps = 40
    S = (C.astype(LD) + C.T.astype(LD)) / 2
    ev = mpmath.eigsy(mpmath.matrix([[mpmath.mpf(str(S[i, j])) for j in range(D)] for i in range(D)]), eigvals_only=True)
    ev = np.sort(np.array([LD(mpmath.nstr(ev[i], 30)) for i in range(D)]))
    weyl = budget + asym
    dl = np.abs(lam - ev).astype(np.float64)
    bound = weyl + 3 * U * np.abs(ev.astype(np.float64))
    r = {'orth': orth / (p_of(D) * U), 'resid': resid / budget if budget > 0 else 0., 'eig': float(np.max(np.where(fin, dl / bound, 0.)))}
    if worst is not None:
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.), x)
    assert r['orth'] <= 1, (label, 'B not orthonormal', orth)
    assert r['resid'] <= 1, (label, 'C B != B diag(diagD^2)', resid, budget)
    assert r['eig'] <= 1, (label, 'diagD^2 vs the 40-digit eigenvalues', float(np.max(dl / bound)))
    nan = ~fin
    assert np.all(np.abs(ev[nan]).astype(np.float64) <= weyl), (label, 'NaN diagD where the eigenvalue is not within the budget of 0')
    lf = dD[fin]
    assert np.all(np.diff(lf) >= 0), (label, 'diagD not ascending', lf)
    return r


# ================================================================================================ the float64 strategy (teeth)
DEFECTS = ('C_new_sigma', 'pc_new_sigma', 'tie_reversed', 'weights_raw', 'hsig_count', 'ps_no_invD', 'eig_unpermuted', 'jacobi_1sweep')


def jacobi_eigh(A, sweeps=60, permute=True):
    """The cyclic Jacobi of the kernel (cl_jacobi_eigh) in numpy float64: eigenvalues ascending, eigenvectors in the columns."""
    A = np.array(A, dtype=np.float64)
    D = A.shape[0]
    V = np.eye(D)
    for _ in range(sweeps):
        off = np.sum(np.triu(A, 1) ** 2)
        if off <= 1e-32 * np.sum(np.diag(A) ** 2):
            break
        for p in range(D - 1):
            for q in range(p + 1, D):
                apq = A[p, q]
                if apq == 0.:
                    continue
                th = (A[q, q] - A[p, p]) / (2. * apq)
                t = (1. if th >= 0 else -1.) / (abs(th) + np.sqrt(th * th + 1.))
                c = 1. / np.sqrt(t * t + 1.)
                s = t * c
                ap, aq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * ap - s * aq, s * ap + c * aq
                ap, aq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * ap - s * aq, s * ap + c * aq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    w = np.diag(A).copy()
    o = np.argsort(w, kind='stable')
    return w[o], (V[:, o] if permute else V)


def strategy64(desc, st_before, seed, NP, D, max_fes, log_interval, nlog, defect=None, early_stop=True):
    """One generation in plain float64 (the restatement's formula, numpy's order), optionally with one defect of DEFECTS."""
    s = split(st_before, D)
    sc = s['sc'].copy()
    gen, episode, sigma, upd = int(sc[SC_GEN]) + 1, int(sc[SC_EPISODE]), float(sc[SC_SIGMA]), int(sc[SC_UPDATES])
    mu = NP // 2
    w = np.log(mu + 0.5) - np.log(np.arange(1, mu + 1))
    if defect != 'weights_raw':
        w = w / w.sum()
    mueff = 1. / np.sum((w / w.sum()) ** 2)
    cc, cs = 4. / (D + 4.), (mueff + 2.) / (D + mueff + 3.)
    ccov1 = 2. / ((D + 1.3) ** 2 + mueff)
    ccovmu = min(2. * (mueff - 2. + 1. / mueff) / ((D + 2.) ** 2 + mueff), 1 - ccov1)
    damps = 1. + 2. * max(0., np.sqrt((mueff - 1.) / (D + 1.)) - 1.) + cs
    chiN = np.sqrt(D) * (1. - 1. / (4. * D) + 1. / (21. * D * D))
    ua, ub = uniforms(seed, gen, episode, NP, D)
    arz = np.sqrt(-2. * np.log(1. - ua)) * np.cos(be.KTWO_PI * ub)
    X = s['centroid'] + sigma * (arz @ (s['B'] * s['diagD'][None, :]).T)
    cost = np.asarray(be.float64_eval(desc, X), dtype=np.float64)
    gbest = min(float(sc[SC_GBEST]), float(np.min(cost)))
    order = np.argsort(cost, kind='stable')
    if defect == 'tie_reversed':
        order = np.lexsort((-np.arange(NP), cost))
    old = s['centroid']
    cen = w @ X[order[:mu]]
    cd = cen - old
    t1 = s['B'].T @ cd
    if defect != 'ps_no_invD':
        t1 = t1 / s['diagD']
    ps = (1. - cs) * s['ps'] + np.sqrt(cs * (2. - cs) * mueff) / sigma * (s['B'] @ t1)
    nps = np.linalg.norm(ps)
    n_upd = upd if defect == 'hsig_count' else upd + 1
    with np.errstate(divide='ignore'):
        hsig = float(nps / np.sqrt(1. - (1. - cs) ** (2. * n_upd)) / chiN < 1.4 + 2. / (D + 1.))
    with np.errstate(over='ignore'):
        sigma_new = sigma * np.exp((nps / chiN - 1.) * cs / damps)
    pc = (1. - cc) * s['pc'] + hsig * np.sqrt(cc * (2. - cc) * mueff) / (sigma_new if defect == 'pc_new_sigma' else sigma) * cd
    A = X[order[:mu]] - old
    rk = (w[:, None] * A).T @ A
    s2 = (sigma_new if defect == 'C_new_sigma' else sigma) ** 2
    keep = 1. - ccov1 - ccovmu + (1. - hsig) * ccov1 * cc * (2. - cc)
    C = keep * s['C'] + ccov1 * np.outer(pc, pc) + ccovmu * rk / s2
    ev, B = jacobi_eigh(C, sweeps=1 if defect == 'jacobi_1sweep' else 60, permute=defect != 'eig_unpermuted')
    with np.errstate(invalid='ignore'):
        dD = np.sqrt(ev)
    fes = float(sc[SC_FES]) + NP
    done = fes >= max_fes or (early_stop and gbest <= 1e-8)
    out = dict(fes=fes, log_index=int(sc[SC_LOG_INDEX]), cost_len=int(sc[SC_COST_LEN]), cost_curve=s['cost'].copy(), log_interval=log_interval,
               nlog=nlog)
    li, cl, curve = _log(out, gbest, done)
    sc[SC_GBEST], sc[SC_FES], sc[SC_LOG_INDEX], sc[SC_COST_LEN], sc[SC_DONE] = gbest, fes, li, cl, float(done)
    sc[SC_GEN], sc[SC_SIGMA], sc[SC_UPDATES] = gen, sigma_new, upd + 1
    return join(D, nlog, cen, C, B, dD, ps, pc, sc, curve), X, cost
