"""LES (src/optimizer/les_optimizer.py, src/agent/les_agent.py): the resident episode kernel (metabox_amd/csrc/mbx_les.hpp), its host classes and the
numpy CMA-ES that stands in for the `cmaes` package.

Fixtures (tools/gen_golden.py les): whole reference episodes with the shipped best_x, recorded at every generation (two full-length ones thinned
to every 25th).  The numpy draws are not stored: LesFeeder regenerates them from the seed in the reference's call order (include/mbx_layout.h
section 18) and must end at the recorded stream position.

The chain to the reference is closed on the CPU: `Restate`, a numpy restatement of reset / generation written from the rules in the header of
mbx_les.hpp, with the two networks as torch float32 modules (what the reference runs), fed the feeder's draws and the reference's recorded costs,
reproduces every recorded quantity of every generation bit for bit.  The kernel's float32 networks differ from torch's in summation order and
exp, so the GPU tests hold the kernel to the SAME restatement with float64 networks, within a tolerance that is measured, not chosen: E_ref, the
largest difference over all fixture generations between the reference's value and the float64-network restatement of that generation; the kernel
may differ from the float64 restatement by 4 E_ref + 4 ulp (`e_ref`, printed by test_e_ref_is_measured_from_the_fixtures).  Everything that is not
network arithmetic -- FEs, the generation counter, gbest, the log, done, the reward -- is exact on the device's own costs.

Measured on this fixture set (CPU), E_ref: W 1.45e-08, alpha 7.54e-08, mu 3.15e-07, sigma 1.05e-07, Pc 1.39e-07, Ps 1.01e-07, children 3.19e-07."""
import copy
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from helpers import GOLDEN, close, problems
from oracle import oracle

TR = {}
for _f in sorted(glob.glob(os.path.join(GOLDEN, 'les_traces*.npz'))):
    with np.load(_f) as _z:
        TR.update({k: _z[k] for k in _z.files})
with np.load(os.path.join(GOLDEN, 'les_policy.npz')) as _z:
    POL = {k: _z[k] for k in _z.files}
CASES = [str(c) for c in TR['cases']]
BUDGET = [c for c in CASES if c.endswith('/budget')]
FULL = [c for c in CASES if c.endswith('/full')]
SKIP50 = [c for c in CASES if c.endswith('/skip50')][0]
SKIP1 = [c for c in CASES if c.endswith('/skip1x60')][0]
NP, NPARAM, NATTN, ALGO_LES = 16, 246, 68, 21
STAMPS = np.array([1, 3, 10, 30, 50, 100, 250, 500, 750, 1000, 1250, 1500, 2000])
ALPHAS = (0.1, 0.5, 0.9)
SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_RETURN, SC_GEN, SC_EPISODE, SC_INIT_Y, SC_CALL_INIT_Y = 0, 1, 2, 3, 4, 5, 6, 7, 10, 11
SITE_MU, SITE_NORMAL = 62, 63
QUANT = ('W', 'alpha', 'mu', 'sigma', 'Pc', 'Ps', 'children')


# ------------------------------------------------------------------------------------------------ layout (include/mbx_layout.h section 18)
def curve_cap(max_fes, log_interval, nlog):
    G = (max_fes - 1) // NP
    return max(nlog + 1, min(G, (G + 1) * NP // log_interval) + 2)


def tape_stride(D):
    return D + NP * D + 3 * NP


def fields(D, cap):
    return (('parents', NP * D), ('costs', NP), ('mu', D), ('sigma', D), ('Pc', 3 * D), ('Ps', 3 * D), ('z', NP * D), ('W', NP), ('alpha', 2 * D),
            ('scalars', 16), ('cost', cap))


def state_doubles(D, cap):
    return sum(n for _, n in fields(D, cap))


def split_state(st, D, cap):
    out, o = {}, 0
    for name, n in fields(D, cap):
        out[name] = st[o:o + n]
        o += n
    assert o == len(st), (o, len(st))
    return out


# ------------------------------------------------------------------------------------------------ the numpy stream
class LesFeeder:
    """numpy's legacy stream as LES consumes it, laid out as the tapes of include/mbx_layout.h section 18."""

    def __init__(self, seed, D, noise_kind):
        self.rs, self.D, self.noise = np.random.RandomState(seed), D, noise_kind

    def _noise(self, n):
        rows, rs = np.zeros((3, n)), self.rs
        if self.noise == 1:
            rows[0] = rs.randn(n)
        elif self.noise == 2:
            rows[0] = rs.rand(n)
            rows[1] = rs.rand(n)
        elif self.noise == 3:
            rows[0] = rs.rand(n)
            rows[1] = rs.randn(n)
            rows[2] = rs.randn(n)
        return rows

    def reset_tape(self):
        D = self.D
        t = np.zeros(tape_stride(D))
        t[:D] = self.rs.rand(D)                                        # :68
        t[D:D + NP * D] = self.rs.standard_normal(NP * D)              # :70: normal(mu, sigma, (16, D)) = mu + sigma * gauss, C order
        t[D + NP * D:] = self._noise(NP).ravel()
        return t

    def generation_tape(self):
        D = self.D
        t = np.zeros(tape_stride(D))
        t[:NP * D] = self.rs.standard_normal(NP * D)                   # :145
        t[NP * D:NP * D + 3 * NP] = self._noise(NP).ravel()
        return t


# ------------------------------------------------------------------------------------------------ the two networks
def unpack(x):
    """vector2nn order (:6-15): attn = Wq.weight, Wq.bias, Wk.weight, Wk.bias, Wv.weight, Wv.bias; mlp = ln1.weight, ln1.bias, ln2.weight, ln2.bias."""
    x = np.asarray(x)
    assert x.shape == (NPARAM,)
    return dict(Wq=x[0:24].reshape(8, 3), bq=x[24:32], Wk=x[32:56].reshape(8, 3), bk=x[56:64], Wv=x[64:67].reshape(1, 3), bv=x[67:68],
                W1=x[68:220].reshape(8, 19), b1=x[220:228], W2=x[228:244].reshape(2, 8), b2=x[244:246])


class TorchNets:
    """SelfAttn (:18-30) and LrNet (:32-40) as the reference runs them: torch's CPU float32 kernels."""

    def __init__(self, x):
        import torch
        self.p = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(torch.float32) for k, v in unpack(x).items()}

    def attn(self, X):
        import torch
        import torch.nn.functional as F
        p, X = self.p, torch.from_numpy(X).to(torch.float32)
        Q, K, V = F.linear(X, p['Wq'], p['bq']), F.linear(X, p['Wk'], p['bk']), F.linear(X, p['Wv'], p['bv'])
        s = torch.softmax(torch.matmul(Q, K.T) / np.sqrt(8), dim=-1)
        return torch.softmax(torch.matmul(s, V), dim=0).squeeze().numpy()

    def mlp(self, X):
        import torch
        import torch.nn.functional as F
        p, X = self.p, torch.from_numpy(X).to(torch.float32)
        return torch.sigmoid(F.linear(F.linear(X, p['W1'], p['b1']), p['W2'], p['b2'])).numpy()


class F64Nets:
    """The same networks with the float32 parameters and float32 inputs widened to float64 and every operation in float64."""

    def __init__(self, x):
        self.p = {k: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64) for k, v in unpack(x).items()}

    @staticmethod
    def _softmax(a, axis):
        e = np.exp(a - np.max(a, axis=axis, keepdims=True))
        return e / np.sum(e, axis=axis, keepdims=True)

    def attn(self, X):
        p, X = self.p, X.astype(np.float32).astype(np.float64)
        Q, K, V = X @ p['Wq'].T + p['bq'], X @ p['Wk'].T + p['bk'], X @ p['Wv'].T + p['bv']
        return self._softmax(self._softmax(Q @ K.T / np.sqrt(8), -1) @ V, 0)[:, 0]

    def mlp(self, X):
        p, X = self.p, X.astype(np.float32).astype(np.float64)
        return 1. / (1. + np.exp(-((X @ p['W1'].T + p['b1']) @ p['W2'].T + p['b2'])))


# ------------------------------------------------------------------------------------------------ the restatement
class Restate:
    """init_population and one generation of update() in numpy, from the rules in the header of mbx_les.hpp.  Costs are handed in."""

    def __init__(self, D, lb, ub, max_fes, log_interval, nlog, has_optimum=True, early_stop=True):
        self.D, self.lb, self.ub, self.max_fes, self.log_interval, self.nlog = D, lb, ub, max_fes, log_interval, nlog
        self.stop_rule = has_optimum and early_stop
        self.cap = curve_cap(max_fes, log_interval, nlog)

    def reset_head(self, tape):
        D = self.D
        self.mu = self.lb + (self.ub - self.lb) * tape[:D]
        self.sigma = np.ones(D) * self.ub * 0.2
        self.z = tape[D:D + NP * D].reshape(NP, D).copy()
        self.parents = np.clip(self.mu + self.sigma * self.z, self.lb, self.ub)
        return self.parents

    def reset_tail(self, costs):
        D = self.D
        self.costs = np.array(costs, dtype=np.float64)
        self.Pc, self.Ps = np.zeros((3, D)), np.zeros((3, D))
        self.t, self.gbest, self.fes, self.log_index, self.done = 0, float(np.min(self.costs)), NP, 1, False
        self.cost = [self.gbest]
        self.init_y = self.call_init_y = 0.
        self.reward = 0.

    def head(self, z, nets):
        """(:130-145) -> W, alpha, the new mu / sigma / Pc / Ps and the children; nothing is committed."""
        D, c = self.D, self.costs
        z = np.asarray(z).reshape(NP, D)
        with np.errstate(all='ignore'):
            zsc = (c - np.mean(c)) / (np.std(c) + 1e-8)
            arg = np.lexsort((np.arange(NP), c)) / NP - 0.5              # np.argsort(costs) with equal costs by (cost, row): the INDEX, not the rank
            imp = c < self.gbest
            W = nets.attn(np.vstack([zsc, arg, imp]).T)
            diff = self.parents - self.mu
            s1 = np.sum(diff * W[:, None], axis=0)
            s2 = np.sum(diff / self.sigma * W[:, None], axis=0)
            s3 = np.sum(diff ** 2 * W[:, None], axis=0)
            Pc = np.vstack([(1 - a) * self.Pc[i] + a * (s1 - self.Pc[i]) for i, a in enumerate(ALPHAS)])
            Ps = np.vstack([(1 - a) * self.Ps[i] + a * (s2 - self.Ps[i]) for i, a in enumerate(ALPHAS)])
            rho = np.tanh(self.t / STAMPS - 1)[None, :].repeat(D, axis=0)
            alpha = nets.mlp(np.hstack([Pc.T, Ps.T, rho]))
            am, asg = alpha[:, 0], alpha[:, 1]
            mu = (1 - am) * self.mu + am * s1
            sigma = (1 - asg) * self.sigma + asg * np.sqrt(s3)
            children = np.clip(mu + sigma * z, self.lb, self.ub)
        return dict(W=W, alpha=alpha, mu=mu, sigma=sigma, Pc=Pc, Ps=Ps, children=children, improved=imp, z=z)

    def commit(self, h, costs, skip=None):
        """(:146-178) with the costs of the children.  skip = None: the budget route; (step, skip_step): step `step` of a skip_step call."""
        self.mu, self.sigma, self.Pc, self.Ps, self.parents, self.z = h['mu'], h['sigma'], h['Pc'], h['Ps'], h['children'], h['z']
        self.costs = np.array(costs, dtype=np.float64)
        self.fes += NP
        self.gbest = float(np.min([np.min(self.costs), self.gbest]))
        if skip is None and self.t == 0:
            self.init_y = self.gbest
        if skip is not None and skip[0] == 0:
            self.call_init_y = self.gbest
        self.t += 1
        end = self.fes >= self.max_fes or (self.stop_rule and self.gbest <= 1e-8)
        if skip is not None:
            end = skip[0] + 1 >= skip[1]
        if self.fes >= self.log_index * self.log_interval:           # once, not "while"; unguarded in the reference, bounded by the block here
            self.log_index += 1
            if len(self.cost) < self.cap:
                self.cost.append(self.gbest)
        if end:
            if len(self.cost) >= self.nlog + 1:
                self.cost[-1] = self.gbest
            else:
                self.cost.append(self.gbest)
        iy = self.init_y if skip is None else self.call_init_y
        with np.errstate(all='ignore'):
            self.reward = float((np.float64(iy) - self.gbest) / np.float64(iy))
        if skip is None:
            self.done = end
        return end

    def block(self):
        """The state block of include/mbx_layout.h section 18 (normals, W and alpha of the last generation zeroed)."""
        D = self.D
        sc = np.zeros(16)
        sc[[SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_RETURN, SC_GEN, SC_EPISODE, SC_INIT_Y, SC_CALL_INIT_Y]] = [
            self.gbest, self.fes, self.log_index, len(self.cost), float(self.done), self.reward if self.done else 0., self.t, 1, self.init_y, self.call_init_y]
        curve = np.zeros(self.cap)
        curve[:len(self.cost)] = self.cost
        return np.concatenate([self.parents.ravel(), self.costs, self.mu, self.sigma, self.Pc.ravel(), self.Ps.ravel(), np.zeros(NP * D), np.zeros(NP),
                               np.zeros(2 * D), sc, curve])

    def load(self, st):
        """Take the evolution state and the counters from a device block."""
        D = self.D
        s = split_state(st, D, self.cap)
        self.parents, self.costs = s['parents'].reshape(NP, D).copy(), s['costs'].copy()
        self.mu, self.sigma, self.Pc, self.Ps = s['mu'].copy(), s['sigma'].copy(), s['Pc'].reshape(3, D).copy(), s['Ps'].reshape(3, D).copy()
        sc = s['scalars']
        self.gbest, self.fes, self.log_index, self.done, self.t = float(sc[SC_GBEST]), int(sc[SC_FES]), int(sc[SC_LOG_INDEX]), bool(sc[SC_DONE]), int(sc[SC_GEN])
        self.init_y, self.call_init_y, self.reward = float(sc[SC_INIT_Y]), float(sc[SC_CALL_INIT_Y]), float(sc[SC_RETURN])
        self.cost = [float(v) for v in s['cost'][:int(sc[SC_COST_LEN])]]
        return self


# ------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def _protein():
    from test_protein import protein
    return protein()[0]


def _problem(suite, dim, fid):
    if suite == 'protein':
        return _protein()[fid], 0
    p = problems(suite, int(dim))[int(fid)]
    return p, p.noise[0]


def _case(case):
    suite, dim, fid, seed, tag = case.split('/')
    p, nk = _problem(suite, dim, fid)
    return dict(p=p, nk=nk, D=int(dim), seed=int(seed), suite=suite, tag=tag, max_fes=int(TR[f'{case}/max_fes']), log_interval=int(TR[f'{case}/log_interval']),
                nlog=int(TR[f'{case}/n_logpoint']), best_x=POL[f'{suite}/best_x'], has_opt=suite != 'protein')


def _restate_for(c, early_stop=True):
    return Restate(c['D'], float(c['p'].lb), float(c['p'].ub), c['max_fes'], c['log_interval'], c['nlog'], c['has_opt'], early_stop)


def _skips(case):
    """Per generation: None (budget route) or (step, skip_step) of the reference's call that ran it; and the generation each call ends with."""
    out, ends = [], []
    for s, n in zip(TR[f'{case}/calls'], TR[f'{case}/call_gens']):
        out += [None if s < 0 else (k, int(s)) for k in range(int(n))]
        ends.append(len(out) - 1)
    return out, ends


@functools.lru_cache(maxsize=None)
def replay(case, check=False):
    """Walks a fixture episode with the torch-float32 restatement on the feeder's draws and the reference's recorded costs.  -> per generation the
    Restate before it, its tape, its head (= the reference's) and its skip tuple; the Restate after the last one; the reset tape; the feeder."""
    c = _case(case)
    gens = [int(g) for g in TR[f'{case}/gens']]
    at = {g: i for i, g in enumerate(gens)}
    G = gens[-1]
    thinned = f'{case}/costs_all' in TR
    cost_of = (lambda g: TR[f'{case}/costs_all'][g]) if thinned else (lambda g: TR[f'{case}/costs'][at[g]])
    fd = LesFeeder(c['seed'], c['D'], c['nk'])
    nets = TorchNets(c['best_x'])
    rs = _restate_for(c)
    t0 = fd.reset_tape()
    rs.reset_head(t0)
    rs.reset_tail(cost_of(0))
    skips, ends = _skips(case)
    assert len(skips) == G, (case, len(skips), G)
    w = {k: TR[f'{case}/{k}'] for k in ('mu', 'sigma', 'Pc', 'Ps', 'parents', 'costs', 'gbest', 'fes', 't', 'cost_len', 'W', 'alpha')}

    def same_state(g):
        i = at[g]
        assert np.array_equal(rs.mu, w['mu'][i]) and np.array_equal(rs.sigma, w['sigma'][i]), (case, g, 'mu / sigma')
        assert np.array_equal(rs.Pc, w['Pc'][i]) and np.array_equal(rs.Ps, w['Ps'][i], equal_nan=True), (case, g, 'Pc / Ps')
        assert np.array_equal(rs.parents, w['parents'][i]) and np.array_equal(rs.costs, w['costs'][i]), (case, g, 'parents / costs')
        assert (rs.gbest, rs.fes, rs.t, len(rs.cost)) == (w['gbest'][i], w['fes'][i], w['t'][i], w['cost_len'][i]), (case, g, 'counters')
    rows = []
    for g in range(G):
        if check and g in at:
            same_state(g)
        before = copy.deepcopy(rs) if (not thinned or g in at) else None
        tape = fd.generation_tape()
        h = rs.head(tape[:NP * c['D']], nets)
        if check:
            assert not h['improved'].any(), (case, g, 'improved must be all-false')
            if g in at:
                assert np.array_equal(h['W'], w['W'][at[g]]) and np.array_equal(h['alpha'], w['alpha'][at[g]]), (case, g, 'W / alpha')
        end = rs.commit(h, cost_of(g + 1), skips[g])
        rows.append(dict(before=before, tape=tape, head=h, skip=skips[g], g=g))
        if check and g in ends:
            k = ends.index(g)
            ret = TR[f'{case}/call_ret'][k]
            assert (rs.gbest, rs.reward, float(end)) == tuple(ret) and len(rs.cost) == TR[f'{case}/call_len'][k], (case, g, ret, rs.reward)
    if check:
        same_state(G)
        assert np.array_equal(rs.cost, TR[f'{case}/cost']) and rs.fes == TR[f'{case}/fes_end'], case
    return rows, rs, t0, fd


@functools.lru_cache(maxsize=None)
def e_ref():
    """E_ref per quantity: the largest |reference - float64-network restatement| over every recorded generation of the unthinned fixtures."""
    E = {q: 0. for q in QUANT}
    for case in BUDGET + [SKIP50, SKIP1]:
        nets = F64Nets(_case(case)['best_x'])
        for r in replay(case)[0]:
            h64 = r['before'].head(r['head']['z'], nets)
            for q in QUANT:
                E[q] = max(E[q], float(np.max(np.abs(h64[q] - r['head'][q]))))
    return E


def within(q, got, want, factor=4):
    """|got - want| <= factor E_ref + 4 ulp of the quantity's type, element-wise (non-finite entries must match exactly)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    if not np.array_equal(fin, np.isfinite(got)) or not np.array_equal(got[~fin], want[~fin], equal_nan=True):
        return False
    ulp = np.spacing(np.abs(want[fin]).astype(np.float32)).astype(np.float64) if q in ('W', 'alpha') else np.spacing(np.abs(want[fin]))
    return bool(np.all(np.abs(got[fin] - want[fin]) <= factor * e_ref()[q] + 4 * ulp))


# ------------------------------------------------------------------------------------------------ CPU: fixtures and restatement
@pytest.mark.parametrize('case', CASES)
def test_restatement_and_feeder_reproduce_the_reference(case):
    """Every recorded quantity of every generation bit for bit, the final cost list, FEs, reward and is_end of every call (both skip cases
    included), and the feeder ends at the recorded stream position."""
    rows, rs, _, fd = replay(case, True)
    assert len(rows) == TR[f'{case}/gens'][-1]
    assert fd.rs.rand() == float(TR[f'{case}/next_rand']), case


def test_fixture_covers_the_quirks():
    assert len(BUDGET) == 10 and len(FULL) == 2
    assert not any(bool(TR[f'{c}/improved_any']) for c in CASES)                         # improved is all-false in every recorded generation
    assert any(int(TR[f'{c}/nclip']) > 0 for c in CASES)                                 # a coordinate clipped
    assert len(TR[f'{SKIP1}/cost']) == 51 and list(TR[f'{SKIP1}/call_len'][-12:]) == [51] * 12    # the closing log fills the list, then overwrites its end
    assert max(len(TR[f'{c}/cost']) for c in BUDGET) > 51                                # the unguarded log append: a list longer than n_logpoint + 1
    for c in CASES:
        k = _case(c)
        assert len(TR[f'{c}/cost']) <= curve_cap(k['max_fes'], k['log_interval'], k['nlog']), c
    assert {_case(c)['nk'] for c in BUDGET} == {0, 1, 2, 3} and {_case(c)['D'] for c in BUDGET} == {10, 12, 30, 40}
    assert all(16 * 41 <= _case(c)['max_fes'] <= 16 * 61 for c in BUDGET if _case(c)['suite'] != 'protein')
    assert all(int(TR[f'{c}/gens'][-1]) == 1249 and len(TR[f'{c}/gens']) == 52 for c in FULL)
    for c in BUDGET + [SKIP50, SKIP1]:                                                   # tie-free: any two costs of a generation differ by > TIE_RTOL relative
        s = np.sort(TR[f'{c}/costs'], axis=1)
        assert np.all(np.diff(s, axis=1) > 1e-9 * np.abs(s[:, 1:])), c


def test_e_ref_is_measured_from_the_fixtures():
    E = e_ref()
    print('E_ref:', {q: f'{v:.2e}' for q, v in E.items()})
    assert all(0 < E[q] < 1e-5 for q in QUANT), E                    # float32 networks against float64 ones: the size the issue's table reports


def test_timestamp_table_rule_equals_numpy():
    """The batch's timestamp table is tanh in extended precision, rounded to double, then to float32 (mbx.hip); the reference takes numpy's
    float64 tanh to float32.  The two agree on every generation counter a 20 000-FE episode and its margin can reach."""
    t = np.arange(0, 20000 // 16 + 65)[:, None]
    a = np.tanh(t / STAMPS - 1).astype(np.float32)
    b = np.tanh((t / STAMPS - 1).astype(np.longdouble)).astype(np.float64).astype(np.float32)
    assert np.array_equal(a, b)


def test_numpy_sums_are_what_the_kernel_header_says():
    """np.mean / np.std over 16 costs are pairwise_sum's eight accumulators and tree; a reduction over axis 0 of a (16, D) array adds row after row."""
    rs = np.random.RandomState(3)
    for _ in range(50):
        c = rs.lognormal(0, 3, 16)
        r = [c[k] + c[k + 8] for k in range(8)]
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        assert np.mean(c) == s / 16
        x = (c - s / 16) ** 2
        r = [x[k] + x[k + 8] for k in range(8)]
        assert np.std(c) == np.sqrt((((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) / 16)
        a = rs.randn(16, 7) * rs.lognormal(0, 3, (16, 1))
        acc = np.zeros(7)
        for i in range(16):
            acc = acc + a[i]
        assert np.array_equal(np.sum(a, axis=0), acc)


def test_io_pairs_of_the_reference_modules():
    nets, n64 = TorchNets(POL['bbob/best_x']), F64Nets(POL['bbob/best_x'])
    for g in (0, 7, 20):
        # the reference hands SelfAttn the TRANSPOSE of a (3, 16) array (:95): torch keeps the strides and its matmul rounds differently on a
        # contiguous copy (one ulp in one of these 48 weights), so the stored input goes in column-major, as it was
        assert np.array_equal(nets.attn(np.asfortranarray(POL[f'io/attn_in/{g}'])), POL[f'io/W/{g}'])
        assert np.array_equal(nets.mlp(POL[f'io/mlp_in/{g}']), POL[f'io/alpha/{g}'])
        assert np.allclose(n64.attn(POL[f'io/attn_in/{g}']), POL[f'io/W/{g}'], rtol=1e-5, atol=1e-7)
        assert np.allclose(n64.mlp(POL[f'io/mlp_in/{g}']), POL[f'io/alpha/{g}'], rtol=1e-5, atol=1e-7)
        assert abs(float(POL[f'io/W/{g}'].sum()) - 1) < 1e-6


# ------------------------------------------------------------------------------------------------ CPU: the meta-optimizer
CMA_CONST = ('_weights', '_c1', '_cmu', '_cc', '_c_sigma', '_d_sigma', '_mu_eff', '_chi_n')


@pytest.mark.parametrize('suite', ['bbob', 'bbob-noisy', 'protein'])
def test_cma_constants_equal_the_recorded_ones(suite):
    from metabox_amd.agent.cma import CMA
    opt = CMA(mean=np.zeros(NPARAM), sigma=0.1, population_size=16)
    for k in CMA_CONST:
        got, want = np.asarray(getattr(opt, k), dtype=np.float64), POL[f'{suite}/ckpt0/cma{k}']
        assert got.shape == want.shape and np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (suite, k)
    assert (opt.dim, opt.population_size, opt._mu, opt._cm) == tuple(int(POL[f'{suite}/ckpt0/cma{k}']) for k in ('_n_dim', '_popsize', '_mu', '_cm'))
    assert opt.sigma == float(POL[f'{suite}/ckpt0/cma_sigma']) and np.array_equal(opt.mean, POL[f'{suite}/ckpt0/cma_mean'])
    assert np.sum(opt._weights[:8]) == pytest.approx(1, abs=1e-12) and np.all(opt._weights[8:] < 0)      # active (negative) weights


def test_cma_ask_matches_its_mean_and_sigma():
    """With the recorded _mean / _sigma and a fixed seed, 16 x 64 asks: per coordinate the sample mean lies within 5 standard errors of the mean
    and the pooled standard deviation within 2 % of sigma (246 x 1024 samples); the shipped x_population passes the same pooled check."""
    from metabox_amd.agent.cma import CMA
    mean, sigma = POL['bbob/ckpt0/cma_mean'], float(POL['bbob/ckpt0/cma_sigma'])
    opt = CMA(mean=mean, sigma=sigma, population_size=16, seed=11)
    x = np.stack([opt.ask() for _ in range(1024)])
    assert np.all(np.abs(x.mean(axis=0) - mean) < 5 * sigma / np.sqrt(1024))
    assert abs(x.std() / sigma - 1) < 0.02
    assert abs(POL['bbob/ckpt0/x_population'].std() / sigma - 1) < 0.05
    assert np.array_equal(POL['bbob/ckpt0/best_x'], POL['bbob/ckpt0/x_population'][0])   # les_agent.py:23


def test_cma_minimises_a_sphere():
    """A sanity floor, not a measurement: on the 246-dimensional sphere around (1, ..., 1), from the reference's own construction (mean 0, sigma 0.1,
    16 candidates), the best value of a generation falls by more than a factor of 10 within 200 generations."""
    from metabox_amd.agent.cma import CMA
    opt = CMA(mean=np.zeros(NPARAM), sigma=0.1, population_size=16, seed=5)
    first = None
    for g in range(200):
        xs = [opt.ask() for _ in range(16)]
        vs = [float(np.sum((x - 1.) ** 2)) for x in xs]
        first = min(vs) if first is None else first
        opt.tell(list(zip(xs, vs)))
    assert min(vs) * 10 <= first, (first, min(vs))
    assert opt.generation == 200 and np.all(np.isfinite(opt.mean))


# ------------------------------------------------------------------------------------------------ CPU: ABI and lookup
def test_abi_geometry_of_les():
    from metabox_amd import _abi
    lib = _abi.load_lib()
    assert _abi.ALGO_LES == ALGO_LES
    for D in (2, 10, 40):
        cfg = oracle.make_cfg(ALGO_LES, NP, D, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(cfg)) == 1 and lib.mbx_action_dim(C.byref(cfg)) == 0
        assert lib.mbx_tape_stride(C.byref(cfg)) == tape_stride(D)
    ok = lambda **kw: lib.mbx_state_dim(C.byref(oracle.make_cfg(ALGO_LES, kw.get('np_', NP), kw.get('dim', 10), kw.get('max_fes', 20000), 400, 50)))   # noqa: E731
    lib.mbx_last_error.restype = C.c_char_p
    assert ok() == 1 and ok(max_fes=17) == 1
    for bad in (dict(np_=15), dict(np_=17), dict(np_=100), dict(dim=1), dict(dim=41), dict(max_fes=16)):
        assert ok(**bad) < 0 and b'LES' in lib.mbx_last_error(), bad
    for algo in (12, 14, 17):                                        # stay unassigned
        assert lib.mbx_state_dim(C.byref(oracle.make_cfg(algo, NP, 10, 20000, 400, 50))) < 0
    # the two entry points live in a header of their own: include/mbx_les.h declares exactly them, the library exports them, include/mbx.h keeps its 45
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r'\b(mbx_les_[a-z_]+)\s*\(', open(os.path.join(root, 'include', 'mbx_les.h')).read()))
    assert declared == set(_abi.LES_SYMBOLS) == {'mbx_les_set_params', 'mbx_les_rollout'} and all(hasattr(lib, n) for n in declared)
    assert not declared & set(_abi.EXPORTED_SYMBOLS) and len(_abi.EXPORTED_SYMBOLS) == 45


def test_les_classes_are_found_by_the_lookup():
    from metabox_amd import agent, optimizer
    from metabox_amd.tester import _lookup
    assert _lookup(agent, 'LES_Agent').__name__ == 'LES_Agent' and _lookup(optimizer, 'LES_Optimizer').__name__ == 'LES_Optimizer'


def test_les_agent_host_logic(tmp_path):
    """Construction as the reference's (16 candidates from CMA(0, 0.1), best_x = the first), the z-score / median meta-cost, tell / ask, checkpoints."""
    from metabox_amd.agent import LES_Agent
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--train_agent', 'LES_Agent', '--train_optimizer', 'LES_Optimizer', '--max_learning_step', '100',
                      '--agent_save_dir', str(tmp_path / 'agents') + '/', '--log_dir', str(tmp_path / 'log')])
    a = LES_Agent(copy.deepcopy(cfg))
    assert (a.meta_pop_size, a.skip_step, a.x_population.shape) == (16, 50, (16, NPARAM)) and np.array_equal(a.best_x, a.x_population[0])
    assert any(f.startswith('checkpoint0') for f in os.listdir(cfg.agent_save_dir))
    rs = np.random.RandomState(2)
    scores = rs.lognormal(0, 2, (16, 3))
    for i in range(16):
        a.meta_performances[i] = list(scores[i])
    pop = a.x_population.copy()
    a.train_epoch()
    want = np.median((scores - scores.mean(axis=0)[None]) / scores.std(axis=0)[None], axis=-1)
    assert np.array_equal(a.costs, want) and a.best_les == int(np.argmin(want)) and np.array_equal(a.best_x, pop[np.argmin(want)])
    assert a.optimizer.generation == 1 and not np.array_equal(a.x_population, pop) and a.meta_performances == [[] for _ in range(16)]
    a.load_exported_weights({'best_x': POL['bbob/best_x']})
    assert np.array_equal(a.best_x, POL['bbob/best_x'])


# ------------------------------------------------------------------------------------------------ GPU
def _batch(c, n=1, pidx=None, seeds=None, flags=0, early_stop=True, suite=None, max_fes=None, log_interval=None):
    from metabox_amd.suite import Batch, Suite
    s = suite if suite is not None else Suite([c['p']])
    mf = c['max_fes'] if max_fes is None else max_fes
    return Batch(s, ALGO_LES, [0] * n if pidx is None else pidx, [c['seed'] + k for k in range(n)] if seeds is None else seeds, NP, mf,
                 (mf // c['nlog'] if max_fes is not None else c['log_interval']) if log_interval is None else log_interval, c['nlog'], early_stop=early_stop, flags=flags)


def _tapes(b, tapes):
    import torch
    b.set_tape(torch.from_numpy(np.ascontiguousarray(np.stack(tapes))).cuda())


def _check_head(got, h64, where):
    """(A): the device's W, alpha, mu, sigma, Pc, Ps and children against the float64-network restatement of the same generation."""
    D = len(h64['mu'])
    pairs = dict(W=got['W'], alpha=got['alpha'].reshape(D, 2), mu=got['mu'], sigma=got['sigma'], Pc=got['Pc'].reshape(3, D), Ps=got['Ps'].reshape(3, D),
                 children=got['parents'].reshape(NP, D))
    for q in QUANT:
        assert within(q, pairs[q], h64[q]), (where, q, float(np.nanmax(np.abs(pairs[q] - h64[q]))), e_ref()[q])
    assert np.array_equal(got['z'].reshape(NP, D), h64['z']), (where, 'the stored normals')


def _check_tail(got, rs, where, d=None, r=None):
    """(C): counters, gbest, log, done and reward against the restatement that was fed the DEVICE's costs: exactly."""
    sc = got['scalars']
    assert (sc[SC_GBEST], sc[SC_FES], sc[SC_GEN], sc[SC_LOG_INDEX], sc[SC_COST_LEN]) == (rs.gbest, rs.fes, rs.t, rs.log_index, len(rs.cost)), (where, sc[:8])
    assert np.array_equal(got['cost'][:len(rs.cost)], rs.cost), (where, 'curve')
    assert sc[SC_DONE] == float(rs.done) and sc[SC_INIT_Y] == rs.init_y and sc[SC_CALL_INIT_Y] == rs.call_init_y, (where, sc)
    if d is not None:
        assert bool(d) == bool(r[0]) and np.array_equal(np.float64(r[1]), np.float64(rs.reward), equal_nan=True), (where, d, r, rs.reward)


@pytest.mark.gpu
@pytest.mark.parametrize('case', BUDGET + [SKIP50, SKIP1])
def test_hip_les_one_generation_from_the_reference_state(case):
    """Every recorded generation of a case as one instance of ONE batch (41 to 63 instances: one launch for the whole case): the reference's state
    injected, one tape generation.  (A) W, alpha, mu', sigma', Pc', Ps', children within 4 E_ref + 4 ulp of the float64-network restatement;
    (B) the children's costs close to the reference's and in the reference's order; (C) with the DEVICE's costs, FEs / gbest / log / done / reward
    exactly the restatement's.  skip1x60 runs every generation as the reference's skip_step = 1 call; skip50's generations run under the budget
    rule here (a tape holds one generation), its call is pinned by test_hip_les_skip_call_bookkeeping.  The reset likewise."""
    import torch
    c = _case(case)
    rows, _, t0, _ = replay(case)
    D, cap, n = c['D'], curve_cap(c['max_fes'], c['log_interval'], c['nlog']), len(rows)
    skip = case == SKIP1
    nets = F64Nets(c['best_x'])
    b = _batch(c, n)
    assert b.tape_stride == tape_stride(D) and len(b.read_state(0)) == state_doubles(D, cap)
    b.les_set_params(c['best_x'])
    # ---- the reset: instance 0 on the reset tape
    _tapes(b, [t0] * n)
    b.reset()
    got = split_state(b.read_state(0), D, cap)
    r0 = _restate_for(c)
    assert np.array_equal(got['parents'].reshape(NP, D), r0.reset_head(t0)) and np.array_equal(got['mu'], r0.mu) and np.array_equal(got['sigma'], r0.sigma), case
    assert close(got['costs'], TR[f'{case}/costs'][0]) and np.array_equal(np.argsort(got['costs']), np.argsort(TR[f'{case}/costs'][0])), case
    r0.reset_tail(got['costs'])
    _check_tail(got, r0, (case, 'reset'))
    assert not got['Pc'].any() and not got['Ps'].any()
    # ---- one generation from every recorded state
    for k, r in enumerate(rows):
        rs = copy.deepcopy(r['before'])
        if not skip:
            rs.done = False
        b.write_state(k, rs.block())
    _tapes(b, [r['tape'] for r in rows])
    _, rew, done = b.les_rollout(1, skip=skip)
    torch.cuda.synchronize()
    rew, done = rew.cpu().numpy(), done.cpu().numpy()
    worst = 0.
    for k, r in enumerate(rows):
        got = split_state(b.read_state(k), D, cap)
        rs = copy.deepcopy(r['before'])
        rs.done = False
        _check_head(got, rs.head(r['head']['z'], nets), (case, k))
        ref_costs = TR[f'{case}/costs'][k + 1]
        worst = max(worst, float(np.max(np.abs(got['costs'] - ref_costs) / np.abs(ref_costs))))
        assert close(got['costs'], ref_costs), (case, k, got['costs'], ref_costs)
        assert np.array_equal(np.argsort(got['costs']), np.argsort(ref_costs)), (case, k, 'order of the costs')
        h = dict(r['head'])
        rs.commit(h, got['costs'], (0, 1) if skip else None)
        _check_tail(got, rs, (case, k), done[k], (done[k], rew[k]))
    print(f'{case}: {n} generations, largest relative cost deviation from the reference {worst:.2e}')
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize('case', BUDGET + FULL + [SKIP1])
def test_hip_les_whole_episode_by_tape(case):
    """The whole episode on the feeder's tapes, one launch per generation, on the device's own costs: FEs, the generation counter, done, the length of
    cost and the log positions exact, cost entries and gbest close, argsort of the costs exact at every recorded generation; mu and sigma within
    8 x the largest difference the float64-network restatement (fed the reference's costs, same tapes) shows against the reference over this episode."""
    import torch
    c = _case(case)
    rows, end, t0, _ = replay(case)
    D, cap = c['D'], curve_cap(c['max_fes'], c['log_interval'], c['nlog'])
    skip = case == SKIP1
    gens = [int(g) for g in TR[f'{case}/gens']]
    at = {g: i for i, g in enumerate(gens)}
    thinned = f'{case}/costs_all' in TR
    # the float64-network restatement over the episode, on the reference's costs
    nets, r64 = F64Nets(c['best_x']), _restate_for(c)
    r64.reset_head(t0)
    r64.reset_tail((TR[f'{case}/costs_all'] if thinned else TR[f'{case}/costs'])[0])
    dmu = dsg = 0.
    for r in rows:
        g = r['g']
        r64.commit(r64.head(r['tape'][:NP * D], nets), (TR[f'{case}/costs_all'][g + 1] if thinned else TR[f'{case}/costs'][at[g + 1]]), r['skip'])
        if g + 1 in at:
            dmu = max(dmu, float(np.max(np.abs(r64.mu - TR[f'{case}/mu'][at[g + 1]]))))
            dsg = max(dsg, float(np.max(np.abs(r64.sigma - TR[f'{case}/sigma'][at[g + 1]]))))
    b = _batch(c)
    b.les_set_params(c['best_x'])
    _tapes(b, [t0])
    b.reset()
    wmu = wsg = 0.
    for r in rows:
        g = r['g']
        _tapes(b, [r['tape']])
        _, _, d = b.les_rollout(1, skip=skip)
        if g + 1 in at:
            i = at[g + 1]
            got = split_state(b.read_state(0), D, cap)
            sc = got['scalars']
            assert (sc[SC_FES], sc[SC_GEN], sc[SC_COST_LEN]) == (TR[f'{case}/fes'][i], TR[f'{case}/t'][i], TR[f'{case}/cost_len'][i]), (case, g, sc[:8])
            assert close(sc[SC_GBEST], TR[f'{case}/gbest'][i]) and close(got['costs'], TR[f'{case}/costs'][i]), (case, g)
            assert np.array_equal(np.argsort(got['costs']), np.argsort(TR[f'{case}/costs'][i])), (case, g, 'order of the costs')
            emu, esg = np.abs(got['mu'] - TR[f'{case}/mu'][i]), np.abs(got['sigma'] - TR[f'{case}/sigma'][i])
            wmu, wsg = max(wmu, float(emu.max())), max(wsg, float(esg.max()))
            assert np.all(emu <= 8 * dmu + 4 * np.spacing(np.abs(TR[f'{case}/mu'][i]))), (case, g, 'mu', float(emu.max()), dmu)
            assert np.all(esg <= 8 * dsg + 4 * np.spacing(np.abs(TR[f'{case}/sigma'][i]))), (case, g, 'sigma', float(esg.max()), dsg)
            if not skip:
                assert bool(d[0].item()) == (g + 1 == gens[-1]), (case, g)
    print(f'{case}: float64 restatement against the reference: mu {dmu:.2e} sigma {dsg:.2e}; device against the reference: mu {wmu:.2e} sigma {wsg:.2e}')
    res = b.results()
    st = split_state(b.read_state(0), D, cap)
    n = int(res['cost_len'][0].item())
    assert n == len(TR[f'{case}/cost']) and close(st['cost'][:n], TR[f'{case}/cost']), (case, n)
    assert res['fes'][0].item() == TR[f'{case}/fes_end'] and close(st['scalars'][SC_GBEST], end.gbest)
    if not skip:
        assert close(res['return'][0].item(), TR[f'{case}/call_ret'][-1][1], rtol=1e-5, atol=1e-9), (case, res['return'][0].item(), TR[f'{case}/call_ret'][-1])
        before = b.read_state(0)
        b.les_rollout(1)                                             # a launch after done changes nothing
        assert np.array_equal(before, b.read_state(0), equal_nan=True)
    b.close()


def _mixed_suite():
    """Six problems at D = 10: Sphere, a Gallagher, one function of each noise model, Rastrigin."""
    from metabox_amd.suite import Suite
    ps = [problems('bbob', 10)[1], problems('bbob', 10)[21], problems('bbob-noisy', 10)[101], problems('bbob-noisy', 10)[102],
          problems('bbob-noisy', 10)[103], problems('bbob', 10)[15]]
    return ps, Suite(ps)


def _blocks(b):
    return [b.read_state(k) for k in range(b.B)]


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.gpu
def test_hip_les_routes_are_bit_identical():
    """n one-generation calls against one n-generation call (n = 7, and a run that crosses the episode end), mbx_step against mbx_les_rollout(1, 0),
    MBX_F_ROLLOUT_PER_GENERATION (budget route and a skip_step call): state blocks, state, reward, done and curves bit for bit."""
    import torch
    from metabox_amd import _abi
    from metabox_amd.suite import Batch
    ps, s = _mixed_suite()
    seeds = np.arange(6, dtype=np.uint64) + 900
    mk = lambda flags=0: Batch(s, ALGO_LES, np.arange(6), seeds, NP, 16 * 12, 16 * 12 // 50 or 1, 50, flags=flags)        # noqa: E731   11 generations to the budget
    x = POL['bbob/best_x']
    out = {}
    for name, flags in (('one', 0), ('many', 0), ('step', 0), ('pergen', _abi.F_ROLLOUT_PER_GENERATION)):
        b = mk(flags)
        b.les_set_params(x)
        b.reset()
        rec = []
        for n in (7, 9):                                             # the second run crosses the end after 4 generations
            if name in ('many', 'pergen'):
                st, r, d = b.les_rollout(n)
            else:
                for _ in range(n):
                    st, r, d = b.step(None) if name == 'step' else b.les_rollout(1)
            torch.cuda.synchronize()
            rec.append((_blocks(b), st.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().copy()))
        out[name] = rec
        b.close()
    for name in ('many', 'step', 'pergen'):
        for (ba, sa, ra, da), (bb, sb, rb, db) in zip(out['one'], out[name]):
            assert _same(ba, bb) and np.array_equal(sa, sb) and np.array_equal(ra, rb, equal_nan=True) and np.array_equal(da, db), name
    assert out['one'][1][3].all() and not out['one'][0][3].any()
    # a skip_step = 9 call: resident against one launch per generation
    res = []
    for flags in (0, _abi.F_ROLLOUT_PER_GENERATION):
        b = mk(flags)
        b.les_set_params(x)
        b.reset()
        st, r, d = b.les_rollout(9, skip=True)
        st2, r2, d2 = (t.cpu().numpy().copy() for t in b.les_rollout(5, skip=True))     # runs past the budget, as the reference's call does
        res.append((_blocks(b), st2, r2, d2))
        b.close()
    assert _same(res[0][0], res[1][0]) and all(np.array_equal(p, q, equal_nan=True) for p, q in zip(res[0][1:], res[1][1:]))
    assert res[0][3].all()


def _u53(w0, w1):
    return ((int(w0) >> 5) * 67108864.0 + (int(w1) >> 6)) / 9007199254740992.0


@pytest.mark.gpu
def test_hip_les_philox_run_replays_as_a_tape():
    """Philox for 5 generations on noise-free functions; the normals stored in the state block are fed back, generation by generation, as a tape to a
    second batch that starts from the first one's reset state: identical state blocks."""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = [problems('bbob', 10)[1], problems('bbob', 10)[21], problems('bbob', 10)[15]]
    s = Suite(ps)
    seeds = np.arange(3, dtype=np.uint64) + 77
    a, b = (Batch(s, ALGO_LES, np.arange(3), seeds, NP, 2000, 40, 50) for _ in range(2))
    for x in (a, b):
        x.les_set_params(POL['bbob/best_x'])
        x.reset()
    for k in range(3):
        b.write_state(k, a.read_state(k))
    for g in range(5):
        a.les_rollout(1)
        tapes = []
        for k in range(3):
            t = np.zeros(tape_stride(10))
            t[:NP * 10] = split_state(a.read_state(k), 10, curve_cap(2000, 40, 50))['z']
            tapes.append(t)
        _tapes(b, tapes)
        b.les_rollout(1)
        torch.cuda.synchronize()
        assert _same(_blocks(a), _blocks(b)), g
    z = np.concatenate([split_state(a.read_state(k), 10, curve_cap(2000, 40, 50))['z'] for k in range(3)])
    assert abs(z.mean()) < 0.2 and 0.8 < z.std() < 1.2 and len(np.unique(z)) == len(z)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize('D', [2, 7, 8, 10, 12, 33, 40])
def test_hip_les_kernel_against_the_restatement_on_its_own_costs(D):
    """Philox route, 12 generations, one launch each: every generation is restated with float64 networks from the device's previous block, the
    device's stored normals and the device's costs: the arithmetic within 4 E_ref + 4 ulp, the bookkeeping exactly.  D = 10 carries a Gallagher and
    one function of each noise model, D = 12 the protein instance."""
    import torch
    from metabox_amd.suite import Batch, Suite
    if D == 12:
        ps, x = [_protein()['1AVX_1']], POL['protein/best_x']
    elif D == 10:
        ps, x = _mixed_suite()[0], POL['bbob-noisy/best_x']
    else:
        ps, x = [problems('bbob', D)[8], problems('bbob-noisy', D)[102]], POL['bbob/best_x']
    s = Suite(ps)
    B, max_fes = len(ps), 16 * 11 if D != 12 else 1000
    b = Batch(s, ALGO_LES, np.arange(B), np.arange(B, dtype=np.uint64) + 5 * D, NP, max_fes, max_fes // 50, 50)
    cap = curve_cap(max_fes, max_fes // 50, 50)
    b.les_set_params(x)
    b.reset()
    nets = F64Nets(x)
    prev = _blocks(b)
    for g in range(12):
        _, rew, done = b.les_rollout(1)
        torch.cuda.synchronize()
        rew, done = rew.cpu().numpy(), done.cpu().numpy()
        cur = _blocks(b)
        for k, p in enumerate(ps):
            rs = Restate(D, float(p.lb), float(p.ub), max_fes, max_fes // 50, 50, D != 12).load(prev[k])
            got = split_state(cur[k], D, cap)
            if rs.done:
                assert np.array_equal(prev[k], cur[k], equal_nan=True) and done[k], (D, g, k, 'a finished instance stays frozen')
                continue
            h = rs.head(got['z'], nets)
            _check_head(got, h, (D, g, k))
            rs.commit(h, got['costs'])
            _check_tail(got, rs, (D, g, k), done[k], (done[k], rew[k]))
        prev = cur
    assert all(split_state(blk, D, cap)['scalars'][SC_DONE] == (D != 12) for blk in prev)
    b.close()


@pytest.mark.gpu
def test_hip_les_skip_call_bookkeeping():
    """One skip_step = 50 call in ONE launch against the restatement: the same instance is stepped one generation at a time under the budget rule
    (bit-identical evolution, test_hip_les_routes_are_bit_identical), its costs and normals feed the restatement's skip route, and the call's curve,
    FEs, init_y, reward and is_end must equal it exactly.  Then skip_step = 1 sixty times: the closing entry fills the list, then overwrites its end."""
    import torch
    c = _case(SKIP50)
    D, cap = c['D'], curve_cap(c['max_fes'], c['log_interval'], c['nlog'])
    a, b, e = _batch(c), _batch(c), _batch(c)
    for x in (a, b, e):
        x.les_set_params(c['best_x'])
        x.reset()
    rs, r1 = _restate_for(c).load(a.read_state(0)), _restate_for(c).load(a.read_state(0))
    nets = F64Nets(c['best_x'])
    lens = []
    for g in range(60):
        a.les_rollout(1)
        _, rew1, d1 = e.les_rollout(1, skip=True)
        got = split_state(a.read_state(0), D, cap)
        h = dict(mu=got['mu'], sigma=got['sigma'], Pc=got['Pc'].reshape(3, D), Ps=got['Ps'].reshape(3, D), children=got['parents'].reshape(NP, D), z=got['z'])
        if g < 50:
            rs.commit(dict(h), got['costs'], (g, 50))
        r1.commit(dict(h), got['costs'], (0, 1))
        ge = split_state(e.read_state(0), D, cap)
        assert np.array_equal(ge['parents'], got['parents']) and np.array_equal(ge['mu'], got['mu'])
        _check_tail(ge, r1, ('skip1', g), d1[0].item(), (True, rew1[0].item()))
        lens.append(len(r1.cost))
    assert lens[-1] == 51 and lens[-5:] == [51] * 5 and r1.fes == 16 + 16 * 60
    _, rew, d = b.les_rollout(50, skip=True)
    torch.cuda.synchronize()
    gb = split_state(b.read_state(0), D, cap)
    _check_tail(gb, rs, 'skip50', d[0].item(), (True, rew[0].item()))
    assert len(rs.cost) == len(TR[f'{SKIP50}/cost']) and rs.fes == TR[f'{SKIP50}/fes_end']
    for x in (a, b, e):
        x.close()


@pytest.mark.gpu
def test_hip_les_parameters_are_per_instance():
    """Three parameter sets, a non-monotone set_of_instance over six instances: every instance equals the same instance run alone with its set, bit for
    bit; changing a neighbour's set or problem changes nothing; a finished instance stays frozen while its neighbours run on."""
    import torch
    from metabox_amd.suite import Batch
    ps, s = _mixed_suite()
    sets = np.stack([POL['bbob/best_x'], POL['bbob-noisy/best_x'], POL['protein/best_x']])
    of = np.array([2, 0, 1, 1, 0, 2])
    pidx, seeds = np.arange(6), np.arange(6, dtype=np.uint64) + 31

    def run(pidx, seeds, sets, of, gens=(5, 4)):
        b = Batch(s, ALGO_LES, pidx, seeds, NP, 16 * 8, 2, 50)       # 7 generations to the budget: the second call crosses it
        b.les_set_params(sets, of)
        b.reset()
        out = []
        for n in gens:
            st, r, d = b.les_rollout(n)
            torch.cuda.synchronize()
            out.append((_blocks(b), r.cpu().numpy().copy(), d.cpu().numpy().copy()))
        b.close()
        return out
    full = run(pidx, seeds, sets, of)
    for k in range(6):
        alone = run(pidx[k:k + 1], seeds[k:k + 1], sets[of[k]], None)
        for (bf, rf, df), (ba, ra, da) in zip(full, alone):
            assert np.array_equal(bf[k], ba[0], equal_nan=True) and np.array_equal(rf[k], ra[0], equal_nan=True) and df[k] == da[0], k
    assert not _same([full[0][0][0]], [run(pidx[:1], seeds[:1], sets[0], None)[0][0][0]])        # ... and the set matters
    other = run(np.array([0, 5, 2, 3, 4, 5]), seeds, sets, np.array([2, 1, 1, 1, 0, 2]))         # instance 1: another problem and another set
    for k in (0, 2, 3, 4, 5):
        assert np.array_equal(full[1][0][k], other[1][0][k], equal_nan=True), k
    # a finished instance stays frozen while its neighbours run on: instance 0 is injected as done
    b = Batch(s, ALGO_LES, pidx, seeds, NP, 16 * 8, 2, 50)
    b.les_set_params(sets, of)
    b.reset()
    blk = b.read_state(0)
    o = len(blk) - curve_cap(128, 2, 50) - 16
    blk[o + SC_DONE] = 1.
    b.write_state(0, blk)
    _, _, d = b.les_rollout(3)
    torch.cuda.synchronize()
    assert np.array_equal(b.read_state(0), blk, equal_nan=True) and d[0].item() == 1 and not d[1:].any()
    assert all(split_state(b.read_state(k), 10, curve_cap(128, 2, 50))['scalars'][SC_GEN] == 3 for k in range(1, 6))
    from metabox_amd._abi import MbxError
    with pytest.raises(MbxError):
        b.les_set_params(sets, np.array([0, 1, 2, 3, 0, 0]))          # a set index outside the table
    b.close()
    b = Batch(s, ALGO_LES, pidx, seeds, NP, 16 * 8, 2, 50)
    b.reset()
    with pytest.raises(MbxError, match='mbx_les_set_params'):
        b.les_rollout(1)                                             # no parameters yet: an error, not a launch
    with pytest.raises(MbxError, match='mbx_les_set_params'):
        b.step(None)
    b.close()


@pytest.mark.gpu
def test_hip_les_crafted_states():
    """Equal costs order by (cost, row); all 16 costs equal (std = 0: the 1e-8 guard gives finite W); gbest exactly 1e-8 stops with early_stop and not
    without; a sigma with a zero entry makes Ps inf / nan exactly as numpy does; every coordinate clipped."""
    import torch
    c = _case(BUDGET[0])
    D, cap = c['D'], curve_cap(20000, 400, 50)
    nets = F64Nets(c['best_x'])
    base = _restate_for(dict(c, max_fes=20000, log_interval=400))
    rsd = np.random.RandomState(8)
    tape = np.zeros(tape_stride(D))
    tape[:D] = rsd.rand(D)
    tape[D:D + NP * D] = rsd.standard_normal(NP * D)
    base.reset_head(tape)
    base.reset_tail(rsd.lognormal(5, 1, NP) + 800.)
    crafted = []
    r = copy.deepcopy(base)                                          # 0: ties -- rows 3, 9 and 12 share the lowest cost, 5 and 6 another
    r.costs[[3, 9, 12]] = r.costs.min()
    r.costs[6] = r.costs[5]
    r.gbest = float(r.costs.min())
    crafted.append(r)
    r = copy.deepcopy(base)                                          # 1: all equal
    r.costs[:] = 812.5
    r.gbest = 812.5
    crafted.append(r)
    r = copy.deepcopy(base)                                          # 2: a zero entry of sigma (and a parent equal to mu there: 0 / 0)
    r.sigma[4] = 0.
    r.parents[7, 4] = r.mu[4]
    crafted.append(r)
    crafted.append(copy.deepcopy(base))                              # 3: every coordinate clipped: its tape holds normals of +- 1e6
    r = copy.deepcopy(base)                                          # 4 / 5: gbest exactly 1e-8
    r.gbest = 1e-8
    r.cost = [1e-8]
    crafted += [r, copy.deepcopy(r)]
    z = rsd.standard_normal(NP * D)
    t = np.zeros(tape_stride(D))
    t[:NP * D] = z
    z3 = np.tile(np.where(np.arange(D) % 2 == 0, 1e6, -1e6), NP)
    t3 = np.zeros(tape_stride(D))
    t3[:NP * D] = z3
    res = []
    for early in (True, False):
        b = _batch(c, 6, early_stop=early, max_fes=20000)
        b.les_set_params(c['best_x'])
        for k, r in enumerate(crafted):
            b.write_state(k, r.block())
        _tapes(b, [t, t, t, t3, t, t])
        _, rew, done = b.les_rollout(1)
        torch.cuda.synchronize()
        res.append(([split_state(b.read_state(k), D, cap) for k in range(6)], done.cpu().numpy().copy()))
        b.close()
    (got, done), (got_ne, done_ne) = res
    for k, r in enumerate(crafted):
        h = copy.deepcopy(r).head(z3 if k == 3 else z, nets)
        _check_head(got[k], h, ('crafted', k))
        assert np.all(np.isfinite(got[k]['W'])) and abs(got[k]['W'].sum() - 1) < 1e-5, k
    ps = got[2]['Ps'].reshape(3, D)
    assert not np.all(np.isfinite(ps[:, 4])) and np.all(np.isfinite(np.delete(ps, 4, axis=1))), ps[:, 4]
    ch = got[3]['parents'].reshape(NP, D)
    assert np.array_equal(ch, np.tile(np.where(np.arange(D) % 2 == 0, 5., -5.), (NP, 1)))
    assert list(done) == [0, 0, 0, 0, 1, 1] and not done_ne.any()
    assert got[4]['scalars'][SC_GBEST] == 1e-8 and got[4]['scalars'][SC_COST_LEN] == 2 and got_ne[4]['scalars'][SC_COST_LEN] == 1


# ------------------------------------------------------------------------------------------------ GPU: the agent
def _config(tmp_path, extra=()):
    from metabox_amd.config import get_config
    return get_config(['--problem', 'bbob', '--dim', '10', '--train_agent', 'LES_Agent', '--train_optimizer', 'LES_Optimizer', '--max_learning_step', '1000',
                       '--agent_save_dir', str(tmp_path / 'agents') + '/', '--log_dir', str(tmp_path / 'log')] + list(extra))


@pytest.mark.gpu
def test_les_agent_rollout_batch_and_train_batch(tmp_path):
    import torch
    from metabox_amd.agent import LES_Agent
    from metabox_amd.distributed import instance_table, philox_seed
    from metabox_amd.environment import BatchedPBO_Env
    from metabox_amd.optimizer import LES_Optimizer
    from metabox_amd.suite import Suite
    cfg = _config(tmp_path, ['--train_batch_size', '16'])
    cfg.maxFEs, cfg.log_interval = 16 * 21, 16 * 21 // cfg.n_logpoint
    ps = [problems('bbob', 10)[1], problems('bbob', 10)[21], problems('bbob-noisy', 10)[102]]
    s = Suite(ps)
    opt = LES_Optimizer(copy.deepcopy(cfg))
    agent = LES_Agent(copy.deepcopy(cfg)).load_exported_weights({'best_x': POL['bbob/best_x']})
    # ---- rollout_batch on 3 problems x 2 runs equals chunk-by-chunk les_rollout calls
    pidx, run = instance_table(3, 2)
    seeds = philox_seed(run, np.arange(6))
    env = BatchedPBO_Env(ps, opt, pidx, seeds, suite=s)
    out = agent.rollout_batch(env, chunk=8)
    b = opt.make_batch(s, pidx, seeds)
    b.les_set_params(POL['bbob/best_x'])
    b.reset()
    for n in (8, 8, 4):
        b.les_rollout(n)
    ref = b.results()
    for k in ('cost', 'fes', 'return', 'steps', 'cost_len'):
        assert torch.equal(out[k], ref[k]), k
    assert (out['fes'] == 16 * 21).all() and (out['steps'] == 20).all()
    env.close()
    b.close()
    # ---- train_batch on 2 problems x 16 candidates
    pidx, run = instance_table(2, 16)
    seeds = philox_seed(run, np.arange(32), epoch_salt=1)
    env = BatchedPBO_Env(ps, opt, pidx, seeds, suite=s)
    pop, ls = agent.x_population.copy(), agent.learn_steps
    exceed, info = agent.train_batch(env)
    assert info['scores'].shape == (16, 2) and agent.learn_steps == ls + 2 == info['learn_steps'] and not exceed
    assert not np.array_equal(agent.x_population, pop) and agent.optimizer.generation == 1
    for i in (0, 7, 15):
        for j in range(2):
            one = opt.make_batch(s, [j], [seeds[j * 16 + i]])
            one.les_set_params(pop[i])
            one.reset()
            st, _, _ = one.les_rollout(50, skip=True)
            assert st[0, 0].item() == info['scores'][i, j], (i, j)
            one.close()
    env.close()
    bad = LES_Agent(copy.deepcopy(_config(tmp_path, ['--train_batch_size', '8'])))
    env = BatchedPBO_Env(ps, opt, *instance_table(2, 8)[:1], philox_seed(np.arange(16), np.arange(16)), suite=s)
    with pytest.raises(ValueError, match='train_batch_size'):
        bad.train_batch(env)
    env.close()


@pytest.mark.gpu
def test_les_optimizer_is_the_b1_view(tmp_path):
    """LES_Optimizer.update through PBO_Env returns the reference's 4-tuple, and the same cost list as the batch route for that seed."""
    import torch
    from metabox_amd.environment import PBO_Env
    from metabox_amd.optimizer import LES_Optimizer
    from metabox_amd.suite import Suite
    cfg = _config(tmp_path)
    cfg.maxFEs, cfg.log_interval = 16 * 61, 16 * 61 // cfg.n_logpoint
    p = problems('bbob', 10)[8]
    Suite([p])
    opt = LES_Optimizer(copy.deepcopy(cfg))
    env = PBO_Env(p, opt)
    np.random.seed(4)
    assert env.reset() is None and opt.FEs == opt.fes == 16 and len(opt.cost) == 1
    x = POL['bbob/best_x']
    out = env.step({'attn': x[:NATTN], 'mlp': x[NATTN:]})
    assert len(out) == 4 and out[2] is True and out[3] == {} and out[0] == opt.evolution_info['gbest'] == opt.cost[-1]
    assert opt.FEs == 16 * 61 and opt.evolution_info['generation_counter'] == 60 and opt.evolution_info['mu'].shape == (10,)
    assert len(opt.cost) == 52                                       # the reference's list at this budget: longer than n_logpoint + 1
    np.random.seed(4)
    seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
    b = opt.make_batch(p._bound_suite(), [p._suite_index], [seed])
    b.les_set_params(x)
    b.reset()
    _, r, d = b.les_rollout(60)
    torch.cuda.synchronize()
    st = split_state(b.read_state(0), 10, curve_cap(cfg.maxFEs, cfg.log_interval, cfg.n_logpoint))
    assert opt.cost == [float(v) for v in st['cost'][:int(st['scalars'][SC_COST_LEN])]] and out[1] == r[0].item() and d[0].item() == 1
    np.random.seed(4)
    env.reset()
    o2 = env.step({'attn': x[:NATTN], 'mlp': x[NATTN:], 'skip_step': 5})
    assert o2[2] is True and opt.FEs == 16 * 6 and opt.evolution_info['generation_counter'] == 5
    b.close()
