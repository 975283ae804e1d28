"""The four stand-alone policy kernels against exact host restatements (tests/policy_exact.py).

CPU: the tools are tested themselves -- `fma32` against fractions.Fraction, E32 measured and printed, every E_ref measured on the inputs the
GPU tests use and shown to be below the tolerance of the kernel's older test, and every planted defect shown rejected (draw: sine for
cosine, words (z, w), index j + 1, generation word gen, episode word 0, seed high word dropped; chain: k descending, pairwise, bias last,
double rounding; rule: GLEET biased variance, GLEET softmax scale dropped, RL-PSO sigma affine).

GPU: * every sampled action of mbx_gauss_policy (both variants), mbx_lde_policy and mbx_gleet_policy is recomputed from oracle.philox, the
       kernel's own (mu, sigma) and the generation / episode words of the instance's scalar block: 16 E32 sigma + 4 ulp, clamp / re-fold
       decisions the host's, seeds with the high word set, after 0 / 1 / 3 steps, a second reset and a rebind;
     * mbx_ddqn_qnet's Q values bit for bit five `chain32` layers, every action their first maximum;
     * mbx_lde_policy's mu bit for bit `chain32` of the device's own h', sigma / h' / c' within the E_ref rule of the float64 cell applied to
       the exact gate chains, at both compile-time instantiations and at run-time shapes off every tile size;
     * mbx_gauss_policy's (mu, sigma) within the rule at the shipped and at seeded shapes, and every probed row of the actor table bit for
       bit the (mu, sigma) of mbx_gauss_policy at state k / maxFEs (rows on both sides of every multiple of the grid stride);
     * mbx_gleet_policy's (mu, sigma) within the rule at NP 4 .. 128 on planted swarms.

Not pinned: whether u1 carries its + 1 offset (it shows at one Philox word in 2^24: x >> 8 == 0 gives log(0) without it), and torch's own
generator on the PyTorch routes (Normal.sample / randn_like), which has no counterpart here -- the kernels replace it by Philox.

Measured figures (E_ref, E32, the device's worst fraction of each bound, undecided-edge counts): docs/EXPERIMENTS.md, "Policy kernels
against exact host restatements"."""
import math
from fractions import Fraction

import numpy as np
import pytest

import policy_exact as pe
from helpers import load, problems
from policy_exact import F32, POLICY_RLEPSO, POLICY_RLPSO, SC_EPISODE, SC_GEN

ALGO_RLEPSO, ALGO_LDE, ALGO_DEDDQN, ALGO_RLPSO, ALGO_GLEET = 1, 2, 3, 5, 6
OLD_TOL = {'gauss': 2e-6, 'lstm': 5e-6, 'gleet': 2e-4}             # the tolerances of the kernels' older tests: E_ref must be below them
MASK64 = 0xFFFFFFFFFFFFFFFF


def _report(*parts):
    print('POLICY_EXACT', *parts)


# ================================================================================================ shared inputs (CPU and GPU tests)
def _cfg(problem='bbob', dim=10):
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', problem, '--dim', str(dim), '--device', 'cpu'])
    cfg.agent_save_dir = None
    return cfg


def _shipped(kind):
    """Packed float32 weights (numpy) of the shipped policies, through the agents' own packers."""
    if kind == 'rlepso':
        from metabox_amd.agent.rlepso_agent import RLEPSO_Agent
        a = RLEPSO_Agent(_cfg()).load_exported_weights(load('rlepso_policy.npz')).actor
        return a.packed_weights().numpy().copy(), (1,) + tuple(a.hidden_sizes()) + (35,), float(a.min_sigma), float(a.max_sigma)
    if kind == 'lde':
        from metabox_amd.agent.lde_agent import LDE_Agent
        return LDE_Agent(_cfg('bbob-noisy', 30)).load_exported_weights(load('lde_policy.npz')).net.packed_weights().numpy().copy()
    if kind == 'ddqn':
        from metabox_amd.agent.de_ddqn_agent import DE_DDQN_Agent
        return DE_DDQN_Agent(_cfg('protein', 12)).load_exported_weights(load('ddqn_policy.npz')).packed_weights().numpy().copy()
    raise KeyError(kind)


def _gleet_actor():
    from metabox_amd.agent import GLEET_Agent
    return GLEET_Agent(_cfg()).load_exported_weights(load('gleet_policy.npz')).actor


MAX_FES, NP_RL = 20000, 100
TABLE_ROWS = MAX_FES + 2 * NP_RL + 1                          # mbx_rlepso_policy_table_rows
GAUSS_B = (1, 3, 4, 5, 9)                                     # 9 rows: the second trip of the grid-stride loop at two blocks of four waves
GAUSS_CASES = ([('rlepso', 'shipped', (1, 64, 32, 35)), ('rlepso', 'seeded', (1, 5, 3, 35)), ('rlepso', 'seeded', (1, 100, 65, 35))] +
               [('rlpso', 'seeded', (2 * D, h1, h2, 1)) for D in (2, 10, 40) for h1, h2 in ((32, 8), (1, 1))])


def _gauss_case(case):
    """weights, dims, (min_sigma, max_sigma), variant and the states [B, in] of every launch of a Gaussian-MLP case."""
    algo, src, dims = case
    rs = np.random.RandomState(1000 + 7 * dims[0] + dims[1])
    if src == 'shipped':
        w, d, lo, hi = _shipped('rlepso')
        assert d == dims
    else:
        w, lo, hi = pe.seeded_gauss(rs, *dims), 0.01, 0.7
    variant = POLICY_RLPSO if algo == 'rlpso' else POLICY_RLEPSO
    IN = dims[0]
    if algo == 'rlepso':
        pool = [0.0, 1.0, (TABLE_ROWS - 1) / MAX_FES] + list(rs.rand(6))       # 0, 1, the largest row index over maxFEs, uniform
        states = {B: np.array([[pool[(i + B) % len(pool)]] for i in range(B)]) for B in GAUSS_B}
        sat = None
    else:
        # rows of +-1e3 on which both heads saturate (|pre-activation| > 20: tanh is exactly +-1 in float32 and float64, so mu is exactly 0 or 1 on
        # the host and on the device) or are switched off, of both signs of the mu head where the net has them; plus 0, 1 and uniform rows
        cand = rs.choice([-1e3, 1e3], size=(256, IN))
        nets = [[p.astype(np.float64) for p in parts] for parts in pe.gauss_split(w, *dims)]
        am, as_ = pe._mlp(nets[0], cand, np)[:, 0], pe._mlp(nets[1], cand, np)[:, 0]
        dead = [np.all(cand @ net[0] + net[1] <= 0, axis=1) for net in nets]          # first layer all off: the head is a constant, exactly
        ok = ((np.abs(am) > 20) | dead[0]) & ((np.abs(as_) > 20) | dead[1])
        hi_rows, lo_rows = cand[ok & (am > 20)][:2], cand[ok & (am < -20)][:2]
        sat = np.concatenate([hi_rows, lo_rows, cand[ok][:2]])
        assert len(sat) >= 2 and (dims[1] == 1 or len(hi_rows) + len(lo_rows) >= 1), case
        pool = [np.zeros(IN), np.ones(IN)] + list(sat) + [rs.rand(IN) for _ in range(4)] + [rs.rand(IN) * 10 - 5 for _ in range(2)]
        states = {B: np.stack([pool[(i + B) % len(pool)] for i in range(B)]) for B in GAUSS_B}
    return w, dims, (lo, hi), variant, states, sat


LSTM_SHAPES = [(50, 50), (100, 50), (30, 7), (4, 64), (30, 64), (4, 7)]      # (NP, hidden): in = NP + 10, out = 2 NP
LSTM_B = (1, 16, 17, 37)


def _lstm_case(NP, H):
    """weights and the (x, h, c) of every launch: uniform states with random (h, c), h = c = 0, (h, c) scaled to saturate the gates, and the
    reference's recorded I/O at the shipped shape."""
    IN, A = NP + 10, 2 * NP
    rs = np.random.RandomState(2000 + 13 * NP + H)
    w = _shipped('lde') if (NP, H) == (50, 50) else pe.seeded_lstm(rs, IN, H, A)
    launches = []
    for B in LSTM_B:
        x = rs.rand(B, IN)
        h, c = (rs.randn(B, H) * 0.5).astype(F32), rs.randn(B, H).astype(F32)
        launches.append(('uniform', x, h, c))
        launches.append(('zero_hc', rs.rand(B, IN), np.zeros((B, H), F32), np.zeros((B, H), F32)))
        launches.append(('saturated', rs.rand(B, IN), (np.sign(rs.randn(B, H)) * 30).astype(F32), (rs.randn(B, H) * 8).astype(F32)))
    if (NP, H) == (50, 50):
        pol = load('lde_policy.npz')
        launches.append(('recorded', pol['io/x'][0].astype(np.float64), pol['io/h'][0], pol['io/c'][0]))
    return w, (IN, H, A), [(k, pe.f32_64(x), h, c) for k, x, h, c in launches]


def _lstm_host(parts, x, h, c, h_dev=None):
    """gate chains, float64 (h', c'), their torch float32 evaluation, and the heads from `h_dev` (the device's h', or the host's rounded)."""
    gates = pe.lstm_gates32(parts, x, h)
    h64, c64 = pe.lstm_cell64(gates, c)
    h32, c32 = pe.lstm_cell_torch32(gates, c)
    hd = h64.astype(F32) if h_dev is None else h_dev
    mu = pe.chain32(hd, parts['WmuT'], parts['bmu'])
    pre = pe.chain32(hd, parts['WsgT'], parts['bsg'])
    return {'gates': gates, 'h64': h64, 'c64': c64, 'h32': h32, 'c32': c32, 'mu': mu, 'sigma64': pe.sigmoid64(pre), 'sigma32': pe.sigmoid_torch32(pre)}


GLEET_NP = (4, 5, 63, 64, 65, 100, 127, 128)


def _gleet_case(NP, actor64):
    rs = np.random.RandomState(3000 + NP)
    ins = pe.gleet_inputs(rs, NP, actor64, load('gleet_policy.npz')['io/x'].astype(np.float64))
    names = list(ins)
    while len(names) % 3:
        names.append(names[len(names) % len(ins)])
    return ins, [names[i:i + 3] for i in range(0, len(names), 3)]


def _gleet_both(actor32, actor64, x):
    import torch
    x = np.ascontiguousarray(x)
    return pe.gleet_forward(actor32, torch.from_numpy(x.astype(F32))), pe.gleet_forward(actor64, torch.from_numpy(x))


def _actors():
    import copy
    a32 = _gleet_actor()
    return a32, copy.deepcopy(a32).double()


# ================================================================================================ CPU: the tools
def _nearest_f32(exact, r):
    """True when float32 r is the correctly rounded (nearest, ties to even) value of the Fraction `exact`."""
    r = F32(r)
    lo, hi = np.nextafter(r, F32(-np.inf)), np.nextafter(r, F32(np.inf))
    d, dl, dh = abs(exact - Fraction(float(r))), abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi)))
    if d > dl or d > dh:
        return False
    if d == dl or d == dh:
        return int(np.array(r).view(np.uint32)) & 1 == 0
    return True


PLANTED = (8392705 * 2.0 ** -35, 8384513 * 2.0 ** -35, 1.0)        # a b = 2^-24 (1 + 2^-46) (1 + ...): the sum sits just above the tie at 1 + 2^-24


def test_fma32_is_correctly_rounded():
    a, b, c = (F32(v) for v in PLANTED)
    assert float(a) == PLANTED[0] and float(b) == PLANTED[1]
    exact = Fraction(float(a)) * Fraction(float(b)) + 1
    assert exact > 1 + Fraction(1, 2 ** 24) and exact - (1 + Fraction(1, 2 ** 24)) < Fraction(1, 2 ** 60)
    assert pe.fma32(a, b, c) == F32(1 + 2.0 ** -23) and pe.fma32_double(a, b, c) == F32(1.0)      # double rounding loses the sticky bit
    rs = np.random.RandomState(7)
    n = 25_000
    blocks = []
    # mixed magnitudes
    m = lambda k: (rs.uniform(1, 2, k) * rs.choice([-1, 1], k) * 2.0 ** rs.randint(-30, 31, k)).astype(F32)
    blocks.append((m(n), m(n), m(n)))
    # cancellation: c = -(a b rounded), perturbed by a few ulp
    a1, b1 = m(n), m(n)
    c1 = -(a1.astype(np.float64) * b1).astype(F32)
    c1 = (c1.view(np.int32) + rs.randint(-3, 4, n).astype(np.int32)).view(F32)
    blocks.append((a1, b1, c1))
    # near ties: c = 1 and a b close to odd multiples of 2^-24, within 2^-24 2^-[20, 30]
    a2 = rs.uniform(1, 2, n).astype(F32)
    t = (2 * rs.randint(0, 8, n) + 1) * 2.0 ** -24 * (1 + rs.choice([-1, 1], n) * 2.0 ** -rs.randint(20, 31, n))
    blocks.append((a2, (t / a2).astype(F32), np.ones(n, F32)))
    # subnormal results and operands
    blocks.append(((rs.uniform(1, 2, n) * 2.0 ** rs.randint(-80, -60, n)).astype(F32), m(n) * F32(2.0 ** -60), (rs.uniform(-1, 1, n) * 2.0 ** -140).astype(F32)))
    a, b, c = (np.concatenate([blk[i] for blk in blocks]) for i in range(3))
    assert a.size >= 100_000 and np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(c))
    got, dbl = pe.fma32(a, b, c), pe.fma32_double(a, b, c)
    assert np.all(np.isfinite(got))
    for k in range(a.size):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        assert _nearest_f32(exact, got[k]), (k, a[k], b[k], c[k], got[k])
    _report('fma32', f'{a.size} triples correctly rounded; the double-rounding form differs on {int((got != dbl).sum())} of them')


def test_chain_check_rejects_planted_orders():
    """Bit equality with chain32 is the check: each planted order or rounding gives other bits."""
    rs = np.random.RandomState(3)
    x, Wt, bias = rs.rand(17, 99).astype(F32), rs.uniform(-0.1, 0.1, (99, 100)).astype(F32), rs.uniform(-0.1, 0.1, 100).astype(F32)
    want = pe.chain32(x, Wt, bias)
    ref = x.astype(np.float64) @ Wt.astype(np.float64) + bias
    assert np.abs(want - ref).max() < 1e-5                           # the chain is a dot product
    for defect in ('k_descending', 'pairwise', 'bias_last'):
        got = pe.chain32(x, Wt, bias, defect)
        assert np.abs(got - ref).max() < 1e-5 and not np.array_equal(got.view(np.uint32), want.view(np.uint32)), defect
        _report('chain defect', defect, f'rejected: {int((got != want).sum())} of {want.size} units differ')
    # double rounding differs on one triple in ~2^29: the planted one, as the last step of a chain
    a, b, c = PLANTED
    xs = np.array([[0.5, 1.0, a]], F32); W = np.array([[1.0], [0.5], [b]], F32); bs = np.array([0.0], F32)
    assert pe.chain32(xs, W, bs)[0, 0] == F32(1 + 2.0 ** -23) and pe.chain32(xs, W, bs, 'double_rounding')[0, 0] == F32(1.0)
    _report('chain defect', 'double_rounding', 'rejected on the planted triple')


def test_e32_is_measured():
    E32 = pe.e32()
    _report('E32', f'{E32:.3e} over {pe.E32_WORDS} Philox words; the device is allowed {pe.DRAW_FACTOR} E32 = {pe.DRAW_FACTOR * E32:.3e} on the deviate')
    assert 2e-7 < E32 < 4e-6
    seeds, gens, eps = pe.draw_word_set_meta(pe.E32_WORDS)
    words = pe.draw_word_set(pe.E32_WORDS)
    assert pe.normal64(seeds[3], 7, gens[3], eps[3]) == pe.normal64_of_words(words[3 * 200 + 7])
    n = pe.normal64_of_words(words)
    assert abs(n.mean()) < 4 / math.sqrt(n.size) and abs(n.var() - 1) < 0.01 and np.abs(n).max() < 5.8      # sqrt(-2 ln 2^-24) = 5.77


N_DRAWS = 10_000


def _draw_inputs(variant):
    seeds, gens, eps = pe.draw_word_set_meta(N_DRAWS)
    words = pe.draw_word_set(N_DRAWS)
    rs = np.random.RandomState(5)
    if variant == POLICY_RLPSO:
        mu, sigma = rs.uniform(0.02, 0.05, N_DRAWS).astype(F32), rs.uniform(0.3, 0.7, N_DRAWS).astype(F32)
    else:
        mu, sigma = rs.uniform(0.4, 0.6, N_DRAWS).astype(F32), rs.uniform(0.01, 0.06, N_DRAWS).astype(F32)     # clamps beyond 6 sigma: every draw shows
    return seeds, gens, eps, words, mu, sigma


@pytest.mark.parametrize('variant', [POLICY_RLEPSO, POLICY_RLPSO])
def test_float32_sampler_passes_the_draw_check(variant):
    _, _, _, words, mu, sigma = _draw_inputs(variant)
    got = pe.sample32(variant, mu, sigma, words)
    msg, st = pe.check_draws(got, mu, sigma, pe.normal64_of_words(words), variant, pe.e32())
    _report('draw check, numpy float32 sampler', 'variant', variant, st)
    assert msg is None and st['worst'] <= 1.0 / pe.DRAW_FACTOR + 0.05, (msg, st)
    if variant == POLICY_RLPSO:
        assert 0.1 * N_DRAWS < st['folded'] < 0.9 * N_DRAWS


@pytest.mark.parametrize('variant', [POLICY_RLEPSO, POLICY_RLPSO])
@pytest.mark.parametrize('defect', pe.DRAW_DEFECTS)
def test_draw_check_rejects(defect, variant):
    """A device that makes the planted mistake is rejected on > 99 % of 1e4 draws."""
    seeds, gens, eps, words, mu, sigma = _draw_inputs(variant)
    if defect == 'episode_zero':
        eps = [1] * len(eps)
    if defect == 'seed_high_dropped':
        seeds = [(0x9E3779B97F4A7C15 + k) & MASK64 for k in range(len(seeds))]
    true_words = pe.philox_words(seeds, 200, gens, eps).reshape(-1, 4)
    if defect in ('sine', 'words_zw'):
        bad_n = pe.normal64_of_words(true_words, defect)
    else:
        bad_n = pe.normal64_of_words(pe.philox_words(seeds, 200, gens, eps, defect).reshape(-1, 4))
    device = pe.post64(variant, mu, sigma, bad_n).astype(F32)            # the defective device, otherwise perfect
    n64 = pe.normal64_of_words(true_words)
    share = pe.draw_reject_share(device, mu, sigma, n64, variant, pe.e32())
    msg, _ = pe.check_draws(device, mu, sigma, n64, variant, pe.e32())
    _report('draw defect', defect, 'variant', variant, f'rejected on {100 * share:.2f} % of {N_DRAWS} draws')
    assert share > 0.99 and msg is not None


def test_gleet_restatement_is_the_module():
    import torch
    a32, a64 = _actors()
    x = torch.from_numpy(load('gleet_policy.npz')['io/x'])
    with torch.no_grad():
        mu, sg = a32.distribution(a32.features(x))
    got = pe.gleet_forward(a32, x)
    assert np.array_equal(got[0], mu[..., 0].numpy()) and np.array_equal(got[1], sg[..., 0].numpy())
    m64 = pe.gleet_forward(a64, x.double())
    assert m64[0].dtype == np.float64 and np.abs(m64[0] - got[0]).max() < 2e-4


def test_e_ref_is_measured_and_below_the_older_tolerances():
    """E_ref per kernel and quantity over the inputs of the GPU tests; 4 E_ref + 4 ulp must be the tighter bound."""
    worst = {}

    def note(key, e):
        worst[key] = max(worst.get(key, 0.0), e)
    for case in GAUSS_CASES:
        w, dims, (lo, hi), variant, states, _ = _gauss_case(case)
        x = np.concatenate(list(states.values()))
        m32, m64 = pe.gauss_torch32(w, dims, lo, hi, variant, x), pe.gauss64(w, dims, lo, hi, variant, x)
        for q, a, b in (('mu', m32[0], m64[0]), ('sigma', m32[1], m64[1])):
            e = pe.e_ref(a, b)
            _report('E_ref gauss', case, q, f'{e:.3e}')
            assert 0 < e < OLD_TOL['gauss'], (case, q, e)
            note(('gauss', q), e)
    for NP, H in LSTM_SHAPES:
        w, (IN, Hh, A), launches = _lstm_case(NP, H)
        parts = pe.lstm_split(w, IN, Hh, A)
        E = {'h': 0.0, 'c': 0.0, 'sigma': 0.0}
        for _, x, h, c in launches:
            r = _lstm_host(parts, x, h, c)
            E = {'h': max(E['h'], pe.e_ref(r['h32'], r['h64'])), 'c': max(E['c'], pe.e_ref(r['c32'], r['c64'])),
                 'sigma': max(E['sigma'], pe.e_ref(r['sigma32'], r['sigma64']))}
        for q, e in E.items():
            _report('E_ref lstm', (NP, H), q, f'{e:.3e}')
            assert 0 < e < OLD_TOL['lstm'], (NP, H, q, e)
            note(('lstm', q), e)
    a32, a64 = _actors()
    for NP in GLEET_NP:
        ins, _ = _gleet_case(NP, a64)
        m32, m64 = _gleet_both(a32, a64, np.stack(list(ins.values())))
        for q, a, b in (('mu', m32[0], m64[0]), ('sigma', m32[1], m64[1])):
            e = pe.e_ref(a, b)
            _report('E_ref gleet', NP, q, f'{e:.3e}')
            assert 0 < e < OLD_TOL['gleet'], (NP, q, e)
            note(('gleet', q), e)
    _report('E_ref, largest per kernel and quantity:', {f'{k[0]} {k[1]}': f'{v:.2e}' for k, v in worst.items()})


@pytest.mark.parametrize('defect', pe.RULE_DEFECTS)
def test_e_ref_rule_rejects(defect):
    """A kernel that is exact apart from the planted mistake misses 4 E_ref + 4 ulp on the test's own inputs."""
    fractions = []
    if defect == 'rlpso_sigma_affine':
        for case in GAUSS_CASES:
            if case[0] != 'rlpso':
                continue
            w, dims, (lo, hi), variant, states, _ = _gauss_case(case)
            x = np.concatenate(list(states.values()))
            want = pe.gauss64(w, dims, lo, hi, variant, x)[1]
            E = pe.e_ref(pe.gauss_torch32(w, dims, lo, hi, variant, x)[1], want)
            fractions.append(pe.rule_fraction(pe.gauss64(w, dims, lo, hi, variant, x, defect)[1].astype(F32), want, E))
    else:
        import torch
        a32, a64 = _actors()
        for NP in GLEET_NP:
            ins, _ = _gleet_case(NP, a64)
            x = np.stack(list(ins.values()))
            m32, m64 = _gleet_both(a32, a64, x)
            bad = pe.gleet_forward(a64, torch.from_numpy(x), defect)
            fractions.append(max(pe.rule_fraction(bad[q].astype(F32), m64[q], pe.e_ref(m32[q], m64[q])) for q in (0, 1)))
    _report('rule defect', defect, 'fraction of the bound per case:', [f'{f:.3g}' for f in fractions])
    assert min(fractions) > 1.0, fractions


def test_sorted_swarm_moves_the_running_maximum_in_every_chunk():
    import torch
    _, a64 = _actors()
    for NP in GLEET_NP:
        ins, _ = _gleet_case(NP, a64)
        s = pe.gleet_scores_head0(a64, torch.from_numpy(ins['sorted_x8']))[0]
        assert np.all(np.diff(s[1:]) >= 0) and pe.chunk_max_moves(s), NP
        assert s.max() - s.min() > 8 or NP < 8, (NP, s.max() - s.min())          # the maximum moves by whole units of the exponent


# ================================================================================================ GPU
def _suite(name, dim):
    from metabox_amd.suite import Suite
    ps = problems(name, dim)
    ids = sorted(ps)
    return Suite([ps[i] for i in ids]), len(ids)


def _seeds(B, salt=0):
    """High word set on the even instances, small seeds on the odd ones."""
    return np.array([(0x9E3779B97F4A7C15 + k + 1000 * salt) & MASK64 if k % 2 == 0 else k + 1 + 7 * salt for k in range(B)], dtype=np.uint64)


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


class _DrawLedger:
    def __init__(self, kernel):
        self.kernel, self.n, self.undecided, self.folded, self.worst = kernel, 0, 0, 0, 0.0

    def add(self, st):
        self.n += st['n']; self.undecided += st['undecided']; self.folded += st['folded']; self.worst = max(self.worst, st['worst'])

    def report(self):
        _report('draws', self.kernel, f'{self.n} draws, worst {self.worst:.3f} of 16 E32 sigma + 4 ulp, {self.undecided} undecided on a clamp edge, '
                                       f'{self.folded} clamped / re-folded')


def _draw_cases(kernel, make_batch, policy, variant, n_pidx, led, plant=None):
    """The draw check after 0, 1 and 3 steps, after a second reset (episode word 1) and after a rebind, for B in {1, 5, 17}.
    policy(batch, ctx) -> (actions, mu_sigma) device tensors; plant(batch, ctx), if given, writes the state the policy reads."""
    import torch
    E32 = pe.e32()
    for B in (1, 5, 17):
        seeds = _seeds(B)
        batch = make_batch(B, seeds)
        ctx = {'B': B}
        A = batch.action_dim

        def check(label, steps, episode=None):
            if plant:
                plant(batch, ctx)
            acts, ms = policy(batch, ctx)
            torch.cuda.synchronize()
            a, m = acts.cpu().numpy().reshape(B, A), ms.cpu().numpy()
            pub = np.stack([batch.read_public(k).copy() for k in range(B)])
            gen, ep = pub[:, SC_GEN], pub[:, SC_EPISODE]
            assert np.all(gen == steps), (kernel, B, label, gen)            # the scalar block's generation is the number of steps taken
            if episode is not None:
                assert np.all(ep == episode), (kernel, B, label, ep)
            n64 = pe.normal64_of_words(pe.philox_words(seeds, A, gen + 1, ep))
            msg, st = pe.check_draws(a, m[:, 0], m[:, 1], n64, variant, E32)
            assert msg is None, (kernel, B, label, msg, st)
            led.add(st)
            return acts
        batch.reset()
        ctx['fresh'] = True
        acts = check('reset', 0, 0)
        steps = 0
        for target in (1, 3):
            while steps < target:
                batch.step(acts.clone())
                steps += 1
                if steps < target:
                    if plant:
                        plant(batch, ctx)
                    acts = policy(batch, ctx)[0]
            acts = check(f'{steps} steps', steps, 0)
        batch.reset()
        ctx['fresh'] = True
        check('second reset', 0, 1)
        seeds = _seeds(B, salt=1)
        batch.rebind((np.arange(B) + 1) % n_pidx, seeds)
        batch.reset()
        ctx['fresh'] = True
        check('rebind', 0)
        batch.close()


@pytest.mark.gpu
def test_rlepso_actor_draws_are_the_host_philox_draws():
    """The shipped actor (whose draws stay inside [0, 1] at the states of a fresh episode) and a seeded 1 -> 5 -> 3 -> 35 actor whose last-layer
    bias puts mu near 0.03, so that a good share of its draws is clamped at 0."""
    from metabox_amd.suite import Batch
    suite, n = _suite('bbob', 10)
    w, dims, lo, hi = _shipped('rlepso')
    led = _DrawLedger('k_gauss_mlp_policy (RLEPSO)')
    for wts, (h1, h2) in ((w, dims[1:3]), (pe.seeded_gauss(np.random.RandomState(12), 1, 5, 3, 35, mu_bias=-1.74), (5, 3))):
        wd = _dev(wts)
        _draw_cases(led.kernel, lambda B, seeds: Batch(suite, ALGO_RLEPSO, np.arange(B) % n, seeds, NP_RL, MAX_FES, 400, 50),
                    lambda b, ctx: b.gauss_policy(wd, h1, h2, lo, hi, want_mu_sigma=True), POLICY_RLEPSO, n, led)
    led.report()
    assert led.undecided <= 0.001 * led.n and 0.05 * led.n < led.folded < 0.95 * led.n


@pytest.mark.gpu
def test_rlpso_actor_draws_and_refold_are_the_host_philox_draws():
    """Seeded weights whose last-layer bias puts mu near 0.03 (sigma near 0.5): about half of the draws leave [0, 1) and are re-folded."""
    from metabox_amd.suite import Batch
    suite, n = _suite('bbob', 10)
    rs = np.random.RandomState(11)
    w = pe.seeded_gauss(rs, 20, 32, 8, 1, mu_bias=-1.74)
    wd = _dev(w)
    led = _DrawLedger('k_gauss_mlp_policy (RL-PSO)')

    def plant(b, ctx):
        b.state.copy_(_dev(rs.rand(ctx['B'], 20)))
    for _ in range(3):                                            # one draw per instance and call: three passes for the shares
        _draw_cases(led.kernel, lambda B, seeds: Batch(suite, ALGO_RLPSO, np.arange(B) % n, seeds, 100, 2500, 50, 50),
                    lambda b, ctx: b.gauss_policy(wd, 32, 8, 0.01, 0.7, want_mu_sigma=True), POLICY_RLPSO, n, led, plant)
    led.report()
    assert led.undecided <= 0.001 * led.n
    assert led.folded >= 0.1 * led.n and led.n - led.folded - led.undecided >= 0.1 * led.n, (led.folded, led.n)


@pytest.mark.gpu
def test_lde_policy_draws_are_the_host_philox_draws():
    import torch
    from metabox_amd.suite import Batch
    suite, n = _suite('bbob', 10)
    wd = _dev(_shipped('lde'))
    led = _DrawLedger('k_lstm_policy')

    def policy(b, ctx):
        if ctx.pop('fresh', False):
            ctx['h'], ctx['c'] = (torch.zeros(ctx['B'], 50, dtype=torch.float32, device='cuda') for _ in range(2))
        return b.lde_policy(wd, 50, ctx['h'], ctx['c'], want_mu_sigma=True)
    _draw_cases(led.kernel, lambda B, seeds: Batch(suite, ALGO_LDE, np.arange(B) % n, seeds, 50, MAX_FES, 400, 50), policy, POLICY_RLEPSO, n, led)
    led.report()
    assert led.undecided <= 0.001 * led.n and led.folded > 0


@pytest.mark.gpu
def test_gleet_policy_draws_are_the_host_philox_draws():
    from metabox_amd.suite import Batch
    suite, n = _suite('bbob', 10)
    actor = _gleet_actor()
    wd = actor.packed_weights().cuda()
    led = _DrawLedger('k_gleet_policy')
    _draw_cases(led.kernel, lambda B, seeds: Batch(suite, ALGO_GLEET, np.arange(B) % n, seeds, 100, MAX_FES, 400, 50),
                lambda b, ctx: b.gleet_policy(wd, actor.min_sigma, actor.max_sigma, want_mu_sigma=True), POLICY_RLEPSO, n, led)
    led.report()
    assert led.undecided <= 0.001 * led.n and led.folded > 0


# ------------------------------------------------------------------------------------------------ k_qnet_argmax
def _qnet_rows(rs, kind, io_x):
    if kind == 'recorded':
        return io_x[rs.randint(len(io_x))].astype(np.float64)
    if kind == 'uniform':
        return rs.rand(99)
    if kind == 'zero':
        return np.zeros(99)
    if kind == 'plus_1e3':
        return np.full(99, 1e3)
    if kind == 'minus_1e3':
        return np.full(99, -1e3)
    if kind == 'mixed_1e3':
        return rs.choice([-1e3, 1e3], 99)
    assert kind == 'subnormal'
    return rs.randint(1, 2 ** 22, 99).astype(np.float64) * 2.0 ** -149 * rs.choice([-1, 1], 99)


QNET_KINDS = ('recorded', 'uniform', 'zero', 'plus_1e3', 'minus_1e3', 'mixed_1e3', 'subnormal')


@pytest.mark.gpu
@pytest.mark.parametrize('weights', ['shipped', 'tie'])
def test_qnet_kernel_is_bit_for_bit_the_fma_chain(weights):
    """Q values bit for bit five chain32 layers with exact ReLU, every action their first maximum, no undecided share.  `tie`: a seeded net whose
    last layer has columns 1 and 3 identical and above columns 0 and 2 -- the action must be 1 everywhere."""
    from metabox_amd.suite import Batch
    suite, n = _suite('bbob', 10)
    rs = np.random.RandomState(17)
    w = _shipped('ddqn') if weights == 'shipped' else pe.seeded_qnet(rs)
    wd = _dev(w)
    io_x = load('ddqn_policy.npz')['io/x']
    rows_checked = 0
    for B in (1, 15, 16, 17, 37):
        batch = Batch(suite, ALGO_DEDDQN, np.arange(B) % n, np.arange(B, dtype=np.uint64) + 1, 100, MAX_FES, 400, 50)
        batch.reset()
        for off in range(len(QNET_KINDS)):
            kinds = [QNET_KINDS[(i + off) % len(QNET_KINDS)] for i in range(B)]
            x = np.stack([_qnet_rows(rs, k, io_x) for k in kinds])
            if B == 16 and off == 0:
                x = np.concatenate([io_x.astype(np.float64), x])[:16]        # the whole recorded batch once
                kinds = ['recorded'] * 16
            batch.state.copy_(_dev(x))
            acts, q = batch.ddqn_qnet(wd, want_q=True)
            acts, q = acts.cpu().numpy(), q.cpu().numpy()
            want_q, want_a = pe.qnet32(w, x)
            bad = np.nonzero((q.view(np.uint32) != want_q.view(np.uint32)).any(1))[0]
            assert bad.size == 0, (weights, B, off, [(int(i), kinds[i], q[i], want_q[i]) for i in bad[:3]])
            assert np.array_equal(acts, want_a), (weights, B, off)
            if weights == 'tie':
                assert np.all(want_q[:, 1] == want_q[:, 3]) and np.all(want_q[:, 1] > want_q[:, 0]) and np.all(acts == 1)
            for i, k in enumerate(kinds):
                if k == 'zero':                                              # a chain of biases
                    assert np.array_equal(want_q[i], pe.qnet32(w, np.zeros((1, 99)))[0][0])
            rows_checked += B
        batch.close()
    if weights == 'shipped':
        assert np.abs(pe.qnet32(w, io_x)[0] - load('ddqn_policy.npz')['io/q']).max() <= 1e-5      # the chain is the reference's network
    _report('qnet', weights, f'{rows_checked} rows x 4 Q values bit for bit, every argmax decided')


# ------------------------------------------------------------------------------------------------ k_lstm_policy
@pytest.mark.gpu
@pytest.mark.parametrize('NP, H', LSTM_SHAPES)
def test_lstm_policy_kernel_against_exact_chains(NP, H):
    """mu bit for bit chain32 of the device's own h'; sigma within the rule of sigmoid of the exact chain; (h', c') within the rule of the float64
    cell applied to the exact gate chains; sample=False leaves the same (h', c')."""
    from metabox_amd.suite import Batch
    suite, n = _suite('bbob', 10)
    w, (IN, Hh, A), launches = _lstm_case(NP, H)
    parts = pe.lstm_split(w, IN, Hh, A)
    wd = _dev(w)
    hosts = [_lstm_host(parts, x, h, c) for _, x, h, c in launches]
    E = {'h': max(pe.e_ref(r['h32'], r['h64']) for r in hosts), 'c': max(pe.e_ref(r['c32'], r['c64']) for r in hosts)}
    got_all, batches = [], {}
    for (kind, x, h, c) in launches:
        B = x.shape[0]
        if B not in batches:
            batches[B] = Batch(suite, ALGO_LDE, np.arange(B) % n, _seeds(B), NP, MAX_FES, 400, 50)
            batches[B].reset()
            assert (batches[B].state_dim, batches[B].action_dim) == (IN, A)
        batch = batches[B]
        batch.state.copy_(_dev(x))
        hd, cd = _dev(h), _dev(c)
        acts, ms = batch.lde_policy(wd, H, hd, cd, want_mu_sigma=True)
        a, ms = acts.cpu().numpy(), ms.cpu().numpy()
        h2, c2 = _dev(h), _dev(c)
        assert batch.lde_policy(wd, H, h2, c2, sample=False) is None
        assert np.array_equal(h2.cpu().numpy(), hd.cpu().numpy()) and np.array_equal(c2.cpu().numpy(), cd.cpu().numpy()), (kind, B)
        assert a.shape == (B, A) and a.min() >= 0 and a.max() <= 1
        got_all.append((ms[:, 0], ms[:, 1], hd.cpu().numpy(), cd.cpu().numpy()))
    # the heads are judged from the DEVICE's h' (what the kernel's second stage read)
    heads = [_lstm_host(parts, x, h, c, h_dev=g[2]) for (_, x, h, c), g in zip(launches, got_all)]
    E['sigma'] = max(pe.e_ref(r['sigma32'], r['sigma64']) for r in heads)
    frac = {'h': 0.0, 'c': 0.0, 'sigma': 0.0}
    for (kind, x, h, c), r, hd_, (mu, sigma, hn, cn) in zip(launches, hosts, heads, got_all):
        B = x.shape[0]
        assert np.array_equal(mu.view(np.uint32), hd_['mu'].view(np.uint32)), (NP, H, kind, B, 'mu is not the fma chain of the device h',
                                                                                 float(np.abs(mu - hd_['mu']).max()))
        for q, got, want in (('h', hn, r['h64']), ('c', cn, r['c64']), ('sigma', sigma, hd_['sigma64'])):
            f = pe.rule_fraction(got, want, E[q])
            frac[q] = max(frac[q], f)
            print(f'  lstm ({NP}, {H}) {kind} B={B} {q}: {f:.3f} of 4 E_ref + 4 ulp')
    _report('lstm', (NP, H), 'E_ref', {q: f'{v:.2e}' for q, v in E.items()}, 'worst fraction of the bound', {q: f'{v:.3f}' for q, v in frac.items()},
            'mu bit for bit')
    for b in batches.values():
        b.close()
    assert all(0 < E[q] < OLD_TOL['lstm'] for q in E) and all(f <= 1.0 for f in frac.values()), (E, frac)


@pytest.mark.gpu
def test_lstm_policy_refuses_hidden_65():
    import torch
    from metabox_amd._abi import MbxError
    from metabox_amd.suite import Batch
    suite, n = _suite('bbob', 10)
    batch = Batch(suite, ALGO_LDE, [0], [1], 30, MAX_FES, 400, 50)
    batch.reset()
    w = _dev(pe.seeded_lstm(np.random.RandomState(1), 40, 65, 60))
    h, c = (torch.zeros(1, 65, dtype=torch.float32, device='cuda') for _ in range(2))
    with pytest.raises(MbxError, match='mbx error -1'):
        batch.lde_policy(w, 65, h, c)
    batch.close()


# ------------------------------------------------------------------------------------------------ k_gauss_mlp_policy
def _gauss_batch(algo, dims, B):
    from metabox_amd.suite import Batch
    if algo == 'rlepso':
        suite, n = _suite('bbob', 10)
        return Batch(suite, ALGO_RLEPSO, np.arange(B) % n, _seeds(B), NP_RL, MAX_FES, 400, 50)
    suite, n = _suite('bbob', dims[0] // 2)
    return Batch(suite, ALGO_RLPSO, np.arange(B) % n, _seeds(B), 100, 2500, 50, 50)


@pytest.mark.gpu
@pytest.mark.parametrize('case', GAUSS_CASES, ids=lambda c: f'{c[0]}-{c[1]}-' + 'x'.join(map(str, c[2])))
def test_gauss_policy_mu_sigma_within_the_rule(case):
    algo = case[0]
    w, dims, (lo, hi), variant, states, sat = _gauss_case(case)
    wd = _dev(w)
    x_all = np.concatenate(list(states.values()))
    m32, m64 = pe.gauss_torch32(w, dims, lo, hi, variant, x_all), pe.gauss64(w, dims, lo, hi, variant, x_all)
    E = {'mu': pe.e_ref(m32[0], m64[0]), 'sigma': pe.e_ref(m32[1], m64[1])}
    frac = {'mu': 0.0, 'sigma': 0.0}
    for B, x in states.items():
        batch = _gauss_batch(algo, dims, B)
        batch.reset()
        assert (batch.state_dim, batch.action_dim) == (dims[0], dims[3])
        batch.state.copy_(_dev(x))
        _, ms = batch.gauss_policy(wd, dims[1], dims[2], lo, hi, want_mu_sigma=True)
        ms = ms.cpu().numpy()
        want = pe.gauss64(w, dims, lo, hi, variant, x)
        for qi, q in enumerate(('mu', 'sigma')):
            f = pe.rule_fraction(ms[:, qi], want[qi], E[q])
            frac[q] = max(frac[q], f)
            print(f'  gauss {case} B={B} {q}: {f:.3f} of 4 E_ref + 4 ulp')
        if sat is not None:                                          # tanh saturated: mu exactly 0 or 1 on the device as on the host
            for i in range(B):
                if any(np.array_equal(x[i], s) for s in sat) and want[0][i, 0] in (0.0, 1.0):
                    assert ms[i, 0, 0] == want[0][i, 0], (case, B, i, ms[i, 0, 0], want[0][i, 0])
        batch.close()
    _report('gauss', case, 'E_ref', {q: f'{v:.2e}' for q, v in E.items()}, 'worst fraction of the bound', {q: f'{v:.3f}' for q, v in frac.items()})
    assert all(0 < E[q] < OLD_TOL['gauss'] for q in E) and all(f <= 1.0 for f in frac.values()), (E, frac)


@pytest.mark.gpu
def test_actor_table_rows_are_the_policy_kernel_at_k_over_maxfes():
    """Row k of mbx_rlepso_policy_table bit for bit the (mu, sigma) of mbx_gauss_policy at state k / maxFEs: k = 0, the last row and the rows on both
    sides of every multiple of the grid stride (2048 workgroups x 4 waves, policy_blocks in mbx.hip) -- the table is the only launch that takes the
    second and third trip of the kernel's row loop beyond a handful of rows."""
    from metabox_amd.suite import Batch
    suite, n = _suite('bbob', 10)
    w, dims, lo, hi = _shipped('rlepso')
    wd = _dev(w)
    stride = min(2048, -(-TABLE_ROWS // 8)) * 4
    assert stride == 8192 and TABLE_ROWS > 2 * stride
    ks = sorted({0, 1, TABLE_ROWS - 1, TABLE_ROWS - 2} | {m * stride + d for m in range(1, TABLE_ROWS // stride + 1) for d in (-2, -1, 0, 1, 2, 3, 4)})
    B = len(ks)
    batch = Batch(suite, ALGO_RLEPSO, np.arange(B) % n, _seeds(B), NP_RL, MAX_FES, 400, 50)
    batch.reset()
    table = batch.policy_table(wd, dims[1], dims[2], lo, hi).cpu().numpy()
    assert table.shape == (TABLE_ROWS, 2, 35)
    batch.state.copy_(_dev(np.array(ks, dtype=np.float64)[:, None] / float(MAX_FES)))
    _, ms = batch.gauss_policy(wd, dims[1], dims[2], lo, hi, want_mu_sigma=True)
    ms = ms.cpu().numpy()
    for i, k in enumerate(ks):
        assert np.array_equal(table[k].view(np.uint32), ms[i].view(np.uint32)), (k, float(np.abs(table[k] - ms[i]).max()))
    x = np.arange(TABLE_ROWS, dtype=np.float64)[:, None] / MAX_FES
    want = pe.gauss64(w, dims, lo, hi, POLICY_RLEPSO, x)
    m32 = pe.gauss_torch32(w, dims, lo, hi, POLICY_RLEPSO, x)
    fr = [pe.rule_fraction(table[:, q], want[q], pe.e_ref(m32[q], want[q])) for q in (0, 1)]
    _report('actor table', f'{B} probed rows bit for bit; all {TABLE_ROWS} rows at {fr[0]:.3f} (mu) / {fr[1]:.3f} (sigma) of 4 E_ref + 4 ulp')
    assert max(fr) <= 1.0
    batch.close()


# ------------------------------------------------------------------------------------------------ k_gleet_policy
@pytest.mark.gpu
@pytest.mark.parametrize('NP', GLEET_NP)
def test_gleet_policy_mu_sigma_within_the_rule(NP):
    from metabox_amd.suite import Batch
    dim = 10 if NP == 100 else 2
    suite, n = _suite('bbob', dim)
    a32, a64 = _actors()
    wd = a32.packed_weights().cuda()
    ins, launches = _gleet_case(NP, a64)
    m32, m64 = _gleet_both(a32, a64, np.stack(list(ins.values())))
    E = {'mu': pe.e_ref(m32[0], m64[0]), 'sigma': pe.e_ref(m32[1], m64[1])}
    batch = Batch(suite, ALGO_GLEET, np.arange(3) % n, _seeds(3), NP, 2000 * dim, 40 * dim, 50)
    batch.reset()
    assert (batch.state_dim, batch.action_dim) == (27 * NP, NP)
    frac = {'mu': 0.0, 'sigma': 0.0}
    for names in launches:
        x = np.stack([ins[k] for k in names])
        batch.state.copy_(_dev(x.reshape(3, -1)))
        _, ms = batch.gleet_policy(wd, a32.min_sigma, a32.max_sigma, want_mu_sigma=True)
        ms = ms.cpu().numpy()
        _, want = _gleet_both(a32, a64, x)
        for qi, q in enumerate(('mu', 'sigma')):
            for r, name in enumerate(names):
                f = pe.rule_fraction(ms[r, qi], want[qi][r], E[q])
                frac[q] = max(frac[q], f)
                print(f'  gleet NP={NP} {name} {q}: {f:.3f} of 4 E_ref + 4 ulp (|err| {np.abs(ms[r, qi] - want[qi][r]).max():.2e})')
    batch.close()
    _report('gleet', NP, 'E_ref', {q: f'{v:.2e}' for q, v in E.items()}, 'worst fraction of the bound', {q: f'{v:.3f}' for q, v in frac.items()})
    assert all(0 < E[q] < OLD_TOL['gleet'] for q in E) and all(f <= 1.0 for f in frac.values()), (E, frac)


@pytest.mark.gpu
def test_gleet_policy_refuses_np_129():
    from metabox_amd._abi import MbxError
    from metabox_amd.suite import Batch
    suite, n = _suite('bbob', 2)
    actor = _gleet_actor()
    batch = Batch(suite, ALGO_GLEET, [0], [1], 129, 4000, 80, 50)
    batch.reset()
    with pytest.raises(MbxError, match='mbx error -3'):          # MBX_E_UNSUPPORTED
        batch.gleet_policy(actor.packed_weights().cuda(), actor.min_sigma, actor.max_sigma)
    batch.close()
