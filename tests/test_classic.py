"""Classic baselines DEAP_DE / DEAP_PSO / DEAP_CMAES.  DEAP is not part of the reference tree and DE's tournament
draws from Python's unseeded `random`, so there are no reference traces: parity is UNPINNED with respect to the reference.  What is
checked: the C oracle's internal consistency and optimisation behaviour (CPU), HIP == oracle under Philox, and the harness (GPU)."""
import numpy as np
import pytest

from helpers import close, problems
from oracle import oracle

ALGOS = {'de': 8, 'pso': 9, 'cmaes': 10}


def _oracle_run(algo, p, seed, maxfes=20000, steps=None, nlog=50):
    cfg = oracle.make_cfg(ALGOS[algo], 50, p.dim, maxfes, maxfes // nlog, nlog)
    o = oracle.ClassicOracle(p.desc(), p.bias, cfg, seed=seed)
    o.reset()
    hist, done, n = [], False, 0
    while not done and (steps is None or n < steps):
        done = o.step()
        hist.append(o.result()['gbest'])
        n += 1
    return o, np.array(hist)


@pytest.mark.parametrize('algo', ['de', 'pso', 'cmaes'])
def test_oracle_classic_baselines_optimise_and_keep_the_wrappers_bookkeeping(algo):
    ps = problems('bbob', 10)
    o, hist = _oracle_run(algo, ps[1], seed=3)                      # Sphere
    r = o.result()
    assert np.all(np.diff(hist) <= 0)                               # best-so-far never gets worse
    if algo == 'cmaes':
        assert r['gbest'] <= 1e-8 and r['fes'] < 20000 and r['fes'] % 50 == 0       # solved to the stop threshold, whole generations
        assert r['sigma'] < 0.05                                        # step size collapsed from 0.5
    else:
        assert r['gbest'] < (1e-3 if algo == 'de' else 5.0)
    assert 2 <= r['cost_len'] <= 51 and np.all(np.diff(r['cost'][:r['cost_len']]) <= 0)
    o2, hist2 = _oracle_run(algo, ps[15], seed=4, steps=60)         # Rastrigin, fixed number of sweeps / generations
    r2 = o2.result()
    assert r2['fes'] == (60 * 50 if algo == 'cmaes' else 50 + 60 * 50) and np.isfinite(hist2).all()
    o3, hist3 = _oracle_run(algo, ps[15], seed=4, steps=60)
    assert np.array_equal(hist2, hist3)                              # deterministic in (problem, seed)
    o4, hist4 = _oracle_run(algo, ps[15], seed=5, steps=60)
    assert not np.array_equal(hist2, hist4)


def test_oracle_jacobi_eigensolver_inside_cmaes():
    """After a generation C = B diag(D^2) B^T with orthonormal B (the Strategy's invariant), read back through the sampling
    distribution: cov of many generated points / sigma^2 ~ C."""
    # exercised indirectly: CMA-ES reaching 1e-8 on the ill-conditioned Ellipsoidal function needs a correct eigen-decomposition
    ps = problems('bbob', 10)
    o, hist = _oracle_run('cmaes', ps[2], seed=7)
    assert o.result()['gbest'] <= 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize('algo', ['de', 'pso', 'cmaes'])
def test_hip_classic_matches_oracle_under_philox(algo):
    import torch
    from metabox_amd.suite import Batch, Suite
    ps_all = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    ids = [1, 2, 8, 15, 21, 103, 117, 130]
    s = Suite([ps_all[i] for i in ids])
    B, G = len(ids), 12
    seeds = np.arange(B, dtype=np.uint64) * 977 + 41
    b = Batch(s, ALGOS[algo], np.arange(B), seeds, 50, 20000, 400, 50)
    assert (b.state_dim, b.action_dim) == (1, 0)
    if algo != 'cmaes':                                          # best-so-far after every sweep and the population at the end: the comparison the geometry sweep shares
        import parity
        assert np.array_equal(seeds, parity.seeds_for(algo, B))
        parity.canonical(algo, b, s.problems, seeds, 50, 10, (20000, 400, 50), G, ids, per_step=True)
        assert torch.allclose(b.state[:, 0].cpu(), torch.full((B,), (50 + G * 50) / 20000, dtype=torch.float64))
        b.close()
        return
    b.reset()
    sc_off = 4 * 10 + 200
    gb = np.zeros((G, B))
    for g in range(G):
        st, _, d = b.step(None)
        torch.cuda.synchronize()
        for k in range(B):
            gb[g, k] = b.read_state(k)[sc_off]
    assert torch.allclose(st[:, 0].cpu(), torch.full((B,), (G * 50) / 20000, dtype=torch.float64))
    for k in range(B):
        p = s.problems[k]
        cfg = oracle.make_cfg(ALGOS[algo], 50, 10, 20000, 400, 50)
        o = oracle.ClassicOracle(p.desc(), p.bias, cfg, seed=int(seeds[k]))
        o.reset()
        want = []
        for g in range(G):
            o.step()
            want.append(o.result()['gbest'])
        want = np.array(want)
        tol = 1e-6                                               # CMA-ES: log / exp / pow of the device library feed the adaptation
        assert np.all(np.abs(gb[:, k] - want) <= tol * np.abs(want) + 1e-12), (algo, ids[k], gb[:, k], want)
    b.close()


@pytest.mark.gpu
def test_classic_baselines_in_the_harness(tmp_path):
    """run_episode / run_batch of the three classes, and Tester picking DEAP_CMAES up by name (config always appends it)."""
    import copy
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import DEAP_CMAES, DEAP_DE, DEAP_PSO
    from metabox_amd.suite import Suite
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda'])
    ps = [problems('bbob', 10)[f] for f in (1, 8)]
    s = Suite(ps)
    for cls, target in ((DEAP_CMAES, 1e-8), (DEAP_DE, 1e-2), (DEAP_PSO, 10.0)):
        opt = cls(copy.deepcopy(cfg))
        res = opt.run_batch(s, np.arange(16) % 2, np.arange(16, dtype=np.uint64) + 1)
        cost, fes = res['cost'].cpu().numpy(), res['fes'].cpu().numpy()
        assert cost.shape == (16, 51) and np.all(np.diff(cost, axis=1) <= 0) and np.all(fes <= 20000)
        assert np.median(cost[::2, -1]) <= target, (cls.__name__, cost[::2, -1])              # Sphere
        np.random.seed(1)
        info = opt.run_episode(ps[0])
        assert info['fes'] <= 20000 and len(info['cost']) <= 51 and info['cost'][-1] <= max(target, 1e-8) * 10
