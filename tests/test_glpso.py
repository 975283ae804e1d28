"""GL-PSO (src/optimizer/gl_pso.py), a classic baseline of the test harness: the batched HIP kernels (metabox_amd/csrc/mbx_glpso.hpp)
replay the reference's episodes from tests/golden/glpso_traces.npz (tools/gen_golden.py glpso) through mbx_set_tape.  The numpy draws
are not stored: GlpsoTapeFeeder regenerates them from the seed in the reference's draw order (include/mbx_layout.h §11).

This module is the recorded episodes (NP = 100, D = 10 / 30 / 12; gbest, fes, pbest, exemplar_cost and the counters, within the parity tolerance), the Philox route
against the rebuilt tape at D = 10, and batch invariance.  What the episodes do not reach is pinned by tests/test_glpso_exact.py against the exact restatement of
tests/glpso_exact.py: positions, velocities and exemplar rows bit for bit, every cost against extended precision, NP from 4 to 256 and D from 2 to 40, the tie and
threshold rules of the kernel header on planted states, and the route equality at edge shapes.  Still unpinned: free-running Philox episodes against the reference in
distribution, and the normal-noise draws on the Philox route."""
import copy
import ctypes as C

import numpy as np
import pytest

from helpers import close, load, print_ledger, problems, prove_tie_arrays
from oracle import oracle

TR = load('glpso_traces.npz')
CASES = [str(c) for c in TR['cases']]
NP, NSEL, SG = 100, 10, 7
ALGO_GLPSO = 11
SITE_ELEM_A, SITE_ELEM_R, SITE_NOISE0_A, SITE_NOISE0_B, SITE_NOISE1_A, SITE_NOISE1_B = 0, 4, 5, 6, 7, 8
SITE_GL_CROSS, SITE_GL_MUT, SITE_GL_NOISE_A, SITE_GL_NOISE_B, SITE_GL_TOUR = 18, 19, 20, 21, 22


def tape_stride(D, NP=NP):
    return 6 * NP * D + 16 * NP


def split_state(st, D, nlog=50, NP=NP):
    NE = NP * D
    o = 4 * NE + 3 * NP + D
    return {'X': st[:NE], 'V': st[NE:2 * NE], 'pbpos': st[2 * NE:3 * NE], 'pbest': st[3 * NE:3 * NE + NP],
            'exemplar': st[3 * NE + NP:4 * NE + NP], 'excost': st[4 * NE + NP:4 * NE + 2 * NP], 'stag': st[4 * NE + 2 * NP:4 * NE + 3 * NP],
            'gbpos': st[4 * NE + 3 * NP:o], 'scalars': st[o:o + 16], 'cost': st[o + 16:o + 17 + nlog]}


class GlpsoTapeFeeder:
    """numpy's legacy stream as GL_PSO consumes it, laid out as the tape of include/mbx_layout.h §11.  The tournament indices are drawn
    speculatively; ``commit(fired)`` rewinds the stream when no counter exceeded sg (the reference draws them only then)."""

    def __init__(self, seed, D, noise_kind, rs=None):
        self.rs = rs if rs is not None else np.random.RandomState(seed)
        self.D, self.noise = D, noise_kind
        self._rewind = None

    def _noise_rows(self):
        rows = np.zeros((3, NP))
        if self.noise == 1:
            rows[0] = self.rs.randn(NP)
        elif self.noise == 2:
            rows[0] = self.rs.rand(NP)
            rows[1] = self.rs.rand(NP)
        elif self.noise == 3:
            rows[0] = self.rs.rand(NP)
            rows[1] = self.rs.randn(NP)
            rows[2] = self.rs.randn(NP)
        return rows.ravel()

    def _exemplar_block(self):
        D = self.D
        parts = [self.rs.randint(low=0, high=NP, size=(NP, D)).astype(np.float64).ravel(),     # crossover (:23)
                 self.rs.rand(NP, D).ravel(),                                                    # (:28)
                 self.rs.rand(NP, D).ravel(),                                                    # mutation: uniform(lb, ub) (:33)
                 self.rs.rand(NP, D).ravel(),                                                    # (:34)
                 self._noise_rows()]                                                            # evaluation of the new exemplars
        self._rewind = self.rs.get_state()
        parts.append(self.rs.randint(low=0, high=NP, size=(NP, NSEL)).astype(np.float64).ravel())   # tournament (:50), speculative
        return np.concatenate(parts)

    def reset_tape(self):
        D = self.D
        head = [self.rs.rand(NP, D).ravel(), self.rs.rand(NP, D).ravel(), self._noise_rows()]        # uniform pos / vel (:82-84), evaluation
        return self._pad(np.concatenate(head + [self._exemplar_block()]))

    def step_tape(self):
        head = [self.rs.rand(NP, self.D).ravel(), self._noise_rows()]                                # rand (:121), evaluation
        return self._pad(np.concatenate(head + [self._exemplar_block()]))

    def _pad(self, t):
        out = np.zeros(tape_stride(self.D))
        out[:len(t)] = t
        return out

    def commit(self, fired):
        if not fired:
            self.rs.set_state(self._rewind)
        self._rewind = None


def _problem(suite, dim, fid):
    if suite == 'protein':
        from test_protein import protein
        return protein()[0][fid], 0
    p = problems(suite, int(dim))[int(fid)]
    return p, p.noise[0]


def _episodes(case):
    """[(problem, noise kind, fixture key prefix)] in the order the generator ran them on one optimizer object."""
    suite, dim, fid, seed = case.split('/')
    if suite == 'second':
        f1, f2 = fid.split('-')
        return int(dim), int(seed), [(*_problem('bbob', dim, f1), f'{case}/first'), (*_problem('bbob', dim, f2), case)]
    return int(dim), int(seed), [(*_problem(suite, dim, fid), case)]


def _fired(stag_row):
    return bool(np.any(np.asarray(stag_row) > SG))


# ------------------------------------------------------------------------------------------------ CPU
def test_gl_pso_is_exported_and_picked_up_by_the_tester(tmp_path):
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import GL_PSO
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--test', '--t_optimizer_for_cp', 'GL_PSO', '--log_dir', str(tmp_path / 'out')])
    t = Tester(cfg)
    assert 'GL_PSO' in [type(o).__name__ for o in t.t_optimizer_for_cp] and 'GL_PSO' not in t.skipped
    assert isinstance(GL_PSO(copy.deepcopy(cfg)), GL_PSO)
    assert all('GL_PSO' in t.test_results['cost'][str(p)] for p in t.test_set.data)


def test_abi_geometry_of_glpso():
    from metabox_amd import _abi
    lib = _abi.load_lib()
    assert _abi.ALGO_GLPSO == ALGO_GLPSO
    for D in (10, 30, 40, 12):
        cfg = oracle.make_cfg(ALGO_GLPSO, NP, D, 2000 * D, 40 * D, 50)
        assert lib.mbx_tape_stride(C.byref(cfg)) == tape_stride(D)
        assert lib.mbx_state_dim(C.byref(cfg)) == 1
        assert lib.mbx_action_dim(C.byref(cfg)) == 0
    bad = oracle.make_cfg(ALGO_GLPSO + 1, NP, 10, 20000, 400, 50)
    assert lib.mbx_state_dim(C.byref(bad)) < 0 and lib.mbx_tape_stride(C.byref(bad)) < 0


@pytest.mark.parametrize('case', CASES)
def test_feeder_consumes_the_reference_stream(case):
    """Over the whole fixture episode(s) the feeder draws exactly what the reference drew: the next np.random.rand() after the episode is
    the one the generator recorded."""
    dim, seed, eps = _episodes(case)
    rs = np.random.RandomState(seed)
    for p, nk, key in eps:
        fd = GlpsoTapeFeeder(seed, dim, nk, rs)
        stag = TR[f'{key}/stag']
        fd.reset_tape()
        fd.commit(_fired(stag[0]))
        for g in range(len(stag) - 1):
            fd.step_tape()
            fd.commit(_fired(stag[g + 1]))
    assert rs.rand() == float(TR[f'{case}/next_rand']), case


def test_fixture_covers_the_quirks():
    """The fixture exercises what it is meant to pin: tournaments, the counter carry-over, every noise kind, a protein case."""
    assert any(_fired(TR[f'{c}/stag'][1:]) for c in CASES)
    first = TR['second/10/3-7/41/first/stag'][-1]
    assert first.max() > 0 and np.array_equal(TR['second/10/3-7/41/stag'][0], first)       # init_population never resets exemplar_stag
    assert {_problem(*c.split('/')[:3])[1] for c in CASES if c.startswith('bbob-noisy')} == {1, 2, 3}
    assert any(c.startswith('protein') for c in CASES)
    assert TR['bbob/10/1/31/fes'][-1] < TR['bbob/10/1/31/max_fes'] and TR['bbob/10/1/31/gbest'][-1] <= 1e-8      # early stop


# ------------------------------------------------------------------------------------------------ GPU
def _replay(b, idx, key, fd, ledger, case, diverged):
    """One fixture episode of instance `idx` of batch `b` driven by the feeder; checks every generation against the reference."""
    import torch
    D = fd.D
    want = {k: TR[f'{key}/{k}'] for k in ('gbest', 'fes', 'pbest', 'exemplar_cost', 'stag')}
    G = len(want['gbest']) - 1
    tape = torch.zeros(b.B, b.tape_stride, dtype=torch.float64, device='cuda')
    tape[idx] = torch.from_numpy(fd.reset_tape())
    b.set_tape(tape)
    b.reset()
    fd.commit(_fired(want['stag'][0]))
    prev = split_state(b.read_state(idx), D)
    for g in range(G + 1):
        if g > 0:
            tape[idx] = torch.from_numpy(fd.step_tape())
            b.set_tape(tape)
            b.step(None)
            fd.commit(_fired(want['stag'][g]))
        st = split_state(b.read_state(idx), D)
        sc = st['scalars']
        assert sc[1] == want['fes'][g], (case, key, g)
        if not diverged and g > 0:
            # the first generation whose stagnation or pbest decisions differ must sit on a proven near-tie; float tolerances only afterwards
            ok = prove_tie_arrays(want['exemplar_cost'][g - 1], want['exemplar_cost'][g], want['stag'][g], prev['excost'], st['excost'],
                                  st['stag'], ledger, 'stag', key, g)
            ref_i = (want['pbest'][g] != want['pbest'][g - 1]).astype(np.float64)
            cur_i = (st['pbest'] != prev['pbest']).astype(np.float64)
            ok = prove_tie_arrays(want['pbest'][g - 1], want['pbest'][g], ref_i, prev['pbest'], st['pbest'], cur_i, ledger, 'pbest', key, g) and ok
            diverged = not ok
        if not diverged:
            assert np.array_equal(st['stag'], want['stag'][g]), (case, key, g)
        assert close(sc[0], want['gbest'][g]), (case, key, g, sc[0], want['gbest'][g])
        assert close(st['pbest'], want['pbest'][g]), (case, key, g)
        assert close(st['excost'], want['exemplar_cost'][g]), (case, key, g)
        prev = st
    assert sc[4] == 1., (case, key)                                # the episode ended where the reference's did
    return diverged


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_glpso_tape_replay_matches_reference(case):
    from metabox_amd.suite import Batch, Suite
    dim, seed, eps = _episodes(case)
    max_fes = int(TR[f'{case}/max_fes'])
    s = Suite([p for p, _, _ in eps])
    b = Batch(s, ALGO_GLPSO, [0], [seed], NP, max_fes, max_fes // 50, 50)
    assert (b.state_dim, b.action_dim, b.tape_stride) == (1, 0, tape_stride(dim))
    rs = np.random.RandomState(seed)
    ledger, diverged = [], False
    for k, (p, nk, key) in enumerate(eps):
        if k > 0:
            b.rebind([k], [seed])                                    # same batch, next problem: exemplar_stag carries over
        diverged = _replay(b, 0, key, GlpsoTapeFeeder(seed, dim, nk, rs), ledger, case, diverged)
    res = b.results()
    n = int(res['cost_len'][0].item())
    ref_cost = TR[f'{case}/cost']
    assert n == len(ref_cost) and close(res['cost'][0, :n].cpu().numpy(), ref_cost), (case, n, len(ref_cost))
    assert res['fes'][0].item() == TR[f'{case}/fes'][-1]
    print_ledger(ledger)
    b.close()


def _u53(w0, w1):
    return ((w0 >> 5) * 67108864.0 + (w1 >> 6)) / 9007199254740992.0


def _mulhi(w, n):
    return (w * n) >> 32


def philox_tape(seed, D, noise_kind, gen, episode=0, NP=NP):
    """The tape that reproduces the Philox stream of (seed, gen, episode) under the site map of include/mbx_layout.h §11."""
    NE = NP * D
    t = np.zeros(tape_stride(D, NP))

    def ph(idx, site):
        return oracle.philox(seed, idx, site, gen, episode)

    def noise(o, sa, sb):
        for i in range(NP):
            w = ph(i, sa)
            if noise_kind == 2:
                t[o + i], t[o + NP + i] = _u53(w[0], w[1]), _u53(w[2], w[3])
            else:
                assert noise_kind == 0, 'only the noise kinds whose draws are exact uniforms are rebuilt here'
    if gen == 0:
        for e in range(NE):
            w = ph(e, SITE_ELEM_R)
            t[e], t[NE + e] = _u53(w[0], w[1]), _u53(w[2], w[3])
        noise(2 * NE, SITE_NOISE1_A, SITE_NOISE1_B)
        xb = 2 * NE + 3 * NP
    else:
        for e in range(NE):
            w = ph(e, SITE_ELEM_A)
            t[e] = _u53(w[0], w[1])
        noise(NE, SITE_NOISE0_A, SITE_NOISE0_B)
        xb = NE + 3 * NP
    for e in range(NE):
        w = ph(e, SITE_GL_CROSS)
        t[xb + e], t[xb + NE + e] = _mulhi(w[0], NP), _u53(w[2], w[3])
        w = ph(e, SITE_GL_MUT)
        t[xb + 2 * NE + e], t[xb + 3 * NE + e] = _u53(w[0], w[1]), _u53(w[2], w[3])
    noise(xb + 4 * NE, SITE_GL_NOISE_A, SITE_GL_NOISE_B)
    for k in range(NP * NSEL):
        t[xb + 4 * NE + 3 * NP + k] = _mulhi(ph(k, SITE_GL_TOUR)[0], NP)
    return t


@pytest.mark.gpu
def test_hip_glpso_philox_equals_tape():
    """The Philox path and the tape path are the same computation: a tape rebuilt on the host from oracle.philox with the documented site
    map gives bit-identical state blocks and results, on a noiseless and a uniform-noise problem, for 20 generations."""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    ids = [15, 102]
    s = Suite([ps[i] for i in ids])
    seeds = np.array([123456789012345, 987654321], dtype=np.uint64)
    a = Batch(s, ALGO_GLPSO, np.arange(2), seeds, NP, 20000, 400, 50)
    t = Batch(s, ALGO_GLPSO, np.arange(2), seeds, NP, 20000, 400, 50)
    fired = False
    for g in range(21):
        tape = np.stack([philox_tape(int(seeds[k]), 10, ps[ids[k]].noise[0], g) for k in range(2)])
        t.set_tape(torch.from_numpy(tape).cuda())
        if g == 0:
            a.reset(); t.reset()
        else:
            a.step(None); t.step(None)
        torch.cuda.synchronize()
        for k in range(2):
            sa, st = a.read_state(k), t.read_state(k)
            assert np.array_equal(sa, st), (ids[k], g, int(np.argmax(sa != st)))
            fired = fired or _fired(split_state(sa, 10)['stag'])
    ra, rt = a.results(), t.results()
    for key in ('cost', 'fes', 'cost_len'):
        assert torch.equal(ra[key], rt[key]), key
    assert fired                                                     # the tournament site was exercised
    a.close(); t.close()


@pytest.mark.gpu
def test_hip_glpso_batch_invariance_and_frozen_done_instances():
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    ids = [1, 5, 8, 15, 20, 24, 103, 117]
    s = Suite([ps[i] for i in ids])
    B, G, max_fes = len(ids), 12, 2000                               # reset + 9 generations reach maxFEs
    pidx = np.arange(B, dtype=np.int32)
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 3
    full = Batch(s, ALGO_GLPSO, pidx, seeds, NP, max_fes, max_fes // 50, 50)
    perm = np.random.RandomState(5).permutation(B)
    parts = [Batch(s, ALGO_GLPSO, pidx[perm[:3]], seeds[perm[:3]], NP, max_fes, max_fes // 50, 50),
             Batch(s, ALGO_GLPSO, pidx[perm[3:]], seeds[perm[3:]], NP, max_fes, max_fes // 50, 50)]
    where = {int(perm[j]): (0, j) if j < 3 else (1, j - 3) for j in range(B)}
    st0 = full.reset().clone()
    for pb in parts:
        pb.reset()
    assert torch.allclose(st0[:, 0].cpu(), torch.full((B,), 2 * NP / max_fes, dtype=torch.float64))
    frozen = {}
    for g in range(1, G + 1):
        st, _, d = full.step(None)
        for pb in parts:
            pb.step(None)
        torch.cuda.synchronize()
        for k in range(B):
            blk = full.read_state(k)
            pb, j = where[k]
            assert np.array_equal(blk, parts[pb].read_state(j)), (ids[k], g)
            sc = split_state(blk, 10)['scalars']
            if k in frozen:
                assert np.array_equal(blk, frozen[k]), (ids[k], g)             # done instances are left untouched
                assert d[k].item() == 1
            else:
                assert sc[1] == 2 * NP * (g + 1), (ids[k], g)                   # 2 NP FEs per generation
                if sc[4] == 1.:
                    frozen[k] = blk.copy()
    assert len(frozen) == B
    ra = full.results()
    for pb, idx in ((0, perm[:3]), (1, perm[3:])):
        rp = parts[pb].results()
        assert torch.equal(ra['cost'][torch.as_tensor(idx).cuda()], rp['cost']) and torch.equal(ra['fes'][torch.as_tensor(idx).cuda()], rp['fes'])
    full.close()
    for pb in parts:
        pb.close()


@pytest.mark.gpu
def test_glpso_in_the_tester_and_the_b1_view(tmp_path):
    import pickle
    import torch
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import GL_PSO
    from metabox_amd.suite import Suite
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda', '--test', '--t_optimizer_for_cp', 'GL_PSO',
                      '--log_dir', str(tmp_path / 'out'), '--test_runs', '2'])
    cfg.maxFEs = 2000
    cfg.log_interval = cfg.maxFEs // cfg.n_logpoint
    cfg.t_optimizer_for_cp = ['GL_PSO']
    t = Tester(cfg)
    t.test()
    with open(t.log_dir + 'test.pkl', 'rb') as f:
        res = pickle.load(f)
    for p in t.test_set.data:
        rows = res['cost'][str(p)]['GL_PSO']
        assert len(rows) == 2 and all(len(r) == 51 for r in rows), str(p)
        assert all(np.all(np.diff(r) <= 0) for r in rows) and all(f <= 2000 for f in res['fes'][str(p)]['GL_PSO'])
    # the B = 1 view is the batch's computation for the same seed
    ps = problems('bbob', 10)
    opt = GL_PSO(copy.deepcopy(cfg))
    np.random.seed(3)
    info = opt.run_episode(ps[8])
    np.random.seed(3)
    seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
    s = ps[8]._bound_suite()
    r = GL_PSO(copy.deepcopy(cfg)).run_batch(s, [ps[8]._suite_index], [seed])
    n = int(r['cost_len'][0].item())
    assert info['fes'] == int(r['fes'][0].item()) and info['cost'] == [float(v) for v in r['cost'][0, :n].cpu().numpy()]
    torch.cuda.synchronize()
