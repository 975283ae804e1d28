"""JDE21 (src/optimizer/jde21.py), a classic baseline of the test harness: the batched HIP kernels (metabox_amd/csrc/mbx_jde21.hpp) replay
the reference's episodes from tests/golden/jde21_traces.npz (tools/gen_golden.py jde21) through mbx_set_tape.  The numpy draws are not
stored: JdeTapeFeeder regenerates them from the seed in the reference's draw order, rejection loops included (include/mbx_layout.h §12).
The crafted-state tests compare one tape step with `restate_step`, a numpy restatement of one update written from the algorithm's rules."""
import copy
import ctypes as C

import numpy as np
import pytest

from helpers import close, load, print_ledger, problems, prove_tie_arrays
from oracle import oracle

TR = load('jde21_traces.npz')
CASES = [str(c) for c in TR['cases']]
NP, SNP, BNP0, ROWS, TRIES = 170, 10, 160, 320, 25
ALGO_JDE21 = 13
SITE_NOISE1_A, SITE_NOISE1_B = 7, 8
SITE_JD_IDX, SITE_JD_PART, SITE_JD_PART2, SITE_JD_CROSS, SITE_JD_RESEED, SITE_JD_NOISE_A, SITE_JD_NOISE_B = 23, 24, 25, 26, 27, 28, 29
T_R1, T_R2, T_R3, T_UF, T_UCR, T_VF, T_VCR, T_JR, T_NOISE, T_CROSS = (k * ROWS for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 11))
SC_GBEST, SC_FES, SC_DONE, SC_EPISODE, SC_BNP, SC_CBEST, SC_CBEST_ID, SC_NRESET = 0, 1, 4, 7, 10, 11, 12, 13


def tape_stride(D):
    return 11 * ROWS + ROWS * D + NP * D


def t_reseed_b(D):
    return 11 * ROWS + ROWS * D


def t_reseed_s(D):
    return t_reseed_b(D) + BNP0 * D


def split_state(st, D, nlog=50):
    o = NP * D
    return {'pop': st[:o].reshape(NP, D), 'cost': st[o:o + NP], 'F': st[o + NP:o + 2 * NP], 'Cr': st[o + 2 * NP:o + 3 * NP],
            'crowd': st[o + 3 * NP:o + 4 * NP], 'scalars': st[o + 4 * NP:o + 4 * NP + 16], 'log': st[o + 4 * NP + 16:o + 4 * NP + 17 + nlog]}


def join_state(s):
    return np.concatenate([s['pop'].ravel(), s['cost'], s['F'], s['Cr'], s['crowd'], s['scalars'], s['log']])


def mig_of(fes, max_fes):
    return 1 if fes < max_fes / 3 else 2 if fes < 2 * max_fes / 3 else 3


class JdeTapeFeeder:
    """numpy's legacy stream as JDE21 consumes it, laid out as the tape of include/mbx_layout.h §12.  The rejection loops and the two
    re-seed draws depend on the optimizer's state (bNP, mig, cbest_id, whether a reset fires): the caller passes what the fixture recorded."""

    def __init__(self, D, noise_kind, rs):
        self.rs, self.D, self.noise = rs, D, noise_kind

    def _noise(self, t, t0, n, total, base):
        r = self.rs
        if self.noise == 1:
            t[base + t0:base + t0 + n] = r.randn(n)
        elif self.noise == 2:
            t[base + t0:base + t0 + n] = r.rand(n)
            t[base + total + t0:base + total + t0 + n] = r.rand(n)
        elif self.noise == 3:
            t[base + t0:base + t0 + n] = r.rand(n)
            t[base + total + t0:base + total + t0 + n] = r.randn(n)
            t[base + 2 * total + t0:base + 2 * total + t0 + n] = r.randn(n)

    def reset_tape(self):
        D = self.D
        t = np.zeros(tape_stride(D))
        t[:NP * D] = self.rs.rand(NP, D).ravel()
        self._noise(t, 0, NP, NP, NP * D)
        return t

    def _draw(self, n, high, reject):
        """randint(high, size=n), then the bounded redraw (:171-193): the rejected entries are redrawn together, 25 times at most."""
        r = self.rs.randint(high, size=n)
        count = 0
        dup = np.where(reject(r))[0]
        while dup.shape[0] > 0 and count < TRIES:
            r[dup] = self.rs.randint(high, size=dup.shape[0])
            dup = np.where(reject(r))[0]
            count += 1
        return r

    def _pass(self, t, t0, n, big, bnp, mig, cid):
        D, rs = self.D, self.rs
        me = np.arange(n)
        if big:
            r1 = self._draw(n, bnp, lambda r: (r == me) * (r == cid))
            r2 = self._draw(n, bnp + mig, lambda r: (r == me) + (r == r1))
            r3 = self._draw(n, bnp + mig, lambda r: (r == me) + (r == r1) + (r == r2))
        else:
            r1 = self._draw(n, SNP, lambda r: r == me) + bnp
            r2 = self._draw(n, SNP, lambda r: (r == me) + (r + bnp == r1)) + bnp
            r3 = self._draw(n, SNP, lambda r: (r == me) + (r + bnp == r1) + (r + bnp == r2)) + bnp
        sl = slice(t0, t0 + n)
        t[T_R1:][sl], t[T_R2:][sl], t[T_R3:][sl] = r1, r2, r3
        t[T_UF:][sl] = rs.rand(n)
        t[T_UCR:][sl] = rs.rand(n)
        t[T_VF:][sl] = rs.rand(n)
        t[T_VCR:][sl] = rs.rand(n)
        t[T_JR:][sl] = rs.randint(D, size=n)
        t[T_CROSS + t0 * D:T_CROSS + (t0 + n) * D] = rs.rand(n, D).ravel()
        self._noise(t, t0, n, ROWS, T_NOISE)

    def step_tape(self, bnp, mig, cid_r1, nreset, sreset):
        D = self.D
        t = np.zeros(tape_stride(D))
        if nreset:
            t[t_reseed_b(D):t_reseed_b(D) + bnp * D] = self.rs.random_sample((bnp, D)).ravel()
        self._pass(t, 0, bnp, True, bnp, mig, cid_r1)
        if sreset:
            t[t_reseed_s(D):t_reseed_s(D) + SNP * D] = self.rs.random_sample((SNP, D)).ravel()
        for p in range(bnp // SNP):
            self._pass(t, BNP0 + SNP * p, SNP, False, bnp, mig, cid_r1)
        return t


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


def _step_args(key, g, max_fes):
    """What the feeder needs for update g (1-based row of the per-generation arrays)."""
    bnp = int(TR[f'{key}/bnp'][g - 1])
    return bnp, mig_of(TR[f'{key}/fes'][g - 1], max_fes), int(TR[f'{key}/cid_r1'][g]), int(TR[f'{key}/nreset'][g]), int(TR[f'{key}/sreset'][g])


# ------------------------------------------------------------------------------------------------ CPU
def test_jde21_is_exported_and_picked_up_by_the_tester(tmp_path):
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import JDE21
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--test', '--t_optimizer_for_cp', 'JDE21', '--log_dir', str(tmp_path / 'out')])
    t = Tester(cfg)
    assert 'JDE21' in [type(o).__name__ for o in t.t_optimizer_for_cp] and 'JDE21' not in t.skipped
    assert isinstance(JDE21(copy.deepcopy(cfg)), JDE21)
    assert all('JDE21' in t.test_results['cost'][str(p)] for p in t.test_set.data)


def test_abi_geometry_of_jde21():
    from metabox_amd import _abi
    lib = _abi.load_lib()
    assert _abi.ALGO_JDE21 == ALGO_JDE21
    for D in (10, 12, 30, 40):
        cfg = oracle.make_cfg(ALGO_JDE21, NP, D, 2000 * D, 40 * D, 50)
        assert lib.mbx_tape_stride(C.byref(cfg)) == tape_stride(D)
        assert lib.mbx_state_dim(C.byref(cfg)) == 1
        assert lib.mbx_action_dim(C.byref(cfg)) == 0
    for algo in (12, 14):                                            # 12 is not assigned, 14 not built
        bad = oracle.make_cfg(algo, NP, 10, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(bad)) < 0 and lib.mbx_tape_stride(C.byref(bad)) < 0
    wrong_np = oracle.make_cfg(ALGO_JDE21, 100, 10, 20000, 400, 50)
    assert lib.mbx_state_dim(C.byref(wrong_np)) < 0


@pytest.mark.parametrize('case', CASES)
def test_feeder_consumes_the_reference_stream(case):
    """Over the whole fixture episode(s) the feeder draws exactly what the reference drew: the next np.random.rand() after the episode is
    the one the generator recorded."""
    dim, seed, eps = _episodes(case)
    max_fes = float(TR[f'{case}/max_fes'])
    rs = np.random.RandomState(seed)
    for p, nk, key in eps:
        fd = JdeTapeFeeder(dim, nk, rs)
        fd.reset_tape()
        for g in range(1, len(TR[f'{key}/fes'])):
            fd.step_tape(*_step_args(key, g, max_fes))
    assert rs.rand() == float(TR[f'{case}/next_rand']), case


def test_fixture_covers_the_quirks():
    """The fixture exercises what it is meant to pin."""
    fes, mf = TR['bbob/10/1/51/fes'], TR['bbob/10/1/51/max_fes']
    assert fes[-1] < mf and TR['bbob/10/1/51/gbest'][-1] <= 1e-8                                   # early stop
    assert TR['bbob-noisy/10/101/52/fes'][-1] < TR['bbob-noisy/10/101/52/max_fes']                  # ... on a noisy function
    k = 'bbob/10/15/53'                                                                            # the missed third halving at the full budget
    assert TR[f'{k}/max_fes'] == 20000 and TR[f'{k}/fes'][-1] == 20010 and TR[f'{k}/bnp'][-1] + SNP == 50 and len(TR[f'{k}/cost']) == 51
    assert sorted(set(TR['bbob/30/10/54/bnp'] + SNP), reverse=True) == [170, 90, 50, 30]             # all three halvings
    assert TR['bbob/10/7/58/counters'][-1][1] > 0 and TR['bbob/10/7/58/max_abs_x'] > 5.0             # sReset, rows outside the box
    assert TR['bbob/10/22/2/counters'][-1][2] > 1                                                  # repeated elite copies
    assert {_problem(*c.split('/')[:3])[1] for c in CASES if c.startswith('bbob-noisy')} == {1, 2, 3}
    assert any(c.startswith('protein') for c in CASES)
    assert any(c.startswith('second') for c in CASES)
    # crowding targets collide in every big pass (the selection rule for shared targets is exercised throughout)
    cr, bnp = TR[f'{k}/crowd'], TR[f'{k}/bnp']
    assert len(np.unique(cr[:bnp[0]])) < bnp[0]


# ------------------------------------------------------------------------------------------------ restatement of one update
def _pymod(a, m):
    r = np.fmod(a, m)
    return np.where((r != 0) & (r < 0), r + m, r)


def restate_step(s, t, evalf, lb, ub, max_fes, D):
    """One update on a split state `s` (copied) with the draws of tape `t`; evalf(X) -> costs.  Returns the new split state and a record
    of what happened (crowding targets, winners, repaired coordinates)."""
    s = {k: np.array(v, dtype=np.float64, copy=True) for k, v in s.items()}
    pop, cost, F, Cr, sc = s['pop'], s['cost'], s['F'], s['Cr'], s['scalars']
    bnp, cbest, cid, fes = int(sc[SC_BNP]), sc[SC_CBEST], int(sc[SC_CBEST_ID]), sc[SC_FES]
    n_live = bnp + SNP
    info = {'repaired_far': 0, 'winners': []}

    def stuck(c, best):
        eqs = int(np.sum(np.fabs(c - best) < 1e-12))
        return eqs > 2 and eqs > len(c) * 0.25

    if stuck(cost[:bnp], sc[SC_GBEST]):
        sc[SC_NRESET] += 1
        pop[:bnp] = t[t_reseed_b(D):t_reseed_b(D) + bnp * D].reshape(bnp, D) * (ub - lb) + ub
        F[:bnp], Cr[:bnp], cost[:bnp] = 0.5, 0.9, 1e15
        cbest, cid = cost[:n_live].min(), int(np.argmin(cost[:n_live]))

    def one_pass(t0, n, big):
        nonlocal cbest, cid
        rows = np.arange(n) if big else np.arange(n) + bnp
        sl = slice(t0, t0 + n)
        r1, r2, r3, jr = (t[o:][sl].astype(int) for o in (T_R1, T_R2, T_R3, T_JR))
        f = np.where(t[T_VF:][sl] < 0.1, t[T_UF:][sl] * 1.1 + (0.1 if big else 0.17), F[rows])
        c = np.where(t[T_VCR:][sl] < 0.1, t[T_UCR:][sl] * 1.1 + (0.0 if big else 0.1), Cr[rows])
        c[c > 1] = 0
        v = pop[r1] + f[:, None] * (pop[r2] - pop[r3])
        info['repaired_far'] += int(np.sum((v > ub + (ub - lb)) | (v < lb - (ub - lb))))
        hi = v > ub
        v[hi] = _pymod(v[hi] - lb, ub - lb) + lb
        lo = v < lb
        v[lo] = _pymod(v[lo] - ub, ub - lb) + lb
        u = np.where(t[T_CROSS + t0 * D:T_CROSS + (t0 + n) * D].reshape(n, D) < c[:, None], v, pop[rows])
        u[np.arange(n), jr] = v[np.arange(n), jr]
        uc = evalf(u)
        if big:
            ids = np.argmin(np.sum((pop[:n][None, :, :] - u[:, None, :]) ** 2, -1), -1)
            info['crowd'] = ids
        else:
            ids = rows
        # per target: the lowest trial cost among its candidates if strictly below the incumbent's, the earliest trial on equal costs
        winners = []
        for tgt in np.unique(ids):
            cand = np.where(ids == tgt)[0]
            k = cand[np.argmin(uc[cand])]
            if uc[k] < cost[tgt]:
                winners.append(k)
        for k in sorted(winners):                                    # cbest: the running strict minimum in trial order
            pop[ids[k]], cost[ids[k]], F[ids[k]], Cr[ids[k]] = u[k], uc[k], f[k], c[k]
            if uc[k] < cbest:
                cbest, cid = uc[k], int(ids[k])
        if big:
            info['winners'] = sorted(winners)
            info['trial_cost'] = uc

    one_pass(0, bnp, True)
    if cid >= bnp and stuck(cost[bnp:n_live], cbest):
        sc[SC_NRESET + 1] += 1
        keep = pop[cid].copy()
        pop[bnp:n_live] = t[t_reseed_s(D):t_reseed_s(D) + SNP * D].reshape(SNP, D) * (ub - lb) + ub
        F[bnp:n_live], Cr[bnp:n_live], cost[bnp:n_live] = 0.5, 0.9, 1e15
        pop[cid], cost[cid] = keep, cbest
    if cid < bnp:
        sc[SC_NRESET + 2] += 1
        cost[bnp], pop[bnp], cid = cbest, pop[cid], bnp
    for p in range(bnp // SNP):
        one_pass(BNP0 + SNP * p, SNP, False)
    fes += 2 * bnp
    sc[SC_GBEST] = cost[:n_live].min()
    if any(fes - n_live <= q * max_fes <= fes for q in (0.25, 0.5, 0.75)):
        h = bnp // 2
        for a in (pop, cost, F, Cr):
            a[:n_live - h] = a[h:n_live].copy()
        bnp = h
        cid = int(np.argmin(cost[:bnp + SNP]))
    sc[SC_BNP], sc[SC_CBEST], sc[SC_CBEST_ID], sc[SC_FES] = bnp, cbest, cid, fes
    s['crowd'][:len(info['crowd'])] = info['crowd']
    return s, info


# ------------------------------------------------------------------------------------------------ GPU
def _rows(key, g):
    """The live costs of row g of the fixture's ragged cost array, and the crowding targets of update g."""
    n = TR[f'{key}/bnp'].astype(int) + SNP
    o = int(n[:g].sum())
    cost = TR[f'{key}/cost_rows'][o:o + n[g]]
    crowd = None
    if g > 0:
        b = TR[f'{key}/bnp'].astype(int)
        oc = int(b[:g - 1].sum())
        crowd = TR[f'{key}/crowd'][oc:oc + b[g - 1]]
    return cost, crowd


def _replay(b, idx, key, fd, ledger, case, max_fes, diverged):
    """One fixture episode of instance `idx` of batch `b` driven by the feeder; checks every generation against the reference."""
    import torch
    D = fd.D
    want = {k: TR[f'{key}/{k}'] for k in ('gbest', 'fes', 'cbest', 'cbest_id', 'bnp', 'counters')}
    snaps = set(int(g) for g in TR[f'{key}/snap_gens'])
    G = len(want['gbest']) - 1
    tape = torch.zeros(b.B, b.tape_stride, dtype=torch.float64, device='cuda')
    prev = prev_want = None
    for g in range(G + 1):
        tape[idx] = torch.from_numpy(fd.reset_tape() if g == 0 else fd.step_tape(*_step_args(key, g, max_fes)))
        b.set_tape(tape)
        if g == 0:
            b.reset()
        else:
            b.step(None)
        st = split_state(b.read_state(idx), D)
        sc = st['scalars']
        wcost, wcrowd = _rows(key, g)
        n = len(wcost)
        assert sc[SC_FES] == want['fes'][g] and sc[SC_BNP] == want['bnp'][g], (case, key, g, sc[SC_FES], sc[SC_BNP])
        if not diverged and g > 0:
            # the first generation whose selection decisions differ must sit on a proven near-tie; float tolerances only afterwards
            h = len(prev_want) - n                                   # rows dropped by a halving in this update
            ref_i = (wcost != prev_want[h:]).astype(np.float64)
            cur_i = (st['cost'][:n] != prev['cost'][h:h + n]).astype(np.float64)
            if np.array_equal(st['crowd'][:len(wcrowd)], wcrowd):
                diverged = not prove_tie_arrays(prev_want[h:], wcost, ref_i, prev['cost'][h:h + n], st['cost'][:n], cur_i, ledger, 'select', key, g)
            else:
                assert False, (case, key, g, 'crowding targets differ', np.nonzero(st['crowd'][:len(wcrowd)] != wcrowd)[0])
        if not diverged:
            assert sc[SC_CBEST_ID] == want['cbest_id'][g], (case, key, g, sc[SC_CBEST_ID], want['cbest_id'][g])
            assert np.array_equal(sc[SC_NRESET:SC_NRESET + 3], want['counters'][g]), (case, key, g, sc[SC_NRESET:SC_NRESET + 3], want['counters'][g])
            assert close(st['cost'][:n], wcost), (case, key, g, np.abs(st['cost'][:n] - wcost).max())
            assert close(sc[SC_CBEST], want['cbest'][g]), (case, key, g)
            if g in snaps:
                assert np.array_equal(st['F'][:n], TR[f'{key}/snap{g}/F']) and np.array_equal(st['Cr'][:n], TR[f'{key}/snap{g}/Cr']), (case, key, g)
                assert np.array_equal(st['pop'][:n], TR[f'{key}/snap{g}/pop']), (case, key, g, np.abs(st['pop'][:n] - TR[f'{key}/snap{g}/pop']).max())
        assert close(sc[SC_GBEST], want['gbest'][g]), (case, key, g, sc[SC_GBEST], want['gbest'][g])
        prev, prev_want = st, wcost
    assert sc[SC_DONE] == 1., (case, key)                             # the episode ended where the reference's did
    return diverged


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_jde21_tape_replay_matches_reference(case):
    """Every fixture episode, every generation: fes, bNP, cbest_id, the counters and the crowding targets equal, costs / cbest / gbest and
    the cost log at helpers.close; a selection that differs must be a proven near-tie (none is expected: the ledger stays empty)."""
    from metabox_amd.suite import Batch, Suite
    dim, seed, eps = _episodes(case)
    max_fes = int(TR[f'{case}/max_fes'])
    s = Suite([p for p, _, _ in eps])
    b = Batch(s, ALGO_JDE21, [0], [seed], NP, max_fes, max_fes // 50, 50)
    assert (b.state_dim, b.action_dim, b.tape_stride) == (1, 0, tape_stride(dim))
    rs = np.random.RandomState(seed)
    ledger, diverged = [], False
    for k, (p, nk, key) in enumerate(eps):
        if k > 0:
            b.rebind([k], [seed])                                    # same batch, next problem: nothing carries over
        diverged = _replay(b, 0, key, JdeTapeFeeder(dim, nk, rs), ledger, case, max_fes, diverged)
    res = b.results()
    n = int(res['cost_len'][0].item())
    ref_cost = TR[f'{case}/cost']
    assert n == len(ref_cost) and close(res['cost'][0, :n].cpu().numpy(), ref_cost), (case, n, len(ref_cost))
    assert res['fes'][0].item() == TR[f'{case}/fes'][-1]
    print_ledger(ledger)
    b.close()


def _crafted(D=10, max_fes=20000, seed=7):
    """A batch of one Sphere instance after a tape reset, its split state, a random valid step tape and the cost function."""
    import torch
    from metabox_amd.suite import Batch, Suite
    p = problems('bbob', D)[1]
    s = Suite([p])
    b = Batch(s, ALGO_JDE21, [0], [seed], NP, max_fes, max_fes // 50, 50)
    rs = np.random.RandomState(seed)
    fd = JdeTapeFeeder(D, 0, rs)
    tape = torch.from_numpy(fd.reset_tape()).cuda().reshape(1, -1)
    b.set_tape(tape)
    b.reset()
    st = split_state(b.read_state(0), D)
    t = fd.step_tape(BNP0, 1, int(st['scalars'][SC_CBEST_ID]), 1, 1)          # both re-seed slots filled

    def evalf(X):
        return s.eval(0, X) - s.optimum(0)
    return b, s, st, t, evalf, p


def _run_crafted(b, st, t, evalf, p, D=10, max_fes=20000):
    import torch
    b.write_state(0, join_state(st))
    b.set_tape(torch.from_numpy(t).cuda().reshape(1, -1))
    b.step(None)
    got = split_state(b.read_state(0), D)
    want, info = restate_step(st, t, evalf, p.lb, p.ub, max_fes, D)
    n = int(want['scalars'][SC_BNP]) + SNP
    assert np.array_equal(got['crowd'][:BNP0], want['crowd'][:BNP0]), np.nonzero(got['crowd'][:BNP0] != want['crowd'][:BNP0])[0]
    for k in (SC_FES, SC_BNP, SC_CBEST_ID, SC_NRESET, SC_NRESET + 1, SC_NRESET + 2):
        assert got['scalars'][k] == want['scalars'][k], (k, got['scalars'][k], want['scalars'][k])
    assert np.array_equal(got['pop'][:n], want['pop'][:n]), np.abs(got['pop'][:n] - want['pop'][:n]).max()
    assert np.array_equal(got['F'][:n], want['F'][:n]) and np.array_equal(got['Cr'][:n], want['Cr'][:n])
    assert close(got['cost'][:n], want['cost'][:n]) and close(got['scalars'][SC_CBEST], want['scalars'][SC_CBEST])
    assert close(got['scalars'][SC_GBEST], want['scalars'][SC_GBEST])
    return got, want, info


@pytest.mark.gpu
def test_hip_jde21_big_reset_on_a_crafted_state():
    """(a) More than a quarter of the big costs within 1e-12 of gbest: the big population is re-seeded outside the box with cost 1e15,
    F / Cr are restored and cbest is recomputed (it was planted far below every cost) before the passes run."""
    b, s, st, t, evalf, p = _crafted()
    st['cost'][:60] = 3.0
    st['scalars'][SC_GBEST] = 3.0 + 5e-13
    st['scalars'][SC_CBEST] = -1e30
    st['F'][:BNP0], st['Cr'][:BNP0] = 0.7, 0.3
    got, want, info = _run_crafted(b, st, t, evalf, p)
    assert got['scalars'][SC_NRESET] == 1 and got['scalars'][SC_CBEST] > -1e30
    untouched = np.setdiff1d(np.arange(BNP0), info['crowd'][info['winners']])
    assert len(untouched) > 0
    assert np.all(got['cost'][untouched] == 1e15) and np.all(got['F'][untouched] == 0.5) and np.all(got['Cr'][untouched] == 0.9)
    assert np.all(got['pop'][untouched] >= p.ub) and np.all(got['pop'][untouched] <= 2 * p.ub - p.lb)
    b.close()


@pytest.mark.gpu
def test_hip_jde21_selection_with_one_shared_target():
    """(b) All 160 trials are nearest to row 7: the lowest trial wins, and of two equal trials the earlier one (trial k and k + 80 are the
    same vector with different Cr draws, so the Cr the row ends with names the winner)."""
    b, s, st, t, evalf, p = _crafted()
    rs = np.random.RandomState(11)
    st['pop'][:BNP0] = 4.0 + 0.01 * rs.rand(BNP0, 10)
    st['pop'][7] = -4.0
    st['cost'][:BNP0] = 1e9
    st['scalars'][SC_GBEST], st['scalars'][SC_CBEST], st['scalars'][SC_CBEST_ID] = st['cost'][BNP0:].min(), st['cost'][BNP0:].min(), BNP0 + int(np.argmin(st['cost'][BNP0:]))
    r2, r3, uf = rs.randint(0, BNP0, 80), rs.randint(0, BNP0, 80), rs.rand(80)
    r2[r2 == 7] = 8
    r3[r3 == 7] = 9
    t[T_R1:T_R1 + BNP0] = 7
    t[T_R2:T_R2 + BNP0], t[T_R3:T_R3 + BNP0], t[T_UF:T_UF + BNP0] = np.tile(r2, 2), np.tile(r3, 2), np.tile(uf, 2)
    t[T_VF:T_VF + BNP0], t[T_VCR:T_VCR + BNP0] = 0.0, 0.0            # F and Cr come from the draws
    t[T_UCR:T_UCR + BNP0] = 0.1 + 0.5 * rs.rand(BNP0)                # distinct Cr in (0, 1)
    t[T_CROSS:T_CROSS + BNP0 * 10] = 0.0                             # every coordinate crosses over
    got, want, info = _run_crafted(b, st, t, evalf, p)
    assert np.all(got['crowd'][:BNP0] == 7) and len(info['winners']) == 1 and info['winners'][0] < 80
    k = info['winners'][0]
    assert info['trial_cost'][k] == info['trial_cost'][k + 80] == info['trial_cost'].min()
    assert got['Cr'][7] == t[T_UCR + k] * 1.1 + 0.0
    b.close()


@pytest.mark.gpu
def test_hip_jde21_crowding_prefers_the_lower_of_two_identical_rows():
    """(c) Rows 5 and 20 are the same point and trial 0 is that point: both distances are zero, the target is row 5."""
    b, s, st, t, evalf, p = _crafted()
    st['pop'][20], st['cost'][20] = st['pop'][5], st['cost'][5]
    t[T_R1], t[T_R2], t[T_R3] = 5, 30, 30
    t[T_CROSS:T_CROSS + 10] = 0.0
    t[T_VCR], t[T_UCR] = 0.0, 0.5
    got, want, info = _run_crafted(b, st, t, evalf, p)
    assert got['crowd'][0] == 5
    b.close()


@pytest.mark.gpu
def test_hip_jde21_bound_repair_is_pythons_modulo():
    """(d) Trial coordinates more than one box width beyond either bound: the repair is Python's float %."""
    b, s, st, t, evalf, p = _crafted()
    st['pop'][1], st['pop'][2], st['pop'][3], st['pop'][4] = 5.0, -5.0, 4.9 - 0.01 * np.arange(10), -4.9 + 0.013 * np.arange(10)
    st['cost'][:BNP0] = 1e9
    up = np.arange(BNP0) % 2 == 0
    t[T_R1:T_R1 + BNP0] = np.where(up, 3, 4)
    t[T_R2:T_R2 + BNP0] = np.where(up, 1, 2)
    t[T_R3:T_R3 + BNP0] = np.where(up, 2, 1)
    t[T_VF:T_VF + BNP0] = 0.0
    t[T_UF:T_UF + BNP0] = 0.92 + 0.0799 * np.random.RandomState(3).rand(BNP0)     # F in (1.11, 1.2): |v| beyond 15
    got, want, info = _run_crafted(b, st, t, evalf, p)
    assert info['repaired_far'] > 1000 and len(info['winners']) > 10
    assert np.all(np.abs(got['pop'][:BNP0][info['crowd'][info['winners']]]) <= 5.0)
    b.close()


def _u53(w0, w1):
    return ((w0 >> 5) * 67108864.0 + (w1 >> 6)) / 9007199254740992.0


def _mulhi(w, n):
    return (w * n) >> 32


def philox_rows(seed, gen, rows, t0, big, bnp, mig, cid, D, episode=1):
    """(r1, r2, r3, jrand) of trial rows t0.. under the site map of include/mbx_layout.h §12: one draw, then at most 25 redraws."""
    out = []
    for k in range(rows):
        tr = t0 + k
        i = k if big else bnp + k
        lo, n1, n23 = (0, bnp, bnp + mig) if big else (bnp, SNP, SNP)
        w = [oracle.philox(seed, tr * 32 + a, SITE_JD_IDX, gen, episode) if a == 0 else None for a in range(TRIES + 1)]

        def word(a, j):
            if w[a] is None:
                w[a] = oracle.philox(seed, tr * 32 + a, SITE_JD_IDX, gen, episode)
            return w[a][j]

        def settle(j, n, reject):
            r = lo + _mulhi(word(0, j), n)
            a = 1
            while a <= TRIES and reject(r):
                r = lo + _mulhi(word(a, j), n)
                a += 1
            return r
        r1 = settle(0, n1, (lambda r: r == i and r == cid) if big else (lambda r: r == i))
        r2 = settle(1, n23, lambda r: r == i or r == r1)
        r3 = settle(2, n23, lambda r: r == i or r == r1 or r == r2)
        out.append((r1, r2, r3, _mulhi(word(0, 3), D)))
    return np.array(out)


def philox_tape(seed, D, noise_kind, gen, bnp=BNP0, mig=1, cid=0, episode=1):
    """The tape that reproduces the Philox stream of (seed, gen, episode)."""
    t = np.zeros(tape_stride(D))

    def ph(idx, site):
        return oracle.philox(seed, idx, site, gen, episode)

    def noise(base, rows, total, sa, sb):
        for i in rows:
            if noise_kind == 2:
                w = ph(i, sa)
                t[base + i], t[base + total + i] = _u53(w[0], w[1]), _u53(w[2], w[3])
            else:
                assert noise_kind == 0, 'only the noise kinds whose draws are exact uniforms are rebuilt here'
    if gen == 0:
        for e in range(NP * D):
            w = ph(e, SITE_JD_CROSS)
            t[e] = _u53(w[0], w[1])
        noise(NP * D, range(NP), NP, SITE_NOISE1_A, SITE_NOISE1_B)
        return t
    passes = [(0, bnp, True)] + [(BNP0 + SNP * p, SNP, False) for p in range(bnp // SNP)]
    for t0, n, big in passes:
        idx = philox_rows(seed, gen, n, t0, big, bnp, mig, cid, D, episode)
        for k in range(n):
            tr = t0 + k
            t[T_R1 + tr], t[T_R2 + tr], t[T_R3 + tr], t[T_JR + tr] = idx[k]
            w = ph(tr, SITE_JD_PART)
            t[T_UF + tr], t[T_UCR + tr] = _u53(w[0], w[1]), _u53(w[2], w[3])
            w = ph(tr, SITE_JD_PART2)
            t[T_VF + tr], t[T_VCR + tr] = _u53(w[0], w[1]), _u53(w[2], w[3])
            for d in range(D):
                w = ph(tr * D + d, SITE_JD_CROSS)
                t[T_CROSS + tr * D + d] = _u53(w[0], w[1])
        noise(T_NOISE, range(t0, t0 + n), ROWS, SITE_JD_NOISE_A, SITE_JD_NOISE_B)
    for e in range(BNP0 * D):
        w = ph(e, SITE_JD_RESEED)
        t[t_reseed_b(D) + e] = _u53(w[0], w[1])
        if e < SNP * D:
            t[t_reseed_s(D) + e] = _u53(w[2], w[3])
    return t


@pytest.mark.gpu
def test_hip_jde21_philox_equals_tape():
    """The Philox path and the tape path are the same computation: a tape rebuilt on the host from oracle.philox with the documented site
    map (bounded redraw included) gives bit-identical state blocks and results, on a noiseless and a uniform-noise problem, across the
    first halving.  The cbest_id the r1 test sees is the one at the start of the step (no big reset fires here: asserted)."""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    ids = [15, 102]
    s = Suite([ps[i] for i in ids])
    seeds = np.array([123456789012345, 987654321], dtype=np.uint64)
    max_fes = 4000
    a = Batch(s, ALGO_JDE21, np.arange(2), seeds, NP, max_fes, max_fes // 50, 50)
    t = Batch(s, ALGO_JDE21, np.arange(2), seeds, NP, max_fes, max_fes // 50, 50)
    redrawn, halved = 0, False
    for g in range(9):
        rows = []
        for k in range(2):
            sc = split_state(a.read_state(k), 10)['scalars']
            if g == 0:
                rows.append(philox_tape(int(seeds[k]), 10, ps[ids[k]].noise[0], 0, episode=int(sc[SC_EPISODE]) + 1))
            else:
                bnp, cid, ep = int(sc[SC_BNP]), int(sc[SC_CBEST_ID]), int(sc[SC_EPISODE])
                rows.append(philox_tape(int(seeds[k]), 10, ps[ids[k]].noise[0], g, bnp, mig_of(sc[SC_FES], max_fes), cid, ep))
                first = np.array([_mulhi(oracle.philox(int(seeds[k]), i * 32, SITE_JD_IDX, g, ep)[1], bnp + mig_of(sc[SC_FES], max_fes)) for i in range(bnp)])
                redrawn += int(np.sum(first != rows[-1][T_R2:T_R2 + bnp]))
                halved = halved or bnp < BNP0
        t.set_tape(torch.from_numpy(np.stack(rows)).cuda())
        if g == 0:
            a.reset(); t.reset()
        else:
            a.step(None); t.step(None)
        torch.cuda.synchronize()
        for k in range(2):
            sa, st = a.read_state(k), t.read_state(k)
            assert np.array_equal(sa, st), (ids[k], g, int(np.argmax(sa != st)))
            assert split_state(sa, 10)['scalars'][SC_NRESET] == 0
    ra, rt = a.results(), t.results()
    for key in ('cost', 'fes', 'cost_len'):
        assert torch.equal(ra[key], rt[key]), key
    assert redrawn > 0 and halved                                    # the redraw and a halved population were exercised
    a.close(); t.close()


def test_philox_index_draws_are_uniform_under_the_bounded_redraw():
    """The resolved indices of the Philox mode (philox_rows, the host restatement that test_hip_jde21_philox_equals_tape proves equal to the
    kernel's draws bit for bit): r1 uniform on [0, bNP), r2 uniform on the bNP + mig - 2 rows other than i and r1, r3 on the rows other
    than i, r1, r2, jrand uniform on [0, D) -- the distributions the reference's rejection loops produce."""
    from scipy import stats
    bnp, mig, D = 40, 2, 10
    rows = np.concatenate([philox_rows(1000003 * k + 17, 1 + k % 97, bnp, 0, True, bnp, mig, -1, D) for k in range(150)])      # 6000 rows
    i = np.tile(np.arange(bnp), 150)
    r1, r2, r3, jr = rows.T
    assert r1.min() >= 0 and r1.max() < bnp and r2.max() < bnp + mig and r3.max() < bnp + mig
    assert not np.any(r2 == i) and not np.any(r2 == r1) and not np.any((r3 == i) | (r3 == r1) | (r3 == r2))
    assert stats.chisquare(np.bincount(r1, minlength=bnp)).pvalue > 1e-4
    assert stats.chisquare(np.bincount(jr, minlength=D)).pvalue > 1e-4
    # rank of r2 among the allowed rows is uniform on [0, bNP + mig - 2) (r1 == i is allowed: one exclusion less there)
    same = r1 == i
    rank2 = r2 - (r2 > i) - ((r2 > r1) & ~same)
    assert stats.chisquare(np.bincount(rank2[~same], minlength=bnp + mig - 2)).pvalue > 1e-4
    excl = np.sort(np.stack([i, r1, r2]), 0)
    ok = (excl[0] != excl[1]) & (excl[1] != excl[2])
    rank3 = r3 - (r3 > excl[0]) - (r3 > excl[1]) - (r3 > excl[2])
    assert stats.chisquare(np.bincount(rank3[ok], minlength=bnp + mig - 3)).pvalue > 1e-4
    # the small passes: r1 != i, all three distinct, uniform over the 10 rows
    small = np.concatenate([philox_rows(7919 * k + 3, 1 + k % 31, SNP, BNP0, False, bnp, mig, 0, D) for k in range(300)])
    j = np.tile(np.arange(SNP), 300) + bnp
    assert small[:, :3].min() >= bnp and small[:, :3].max() < bnp + SNP
    assert not np.any(small[:, 0] == j) and not np.any((small[:, 1] == j) | (small[:, 1] == small[:, 0]))
    assert not np.any((small[:, 2] == j) | (small[:, 2] == small[:, 0]) | (small[:, 2] == small[:, 1]))
    assert stats.chisquare(np.bincount(small[:, 0] - bnp, minlength=SNP)).pvalue > 1e-4


@pytest.mark.gpu
def test_hip_jde21_batch_invariance_and_frozen_done_instances():
    """Results do not depend on the batch order or on how the batch is split; done instances are left untouched; with early_stop = False an
    instance that reaches 1e-8 keeps running to the budget."""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    ids = [1, 5, 8, 15, 20, 24, 103, 117]
    s = Suite([ps[i] for i in ids])
    B, max_fes = len(ids), 3000
    pidx = np.arange(B, dtype=np.int32)
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 3
    full = Batch(s, ALGO_JDE21, pidx, seeds, NP, max_fes, max_fes // 50, 50)
    perm = np.random.RandomState(5).permutation(B)
    parts = [Batch(s, ALGO_JDE21, pidx[perm[:3]], seeds[perm[:3]], NP, max_fes, max_fes // 50, 50),
             Batch(s, ALGO_JDE21, pidx[perm[3:]], seeds[perm[3:]], NP, max_fes, max_fes // 50, 50)]
    where = {int(perm[j]): (0, j) if j < 3 else (1, j - 3) for j in range(B)}
    st0 = full.reset().clone()
    for pb in parts:
        pb.reset()
    assert torch.allclose(st0[:, 0].cpu(), torch.full((B,), NP / max_fes, dtype=torch.float64))
    frozen = {}
    for g in range(1, 30):
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
            elif sc[SC_DONE] == 1.:
                frozen[k] = blk.copy()
        if len(frozen) == B:
            break
    assert len(frozen) == B
    ra = full.results()
    for pb, idx in ((0, perm[:3]), (1, perm[3:])):
        rp = parts[pb].results()
        assert torch.equal(ra['cost'][torch.as_tensor(idx).cuda()], rp['cost']) and torch.equal(ra['fes'][torch.as_tensor(idx).cuda()], rp['fes'])
    full.close()
    for pb in parts:
        pb.close()
    # Sphere reaches 1e-8 well inside 20000 FEs (fixture: fes 5290); without the early stop it runs to the budget
    s1 = Suite([ps[1]])
    nb = Batch(s1, ALGO_JDE21, [0], [51], NP, 20000, 400, 50, early_stop=False)
    nb.reset()
    below_at = None
    for g in range(1, 200):
        _, _, d = nb.step(None)
        sc = split_state(nb.read_state(0), 10)['scalars']
        if below_at is None and sc[SC_GBEST] <= 1e-8:
            below_at = sc[SC_FES]
            assert sc[SC_DONE] == 0.
        if sc[SC_DONE] == 1.:
            break
    assert below_at is not None and below_at < 20000 <= sc[SC_FES]
    nb.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dim', [10, 30, 40])
def test_hip_jde21_runs_at_every_bbob_dimension(dim):
    """The kernels launch at D = 10, 30 and 40 (D = 12 is the protein replay case): five Philox steps advance fes by 320 each, the
    population stays finite and inside [lb, 2 ub - lb], gbest never rises."""
    from metabox_amd.suite import Batch, Suite
    ps = problems('bbob', dim)
    ids = [1, 8, 15, 21]
    s = Suite([ps[i] for i in ids])
    b = Batch(s, ALGO_JDE21, np.arange(4), np.arange(4, dtype=np.uint64) + 11, NP, 2000 * dim, 40 * dim, 50)
    b.reset()
    last = [split_state(b.read_state(k), dim)['scalars'][SC_GBEST] for k in range(4)]
    for g in range(1, 6):
        b.step(None)
        for k in range(4):
            st = split_state(b.read_state(k), dim)
            assert st['scalars'][SC_FES] == NP + 320 * g and st['scalars'][SC_BNP] == BNP0
            assert np.all(np.isfinite(st['pop'])) and st['pop'].min() >= -5.0 and st['pop'].max() <= 15.0
            assert np.all(st['crowd'][:BNP0] >= 0) and np.all(st['crowd'][:BNP0] < BNP0)
            assert st['scalars'][SC_GBEST] <= last[k] and st['scalars'][SC_GBEST] == st['cost'].min()
            last[k] = st['scalars'][SC_GBEST]
    b.close()


@pytest.mark.gpu
def test_jde21_in_the_tester_and_the_b1_view(tmp_path):
    import pickle
    import torch
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import JDE21
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda', '--test', '--t_optimizer_for_cp', 'JDE21',
                      '--log_dir', str(tmp_path / 'out'), '--test_runs', '2'])
    cfg.t_optimizer_for_cp = ['JDE21']
    assert cfg.maxFEs == 20000
    t = Tester(cfg)
    t.test()
    with open(t.log_dir + 'test.pkl', 'rb') as f:
        res = pickle.load(f)
    for p in t.test_set.data:
        rows = res['cost'][str(p)]['JDE21']
        assert len(rows) == 2 and all(len(r) == 51 for r in rows), str(p)
        assert all(np.all(np.diff(r) <= 0) for r in rows), str(p)
        # an episode ends at 20010 (170 + 320 k ... with two halvings) or earlier, at 1e-8
        assert all(f == 20010 or (f < 20010 and r[-1] <= 1e-8) for f, r in zip(res['fes'][str(p)]['JDE21'], rows)), str(p)
    # run_batch, and the B = 1 view twice on one object and on two suites: the batch's computation for the same seed
    ps10, ps30 = problems('bbob', 10), problems('bbob', 30)
    opt = JDE21(copy.deepcopy(cfg))
    for p in (ps10[8], ps10[3], ps30[10]):
        c = copy.deepcopy(cfg)
        if p is ps30[10]:
            opt._config.maxFEs = c.maxFEs = 12000
            opt._config.log_interval = c.log_interval = 240
        np.random.seed(3)
        info = opt.run_episode(p)
        np.random.seed(3)
        seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
        r = JDE21(c).run_batch(p._bound_suite(), [p._suite_index], [seed])
        n = int(r['cost_len'][0].item())
        assert n == 51 and r['cost'].shape[1] >= 51
        assert info['fes'] == int(r['fes'][0].item()) and info['cost'] == [float(v) for v in r['cost'][0, :n].cpu().numpy()]
        assert info['fes'] in (20010, 12010) or info['cost'][-1] <= 1e-8
    torch.cuda.synchronize()
