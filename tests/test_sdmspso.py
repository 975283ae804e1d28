"""sDMS_PSO (src/optimizer/sdms_pso.py), a classic baseline of the test harness: the batched HIP kernels (metabox_amd/csrc/mbx_sdmspso.hpp)
replay the reference's episodes from tests/golden/sdmspso_traces*.npz (tools/gen_golden.py sdmspso) through mbx_set_tape.  The numpy draws
are not stored: SdmsTapeFeeder regenerates them from the seed in the reference's draw order (include/mbx_layout.h §15); the permutations
come from torch's stream and are part of the fixture.

The chain to the reference is closed on the CPU: `Restate`, a numpy restatement of reset / update / epilogue written from the rules in the
header of mbx_sdmspso.hpp, fed the feeder's draws and the reference's recorded costs, reproduces every recorded quantity of every update and
every snapshot exactly.  The GPU tests then hold the kernels to the same records.

Costs enter the algorithm through comparisons only (<, argmin, argmax; the parameter set holds weights), so a whole episode is replayed: the
positions stay bit-identical and the integer bookkeeping exact up to the first proven near-tie (helpers.prove_tie_arrays); there is no
mismatch budget.

No fixture case reaches gbest <= 1e-8 (F1 ends a default episode at 1.8), so "no early stop" is pinned by the horizon instead: every case
ends at the update count of the integer loop, with fes past max_fes."""
import copy
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from helpers import GOLDEN, close, print_ledger, problems, prove_tie_arrays
from oracle import oracle

TR = {}
for _f in sorted(glob.glob(os.path.join(GOLDEN, 'sdmspso_traces*.npz'))):
    with np.load(_f) as _z:
        TR.update({k: _z[k] for k in _z.files})
CASES = [str(c) for c in TR['cases']] if TR else []
NP, M, NS, LP, LA, R = 99, 3, 33, 10, 8, 10
C1 = C2 = 1.49445
ALGO_SDMSPSO = 18
SITE_ELEM_R, SITE_PART, SITE_IWT_U, SITE_IWT_Z, SITE_PERM, SITE_NOISE_A, SITE_NOISE_B = 4, 42, 43, 44, 45, 46, 47
SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_GEN, SC_STEP, SC_MODE, SC_W, SC_NPAR, SC_IWTMODE, SC_RGEN = 0, 1, 2, 3, 4, 6, 10, 11, 12, 13, 14, 15


def tape_stride(D):
    return 2 * NP * D + 4 * NP


def state_doubles(D, nlog):
    return 3 * NP * D + 2 * NP + NS * D + D + 6 * NS + LA + 16 + nlog + 1


def split_state(st, D, nlog=50):
    out, o = {}, 0
    for name, n in (('X', NP * D), ('V', NP * D), ('pbpos', NP * D), ('c_cost', NP), ('pbest', NP), ('lbpos', NS * D), ('gbpos', D), ('lbest_cost', NS),
                    ('lbest_index', NS), ('success_num', NS), ('success_last', NS), ('iwt', NS), ('iwt_z', NS), ('pset', LA), ('scalars', 16),
                    ('cost', nlog + 1)):
        out[name] = st[o:o + n]
        o += n
    assert o == len(st)
    return out


def n_updates(max_fes):
    """run_episode's loop (sdms_pso.py:209-230) on integers -> (updates, local generations)."""
    fes, steps, gens = NP, 0, 0
    while fes < max_fes:
        while fes < 0.95 * max_fes:
            gens, steps, fes = gens + 1, steps + LP, fes + LP * NP
        while fes < max_fes:
            steps, fes = steps + 1, fes + NP
    return steps, gens


class SdmsTapeFeeder:
    """numpy's legacy stream as sDMS_PSO consumes it, laid out as the tape of include/mbx_layout.h §15."""

    def __init__(self, seed, D, noise_kind, rs=None):
        self.rs = rs if rs is not None else np.random.RandomState(seed)
        self.D, self.noise = D, noise_kind

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

    def reset_tape(self, perm):
        D = self.D
        parts = [self.rs.rand(NP, D).ravel(), self.rs.rand(NP, D).ravel(), self._noise_rows(), np.asarray(perm, dtype=np.float64)]   # (:46-50, 88)
        return np.concatenate(parts)

    def step_tape(self, iwt_mode, perm=None):
        t = np.zeros(tape_stride(self.D))
        t[:NP] = self.rs.rand(NP)                                    # rand1 (:136)
        t[NP:2 * NP] = self.rs.rand(NP)                              # rand2 (:137)
        if iwt_mode == 0:
            t[2 * NP:2 * NP + NS] = self.rs.rand(NS)                 # (:130)
        elif iwt_mode == 1:
            t[2 * NP + NS:2 * NP + 2 * NS] = self.rs.standard_normal(NS)       # (:133)
        t[2 * NP + 2 * NS:5 * NP + 2 * NS] = self._noise_rows()      # the evaluation's own draws (:151)
        if perm is not None:
            t[5 * NP + 2 * NS:6 * NP + 2 * NS] = perm
        return t


class Restate:
    """reset / update / epilogue of sDMS_PSO in numpy, from the rules in the header of mbx_sdmspso.hpp.  Costs are handed in."""

    def __init__(self, D, lb, ub, max_fes, log_interval, n_logpoint):
        self.D, self.lb, self.ub, self.max_fes, self.log_interval, self.n_logpoint = D, lb, ub, max_fes, log_interval, n_logpoint
        self.vmax = 0.1 * (ub - lb)

    def _lbest_init(self):
        g = self.pbest.reshape(NS, M)
        idx = np.argmin(g, axis=-1)
        self.lbest_cost = np.min(g, axis=-1)
        self.lbest_index = idx + np.arange(NS) * M
        self.lbpos = self.pbpos[self.lbest_index].copy()

    def reset(self, tape, c_cost_regrouped):
        D, NE = self.D, NP * self.D
        perm = tape[2 * NE + 3 * NP:2 * NE + 4 * NP].astype(int)
        X = (self.lb + (self.ub - self.lb) * tape[:NE]).reshape(NP, D)
        V = (-self.vmax + (self.vmax - (-self.vmax)) * tape[NE:2 * NE]).reshape(NP, D)
        self.X, self.V, self.pbpos = X[perm], V[perm], X[perm].copy()
        self.c_cost = np.array(c_cost_regrouped)
        self.pbest = self.c_cost.copy()
        self.gbest = float(np.min(self.c_cost))
        self.gbpos = self.X[int(np.argmin(self.c_cost))].copy()
        self._lbest_init()
        self.success = np.zeros(NS)
        self.success_last = np.zeros(NS)
        self.iwt = np.zeros(NS)
        self.pset = []
        self.fes, self.log_index, self.cost, self.done = NP, 1, [self.gbest], False
        self.w, self.mode, self.sip, self.gen, self.iwt_mode = 0.9, 0, 0, 0, 0

    def begin(self):
        """What an update decides before it draws: the phase (at a generation boundary only) and how iwt is drawn."""
        if self.mode == 0 and self.sip == 0:
            if self.fes < 0.95 * self.max_fes:
                self.gen += 1
                self.w -= 0.5 / (self.max_fes / NP)
            else:
                self.mode = 1
        if self.mode == 1:
            self.iwt_mode = 2
        else:
            self.iwt_mode = 0 if len(self.pset) < LA or np.sum(self.success) <= LP else 1
        return self.iwt_mode

    def regroup_due(self):
        return self.mode == 0 and self.sip + 1 == LP and self.gen % R == 0

    def move(self, tape):
        """-> the new positions; to be evaluated by the caller."""
        r1, r2 = tape[:NP, None], tape[NP:2 * NP, None]
        grp = np.arange(NP) // M
        vp = r1 * (self.pbpos - self.X)
        if self.mode == 0:
            if self.iwt_mode == 0:
                self.iwt = 0.5 * tape[2 * NP:2 * NP + NS] + 0.4
            else:
                s = np.sort(np.array(self.pset))
                self.iwt = (s[3] + s[4]) / 2 + 0.1 * tape[2 * NP + NS:2 * NP + 2 * NS]
            v = self.iwt[grp][:, None] * self.V + C1 * vp + C2 * (r2 * (self.lbpos[grp] - self.X))
        else:
            v = self.w * self.V + C1 * vp + C2 * (r2 * (self.gbpos[None, :] - self.X))
        self.V = np.minimum(np.maximum(v, -self.vmax), self.vmax)
        self.X = np.minimum(np.maximum(self.X + self.V, self.lb), self.ub)
        return self.X

    def finish(self, tape, new_cost):
        new_cost = np.asarray(new_cost, dtype=np.float64)
        impr = new_cost < self.pbest
        self.pbpos = np.where(impr[:, None], self.X, self.pbpos)
        self.pbest = np.where(impr, new_cost, self.pbest)
        self.c_cost = new_cost.copy()
        cb = int(np.argmin(new_cost))
        if new_cost[cb] < self.gbest:
            self.gbest, self.gbpos = float(new_cost[cb]), self.X[cb].copy()
        self.fes += NP
        if self.fes >= self.log_index * self.log_interval:           # once, not "while"
            self.log_index += 1
            self.cost.append(self.gbest)
        period_end = self.mode == 0 and self.sip + 1 == LP
        if self.mode == 0:
            g = self.pbest.reshape(NS, M)
            self.success = self.success + np.sum(g < self.lbest_cost[:, None], axis=-1)     # against the OLD lbest_cost
            cur, idx = np.min(g, axis=-1), np.argmin(g, axis=-1)
            better = cur < self.lbest_cost
            self.lbest_index = np.where(better, idx + np.arange(NS) * M, self.lbest_index)
            self.lbpos = np.where(better[:, None], self.pbpos[idx + np.arange(NS) * M], self.lbpos)
            self.lbest_cost = np.where(better, cur, self.lbest_cost)
            if period_end:
                self.pset.append(self.iwt[int(np.argmax(self.success))])
                self.pset = self.pset[-LA:]
                self.success_last, self.success = self.success, np.zeros(NS)
                if self.gen % R == 0:
                    perm = tape[5 * NP + 2 * NS:6 * NP + 2 * NS].astype(int)
                    self.X, self.c_cost, self.pbpos, self.pbest, self.V = self.X[perm], self.c_cost[perm], self.pbpos[perm], self.pbest[perm], self.V[perm]
                    self._lbest_init()
            self.sip = (self.sip + 1) % LP
        if self.fes >= self.max_fes and (self.mode == 1 or period_end):
            self.done = True
            if len(self.cost) >= self.n_logpoint + 1:
                self.cost[-1] = self.gbest
            else:
                self.cost.append(self.gbest)


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
    suite, dim, fid, seed = case.split('/')
    p, nk = _problem(suite, dim, fid)
    return p, nk, int(dim), int(seed), int(TR[f'{case}/max_fes']), int(TR[f'{case}/log_interval']), int(TR[f'{case}/n_logpoint'])


class Walker:
    """Walks a fixture case update by update: hands out the tape of each launch (reset first) and the reference's records after it."""

    def __init__(self, case):
        self.case = case
        self.p, self.nk, self.D, self.seed, self.max_fes, self.log_interval, self.nlog = _case(case)
        self.rs = np.random.RandomState(self.seed)
        self.fd = SdmsTapeFeeder(self.seed, self.D, self.nk, self.rs)
        self.want = {k: TR[f'{case}/{k}'] for k in ('gbest', 'fes', 'pbest', 'lbest_cost', 'lbest_index', 'success_num', 'iwt', 'iwt_mode', 'c_cost',
                                                    'gen_parameter_set', 'gen_w', 'gen_success_end', 'perms', 'snaps', 'snap_at', 'cost')}
        self.U = len(self.want['gbest']) - 1
        self.n_perm = 0

    def next_perm(self):
        self.n_perm += 1
        return self.want['perms'][self.n_perm - 1]

    def reset_tape(self):
        t = np.zeros(tape_stride(self.D))
        r = self.fd.reset_tape(self.next_perm())
        t[:len(r)] = r
        return t

    def step_tape(self, u, regroup):
        return self.fd.step_tape(int(self.want['iwt_mode'][u]), self.next_perm() if regroup else None)

    def snapshot(self, u):
        at = np.nonzero(self.want['snap_at'] == u)[0]
        return self.want['snaps'][at[0]] if len(at) else None


# ------------------------------------------------------------------------------------------------ CPU
def test_sdms_pso_is_exported_and_picked_up_by_the_tester(tmp_path):
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import sDMS_PSO
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--test', '--t_optimizer_for_cp', 'sDMS_PSO', '--log_dir', str(tmp_path / 'out')])
    t = Tester(cfg)
    assert 'sDMS_PSO' in [type(o).__name__ for o in t.t_optimizer_for_cp] and 'sDMS_PSO' not in t.skipped
    assert isinstance(sDMS_PSO(copy.deepcopy(cfg)), sDMS_PSO)
    assert all('sDMS_PSO' in t.test_results['cost'][str(p)] for p in t.test_set.data)


def _first_rejected_max_fes():
    m = NP + 1
    while n_updates(m)[1] < 100:                                     # coarse, then exact: the generation count is monotone in max_fes
        m += 1000
    while n_updates(m - 1)[1] >= 100:
        m -= 1
    return m


def test_abi_geometry_of_sdmspso():
    from metabox_amd import _abi
    lib = _abi.load_lib()
    assert _abi.ALGO_SDMSPSO == ALGO_SDMSPSO
    for D in (10, 12, 30, 40):
        cfg = oracle.make_cfg(ALGO_SDMSPSO, NP, D, 2000 * D, 40 * D, 50)
        assert lib.mbx_tape_stride(C.byref(cfg)) == tape_stride(D)
        assert lib.mbx_state_dim(C.byref(cfg)) == 1
        assert lib.mbx_action_dim(C.byref(cfg)) == 0
    ok = lambda **kw: lib.mbx_state_dim(C.byref(oracle.make_cfg(ALGO_SDMSPSO, kw.get('np_', NP), kw.get('dim', 10), kw.get('max_fes', 20000), 400, 50)))   # noqa: E731
    assert ok() == 1
    assert ok(np_=100) < 0 and ok(np_=96) < 0 and ok(dim=41) < 0 and ok(max_fes=99) < 0 and ok(max_fes=100) == 1
    m = _first_rejected_max_fes()
    assert n_updates(m)[1] == 100 and n_updates(m - 1)[1] == 99
    assert ok(max_fes=m) < 0 and ok(max_fes=m - 1) == 1 and ok(max_fes=10 * m) < 0
    lib.mbx_last_error.restype = C.c_char_p
    ok(max_fes=m)
    assert b'quasi-Newton' in lib.mbx_last_error()
    assert lib.mbx_state_dim(C.byref(oracle.make_cfg(17, NP, 10, 20000, 400, 50))) < 0      # 17 stays unassigned


def test_n_steps_equals_the_fixture():
    from metabox_amd.optimizer import sDMS_PSO
    for case in CASES:
        max_fes = int(TR[f'{case}/max_fes'])
        U = len(TR[f'{case}/gbest']) - 1
        assert n_updates(max_fes)[0] == U and sDMS_PSO.n_updates(max_fes) == n_updates(max_fes), case
        assert TR[f'{case}/fes'][-1] == NP * (U + 1)


@pytest.mark.parametrize('case', CASES)
def test_feeder_consumes_the_reference_stream(case):
    """Over the whole fixture episode the feeder draws exactly what the reference drew: the next np.random.rand() after the episode is the
    one the generator recorded.  The iwt branch comes from the recorded iwt_mode."""
    wk = Walker(case)
    wk.reset_tape()
    for u in range(1, wk.U + 1):
        wk.step_tape(u, False)
    assert wk.rs.rand() == float(TR[f'{case}/next_rand']), case


@pytest.mark.parametrize('case', CASES)
def test_numpy_restatement_reproduces_the_reference(case):
    """The rules as the kernel header states them, in numpy, on the feeder's draws and the reference's costs: every recorded quantity of
    every update and every snapshot, exactly."""
    wk = Walker(case)
    w = wk.want
    rs = Restate(wk.D, wk.p.lb, wk.p.ub, wk.max_fes, wk.log_interval, wk.nlog)
    rs.reset(wk.reset_tape(), w['c_cost'][0])
    gens = 0
    for u in range(wk.U + 1):
        if u > 0:
            assert not rs.done, (case, u)
            assert rs.begin() == w['iwt_mode'][u], (case, u)
            regroup = rs.regroup_due()
            tape = wk.step_tape(u, regroup)
            rs.move(tape)
            period_end = rs.mode == 0 and rs.sip + 1 == LP
            rs.finish(tape, w['c_cost'][u])                        # (the record holds the new costs in evaluation order, before any regroup)
            if period_end:
                gens += 1
                ps = w['gen_parameter_set'][gens - 1]
                assert np.array_equal(rs.pset, ps[:len(rs.pset)]) and np.all(np.isnan(ps[len(rs.pset):])), (case, u)
                assert rs.w == w['gen_w'][gens - 1] and rs.gen == gens, (case, u)
                assert np.array_equal(rs.success_last, w['gen_success_end'][gens - 1]) and not rs.success.any(), (case, u)
                assert np.array_equal(rs.success_last, w['success_num'][u]), (case, u)
            else:
                assert np.array_equal(rs.success, w['success_num'][u]) or rs.mode == 1, (case, u)
            assert np.array_equal(rs.iwt, w['iwt'][u]), (case, u)
        assert rs.gbest == w['gbest'][u] and rs.fes == w['fes'][u], (case, u)
        assert np.array_equal(rs.pbest, w['pbest'][u]) and np.array_equal(rs.lbest_cost, w['lbest_cost'][u]), (case, u)
        assert np.array_equal(rs.lbest_index, w['lbest_index'][u]), (case, u)
        assert np.array_equal(rs.lbpos, rs.pbpos[rs.lbest_index]) or rs.mode == 1, (case, u)
        snap = wk.snapshot(u)
        if snap is not None:
            assert np.array_equal(rs.X, snap[0]) and np.array_equal(rs.V, snap[1]) and np.array_equal(rs.pbpos, snap[2]), (case, u)
    assert rs.done and wk.n_perm == len(w['perms']) and gens == len(w['gen_w'])
    assert np.array_equal(rs.cost, w['cost'])


def test_fixture_covers_the_quirks():
    """The fixture exercises what it is meant to pin."""
    modes = np.concatenate([TR[f'{c}/iwt_mode'][1:] for c in CASES])
    assert {0, 1, 2} <= set(modes.tolist())
    for c in CASES:
        if int(TR[f'{c}/max_fes']) == 10000:
            assert (TR[f'{c}/iwt_mode'] == 1).any() and len(TR[f'{c}/perms']) == 2 and len(TR[f'{c}/gbest']) == 102 and TR[f'{c}/fes'][-1] == 10098, c
    assert any(len(TR[f'{c}/perms']) > 1 for c in CASES)                               # a regroup after the reset's
    ties = 0
    for c in CASES:
        s = TR[f'{c}/gen_success_end']
        ties += int(np.sum(np.sum(s == s.max(axis=1, keepdims=True), axis=1) > 1))
    assert ties > 0                                                                    # arg-max of success_num on an exact tie
    assert all(TR[f'{c}/fes'][-1] > TR[f'{c}/max_fes'] for c in CASES)
    short = [c for c in CASES if int(TR[f'{c}/max_fes']) == 2000]
    assert len(short) == 1 and len(TR[f'{short[0]}/cost']) == 22 and int(TR[f'{short[0]}/log_interval']) == 40
    assert {_problem(*c.split('/')[:3])[1] for c in CASES if c.startswith('bbob-noisy')} == {1, 2, 3}
    prot = [c for c in CASES if c.startswith('protein')]
    assert len(prot) == 1 and not (TR[f'{prot[0]}/iwt_mode'] == 2).any() and len(TR[f'{prot[0]}/gen_w']) == 1
    assert {c.split('/')[1] for c in CASES} >= {'10', '30'} and sum(int(TR[f'{c}/max_fes']) == 20000 for c in CASES) == 2


# ------------------------------------------------------------------------------------------------ GPU
def _unpermute(v, perm):
    out = np.empty_like(v)
    out[perm] = v
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_sdmspso_tape_replay_matches_reference(case):
    import torch
    from metabox_amd.suite import Batch, Suite
    wk = Walker(case)
    w, D = wk.want, wk.D
    b = Batch(Suite([wk.p]), ALGO_SDMSPSO, [0], [wk.seed], NP, wk.max_fes, wk.log_interval, wk.nlog)
    assert (b.state_dim, b.action_dim, b.tape_stride) == (1, 0, tape_stride(D))
    mirror = Restate(D, wk.p.lb, wk.p.ub, wk.max_fes, wk.log_interval, wk.nlog)       # only its phase bookkeeping is used: when a regroup is due
    tape0 = wk.reset_tape()
    mirror.reset(tape0, w['c_cost'][0])
    ledger, diverged, gens = [], False, 0
    prev = None
    for u in range(wk.U + 1):
        regroup = period_end = False
        if u == 0:
            tape = tape0
        else:
            mirror.begin()
            regroup = mirror.regroup_due()
            period_end = mirror.mode == 0 and mirror.sip + 1 == LP
            tape = wk.step_tape(u, regroup)
            mirror.move(tape)
            mirror.finish(tape, w['c_cost'][u])
        b.set_tape(torch.from_numpy(tape[None]).cuda())
        if u == 0:
            b.reset()
        else:
            _, _, d = b.step(None)
        st = split_state(b.read_state(0), D, wk.nlog)
        sc = st['scalars']
        assert sc[SC_FES] == w['fes'][u], (case, u)
        if u > 0:
            assert sc[SC_DONE] == (1. if u == wk.U else 0.) and int(d[0].item()) == int(u == wk.U), (case, u)
            perm = tape[5 * NP + 2 * NS:6 * NP + 2 * NS].astype(int) if regroup else np.arange(NP)
            succ = st['success_last'] if period_end else st['success_num']
            if not diverged:
                # the first update whose improved mask or success count differs must sit on a proven near-tie; float tolerances only afterwards
                ref_pb, cur_pb = _unpermute(w['pbest'][u], perm), _unpermute(st['pbest'], perm)
                cur_cc = _unpermute(st['c_cost'], perm)
                ref_i = (ref_pb != w['pbest'][u - 1]).astype(np.float64)
                cur_i = (cur_pb != prev['pbest']).astype(np.float64)
                ok = prove_tie_arrays(w['pbest'][u - 1], w['c_cost'][u], ref_i, prev['pbest'], cur_cc, cur_i, ledger, 'pbest', case, u)
                if mirror.mode == 0:
                    grp = np.arange(NP) // M
                    ref_s = (ref_pb < w['lbest_cost'][u - 1][grp]).astype(np.float64)
                    cur_s = (cur_pb < prev['lbest_cost'][grp]).astype(np.float64)
                    ok = prove_tie_arrays(w['lbest_cost'][u - 1][grp], ref_pb, ref_s, prev['lbest_cost'][grp], cur_pb, cur_s, ledger, 'success', case, u) and ok
                    ok = ok and np.array_equal(succ, w['success_num'][u])
                diverged = not ok
        if not diverged:
            assert close(st['pbest'], w['pbest'][u]) and close(st['lbest_cost'], w['lbest_cost'][u]), (case, u)
            assert np.array_equal(st['lbest_index'], w['lbest_index'][u]), (case, u)
            assert np.array_equal(st['lbpos'], st['pbpos'].reshape(NP, D)[st['lbest_index'].astype(int)].ravel()) or sc[SC_MODE] == 1, (case, u)
            if u > 0:
                assert sc[SC_IWTMODE] == w['iwt_mode'][u] and sc[SC_MODE] == float(w['iwt_mode'][u] == 2), (case, u)
                assert np.array_equal(st['iwt'], w['iwt'][u]), (case, u)
                assert sc[SC_RGEN] == mirror.gen and sc[SC_W] == mirror.w and sc[SC_STEP] == mirror.sip and sc[SC_GEN] == u, (case, u)
                if mirror.mode == 0:
                    assert np.array_equal(st['success_last'] if period_end else st['success_num'], w['success_num'][u]), (case, u)
                    assert not period_end or not st['success_num'].any(), (case, u)
                if period_end:
                    gens += 1
                    n = int(sc[SC_NPAR])
                    ps = w['gen_parameter_set'][gens - 1]
                    assert n == min(gens, LA) and np.array_equal(st['pset'][:n], ps[:n]) and sc[SC_W] == w['gen_w'][gens - 1], (case, u)
            snap = wk.snapshot(u)
            if snap is not None:
                assert np.array_equal(st['X'], snap[0].ravel()), (case, u, 'position')
                assert np.array_equal(st['V'], snap[1].ravel()), (case, u, 'velocity')
                assert np.array_equal(st['pbpos'], snap[2].ravel()), (case, u, 'pbest position')
        assert close(sc[SC_GBEST], w['gbest'][u]), (case, u, sc[SC_GBEST], w['gbest'][u])
        prev = st
    res = b.results()
    n = int(res['cost_len'][0].item())
    assert n == len(w['cost']) and close(res['cost'][0, :n].cpu().numpy(), w['cost']), (case, n, len(w['cost']))
    assert res['fes'][0].item() == w['fes'][-1] and wk.n_perm == len(w['perms'])
    print_ledger(ledger)
    b.close()


def _u53(w0, w1):
    return ((w0 >> 5) * 67108864.0 + (w1 >> 6)) / 9007199254740992.0


def philox_tape(seed, D, noise_kind, gen, iwt_z=None, episode=0):
    """The tape that reproduces the Philox stream of (seed, gen, episode) under the site map of include/mbx_layout.h §15.  iwt_z: the normals
    of the Philox run's own state block (the device's log / cos are not reproduced on the host)."""
    NE = NP * D
    t = np.zeros(tape_stride(D))

    def ph(idx, site):
        return oracle.philox(seed, idx, site, gen, episode)

    def noise(o):
        for i in range(NP):
            w = ph(i, SITE_NOISE_A)
            if noise_kind == 2:
                t[o + i], t[o + NP + i] = _u53(w[0], w[1]), _u53(w[2], w[3])
            else:
                assert noise_kind == 0, 'only the noise kinds whose draws are exact uniforms are rebuilt here'
    keys = np.array([ph(i, SITE_PERM)[0] for i in range(NP)], dtype=np.int64)
    perm = np.empty(NP)
    perm[np.lexsort((np.arange(NP), keys))] = np.arange(NP)            # perm[i] = rank of key i, the lower index first among equal keys
    if gen == 0:
        for e in range(NE):
            w = ph(e, SITE_ELEM_R)
            t[e], t[NE + e] = _u53(w[0], w[1]), _u53(w[2], w[3])
        noise(2 * NE)
        t[2 * NE + 3 * NP:2 * NE + 4 * NP] = perm
    else:
        for i in range(NP):
            w = ph(i, SITE_PART)
            t[i], t[NP + i] = _u53(w[0], w[1]), _u53(w[2], w[3])
        for s in range(NS):
            w = ph(s, SITE_IWT_U)
            t[2 * NP + s] = _u53(w[0], w[1])
        if iwt_z is not None:
            t[2 * NP + NS:2 * NP + 2 * NS] = iwt_z
        noise(2 * NP + 2 * NS)
        t[5 * NP + 2 * NS:6 * NP + 2 * NS] = perm
    return t


def _force_generation(b, k, D, gen, pset=None, nlog=50):
    """Write the reference's `gen` (and optionally a full parameter set) into instance k: the next generation is gen + 1."""
    blk = b.read_state(k)
    st = split_state(blk, D, nlog)                                    # views into blk
    st['scalars'][SC_RGEN] = gen
    if pset is not None:
        st['pset'][:] = pset
        st['scalars'][SC_NPAR] = LA
    b.write_state(k, blk)


@pytest.mark.gpu
def test_hip_sdmspso_philox_equals_tape():
    """The Philox path and the tape path are the same computation: a tape rebuilt on the host from oracle.philox with the documented site
    map gives bit-identical state blocks, on a noiseless and a uniform-noise problem, over the reset and 21 updates that include the
    normal-draw mode, a regroup (generation 10 is forced by writing gen = 9 and a full parameter set after the reset) and the step after it."""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    ids = [15, 102]
    s = Suite([ps[i] for i in ids])
    seeds = np.array([123456789012345, 987654321], dtype=np.uint64)
    a = Batch(s, ALGO_SDMSPSO, np.arange(2), seeds, NP, 20000, 400, 50)
    t = Batch(s, ALGO_SDMSPSO, np.arange(2), seeds, NP, 20000, 400, 50)
    pset = np.array([0.52, 0.81, 0.47, 0.66, 0.73, 0.58, 0.44, 0.69])
    seen, regrouped = set(), False
    for g in range(22):
        if g == 0:
            a.reset()
        else:
            a.step(None)
        torch.cuda.synchronize()
        sa = [a.read_state(k) for k in range(2)]
        tape = np.stack([philox_tape(int(seeds[k]), 10, ps[ids[k]].noise[0], g, split_state(sa[k], 10)['iwt_z']) for k in range(2)])
        t.set_tape(torch.from_numpy(tape).cuda())
        if g == 0:
            t.reset()
        else:
            t.step(None)
        torch.cuda.synchronize()
        for k in range(2):
            st = t.read_state(k)
            assert np.array_equal(sa[k], st), (ids[k], g, int(np.argmax(sa[k] != st)))
            sp = split_state(sa[k], 10)
            seen.add(int(sp['scalars'][SC_IWTMODE]))
            if g == 10:
                assert sp['scalars'][SC_RGEN] == 10 and sp['scalars'][SC_STEP] == 0 and sp['scalars'][SC_NPAR] == LA
                assert np.array_equal(np.sort(tape[k, 5 * NP + 2 * NS:6 * NP + 2 * NS]), np.arange(NP))
                regrouped = True
            if g == 0:
                _force_generation(a, k, 10, 9, pset)
                _force_generation(t, k, 10, 9, pset)
    ra, rt = a.results(), t.results()
    for key in ('cost', 'fes', 'cost_len'):
        assert torch.equal(ra[key], rt[key]), key
    assert regrouped and {0, 1} <= seen                              # both iwt sites were exercised
    a.close(); t.close()


def _invariance(ps, ids, dim, n_split, G, max_fes):
    import torch
    from metabox_amd.suite import Batch, Suite
    s = Suite([ps[i] for i in ids])
    B = len(ids)
    pidx = np.arange(B, dtype=np.int32)
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 3
    mk = lambda sel: Batch(s, ALGO_SDMSPSO, pidx[sel], seeds[sel], NP, max_fes, max_fes // 50, 50, early_stop=bool(len(sel) % 2))   # noqa: E731
    full = mk(np.arange(B))
    perm = np.random.RandomState(5).permutation(B)
    parts = [mk(perm[:n_split]), mk(perm[n_split:])]
    where = {int(perm[j]): (0, j) if j < n_split else (1, j - n_split) for j in range(B)}
    st0 = full.reset().clone()
    for pb in parts:
        pb.reset()
    assert torch.allclose(st0[:, 0].cpu(), torch.full((B,), NP / max_fes, dtype=torch.float64))
    for k in range(B):                                               # the next generation is the tenth: the launch of update 10 regroups
        _force_generation(full, k, dim, 9)
        _force_generation(parts[where[k][0]], where[k][1], dim, 9)
    frozen = {}
    for g in range(1, G + 1):
        _, _, d = full.step(None)
        for pb in parts:
            pb.step(None)
        torch.cuda.synchronize()
        for k in range(B):
            blk = full.read_state(k)
            pb, j = where[k]
            assert np.array_equal(blk, parts[pb].read_state(j)), (ids[k], g)     # (the parts differ in early_stop too: it has no effect)
            sc = split_state(blk, dim)['scalars']
            if k in frozen:
                assert np.array_equal(blk, frozen[k]), (ids[k], g)               # done instances are left untouched
                assert d[k].item() == 1
            else:
                assert sc[SC_FES] == NP * (g + 1), (ids[k], g)
                assert sc[SC_DONE] == float(g == n_updates(max_fes)[0]), (ids[k], g)
                if sc[SC_DONE] == 1.:
                    frozen[k] = blk.copy()
    assert len(frozen) == B
    ra = full.results()
    for pb, idx in ((0, perm[:n_split]), (1, perm[n_split:])):
        rp = parts[pb].results()
        assert torch.equal(ra['cost'][torch.as_tensor(idx).cuda()], rp['cost']) and torch.equal(ra['fes'][torch.as_tensor(idx).cuda()], rp['fes'])
    full.close()
    for pb in parts:
        pb.close()


@pytest.mark.gpu
def test_hip_sdmspso_batch_invariance_and_frozen_done_instances():
    """Eight mixed problems: the full batch against a 3 + 5 split in permuted order, bit for bit, through a regroup, the global phase and
    the end of the episode (max_fes 2000: 20 updates; 2150: 20 local + 1 global); done instances stay frozen."""
    ps = {**problems('bbob', 10), **problems('bbob-noisy', 10)}
    _invariance(ps, [1, 5, 8, 15, 20, 24, 103, 117], 10, 3, 22, 2000)
    assert n_updates(2000) == (20, 2) and n_updates(2150) == (21, 2)
    _invariance(ps, [3, 10, 16, 101, 102], 10, 2, 23, 2150)


@pytest.mark.gpu
def test_hip_sdmspso_batch_invariance_at_dim_40():
    """The largest LDS shape."""
    _invariance(problems('bbob', 40), [2, 10, 21], 40, 1, 21, 2000)


@pytest.mark.gpu
def test_hip_sdmspso_regroup_is_a_permutation():
    """Two batches on the Philox route that differ only in the generation number written after the reset: in one the launch of update 10
    ends generation 10 and regroups, in the other it ends generation 9 and does not.  The regrouped swarm is the other one with its rows
    permuted -- position, velocity, pbest position, c_cost and pbest of a particle move together -- and lbest is found afresh."""
    import torch
    from metabox_amd.suite import Batch, Suite
    for dim, ids in ((10, [8, 21]), (30, [15])):
        ps = problems('bbob', dim)
        s = Suite([ps[i] for i in ids])
        B = len(ids)
        seeds = np.arange(B, dtype=np.uint64) + 77
        a = Batch(s, ALGO_SDMSPSO, np.arange(B), seeds, NP, 20000, 400, 50)
        c = Batch(s, ALGO_SDMSPSO, np.arange(B), seeds, NP, 20000, 400, 50)
        a.reset(); c.reset()
        for k in range(B):
            _force_generation(a, k, dim, 9)
            _force_generation(c, k, dim, 8)
        for g in range(10):
            a.step(None); c.step(None)
        torch.cuda.synchronize()
        for k in range(B):
            sa, sc_ = split_state(a.read_state(k), dim), split_state(c.read_state(k), dim)
            rows = lambda st: np.column_stack([st['pbest'], st['c_cost'], st['pbpos'].reshape(NP, dim), st['V'].reshape(NP, dim), st['X'].reshape(NP, dim)])   # noqa: E731
            ra, rc = rows(sa), rows(sc_)
            assert not np.array_equal(ra, rc)                                        # rows did move
            order = lambda r: r[np.lexsort(r.T[::-1])]                               # noqa: E731
            assert np.array_equal(order(ra), order(rc)), (dim, ids[k])               # ... together
            g3 = sa['pbest'].reshape(NS, M)
            assert np.array_equal(sa['lbest_cost'], g3.min(axis=1)) and np.array_equal(sa['lbest_index'], g3.argmin(axis=1) + M * np.arange(NS))
            assert np.array_equal(sa['lbpos'], sa['pbpos'].reshape(NP, dim)[sa['lbest_index'].astype(int)].ravel())
            assert sa['scalars'][SC_RGEN] == 10 and sc_['scalars'][SC_RGEN] == 9
            for name in ('gbpos', 'iwt', 'pset', 'success_last', 'cost'):            # everything the regroup leaves alone
                assert np.array_equal(sa[name], sc_[name]), name
            assert sa['scalars'][SC_GBEST] == sc_['scalars'][SC_GBEST]
        a.close(); c.close()


@pytest.mark.gpu
def test_sdmspso_in_the_tester_and_the_b1_view(tmp_path):
    import pickle
    import torch
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import sDMS_PSO
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda', '--test', '--t_optimizer_for_cp', 'sDMS_PSO',
                      '--log_dir', str(tmp_path / 'out'), '--test_runs', '2'])
    cfg.maxFEs = 2000
    cfg.log_interval = cfg.maxFEs // cfg.n_logpoint
    cfg.t_optimizer_for_cp = ['sDMS_PSO']
    t = Tester(cfg)
    t.test()
    with open(t.log_dir + 'test.pkl', 'rb') as f:
        res = pickle.load(f)
    for p in t.test_set.data:
        rows = res['cost'][str(p)]['sDMS_PSO']
        assert len(rows) == 2 and all(len(r) == 51 for r in rows), str(p)
        assert all(np.all(np.diff(r) <= 0) for r in rows) and all(f == 2079 for f in res['fes'][str(p)]['sDMS_PSO'])
    # the B = 1 view is the batch's computation for the same seed
    ps = problems('bbob', 10)
    opt = sDMS_PSO(copy.deepcopy(cfg))
    np.random.seed(3)
    info = opt.run_episode(ps[8])
    np.random.seed(3)
    seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
    s = ps[8]._bound_suite()
    r = sDMS_PSO(copy.deepcopy(cfg)).run_batch(s, [ps[8]._suite_index], [seed])
    n = int(r['cost_len'][0].item())
    assert info['fes'] == int(r['fes'][0].item()) == 2079 and info['cost'] == [float(v) for v in r['cost'][0, :n].cpu().numpy()]
    torch.cuda.synchronize()
