"""SAHLPSO (src/optimizer/sahlpso.py), a classic baseline of the test harness: the batched HIP kernels (metabox_amd/csrc/mbx_sahlpso.hpp)
replay the reference's episodes from tests/golden/sahlpso_traces*.npz (tools/gen_golden.py sahlpso) through mbx_set_tape.  The numpy draws
are not stored: SahlTapeFeeder regenerates them from the seed in the reference's call order (include/mbx_layout.h section 17), the legacy gauss
cache shared between the noise models and standard_cauchy included, because it calls the same RandomState methods in the same order.

The chain to the reference is closed on the CPU: `Restate`, a numpy restatement of reset / move / end of generation written from the rules in
the header of mbx_sahlpso.hpp, fed the feeder's draws and the reference's recorded costs, reproduces every recorded quantity of every move
and generation and every snapshot exactly.  The GPU tests then hold the kernels to Restate on the same draws, launch by launch.

Costs enter the algorithm through comparisons only (success, the gBest update, the exemplar of an exploration particle), so a whole episode
is replayed: positions, velocities, pBest rows, w and the selection probabilities stay bit-identical and the integer bookkeeping exact up to
the first proven near-tie (helpers.prove_tie_arrays); there is no mismatch budget.

Fixture coverage (asserted by the generator and again here): an early stop in the middle of a pass, a budget that ends in the middle of a
pass, a stale gBest_cost, a pBest row changed by the crossover of a failed move, 36 population reductions.  NOT covered by a fixture: a
P_cr with a zero entry -- none of 156 reference episodes tried has one (ns_cr is cumulative and a move succeeds against the particle's
INITIAL cost); that clause was dropped from the generator and is pinned on a crafted state instead, next to the one deliberate departure
(sum(S_cr) == 0 keeps H_cr = 5 and makes P_cr uniform), which no fixture may reach."""
import copy
import ctypes as C
import glob
import os

import numpy as np
import pytest

from helpers import GOLDEN, close, print_ledger, problems, prove_tie_arrays
from oracle import oracle

TR = {}
for _f in sorted(glob.glob(os.path.join(GOLDEN, 'sahlpso_traces*.npz'))):
    with np.load(_f) as _z:
        TR.update({k: _z[k] for k in _z.files})
CASES = [str(c) for c in TR['cases']] if TR else []
NP0, NSEL, HCR, HLS, LP = 40, 8, 5, 15, 5
M_CR = [0.0001, 0.0005, 0.001, 0.005, 0.01, 0.05, 0.1, 0.5]
C1 = 1.49445
ALGO_SAHLPSO = 20
R_UCR, R_ULS, R_M, R_N, R_PICK, R_RND2, R_CAUCHY, R_NOISE, R_CROSS = 0, 1, 2, 3, 4, 5, 6, 7, 10
SITE_ELEM_R, SITE_CHOICE, SITE_PICK, SITE_ELEM, SITE_VEL, SITE_FAIL, SITE_NOISE_A, SITE_NOISE_B, SITE_PERM = 4, 54, 55, 56, 57, 58, 59, 60, 61
SC_GBEST, SC_FES, SC_LOG_INDEX, SC_COST_LEN, SC_DONE, SC_GEN, SC_NP, SC_GROW, SC_MOVES = 0, 1, 2, 3, 4, 6, 10, 11, 12


def rec_len(D):
    return 10 + 3 * D


def tape_stride(D):
    return NP0 * rec_len(D)


def state_doubles(D, nlog):
    return 3 * NP0 * D + 4 * NP0 + 8 + 3 * 8 + 3 * 16 + 5 * NP0 + 16 + nlog + 1


def split_state(st, D, nlog=50):
    out, o = {}, 0
    for name, n in (('X', NP0 * D), ('V', NP0 * D), ('pbpos', NP0 * D), ('fX', NP0), ('pbcost0', NP0), ('w', NP0), ('rank', NP0), ('sel', 8),
                    ('P_cr', 8), ('nf_cr', 8), ('ns_cr', 8), ('P_ls', 16), ('nf_ls', 16), ('ns_ls', 16), ('move_i', NP0), ('move_cr', NP0),
                    ('move_ls', NP0), ('move_succ', NP0), ('move_cauchy', NP0), ('scalars', 16), ('cost', nlog + 1)):
        out[name] = st[o:o + n]
        o += n
    assert o == len(st) == state_doubles(D, nlog)
    return out


def n_generations(max_fes):
    """The reference's outer loop (:48-155) on integers for an episode that runs to its budget -> passes, the cut-short last one included."""
    fes, NP, gens = NP0, NP0, 0
    while fes < max_fes and NP >= 4:
        gens += 1
        fes += NP
        if fes >= max_fes:
            break
        NP_ = round((4 - NP0) * fes / max_fes + NP0)
        if NP_ < NP:
            NP = NP_
    return gens


class SahlTapeFeeder:
    """numpy's legacy stream as SAHLPSO consumes it, laid out as the tape of include/mbx_layout.h section 17."""

    def __init__(self, seed, D, noise_kind, rs=None):
        self.rs = rs if rs is not None else np.random.RandomState(seed)
        self.D, self.noise = D, noise_kind

    def _noise(self, n):
        rows, rs = np.zeros((3, n)), self.rs
        if self.noise == 1:
            rows[0] = rs.randn(n) if n > 1 else rs.randn()
        elif self.noise == 2:
            rows[0] = rs.rand(n) if n > 1 else rs.rand()
            rows[1] = rs.rand(n) if n > 1 else rs.rand()
        elif self.noise == 3:
            rows[0] = rs.rand(n) if n > 1 else rs.rand()
            rows[1] = rs.randn(n) if n > 1 else rs.randn()
            rows[2] = rs.randn(n) if n > 1 else rs.randn()
        return rows

    def reset_tape(self):
        D = self.D
        t = np.zeros(tape_stride(D))
        t[:NP0 * D] = self.rs.rand(NP0, D).ravel()                   # V (:23)
        t[NP0 * D:2 * NP0 * D] = self.rs.rand(NP0, D).ravel()        # X (:24)
        t[2 * NP0 * D:2 * NP0 * D + 3 * NP0] = self._noise(NP0).ravel()
        t[2 * NP0 * D + 3 * NP0:2 * NP0 * D + 3 * NP0 + NSEL] = self.rs.permutation(np.arange(NP0))[:NSEL]     # :47
        return t

    def move_head(self, adapt, sel, remain, best_p):
        """The draws of a move up to its evaluation (:54-91) -> the slot's record."""
        D, rs = self.D, self.rs
        r = np.zeros(rec_len(D))
        if adapt:
            r[R_UCR] = rs.random_sample()                            # np.random.choice(range(H), p=P): one uniform each
            r[R_ULS] = rs.random_sample()
        if sel:
            r[R_M], r[R_N] = rs.choice(remain, 2)
        else:
            r[R_PICK] = rs.choice(best_p)
        r[R_CROSS:R_CROSS + D] = rs.rand(D)
        if not sel:
            r[R_CROSS + D:R_CROSS + 2 * D] = rs.rand(D)
        r[R_CROSS + 2 * D:R_CROSS + 3 * D] = rs.rand(D)
        r[R_NOISE:R_NOISE + 3] = self._noise(1)[:, 0]
        return r

    def move_tail(self, r, failed):
        if failed:
            r[R_RND2] = self.rs.rand()
            r[R_CAUCHY] = self.rs.standard_cauchy()
        return r


def choose(P, u):
    """np.random.choice(range(H), p=P) for the uniform u: cumsum, / its last entry, searchsorted on the right; never past the last entry."""
    cdf = np.cumsum(P)
    cdf = cdf / cdf[-1]
    return min(int(np.searchsorted(cdf, u, side='right')), len(P) - 1)


class Restate:
    """reset / move / end of generation of SAHLPSO in numpy, from the rules in the header of mbx_sahlpso.hpp.  Costs are handed in."""

    def __init__(self, D, max_fes, log_interval, n_logpoint, has_optimum=True, early_stop=True):
        self.D, self.max_fes, self.log_interval, self.n_logpoint = D, max_fes, log_interval, n_logpoint
        self.stop_rule = has_optimum and early_stop

    def reset(self, tape, f0):
        D, NE = self.D, NP0 * self.D
        self.V = (-1. + 2. * tape[:NE]).reshape(NP0, D)
        self.X = (-5. + 10. * tape[NE:2 * NE]).reshape(NP0, D)
        self.PB = self.X.copy()
        self.fX = np.array(f0, dtype=np.float64)
        self.pc0 = self.fX.copy()
        self.rank = np.lexsort((np.arange(NP0), self.pc0))            # cost, then the lower index
        self.sel = tape[2 * NE + 3 * NP0:2 * NE + 3 * NP0 + NSEL].astype(int)
        self.w = np.full(NP0, 0.9)
        self.g, self.gbest = int(np.argmin(self.fX)), float(np.min(self.fX))
        self.P_cr, self.nf_cr, self.ns_cr = np.ones(HCR) / HCR, np.zeros(HCR), np.zeros(HCR)
        self.P_ls, self.nf_ls, self.ns_ls = np.ones(HLS) / HLS, np.zeros(HLS), np.zeros(HLS)
        self.NP, self.G, self.fes, self.log_index, self.cost, self.done = NP0, 1, NP0, 1, [self.gbest], False

    # what a move decides before it draws
    def remain(self):
        return np.arange(NP0) if self.NP == NP0 else self.rank[:self.NP]

    def best_p(self):
        return self.rank[:max(1, int(0.2 * self.NP))]

    def adapt(self):
        return bool(self.G % LP) or self.G == 1

    def is_sel(self, i):
        return i in self.sel

    def move(self, i, r):
        """-> the new row X[i]; to be evaluated by the caller."""
        D = self.D
        self.cri = self.lsi = 0
        cr = 0.
        if self.adapt():
            self.cri, self.lsi = choose(self.P_cr, r[R_UCR]), choose(self.P_ls, r[R_ULS])
            cr = M_CR[self.cri]
        sel = self.is_sel(i)
        if sel:
            m, n = int(r[R_M]), int(r[R_N])
            o = m if self.fX[m] < self.fX[n] else n
        else:
            o = int(r[R_PICK])
        mask = r[R_CROSS:R_CROSS + D] < cr
        self.PB[i] = np.where(mask, self.PB[o], self.PB[i])          # into the row, whatever the move's outcome
        e = self.PB[i]
        if not sel:
            r1 = r[R_CROSS + D:R_CROSS + 2 * D]
            e = r1 * e + (1 - r1) * self.X[self.g]
        self.nf_cr[self.cri] += 1
        self.nf_ls[self.lsi] += 1
        v = self.w[i] * self.V[i] + C1 * r[R_CROSS + 2 * D:R_CROSS + 3 * D] * (e - self.X[i])
        self.V[i] = np.minimum(np.maximum(v, -1.), 1.)
        self.X[i] = np.minimum(np.maximum(self.X[i] + self.V[i], -5.), 5.)
        return self.X[i]

    def success(self, i, f):
        return bool(f < self.pc0[i])

    def finish_move(self, i, r, f):
        self.fX[i] = f
        succ = self.success(i, f)
        if succ:
            self.PB[i] = self.X[i]
            if f < self.gbest:
                self.g, self.gbest = i, float(f)
            self.ns_cr[self.cri] += 1
            self.ns_ls[self.lsi] += 1
        else:
            self.w[i] = min(max((0.7 if r[R_RND2] < 0.5 else 0.3) + 0.1 * r[R_CAUCHY], 0.2), 0.9)
        self.fes += 1
        if self.fes >= self.log_index * self.log_interval:           # once, not "while"
            self.log_index += 1
            if len(self.cost) <= self.n_logpoint:
                self.cost.append(self.gbest)
        self.done = self.fes >= self.max_fes or (self.stop_rule and self.gbest <= 1e-8)
        if self.done:
            if len(self.cost) >= self.n_logpoint + 1:
                self.cost[-1] = self.gbest
            else:
                self.cost.append(self.gbest)
        return succ

    def end_generation(self):
        if self.G % LP == 0:
            S = np.zeros(HCR)
            nz = self.nf_cr != 0
            S[nz] = self.ns_cr[nz] / self.nf_cr[nz]
            self.P_cr = np.ones(HCR) / HCR if np.sum(S) == 0 else S / np.sum(S)     # (sum == 0: the departure -- H_cr stays 5)
            S = np.zeros(HLS)
            nz = self.nf_ls != 0
            S[nz] = self.ns_ls[nz] / self.nf_ls[nz]
            self.P_ls = np.ones(HLS) / HLS if np.sum(S) == 0 else S / np.sum(S)
        NP_ = round((4 - NP0) * self.fes / self.max_fes + NP0)
        if NP_ < self.NP:
            self.NP = NP_
        self.G += 1


def _problem(suite, dim, fid):
    p = problems(suite, int(dim))[int(fid)]
    return p, p.noise[0]


def _case(case):
    suite, dim, fid, seed = case.split('/')
    p, nk = _problem(suite, dim, fid)
    return p, nk, int(dim), int(seed), int(TR[f'{case}/max_fes']), int(TR[f'{case}/log_interval']), int(TR[f'{case}/n_logpoint'])


class Walker:
    """Walks a fixture case launch by launch (reset first): Restate on the feeder's draws and the recorded costs, with the tape of each launch."""

    def __init__(self, case, check=False):
        self.case, self.check = case, check
        self.p, self.nk, self.D, self.seed, self.max_fes, self.log_interval, self.nlog = _case(case)
        self.rs = np.random.RandomState(self.seed)
        self.fd = SahlTapeFeeder(self.seed, self.D, self.nk, self.rs)
        self.want = {k: TR[f'{case}/{k}'] for k in ('f0', 'sel', 'g0', 'mv_i', 'mv_cr', 'mv_ls', 'mv_f', 'mv_succ', 'mv_w', 'mv_stale', 'mv_pbx', 'gen_pcr', 'gen_pls',
                                                    'gen_np', 'gen_fes', 'gen_gcost', 'gen_g', 'end_gcost', 'end_g', 'snaps', 'snap_at', 'cost', 'fes')}
        self.U = len(self.want['gen_np']) + 1                         # launches after the reset; the last one is the pass the episode ends in
        self.rs_ = Restate(self.D, self.max_fes, self.log_interval, self.nlog)
        self.n_moves = 0

    def reset(self):
        t = self.fd.reset_tape()
        self.rs_.reset(t, self.want['f0'])
        if self.check:
            assert np.array_equal(self.rs_.sel, self.want['sel']) and self.rs_.g == self.want['g0'], self.case
            assert np.array_equal(self.rs_.rank, np.argsort(self.want['f0'])), self.case
        return t

    def launch(self, u):
        """-> (tape, [(slot, particle, cr_index, ls_index, success, recorded cost)]) of launch u; Restate is advanced through it."""
        rs, w, D = self.rs_, self.want, self.D
        assert rs.G == u and not rs.done
        t = np.zeros(tape_stride(D))
        moves = []
        pcr_before = rs.P_cr.copy()
        for k, i in enumerate(rs.remain()):
            i = int(i)
            r = self.fd.move_head(rs.adapt(), rs.is_sel(i), rs.remain(), rs.best_p())
            pb_before = rs.PB[i].copy()
            rs.move(i, r)
            n = self.n_moves
            f = float(w['mv_f'][n])
            self.fd.move_tail(r, not rs.success(i, f))
            succ = rs.finish_move(i, r, f)
            t[k * rec_len(D):(k + 1) * rec_len(D)] = r
            moves.append((k, i, rs.cri, rs.lsi, succ, f))
            if self.check:
                assert (i, rs.cri, rs.lsi, succ) == (w['mv_i'][n], w['mv_cr'][n], w['mv_ls'][n], bool(w['mv_succ'][n])), (self.case, u, k)
                assert rs.w[i] == w['mv_w'][n] and (rs.gbest != rs.fX[rs.g]) == bool(w['mv_stale'][n]), (self.case, u, k)
                assert (not succ and not np.array_equal(pb_before, rs.PB[i])) == bool(w['mv_pbx'][n]), (self.case, u, k)
            self.n_moves += 1
            if rs.done:
                break
        if not rs.done:
            rs.end_generation()
            if self.check:
                assert np.array_equal(rs.P_cr, w['gen_pcr'][u - 1]) and np.array_equal(rs.P_ls, w['gen_pls'][u - 1]), (self.case, u, pcr_before)
                assert (rs.NP, rs.fes, rs.gbest, rs.g) == (w['gen_np'][u - 1], w['gen_fes'][u - 1], w['gen_gcost'][u - 1], w['gen_g'][u - 1]), (self.case, u)
        return t, moves

    def snapshot(self, u):
        at = np.nonzero(self.want['snap_at'] == u)[0]
        return self.want['snaps'][at[-1]] if len(at) else None


# ------------------------------------------------------------------------------------------------ CPU
def test_sahlpso_is_exported_and_picked_up_by_the_tester(tmp_path):
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import SAHLPSO
    from metabox_amd.tester import Tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--test', '--t_optimizer_for_cp', 'GL_PSO', 'sDMS_PSO', 'SAHLPSO', '--log_dir', str(tmp_path / 'out')])
    t = Tester(cfg)
    assert [type(o).__name__ for o in t.t_optimizer_for_cp][:3] == ['GL_PSO', 'sDMS_PSO', 'SAHLPSO'] and t.skipped == []
    assert isinstance(SAHLPSO(copy.deepcopy(cfg)), SAHLPSO)
    assert all('SAHLPSO' in t.test_results['cost'][str(p)] for p in t.test_set.data)


def test_abi_geometry_of_sahlpso():
    from metabox_amd import _abi
    lib = _abi.load_lib()
    assert _abi.ALGO_SAHLPSO == ALGO_SAHLPSO
    for D in (2, 10, 40):
        cfg = oracle.make_cfg(ALGO_SAHLPSO, NP0, D, 2000 * D, 40 * D, 50)
        assert lib.mbx_tape_stride(C.byref(cfg)) == tape_stride(D) >= 2 * NP0 * D + 3 * NP0 + NSEL
        assert lib.mbx_state_dim(C.byref(cfg)) == 1
        assert lib.mbx_action_dim(C.byref(cfg)) == 0
    ok = lambda **kw: lib.mbx_state_dim(C.byref(oracle.make_cfg(ALGO_SAHLPSO, kw.get('np_', NP0), kw.get('dim', 10), kw.get('max_fes', 20000), 400, 50)))   # noqa: E731
    lib.mbx_last_error.restype = C.c_char_p
    assert ok() == 1
    for bad in (dict(np_=39), dict(np_=41), dict(dim=1), dict(dim=41), dict(max_fes=40)):
        assert ok(**bad) < 0 and b'SAHLPSO' in lib.mbx_last_error(), bad
    assert ok(max_fes=41) == 1
    for algo in (12, 14, 17):                                        # stay unassigned
        assert lib.mbx_state_dim(C.byref(oracle.make_cfg(algo, NP0, 10, 20000, 400, 50))) < 0
    assert len(_abi.EXPORTED_SYMBOLS) == 45


def test_n_generations_equals_the_fixture():
    from metabox_amd.optimizer import SAHLPSO
    full = 0
    for case in CASES:
        max_fes, fes = int(TR[f'{case}/max_fes']), int(TR[f'{case}/fes'])
        if fes >= max_fes:                                           # ran to its budget
            full += 1
            assert fes == max_fes, case
            assert n_generations(max_fes) == SAHLPSO.n_generations(max_fes) == len(TR[f'{case}/gen_np']) + 1, case
        else:
            assert SAHLPSO.n_generations(max_fes) > len(TR[f'{case}/gen_np']) + 1, case
    assert full >= 6
    assert SAHLPSO.n_generations(41) == 1 and SAHLPSO.n_generations(80) == 1 and SAHLPSO.n_generations(81) == 2


@pytest.mark.parametrize('case', CASES)
def test_restatement_and_feeder_reproduce_the_reference(case):
    """The rules as the kernel header states them, in numpy, on the feeder's draws and the reference's costs: every recorded quantity of every
    move and generation and every snapshot, exactly; and over the whole episode the feeder draws exactly what the reference drew: the next
    np.random.rand() after the episode is the one the generator recorded."""
    wk = Walker(case, check=True)
    wk.reset()
    rs, w = wk.rs_, wk.want
    for u in range(wk.U + 1):
        if u > 0:
            wk.launch(u)
        snap = wk.snapshot(u)
        if snap is not None:
            assert np.array_equal(rs.X, snap[0]) and np.array_equal(rs.V, snap[1]) and np.array_equal(rs.PB, snap[2]), (case, u)
    assert rs.done and wk.n_moves == len(w['mv_f']) and rs.fes == w['fes'] and w['snap_at'][-1] == wk.U
    assert (rs.gbest, rs.g) == (w['end_gcost'], w['end_g'])
    assert np.array_equal(rs.cost, w['cost'])
    assert wk.rs.rand() == float(TR[f'{case}/next_rand']), case


def test_fixture_covers_the_quirks():
    """The fixture exercises what it is meant to pin (the clause on a P_cr with a zero entry was dropped: see the module docstring)."""
    early = budget_mid = 0
    for c in CASES:
        live = np.concatenate([[NP0], TR[f'{c}/gen_np']])
        last = int(TR[f'{c}/fes']) - NP0 - int(np.sum(live[:-1]))
        assert 1 <= last <= live[-1], c
        mid = last < live[-1]
        if int(TR[f'{c}/fes']) < int(TR[f'{c}/max_fes']):
            assert TR[f'{c}/end_gcost'] <= 1e-8, c
            early += mid
        else:
            budget_mid += mid
    assert early >= 1 and budget_mid >= 1
    assert any(TR[f'{c}/mv_stale'].any() for c in CASES) and any(TR[f'{c}/mv_pbx'].any() for c in CASES)
    assert max(int(np.sum(np.diff(np.concatenate([[NP0], TR[f'{c}/gen_np']])) < 0)) for c in CASES) >= 10
    assert min(int(TR[f'{c}/gen_np'].min()) for c in CASES) == 4
    assert all(np.all(TR[f'{c}/gen_pcr'] > 0) for c in CASES)                          # what the generator found: no zero entry anywhere
    for c in CASES:                                                                    # G % 5 == 0: both counters go to index 0
        live = np.concatenate([[NP0], TR[f'{c}/gen_np']])
        start = int(np.sum(live[:4]))                                        # first move of generation 5
        if len(live) > 5:
            assert not TR[f'{c}/mv_cr'][start:start + int(live[4])].any() and not TR[f'{c}/mv_ls'][start:start + int(live[4])].any(), c
    assert {_problem(*c.split('/')[:3])[1] for c in CASES if c.startswith('bbob-noisy')} == {1, 2, 3}
    assert {c.split('/')[1] for c in CASES} >= {'10', '30'} and sum(int(TR[f'{c}/max_fes']) == 20000 for c in CASES) == 1
    assert all(400 <= int(TR[f'{c}/max_fes']) <= 4000 for c in CASES if int(TR[f'{c}/max_fes']) != 20000)


def _crafted():
    rs = Restate(3, 4000, 80, 50)
    t = np.zeros(tape_stride(3))
    t[:2 * NP0 * 3] = np.random.RandomState(1).rand(2 * NP0 * 3)
    t[2 * NP0 * 3 + 3 * NP0:2 * NP0 * 3 + 3 * NP0 + NSEL] = np.arange(NSEL)
    rs.reset(t, np.arange(NP0, dtype=np.float64)[::-1] + 1.)
    return rs


def test_the_departure_branch_and_a_zero_entry_behave_as_documented():
    """sum(S_cr) == 0 at the end of a generation with G % 5 == 0: the reference would grow H_cr (and fail five generations later); here H_cr
    stays 5 and P_cr is uniform again.  A P_cr with a zero entry -- no fixture has one -- is never chosen, whatever the uniform."""
    rs = _crafted()
    rs.G, rs.fes = 5, 240
    rs.nf_cr[:] = [9, 8, 7, 6, 10]
    rs.nf_ls[:] = 3
    rs.ns_ls[2] = 1
    rs.P_cr = np.array([.1, .2, .3, .2, .2])
    rs.end_generation()
    assert len(rs.P_cr) == HCR and np.array_equal(rs.P_cr, np.full(HCR, 1. / HCR)) and rs.G == 6
    assert np.array_equal(rs.P_ls, np.eye(HLS)[2]) and rs.NP == round(-36 * 240 / 4000 + 40) == 38
    rs = _crafted()
    rs.G, rs.fes = 10, 500
    rs.nf_cr[:] = [10, 10, 10, 10, 10]
    rs.ns_cr[:] = [5, 0, 2, 0, 3]
    rs.end_generation()
    assert np.array_equal(rs.P_cr, np.array([.5, 0., .2, 0., .3]) / np.sum([.5, 0., .2, 0., .3]))
    picks = {choose(rs.P_cr, u) for u in np.concatenate([np.linspace(0., 1., 2001)[:-1], [np.nextafter(1., 0.), 0.5, np.nextafter(0.5, 0.), 0.7]])}
    assert picks == {0, 2, 4}
    assert choose(rs.P_cr, 1.0) == 4                                 # a tape value of 1 cannot leave the table
    # the iteration order after a reduction is rank order, and best_p is its prefix
    assert np.array_equal(rs.remain(), rs.rank[:rs.NP]) and rs.NP < NP0 and np.array_equal(rs.rank, np.arange(NP0)[::-1])
    assert np.array_equal(rs.best_p(), rs.rank[:int(0.2 * rs.NP)])


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_hip_sahlpso_tape_replay_matches_reference(case):
    import torch
    from metabox_amd.suite import Batch, Suite
    wk = Walker(case)
    w, D, rs = wk.want, wk.D, wk.rs_
    b = Batch(Suite([wk.p]), ALGO_SAHLPSO, [0], [wk.seed], NP0, wk.max_fes, wk.log_interval, wk.nlog)
    assert (b.state_dim, b.action_dim, b.tape_stride) == (1, 0, tape_stride(D))
    ledger, diverged = [], False
    for u in range(wk.U + 1):
        if u == 0:
            tape, moves = wk.reset(), []
        else:
            tape, moves = wk.launch(u)
        b.set_tape(torch.from_numpy(tape[None]).cuda())
        if u == 0:
            b.reset()
        else:
            _, _, d = b.step(None)
        st = split_state(b.read_state(0), D, wk.nlog)
        sc = st['scalars']
        if u == 0:
            assert close(st['pbcost0'], w['f0']) and np.array_equal(st['fX'], st['pbcost0']), case
            assert np.array_equal(st['rank'], rs.rank) and np.array_equal(st['sel'], rs.sel) and sc[SC_GROW] == rs.g, case
            assert np.array_equal(st['w'], rs.w) and np.array_equal(st['P_cr'][:HCR], rs.P_cr) and np.array_equal(st['P_ls'][:HLS], rs.P_ls), case
        elif not diverged:
            # the first launch whose success flags differ must sit on a proven near-tie; float tolerances only afterwards
            idx = np.array([m[1] for m in moves])
            n = len(moves)
            ref_f, ref_s = np.array([m[5] for m in moves]), np.array([float(m[4]) for m in moves])
            ok = sc[SC_MOVES] == n and np.array_equal(st['move_i'][:n], idx)
            assert ok, (case, u, 'the pass did not walk the same particles', sc[SC_MOVES], n)
            ok = prove_tie_arrays(w['f0'][idx], ref_f, ref_s, st['pbcost0'][idx], st['fX'][idx], st['move_succ'][:n], ledger, 'success', case, u)
            diverged = not ok
        if not diverged:
            assert sc[SC_FES] == rs.fes and sc[SC_GEN] == u and sc[SC_NP] == rs.NP and sc[SC_GROW] == rs.g, (case, u)
            assert sc[SC_DONE] == float(rs.done) and (u == 0 or int(d[0].item()) == int(rs.done)), (case, u)
            assert np.array_equal(st['X'], rs.X.ravel()), (case, u, 'position')
            assert np.array_equal(st['V'], rs.V.ravel()), (case, u, 'velocity')
            assert np.array_equal(st['pbpos'], rs.PB.ravel()), (case, u, 'pBest rows')
            assert np.array_equal(st['w'], rs.w), (case, u, 'w')
            assert np.array_equal(st['P_cr'][:HCR], rs.P_cr) and np.array_equal(st['P_ls'][:HLS], rs.P_ls), (case, u, 'P')
            assert np.array_equal(st['nf_cr'][:HCR], rs.nf_cr) and np.array_equal(st['ns_cr'][:HCR], rs.ns_cr), (case, u)
            assert np.array_equal(st['nf_ls'][:HLS], rs.nf_ls) and np.array_equal(st['ns_ls'][:HLS], rs.ns_ls), (case, u)
            if moves:
                n = len(moves)
                assert np.array_equal(st['move_cr'][:n], [m[2] for m in moves]) and np.array_equal(st['move_ls'][:n], [m[3] for m in moves]), (case, u)
            assert close(st['fX'], rs.fX), (case, u)
            snap = wk.snapshot(u)
            if snap is not None:
                assert np.array_equal(st['X'], snap[0].ravel()) and np.array_equal(st['V'], snap[1].ravel()) and np.array_equal(st['pbpos'], snap[2].ravel()), (case, u)
        assert close(sc[SC_GBEST], rs.gbest), (case, u, sc[SC_GBEST], rs.gbest)
    res = b.results()
    n = int(res['cost_len'][0].item())
    assert rs.done and n == len(w['cost']) and close(res['cost'][0, :n].cpu().numpy(), w['cost']), (case, n, len(w['cost']))
    assert diverged or res['fes'][0].item() == w['fes']
    before = b.read_state(0)
    b.step(None)                                                     # a launch after done changes nothing
    assert np.array_equal(before, b.read_state(0))
    print_ledger(ledger)
    b.close()


def _u53(w0, w1):
    return ((w0 >> 5) * 67108864.0 + (w1 >> 6)) / 9007199254740992.0


def philox_tape(seed, D, noise_kind, gen, st, episode=0):
    """The tape that reproduces the Philox stream of (seed, gen, episode) under the site map of include/mbx_layout.h section 17.  st: for a
    pass, the state block BEFORE it (NP and the ranking decide who m, n and pick are) with move_cauchy of the Philox run's block AFTER it
    (the device's tan is not reproduced on the host)."""
    t = np.zeros(tape_stride(D))

    def ph(idx, site):
        return oracle.philox(seed, idx, site, gen, episode)

    def noise(idx):
        if noise_kind == 2:
            w = ph(idx, SITE_NOISE_A)
            return _u53(w[0], w[1]), _u53(w[2], w[3]), 0.
        assert noise_kind == 0, 'only the noise kinds whose draws are exact uniforms are rebuilt here'
        return 0., 0., 0.

    if gen == 0:
        NE = NP0 * D
        for e in range(NE):
            w = ph(e, SITE_ELEM_R)
            t[NE + e], t[e] = _u53(w[0], w[1]), _u53(w[2], w[3])
        for i in range(NP0):
            t[2 * NE + i], t[2 * NE + NP0 + i], t[2 * NE + 2 * NP0 + i] = noise(i)
        keys = np.array([ph(i, SITE_PERM)[0] for i in range(NP0)], dtype=np.int64)
        t[2 * NE + 3 * NP0:2 * NE + 3 * NP0 + NSEL] = np.lexsort((np.arange(NP0), keys))[:NSEL]
        return t
    NP, rank = int(st['scalars'][SC_NP]), st['rank'].astype(int)
    remain = np.arange(NP0) if NP == NP0 else rank[:NP]
    nbp = max(1, int(0.2 * NP))
    for k in range(NP):
        r = t[k * rec_len(D):(k + 1) * rec_len(D)]
        w = ph(k, SITE_CHOICE)
        r[R_UCR], r[R_ULS] = _u53(w[0], w[1]), _u53(w[2], w[3])
        w = ph(k, SITE_PICK)
        r[R_M], r[R_N], r[R_PICK] = remain[(w[0] * NP) >> 32], remain[(w[1] * NP) >> 32], rank[(w[2] * nbp) >> 32]
        w = ph(k, SITE_FAIL)
        r[R_RND2], r[R_CAUCHY] = _u53(w[0], w[1]), st['move_cauchy'][k]
        r[R_NOISE:R_NOISE + 3] = noise(k)
        for d in range(D):
            w, v = ph(64 * k + d, SITE_ELEM), ph(64 * k + d, SITE_VEL)
            r[R_CROSS + d], r[R_CROSS + D + d], r[R_CROSS + 2 * D + d] = _u53(w[0], w[1]), _u53(w[2], w[3]), _u53(v[0], v[1])
    return t


@pytest.mark.gpu
@pytest.mark.parametrize('dim,ids,max_fes,G', [(10, [15, 102], 1200, 14), (2, [8, 1], 400, 12)])
def test_hip_sahlpso_philox_equals_tape(dim, ids, max_fes, G):
    """The Philox path and the tape path are the same computation: a tape rebuilt on the host from oracle.philox with the documented site map
    (the cauchy values read back from the Philox run's own state block) gives bit-identical state blocks, on a noiseless and a uniform-noise
    problem at D = 10 and on two noiseless ones at the smallest shape, D = 2, over the reset and passes that include G % 5 == 0, the first
    probability update and several reductions."""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = {**problems('bbob', dim), **(problems('bbob-noisy', dim) if max(ids) > 100 else {})}
    s = Suite([ps[i] for i in ids])
    seeds = np.array([123456789012345, 987654321], dtype=np.uint64)
    a = Batch(s, ALGO_SAHLPSO, np.arange(2), seeds, NP0, max_fes, max_fes // 50, 50, early_stop=False)
    t = Batch(s, ALGO_SAHLPSO, np.arange(2), seeds, NP0, max_fes, max_fes // 50, 50, early_stop=False)
    before = [None, None]
    reduced = failed = 0
    for g in range(G + 1):
        if g == 0:
            a.reset()
        else:
            a.step(None)
        torch.cuda.synchronize()
        sa = [a.read_state(k) for k in range(2)]
        tapes = []
        for k in range(2):
            st = dict(split_state(before[k], dim)) if g else None
            if g:
                st['move_cauchy'] = split_state(sa[k], dim)['move_cauchy']
            tapes.append(philox_tape(int(seeds[k]), dim, ps[ids[k]].noise[0], g, st))
        t.set_tape(torch.from_numpy(np.stack(tapes)).cuda())
        if g == 0:
            t.reset()
        else:
            t.step(None)
        torch.cuda.synchronize()
        for k in range(2):
            st = t.read_state(k)
            assert np.array_equal(sa[k], st), (ids[k], g, int(np.argmax(sa[k] != st)))
            sp = split_state(sa[k], dim)
            reduced += sp['scalars'][SC_NP] < NP0
            failed += int(np.sum(sp['move_succ'][:int(sp['scalars'][SC_MOVES])] == 0)) if g else 0
            if g == 0:
                assert np.array_equal(np.sort(sp['rank']), np.arange(NP0)) and len(set(sp['sel'].tolist())) == NSEL
        before = sa
    assert reduced and failed                                        # both routes went through reductions and through the failed-move draws
    ra, rt = a.results(), t.results()
    for key in ('cost', 'fes', 'cost_len'):
        assert torch.equal(ra[key], rt[key]), key
    a.close(); t.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dim,ids', [(3, [1, 5, 8, 15, 21]), (40, [2, 5, 10, 17, 24])])
def test_hip_sahlpso_batch_invariance_and_frozen_done_instances(dim, ids):
    """Each instance alone (B = 1) against the same instance inside B = 5 with mixed function kinds, bit for bit, pass by pass, to the end of
    the episode (at the budget, in the middle of a pass, or earlier where gBest_cost <= 1e-8 is reached); done instances stay frozen with their exact fes, and
    further launches change nothing."""
    import torch
    from metabox_amd.suite import Batch, Suite
    ps = problems('bbob', dim)
    s = Suite([ps[i] for i in ids])
    B, max_fes = len(ids), 330
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 3
    full = Batch(s, ALGO_SAHLPSO, np.arange(B, dtype=np.int32), seeds, NP0, max_fes, 10, 50)
    ones = [Batch(s, ALGO_SAHLPSO, np.array([k], dtype=np.int32), seeds[k:k + 1], NP0, max_fes, 10, 50) for k in range(B)]
    st0 = full.reset().clone()
    for o in ones:
        o.reset()
    assert torch.allclose(st0[:, 0].cpu(), torch.full((B,), NP0 / max_fes, dtype=torch.float64))
    G = n_generations(max_fes)
    frozen, live_np = {}, [NP0] * B
    for g in range(1, G + 3):
        _, _, d = full.step(None)
        for o in ones:
            o.step(None)
        torch.cuda.synchronize()
        for k in range(B):
            blk = full.read_state(k)
            assert np.array_equal(blk, ones[k].read_state(0)), (ids[k], g)
            sp = split_state(blk, dim)
            sc = sp['scalars']
            if k in frozen:
                assert np.array_equal(blk, frozen[k]) and d[k].item() == 1, (ids[k], g)
                continue
            assert sc[SC_GEN] == g and 1 <= sc[SC_MOVES] <= live_np[k], (ids[k], g)
            if sc[SC_DONE] == 1.:
                assert sc[SC_FES] == max_fes or (sc[SC_GBEST] <= 1e-8 and sc[SC_FES] < max_fes), (ids[k], g)
                frozen[k] = blk.copy()
            else:
                assert sc[SC_MOVES] == live_np[k] and sc[SC_FES] < max_fes, (ids[k], g)
                live_np[k] = int(sc[SC_NP])
    assert len(frozen) == B
    fes = full.results()['fes'].cpu().numpy()
    assert all(f == max_fes for k, f in enumerate(fes) if ids[k] != 5)
    full.close()
    for o in ones:
        o.close()


@pytest.mark.gpu
def test_hip_sahlpso_structure_after_every_generation():
    """A short Philox run at D = 7 (no multiple of anything): after every pass the live set is the prefix of the reset's ranking of the
    scheduled length, walked in order; P_cr and P_ls sum to 1 within 1 ulp x H; w lies in [0.2, 0.9], X in [-5, 5], |V| <= 1; pbest_cost0,
    the ranking and the exploration particles never change; untouched particles keep their rows."""
    import torch
    from metabox_amd.suite import Batch, Suite
    dim, ids, max_fes = 7, [3, 15, 20, 24], 600
    ps = problems('bbob', dim)
    b = Batch(Suite([ps[i] for i in ids]), ALGO_SAHLPSO, np.arange(len(ids)), np.arange(len(ids), dtype=np.uint64) + 11, NP0, max_fes, 12, 50)
    b.reset()
    torch.cuda.synchronize()
    prev = [split_state(b.read_state(k), dim) for k in range(len(ids))]
    for sp in prev:
        assert np.array_equal(sp['rank'], np.lexsort((np.arange(NP0), sp['pbcost0']))) and np.array_equal(sp['fX'], sp['pbcost0'])
        assert sp['scalars'][SC_GROW] == sp['rank'][0] and sp['scalars'][SC_GBEST] == sp['pbcost0'].min() and np.all(sp['w'] == 0.9)
    done = [False] * len(ids)
    for g in range(1, n_generations(max_fes) + 1):
        b.step(None)
        torch.cuda.synchronize()
        for k in range(len(ids)):
            if done[k]:
                continue
            sp, pv = split_state(b.read_state(k), dim), prev[k]
            sc, NPb = sp['scalars'], int(pv['scalars'][SC_NP])
            n = int(sc[SC_MOVES])
            remain = np.arange(NP0) if NPb == NP0 else sp['rank'][:NPb].astype(int)
            assert np.array_equal(sp['move_i'][:n], remain[:n]) and sc[SC_FES] == pv['scalars'][SC_FES] + n, (ids[k], g)
            done[k] = sc[SC_DONE] == 1.
            if not done[k]:
                assert n == NPb and sc[SC_NP] == min(NPb, round((4 - NP0) * int(sc[SC_FES]) / max_fes + NP0)) >= 4, (ids[k], g)
            for name in ('pbcost0', 'rank', 'sel'):
                assert np.array_equal(sp[name], pv[name]), (ids[k], g, name)
            idle = np.setdiff1d(np.arange(NP0), remain[:n])
            for name in ('X', 'V'):
                assert np.array_equal(sp[name].reshape(NP0, dim)[idle], pv[name].reshape(NP0, dim)[idle]), (ids[k], g, name)
            assert np.array_equal(sp['fX'][idle], pv['fX'][idle]) and np.array_equal(sp['w'][idle], pv['w'][idle]), (ids[k], g)
            assert abs(np.sum(sp['P_cr'][:HCR]) - 1.) <= HCR * np.spacing(1.) and abs(np.sum(sp['P_ls'][:HLS]) - 1.) <= HLS * np.spacing(1.), (ids[k], g)
            assert np.all(sp['P_cr'] >= 0) and np.all(sp['P_ls'] >= 0) and not sp['P_cr'][HCR:].any() and not sp['P_ls'][HLS:].any()
            if g % LP:
                assert np.array_equal(sp['P_cr'], pv['P_cr']) and np.array_equal(sp['P_ls'], pv['P_ls']), (ids[k], g)
            if g % LP == 0 and g != 1:
                assert not sp['move_cr'][:n].any() and not sp['move_ls'][:n].any(), (ids[k], g)
            assert np.sum(sp['nf_cr']) == np.sum(sp['nf_ls']) == sc[SC_FES] - NP0 and np.sum(sp['ns_cr']) == np.sum(sp['ns_ls']), (ids[k], g)
            assert np.all((sp['w'] >= 0.2) & (sp['w'] <= 0.9)) and np.all(np.abs(sp['X']) <= 5.) and np.all(np.abs(sp['V']) <= 1.), (ids[k], g)
            succ = sp['move_succ'][:n] == 1
            mi = sp['move_i'][:n].astype(int)
            assert np.array_equal(succ, sp['fX'][mi] < sp['pbcost0'][mi]), (ids[k], g)
            assert np.array_equal(sp['pbpos'].reshape(NP0, dim)[mi[succ]], sp['X'].reshape(NP0, dim)[mi[succ]]), (ids[k], g)
            assert sc[SC_GBEST] <= pv['scalars'][SC_GBEST], (ids[k], g)
            prev[k] = sp
    assert all(done)
    b.close()


@pytest.mark.gpu
def test_sahlpso_in_the_tester_and_the_b1_view(tmp_path):
    import pickle
    import torch
    from metabox_amd.config import get_config
    from metabox_amd.optimizer import SAHLPSO
    from metabox_amd.tester import Tester
    names = ['GL_PSO', 'sDMS_PSO', 'SAHLPSO']
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda', '--test', '--t_optimizer_for_cp'] + names +
                     ['--log_dir', str(tmp_path / 'out'), '--test_runs', '2'])
    cfg.maxFEs = 2000
    cfg.log_interval = cfg.maxFEs // cfg.n_logpoint
    cfg.t_optimizer_for_cp = names
    t = Tester(cfg)
    assert t.skipped == []
    t.test()
    with open(t.log_dir + 'test.pkl', 'rb') as f:
        res = pickle.load(f)
    for p in t.test_set.data:
        for name in names:                                           # three filled columns
            rows = res['cost'][str(p)][name]
            assert len(rows) == 2 and all(len(r) == 51 for r in rows) and all(np.all(np.diff(r) <= 0) for r in rows), (str(p), name)
        assert all(f == 2000 or (f < 2000 and r[-1] <= 1e-8) for f, r in zip(res['fes'][str(p)]['SAHLPSO'], res['cost'][str(p)]['SAHLPSO'])), str(p)
    # the B = 1 view is the batch's computation for the same seed; F5 stops early, and its short curve is padded with its last entry
    ps = problems('bbob', 10)
    for fid in (8, 5):
        opt = SAHLPSO(copy.deepcopy(cfg))
        np.random.seed(3)
        info = opt.run_episode(ps[fid])
        np.random.seed(3)
        seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
        s = ps[fid]._bound_suite()
        r = SAHLPSO(copy.deepcopy(cfg)).run_batch(s, [ps[fid]._suite_index], [seed])
        n = int(r['cost_len'][0].item())
        assert info['fes'] == int(r['fes'][0].item()) and info['cost'] == [float(v) for v in r['cost'][0, :n].cpu().numpy()], fid
        if fid == 8:
            assert info['fes'] == 2000 and n == 51
        else:
            from metabox_amd.tester import _pad51
            assert info['fes'] < 2000 and n < 51 and info['cost'][-1] <= 1e-8
            assert _pad51(info['cost']) == info['cost'] + [info['cost'][-1]] * (51 - n)
            assert [float(v) for v in r['cost'][0].cpu().numpy()][:n] == info['cost']
    torch.cuda.synchronize()
