"""The curve bound (include/mbx.h): the reference's cost list can outgrow the n_logpoint + 1 slots of an instance's curve, because its log point appends without
looking at the length.  The rule: a write to curve index > n_logpoint is dropped, cost_len goes on counting.  Here the C oracle is held to a list model of the
reference's bookkeeping on both sides of the bound (CPU), and its over-long episodes run under the address / undefined-behaviour sanitizer in a stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity
from helpers import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGOS = ('lde', 'gleet', 'rlpso', 'qlpso', 'de', 'pso')
# (NP, D, max_fes, log_interval, n_logpoint).  The list fits while log_interval * (n_logpoint + 1) > max_fes (first three rows: the shipped setting of QLPSO / RL-PSO,
# an interval the budget does not divide, a short run); the others outgrow it for at least one family of algorithms.  (4, 2, 45, 2, 5) is at least three entries too
# long for every algorithm; (30, 10, 976, 19, 50) is `--maxFEs 976` with 50 log points: 52 entries where a step spends one evaluation.
GRID = [(30, 10, 2500, 50, 50), (30, 10, 950, 19, 50), (4, 2, 29, 6, 5),
        (4, 2, 29, 5, 5), (30, 10, 976, 19, 50), (4, 2, 45, 2, 5), (5, 3, 45, 5, 5), (7, 3, 33, 5, 5)]
TOO_LONG_BY_THREE = (4, 2, 45, 2, 5)


class ListModel:
    """optimizer.cost as the reference keeps it (e.g. rlepso_optimizer.py:241-261): a Python list, appended to at a log point whatever its length."""

    def __init__(self, gbest, log_interval, n_logpoint):
        self.cost, self.log_index, self.log_interval, self.n_logpoint = [gbest], 1, log_interval, n_logpoint

    def update(self, fes, gbest, done):
        if fes >= self.log_index * self.log_interval:
            self.log_index += 1
            self.cost.append(gbest)
        if done:
            if len(self.cost) >= self.n_logpoint + 1:
                self.cost[-1] = gbest
            else:
                self.cost.append(gbest)


def _episode(name, NP, D, max_fes, li, nlog):
    """One oracle episode to its end -> (list model, fes the model expects, the oracle's last view)."""
    p = problems('bbob', D)[15]                                        # Rastrigin: nowhere near 1e-8 inside these budgets
    steps = 4 * max_fes
    acts = parity.actions_for(name, steps, 1, NP)
    rec = parity.oracle_record(name, p, NP, D, (max_fes, li, nlog), 11, None if acts is None else acts[:, 0], steps)
    assert rec['done'][-1] and not rec['done'][:-1].any()
    v = rec['views']
    model, fes = ListModel(v[0]['sc']['gbest'], li, nlog), NP
    for g in range(len(rec['done'])):
        if name in ('de', 'pso'):                                      # a sweep logs after every trial: trial k can only lower the k-th (personal) best
            gbest = v[g]['sc']['gbest']
            for k in range(NP):
                fes += 1
                gbest = min(gbest, v[g + 1]['best'][k])
                model.update(fes, gbest, fes >= max_fes)
                if fes >= max_fes:
                    break
        else:
            fes += 1 if name in parity.PER_PARTICLE else NP
            model.update(fes, v[g + 1]['sc']['gbest'], fes >= max_fes)
        assert (fes >= max_fes) == bool(rec['done'][g]), (name, g, fes)
    return model, fes, v[-1]


@pytest.mark.parametrize('name', ALGOS)
def test_oracle_keeps_the_first_entries_and_the_true_length(name):
    seen = set()
    for NP, D, max_fes, li, nlog in GRID:
        model, fes, last = _episode(name, NP, D, max_fes, li, nlog)
        where = (name, NP, D, max_fes, li, nlog)
        assert last['sc']['cost_len'] == len(model.cost), (where, last['sc']['cost_len'], len(model.cost))
        n = min(len(model.cost), nlog + 1)
        assert np.array_equal(last['curve'][:n], np.array(model.cost[:n])), (where, last['curve'], model.cost)
        assert last['sc']['fes'] == fes, where
        seen.add(len(model.cost) > nlog + 1)
        if (NP, D, max_fes, li, nlog) == TOO_LONG_BY_THREE:
            assert len(model.cost) >= nlog + 4, (where, len(model.cost))
        if (NP, D, max_fes, li, nlog) == (4, 2, 29, 5, 5) and name in ('lde', 'gleet'):
            assert len(model.cost) == 7
        if (NP, D, max_fes, li, nlog) == (30, 10, 976, 19, 50) and name in parity.PER_PARTICLE:
            assert len(model.cost) == 52
    assert seen == {False, True}                                       # both sides of the bound


def test_list_model_is_the_reference_bookkeeping():
    """The model on the budget the LES fixture pins to the reference (tests/test_les.py: 52 entries at maxFEs 976, interval 19, 16 evaluations a generation)."""
    m, fes = ListModel(1., 19, 50), 16
    while fes < 976:
        fes += 16
        m.update(fes, 1., fes >= 976)
    assert len(m.cost) == 52


def test_over_long_episodes_are_clean_under_the_sanitizers(tmp_path):
    """oracle/curve_bound_main.c: whole over-long episodes of the six algorithms in a stand-alone program built with -fsanitize=address,undefined (a child process of
    its own; nothing of it is loaded here).  Before the bound the log point of the (4, 2, 45, 2, 5) episode wrote past the oracle's n_logpoint + 2 slots."""
    cc = shutil.which(os.environ.get('CC', 'gcc')) or shutil.which('cc')
    assert cc, 'no C compiler'
    exe = str(tmp_path / 'curve_bound')
    subprocess.check_call([cc, '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan', '-ffp-contract=off',
                           '-mfma', '-w', '-o', exe, os.path.join(ROOT, 'oracle', 'curve_bound_main.c'), '-lm'])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, (r.returncode, r.stderr[-2000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 24 and {row[0] for row in rows} == set(ALGOS)
    long3 = [int(row[-1]) for row in rows if tuple(int(x) for x in row[1:6]) == TOO_LONG_BY_THREE]
    assert len(long3) == 6 and min(long3) >= 5 + 4, rows
