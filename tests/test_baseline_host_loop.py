"""The host loops of the nine agent-less optimizers (Random_search, DEAP_DE, DEAP_PSO, DEAP_CMAES, GL_PSO, JDE21, MadDE, sDMS_PSO, SAHLPSO), pinned
call by call.  A recording stand-in takes the place of ``metabox_amd.suite.Batch`` (``make_batch`` imports it when called), so no library and no
device are needed.  Every class runs three episodes of the B = 1 view -- two problems of one suite, then a problem of another suite -- and one
``run_batch``; the expected sequences below are what the classes did when each still carried its own copy of the loop.  They hold the seeds, the
``rebind`` of the classes that keep their batch, the fresh batch of those that must not (a kept batch advances the episode counter, which feeds the
Philox stream), and the read / write of the state slice that MadDE (pm) and GL_PSO (exemplar_stag) carry into a batch on another suite.
"""
import types

import numpy as np
import pytest
import torch

MAX_FES, LOG_INTERVAL, N_LOGPOINT = 2000, 400, 5
DONE_AFTER = 3                      # the stand-in reports every instance done from its third step on
STATE_DOUBLES = 20000


class Recorder:
    """Stand-in for suite.Batch: appends every call to the shared log; consecutive ``step(None)`` calls are counted, not listed."""
    log = None
    serial = 0

    def __init__(self, suite, algo, problem_idx, seeds, np_, max_fes, log_interval, n_logpoint, early_stop=True):
        Recorder.serial += 1
        self.id = Recorder.serial
        self.B = len(problem_idx)
        self.cfg = types.SimpleNamespace(dim=suite.dim, n_logpoint=n_logpoint)
        self.steps = 0
        self.log.append(('Batch', self.id, suite.name, int(algo), list(problem_idx), list(seeds), np_, max_fes, log_interval, n_logpoint, early_stop))

    def _say(self, *entry):
        self.log.append((entry[0], self.id) + entry[1:])

    def reset(self):
        self.steps = 0
        self._say('reset')

    def step(self, actions):
        assert actions is None
        self.steps += 1
        last = self.log[-1]
        if last[:2] == ('steps', self.id):
            self.log[-1] = ('steps', self.id, last[2] + 1)
        else:
            self._say('steps', 1)
        return None, None, torch.full((self.B,), self.steps >= DONE_AFTER)

    def rebind(self, problem_idx, seeds):
        self._say('rebind', list(problem_idx), list(seeds))

    def read_state(self, instance):
        self._say('read_state', instance)
        return np.full(STATE_DOUBLES, float(self.id))

    def write_state(self, instance, block):
        other = np.flatnonzero(block != float(self.id))            # what the caller changed in the block it read from this batch
        self._say('write_state', instance, int(other[0]), len(other), sorted(set(block[other].tolist())))

    def read_public(self, instance=0):
        self._say('read_public', instance)
        sc = np.zeros(16 + N_LOGPOINT + 1)
        sc[1], sc[2], sc[3] = 1000 + self.id, 2, 3
        sc[16:19] = (9., 8., 7. + self.id)
        return sc

    def results(self):
        self._say('results')
        cost = torch.tensor([[9., 8., 7. + self.id, 7. + self.id, 7. + self.id, 7. + self.id]] * self.B, dtype=torch.float64)
        return {'cost': cost, 'fes': torch.full((self.B,), 1000. + self.id, dtype=torch.float64), 'cost_len': torch.full((self.B,), 3, dtype=torch.int32)}

    def close(self):
        self._say('close')


def _problem(suite, index):
    return types.SimpleNamespace(reset=lambda: None, _bound_suite=lambda: suite, _suite_index=index)


def _scenario(cls, monkeypatch):
    """-> (log, the three episode results, the optimizer, its config)."""
    import metabox_amd.suite
    monkeypatch.setattr(metabox_amd.suite, 'Batch', Recorder)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a: None)
    Recorder.log, Recorder.serial = [], 0
    config = types.SimpleNamespace(maxFEs=MAX_FES, log_interval=LOG_INTERVAL, n_logpoint=N_LOGPOINT)
    opt = cls(config)
    A, B = types.SimpleNamespace(dim=10, name='A'), types.SimpleNamespace(dim=10, name='B')
    np.random.seed(7)
    infos = [opt.run_episode(_problem(A, 3)), opt.run_episode(_problem(A, 5)), opt.run_episode(_problem(B, 1))]
    res = opt.run_batch(A, [0, 2], [11, 12])
    assert sorted(res) == ['cost', 'cost_len', 'fes'] and res['cost'].shape == (2, 6)
    return Recorder.log, infos, opt, config


# the three seeds np.random.seed(7) gives the expression int(randint(0, 2**31 - 1)) * 2654435761 + int(randint(0, 2**31 - 1))
S1, S2, S3 = 869969064200307907, 3191274353319947839, 4998178532741505062


def _fresh(algo, np_, n):
    """A class whose B = 1 view builds a batch per episode and reads it through results()."""
    out = []
    for k, (suite, idx, seeds) in enumerate((('A', [3], [S1]), ('A', [5], [S2]), ('B', [1], [S3]), ('A', [0, 2], [11, 12])), 1):
        out += [('Batch', k, suite, algo, idx, seeds, np_, MAX_FES, LOG_INTERVAL, N_LOGPOINT, True), ('reset', k), ('steps', k, n), ('results', k), ('close', k)]
    return out


def _kept(algo, np_, n, n_b1=None, carry=None):
    """A class whose B = 1 view keeps its batch: rebind on the same suite; on another suite the carried slice (offset, length) travels."""
    n_b1 = n if n_b1 is None else n_b1
    out = [('Batch', 1, 'A', algo, [3], [S1], np_, MAX_FES, LOG_INTERVAL, N_LOGPOINT, True), ('reset', 1), ('steps', 1, n_b1), ('read_public', 1, 0),
           ('rebind', 1, [5], [S2]), ('reset', 1), ('steps', 1, n_b1), ('read_public', 1, 0)]
    if carry:
        out += [('read_state', 1, 0)]
    out += [('close', 1), ('Batch', 2, 'B', algo, [1], [S3], np_, MAX_FES, LOG_INTERVAL, N_LOGPOINT, True)]
    if carry:
        out += [('read_state', 2, 0), ('write_state', 2, 0, carry[0], carry[1], [1.0])]
    out += [('reset', 2), ('steps', 2, n_b1), ('read_public', 2, 0),
            ('Batch', 3, 'A', algo, [0, 2], [11, 12], np_, MAX_FES, LOG_INTERVAL, N_LOGPOINT, True), ('reset', 3), ('steps', 3, n), ('results', 3), ('close', 3)]
    return out


EXPECTED = {
    'Random_search': _fresh(4, 100, 19),
    'DEAP_DE': _fresh(8, 50, 39),
    'DEAP_PSO': _fresh(9, 50, 39),
    'DEAP_CMAES': _fresh(10, 50, 40),                  # CMA-ES evaluates nothing at construction: one generation more
    'GL_PSO': _kept(11, 100, 9, carry=(4200, 100)),    # MBX_GLPSO_ST_STAG at NP 100 / D 10, NP counters
    'JDE21': _kept(13, 170, 8),                        # launch until done: the first look at `done` comes after the eighth launch (k = 7)
    'MadDE': _kept(15, 200, 37, carry=(11990, 3)),     # MBX_MADDE_ST_PM at D 10, three probabilities
    'sDMS_PSO': _kept(18, 99, 20),
    'SAHLPSO': _kept(20, 40, 126, n_b1=DONE_AFTER),     # the B = 1 view stops at the first done, run_batch runs the horizon
}


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_host_loop_call_sequence(name, monkeypatch):
    import metabox_amd.optimizer as O
    log, infos, opt, config = _scenario(getattr(O, name), monkeypatch)
    assert log == EXPECTED[name], '\n'.join(map(str, log))
    kept = name not in ('Random_search', 'DEAP_DE', 'DEAP_PSO', 'DEAP_CMAES')
    ids = (1, 1, 2) if kept else (1, 2, 3)
    assert infos == [{'cost': [9., 8., 7. + i], 'fes': 1000 + i} for i in ids]
    assert opt.cost == [9., 8., 7. + ids[2]] and opt.log_index == (2 if kept else None) and opt.log_interval == LOG_INTERVAL
    side = {'DEAP_DE': dict(NP=50, F=0.5, Cr=0.5), 'DEAP_PSO': dict(phi1=2., phi2=2., population_size=50), 'DEAP_CMAES': dict(NP=50)}.get(name, {})
    assert {k: v for k, v in vars(config).items() if k not in ('maxFEs', 'log_interval', 'n_logpoint')} == side


def test_jde21_looks_at_done_every_eighth_launch(monkeypatch):
    """With a budget whose step bound exceeds 8, the loop ends at the first look (k = 7) that finds every instance done."""
    import metabox_amd.suite
    from metabox_amd.optimizer import JDE21
    monkeypatch.setattr(metabox_amd.suite, 'Batch', Recorder)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a: None)
    Recorder.log, Recorder.serial = [], 0
    opt = JDE21(types.SimpleNamespace(maxFEs=20000, log_interval=400, n_logpoint=50))
    assert opt._step_bound(20000) > 16
    opt.run_batch(types.SimpleNamespace(dim=10, name='A'), [0], [1])
    assert [e for e in Recorder.log if e[0] == 'steps'] == [('steps', 1, 8)]


def test_names_the_tests_and_tools_use():
    import metabox_amd.optimizer as O
    assert (O.DEAP_DE._NP, O.GL_PSO._NP, O.JDE21._NP, O.sDMS_PSO._NP, O.SAHLPSO._NP) == (50, 100, 170, 99, 40)
    assert O.MadDE.population_size(10) == 200 and O.MadDE.n_updates(10, 2000) == 37 and O.MadDE(types.SimpleNamespace(log_interval=1)).pm() is None
    assert O.sDMS_PSO.n_updates(2000) == (20, 2) and O.SAHLPSO.n_generations(2000) == 126 and O.JDE21._step_bound(2000) == 21
    for cls in (O.DEAP_DE, O.GL_PSO, O.sDMS_PSO):
        assert callable(cls._n_steps)
    assert callable(O.MadDE._pm_slice) and callable(O.GL_PSO._stag_slice)
