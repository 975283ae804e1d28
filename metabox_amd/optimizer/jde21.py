"""JDE21 — self-adaptive DE with a big and a small population (reference: src/optimizer/jde21.py:6-277), a classic baseline of the test harness.

Big population 160 rows with crowding selection, small population 10 rows; one update is a big pass of bNP trials and bNP / 10 small
passes of 10 trials (2 bNP evaluations), and bNP halves up to three times over the budget.  All arithmetic runs in
metabox_amd/csrc/mbx_jde21.hpp, pinned to reference traces by tape replay (tests/test_jde21.py).

``run_batch`` runs many (problem x run) pairs in lock step.  ``run_episode`` is the B = 1 view; it keeps one batch across calls
(``mbx_batch_rebind``) and needs no state hand-over between episodes: the reference's __init_population resets the population sizes,
F and Cr, and gbest is overwritten, so nothing observable carries over from one episode to the next (the reset / copy counters of the
reference are counters only; the state block restarts them at every reset).
"""
import numpy as np
import torch

from .._abi import ALGO_JDE21
from .basic_optimizer import Basic_Optimizer


class JDE21(Basic_Optimizer):
    _NP = 170                 # bNP 160 + sNP 10

    def __init__(self, config):
        super().__init__(config)
        self._config = config
        self.log_interval = config.log_interval
        self.cost = None
        self.log_index = None
        self._batch = None
        self._batch_key = None

    def make_batch(self, suite, problem_idx, seeds, early_stop=True):
        from ..suite import Batch
        c = self._config
        return Batch(suite, ALGO_JDE21, problem_idx, seeds, self._NP, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop)

    @staticmethod
    def _step_bound(max_fes):
        """An upper bound of the updates an episode can take: the longest run has every halving at its earliest, the first update after the
        budget reaches a quarter / a half / three quarters.  Done instances stay frozen, so extra launches change nothing."""
        fes, bnp, steps = 170, 160, 0
        marks = [0.25 * max_fes, 0.5 * max_fes, 0.75 * max_fes]
        while fes < max_fes:
            fes += 2 * bnp
            steps += 1
            if marks and fes >= marks[0] and bnp > 20:
                bnp //= 2
            while marks and fes >= marks[0]:
                marks.pop(0)
        return steps

    def _run(self, batch):
        # the number of updates depends on which halvings an instance meets: launch until every instance is done
        n = self._step_bound(self._config.maxFEs)
        done = None
        for k in range(n):
            _, _, done = batch.step(None)
            if (k % 8 == 7 or k == n - 1) and bool(done.all().item()):
                break
        assert done is None or bool(done.all().item()), 'JDE21: an instance outlived the step bound'

    def run_batch(self, suite, problem_idx, seeds):
        """-> dict of device tensors (cost [B, n_logpoint+1] padded, fes [B], cost_len [B], ...)."""
        batch = self.make_batch(suite, problem_idx, seeds)
        batch.reset()
        self._run(batch)
        res = batch.results()
        torch.cuda.synchronize()
        batch.close()
        return res

    def run_episode(self, problem):
        problem.reset()
        suite = problem._bound_suite()
        seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
        if self._batch is not None and self._batch_key == id(suite):
            self._batch.rebind([problem._suite_index], [seed])
        else:
            if self._batch is not None:
                self._batch.close()
            self._batch = self.make_batch(suite, [problem._suite_index], [seed])
            self._batch_key = id(suite)
        self._batch.reset()
        self._run(self._batch)
        sc = self._batch.read_public(0)
        n = int(sc[3])
        self.log_index = int(sc[2])
        self.cost = [float(v) for v in sc[16:16 + n]]
        return {'cost': self.cost, 'fes': int(sc[1])}
