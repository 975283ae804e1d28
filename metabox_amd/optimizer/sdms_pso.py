"""sDMS_PSO — dynamic multi-swarm PSO with self-adapted inertia weights (reference: src/optimizer/sdms_pso.py:7-243), a classic baseline
of the test harness.

NP = 99 particles in 33 sub-swarms of 3, c1 = c2 = 1.49445, velocity cap 0.1 (ub - lb).  While fes < 0.95 maxFEs at the start of a
generation, a generation is ten updates towards pbest and the sub-swarm's lbest, with one inertia weight per sub-swarm and update; the
weight of the most successful sub-swarm enters a parameter set of 8 and every tenth generation the swarm is regrouped at random.
Afterwards the swarm follows gbest until fes >= maxFEs.  There is no early stop: the horizon depends on maxFEs alone (``_n_steps``),
and fes overshoots maxFEs.  All arithmetic runs in metabox_amd/csrc/mbx_sdmspso.hpp, pinned to reference traces by tape replay
(tests/test_sdmspso.py).

The reference's quasi-Newton refinement belongs to generation 100 only and fails there in the reference itself; a maxFEs whose local phase
would reach it (above 103 272) is rejected when the batch is created, and so is maxFEs <= 99.

``run_batch`` runs many (problem x run) pairs in lock step.  ``run_episode`` is the B = 1 view; __reset clears everything, so nothing
carries over from one episode to the next.
"""
import numpy as np
import torch

from .._abi import ALGO_SDMSPSO
from .basic_optimizer import Basic_Optimizer


class sDMS_PSO(Basic_Optimizer):
    _NP = 99
    _LP = 10

    def __init__(self, config):
        super().__init__(config)
        self._config = config
        self.log_interval = config.log_interval
        self.cost = None
        self.log_index = None
        self._batch = None
        self._batch_key = None

    def make_batch(self, suite, problem_idx, seeds, early_stop=True):
        """`early_stop` is accepted for the callers' sake and has no effect: the reference evaluates `done` only after its last update."""
        from ..suite import Batch
        c = self._config
        return Batch(suite, ALGO_SDMSPSO, problem_idx, seeds, self._NP, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop)

    @classmethod
    def n_updates(cls, max_fes):
        """(updates, local generations) of an episode: run_episode's own loop (:209-230) on integers, comparisons as the reference makes them."""
        fes, steps, gens = cls._NP, 0, 0
        while fes < max_fes:
            while fes < 0.95 * max_fes:
                gens += 1
                steps += cls._LP
                fes += cls._LP * cls._NP
            while fes < max_fes:
                steps += 1
                fes += cls._NP
        return steps, gens

    def _n_steps(self):
        return self.n_updates(self._config.maxFEs)[0]

    def run_batch(self, suite, problem_idx, seeds):
        """-> dict of device tensors (cost [B, n_logpoint+1] padded, fes [B], cost_len [B], ...)."""
        batch = self.make_batch(suite, problem_idx, seeds)
        batch.reset()
        for _ in range(self._n_steps()):
            batch.step(None)
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
        for _ in range(self._n_steps()):
            self._batch.step(None)
        sc = self._batch.read_public(0)
        n = int(sc[3])
        self.log_index = int(sc[2])
        self.cost = [float(v) for v in sc[16:16 + n]]
        return {'cost': self.cost, 'fes': int(sc[1])}
