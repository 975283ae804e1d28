"""SAHLPSO — self-adaptive PSO with two learning strategies (reference: src/optimizer/sahlpso.py:6-161), a classic baseline of the test
harness.

40 particles shrinking linearly to 4 by their initial rank; 8 fixed exploration particles learn from the better of two random live
particles, the others from one of the best 20 % blended with gBest; the crossover rate and the history depth are picked per move with
probabilities re-estimated every 5 generations; a failed move redraws the particle's inertia weight.  The particles of a generation move
one after the other, each seeing the one before it, and the episode may end after any move (maxFEs, or gBest_cost <= 1e-8 on problems
with a known optimum).  One ``step`` of the batch is one such pass in one kernel launch.  All arithmetic runs in
metabox_amd/csrc/mbx_sahlpso.hpp, whose header lists the reference's own behaviour that is kept; it is pinned to reference traces by tape
replay (tests/test_sahlpso.py).

``run_batch`` runs many (problem x run) pairs in lock step for ``n_generations(maxFEs)`` passes, the horizon of an episode that never stops
early; instances that do are frozen by the kernel.  ``run_episode`` is the B = 1 view; the reset clears everything, so nothing carries over
from one episode to the next.
"""
import numpy as np
import torch

from .._abi import ALGO_SAHLPSO
from .basic_optimizer import Basic_Optimizer


class SAHLPSO(Basic_Optimizer):
    _NP = 40

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
        return Batch(suite, ALGO_SAHLPSO, problem_idx, seeds, self._NP, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop)

    @classmethod
    def n_generations(cls, max_fes):
        """Passes of an episode that runs to its budget: the reference's outer loop (:48-155) on integers, fes += NP per generation and the
        same round(); the last pass may be cut short by the budget."""
        fes, NP, gens = cls._NP, cls._NP, 0
        while fes < max_fes and NP >= 4:
            gens += 1
            fes += NP
            if fes >= max_fes:
                break
            NP_ = round((4 - cls._NP) * fes / max_fes + cls._NP)
            if NP_ < NP:
                NP = NP_
        return gens

    def run_batch(self, suite, problem_idx, seeds):
        """-> dict of device tensors (cost [B, n_logpoint+1] padded, fes [B], cost_len [B], ...)."""
        batch = self.make_batch(suite, problem_idx, seeds)
        batch.reset()
        for _ in range(self.n_generations(self._config.maxFEs)):
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
        for _ in range(self.n_generations(self._config.maxFEs)):
            _, _, done = self._batch.step(None)
            if bool(done[0].item()):
                break
        sc = self._batch.read_public(0)
        n = int(sc[3])
        self.log_index = int(sc[2])
        self.cost = [float(v) for v in sc[16:16 + n]]
        return {'cost': self.cost, 'fes': int(sc[1])}
