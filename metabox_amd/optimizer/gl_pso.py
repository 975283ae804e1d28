"""GL_PSO — PSO with genetic-learning exemplars (reference: src/optimizer/gl_pso.py:5-177), a classic baseline of the test harness.

NP = 100, pm = 0.01, nsel = 10, w = 0.7298, c1 = 1.49618, sg = 7, velocity cap 0.2 (ub - lb).  init_population and every update()
evaluate two populations (the swarm and the NP bred exemplars).  All arithmetic runs in metabox_amd/csrc/mbx_glpso.hpp, pinned to
reference traces by tape replay (tests/test_glpso.py).

``run_batch`` runs many (problem x run) pairs in lock step, each instance starting with zero stagnation counters.  ``run_episode`` is
the B = 1 view and, like the reference, keeps its ``exemplar_stag`` from one episode to the next: the reference's counters live on the
optimizer object and init_population never resets them (:19), so a second episode starts where the first left them.  It keeps one
batch across calls (``mbx_batch_rebind``; for a problem of another suite the counters are copied into the new batch).  The batched
``Tester`` tables therefore differ from the reference's in one respect: the reference threads a single object through its 51 runs x
problems one after the other, while every instance of an independent-instance table starts at zero counters.
"""
import numpy as np
import torch

from .._abi import ALGO_GLPSO
from .basic_optimizer import Basic_Optimizer


class GL_PSO(Basic_Optimizer):
    _NP = 100

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
        return Batch(suite, ALGO_GLPSO, problem_idx, seeds, self._NP, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop)

    def _n_steps(self):
        # 2 NP FEs per generation after the 2 NP of init_population; done instances stay frozen
        return max(0, -(-(self._config.maxFEs - 2 * self._NP) // (2 * self._NP)))

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

    def _stag_slice(self):
        NP, D = self._NP, self._batch.cfg.dim
        o = 4 * NP * D + 2 * NP                     # MBX_GLPSO_ST_STAG (include/mbx_layout.h §11)
        return slice(o, o + NP)

    def run_episode(self, problem):
        problem.reset()
        suite = problem._bound_suite()
        seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
        if self._batch is not None and self._batch_key == id(suite):
            self._batch.rebind([problem._suite_index], [seed])
        else:
            stag = None
            if self._batch is not None:
                stag = self._batch.read_state(0)[self._stag_slice()].copy()
                self._batch.close()
            self._batch = self.make_batch(suite, [problem._suite_index], [seed])
            self._batch_key = id(suite)
            if stag is not None and len(stag) == self._NP:
                blk = self._batch.read_state(0)
                blk[self._stag_slice()] = stag
                self._batch.write_state(0, blk)
        self._batch.reset()
        for _ in range(self._n_steps()):
            self._batch.step(None)
        sc = self._batch.read_public(0)
        n = int(sc[3])
        self.log_index = int(sc[2])
        self.cost = [float(v) for v in sc[16:16 + n]]
        return {'cost': self.cost, 'fes': int(sc[1])}
