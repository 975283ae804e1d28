"""MadDE — DE with three mutation strategies, a success-history memory, an archive and a linearly shrinking population (reference:
src/optimizer/madde.py:6-284), a classic baseline of the test harness.

The population starts at 2 D^2 rows (200 at D = 10, 3200 at D = 40) and shrinks to 4; one update makes and evaluates one trial per live
row.  All arithmetic runs in metabox_amd/csrc/mbx_madde.hpp, pinned to reference traces one update at a time (tests/test_madde.py): the
memory and the strategy probabilities are arithmetic in the cost values, so a whole episode cannot be replayed against the reference.
The kernels sort by (cost, row), numpy's kind='stable' order; the reference's introsort is not reproducible among equal costs.

``run_batch`` runs many (problem x run) pairs in lock step; every instance starts with the strategy probabilities pm = 1/3, because the
instances of a batch have no order.  ``run_episode`` is the B = 1 view and, like the reference, keeps pm from one episode to the next:
the reference sets pm in __init__ only (:14), so a second episode on the same object starts with the pm the first one ended with.  It
keeps one batch across calls (``mbx_batch_rebind``; for a problem of another suite pm is copied into the new batch).  Everything else is
reset by __init_population.  The batched ``Tester`` tables therefore differ from the reference's in one respect: the reference threads a
single object through its 51 runs x problems, while every instance of an independent-instance table starts at pm = 1/3.
"""
import numpy as np
import torch

from .._abi import ALGO_MADDE
from .basic_optimizer import Basic_Optimizer


class MadDE(Basic_Optimizer):
    _NMIN = 4

    def __init__(self, config):
        super().__init__(config)
        self._config = config
        self.log_interval = config.log_interval
        self.cost = None
        self.log_index = None
        self._batch = None
        self._batch_key = None

    @staticmethod
    def population_size(dim):
        return 2 * dim * dim

    def make_batch(self, suite, problem_idx, seeds, early_stop=True):
        from ..suite import Batch
        c = self._config
        return Batch(suite, ALGO_MADDE, problem_idx, seeds, self.population_size(suite.dim), c.maxFEs, c.log_interval, c.n_logpoint,
                     early_stop=early_stop)

    @classmethod
    def n_updates(cls, dim, max_fes):
        """The updates of an episode that runs to the budget: NP is a function of the evaluations spent, not of the costs (:256)."""
        n0 = cls.population_size(dim)
        fes, n, steps = n0, n0, 0
        while fes < max_fes:
            fes += n
            n = int(np.round(n0 + (cls._NMIN - n0) * fes / max_fes))
            steps += 1
        return steps

    def _run(self, batch):
        # done instances stay frozen, so the launches past an early stop change nothing
        for _ in range(self.n_updates(batch.cfg.dim, self._config.maxFEs)):
            batch.step(None)

    def run_batch(self, suite, problem_idx, seeds):
        """-> dict of device tensors (cost [B, n_logpoint+1] padded, fes [B], cost_len [B], ...)."""
        batch = self.make_batch(suite, problem_idx, seeds)
        batch.reset()
        self._run(batch)
        res = batch.results()
        torch.cuda.synchronize()
        batch.close()
        return res

    def _pm_slice(self):
        D = self._batch.cfg.dim
        n0 = self.population_size(D)
        o = 3 * n0 * D + 6 * n0 + int(2.3 * n0) * D + 20 * D      # MBX_MADDE_ST_PM (include/mbx_layout.h §13)
        return slice(o, o + 3)

    def run_episode(self, problem):
        problem.reset()
        suite = problem._bound_suite()
        seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
        if self._batch is not None and self._batch_key == id(suite):
            self._batch.rebind([problem._suite_index], [seed])
        else:
            pm = None
            if self._batch is not None:
                pm = self._batch.read_state(0)[self._pm_slice()].copy()
                self._batch.close()
            self._batch = self.make_batch(suite, [problem._suite_index], [seed])
            self._batch_key = id(suite)
            if pm is not None:
                blk = self._batch.read_state(0)
                blk[self._pm_slice()] = pm
                self._batch.write_state(0, blk)
        self._batch.reset()
        self._run(self._batch)
        sc = self._batch.read_public(0)
        n = int(sc[3])
        self.log_index = int(sc[2])
        self.cost = [float(v) for v in sc[16:16 + n]]
        return {'cost': self.cost, 'fes': int(sc[1])}

    def pm(self):
        """The strategy probabilities the next episode of the B = 1 view starts with."""
        return None if self._batch is None else self._batch.read_state(0)[self._pm_slice()].copy()
