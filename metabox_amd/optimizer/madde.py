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

from .._abi import ALGO_MADDE
from .basic_optimizer import Batched_Baseline


class MadDE(Batched_Baseline):
    _ALGO = ALGO_MADDE
    _NMIN = 4

    @staticmethod
    def population_size(dim):
        return 2 * dim * dim

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

    def _run(self, batch, single=False):
        # done instances stay frozen, so the launches past an early stop change nothing
        for _ in range(self.n_updates(batch.cfg.dim, self._config.maxFEs)):
            batch.step(None)

    def _pm_slice(self):
        D = self._batch.cfg.dim
        n0 = self.population_size(D)
        o = 3 * n0 * D + 6 * n0 + int(2.3 * n0) * D + 20 * D      # MBX_MADDE_ST_PM (include/mbx_layout.h §13)
        return slice(o, o + 3)

    _carry_slice = _pm_slice

    def pm(self):
        """The strategy probabilities the next episode of the B = 1 view starts with."""
        return None if self._batch is None else self._batch.read_state(0)[self._pm_slice()].copy()
