"""NL_SHADE_LBC — SHADE-style DE with a rank-weighted r2, a binomial and an exponential crossover side by side, an archive and a non-linearly
shrinking population (reference: src/optimizer/nl_shade_lbc.py:11-285), a classic baseline of the test harness.

The population starts at 23 D rows (230 at D = 10, 920 at D = 40) and collapses early: at D = 10 / 20 000 FEs an episode is 919 updates, NP is at
most 8 from update 386 and 4 from update 687.  All arithmetic runs in metabox_amd/csrc/mbx_nlshade.hpp, pinned to reference traces one update at a
time (tests/test_nlshade.py).  The population size is a function of (dim, maxFEs) alone: ``n_schedule`` is the table the library builds for the
kernel, in numpy.  ``_run`` drives the episode through ``mbx_nlshade_run`` (n updates per launch) in a few launches, because most updates move a
handful of rows and one launch per update would be all launch latency; the launches are bit-identical to single-update ones.

``run_batch`` runs many (problem x run) pairs in lock step; every instance starts at pb = 0.4 and NA = 23 D, because the instances of a batch have
no order.  ``run_episode`` is the B = 1 view and, like the reference, keeps (pb, NA) from one episode to the next: the reference sets them in
__init__ only (:14, :24), so a second episode on the same object starts with pb = 0.2 + 0.1 FEs / MaxFEs of the first one's end (about 0.3) and with
the NA the first one ended with, which is 4: its archive never reaches 25 rows and is never used (:206).  pa is reset at the start of every update
(:168) and is not carried.  It keeps one batch across calls (``mbx_batch_rebind``; for a problem of another suite the pair is copied into the new
batch).  The batched ``Tester`` tables therefore differ from the reference's in one respect: the reference threads a single object through its
51 runs x problems, so only its very first episode uses the archive in the mutation, while every instance of an independent-instance table starts
at pb = 0.4, NA = 23 D and does.
"""
import numpy as np

from .._abi import ALGO_NLSHADE
from .basic_optimizer import Batched_Baseline


class NL_SHADE_LBC(Batched_Baseline):
    _ALGO = ALGO_NLSHADE
    _NMIN = 4
    _CHUNK = 128          # updates per launch

    @staticmethod
    def population_size(dim):
        return 23 * dim

    @classmethod
    def n_schedule(cls, dim, max_fes, dtype=np.float64):
        """N after the reset and after every update of an episode that runs to the budget (:135-147): N = round(Nmax + (4 - Nmax) x^(1 - x)),
        x = FEs / MaxFEs; FEs advances by the live population, which only ever shrinks.  The live population after update g is
        ``np.minimum.accumulate(n_schedule(...))[g]``."""
        n0 = cls.population_size(dim)
        out, fes, live = [n0], n0, n0
        while fes < max_fes:
            fes += live
            x = dtype(fes) / dtype(max_fes)
            n = int(np.round(dtype(n0) + dtype(cls._NMIN - n0) * np.power(x, dtype(1) - x)))
            live = min(live, n)
            out.append(n)
        return np.array(out, dtype=np.int64)

    @classmethod
    def n_updates(cls, dim, max_fes):
        """The updates of an episode that runs to the budget."""
        return len(cls.n_schedule(dim, max_fes)) - 1

    def _run(self, batch, single=False):
        # done instances stay frozen, so the launches past an early stop change nothing
        left = self.n_updates(batch.cfg.dim, self._config.maxFEs)
        while left > 0:
            n = min(self._CHUNK, left)
            batch.nlshade_run(n)
            left -= n

    def _carry_slice(self):
        D = self._batch.cfg.dim
        n0 = self.population_size(D)
        o = 4 * n0 * D + 11 * n0 + 40 * D                         # MBX_NLSHADE_ST_CARRY (include/mbx_layout.h §20)
        return slice(o, o + 2)

    def carried(self):
        """(pb, NA) the next episode of the B = 1 view starts with."""
        return None if self._batch is None else self._batch.read_state(0)[self._carry_slice()].copy()
