"""JDE21 — self-adaptive DE with a big and a small population (reference: src/optimizer/jde21.py:6-277), a classic baseline of the test harness.

Big population 160 rows with crowding selection, small population 10 rows; one update is a big pass of bNP trials and bNP / 10 small
passes of 10 trials (2 bNP evaluations), and bNP halves up to three times over the budget.  All arithmetic runs in
metabox_amd/csrc/mbx_jde21.hpp, pinned to reference traces by tape replay (tests/test_jde21.py).

``run_batch`` runs many (problem x run) pairs in lock step.  ``run_episode`` is the B = 1 view; it keeps one batch across calls
(``mbx_batch_rebind``) and needs no state hand-over between episodes: the reference's __init_population resets the population sizes,
F and Cr, and gbest is overwritten, so nothing observable carries over from one episode to the next (the reset / copy counters of the
reference are counters only; the state block restarts them at every reset).
"""
from .._abi import ALGO_JDE21
from .basic_optimizer import Batched_Baseline


class JDE21(Batched_Baseline):
    _ALGO = ALGO_JDE21
    _NP = 170                 # bNP 160 + sNP 10

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

    def _run(self, batch, single=False):
        # the number of updates depends on which halvings an instance meets: launch until every instance is done
        n = self._step_bound(self._config.maxFEs)
        done = None
        for k in range(n):
            _, _, done = batch.step(None)
            if (k % 8 == 7 or k == n - 1) and bool(done.all().item()):
                break
        assert done is None or bool(done.all().item()), 'JDE21: an instance outlived the step bound'
