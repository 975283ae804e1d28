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
from .._abi import ALGO_SDMSPSO
from .basic_optimizer import Batched_Baseline


class sDMS_PSO(Batched_Baseline):
    """``make_batch`` accepts `early_stop` for the callers' sake; it has no effect: the reference evaluates `done` only after its last update."""
    _ALGO = ALGO_SDMSPSO
    _NP = 99
    _LP = 10

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
