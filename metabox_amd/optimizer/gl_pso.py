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
from .._abi import ALGO_GLPSO
from .basic_optimizer import Batched_Baseline


class GL_PSO(Batched_Baseline):
    _ALGO = ALGO_GLPSO
    _NP = 100

    def _n_steps(self):
        # 2 NP FEs per generation after the 2 NP of init_population; done instances stay frozen
        return max(0, -(-(self._config.maxFEs - 2 * self._NP) // (2 * self._NP)))

    def _stag_slice(self):
        NP, D = self._NP, self._batch.cfg.dim
        o = 4 * NP * D + 2 * NP                     # MBX_GLPSO_ST_STAG (include/mbx_layout.h §11)
        return slice(o, o + NP)

    _carry_slice = _stag_slice
