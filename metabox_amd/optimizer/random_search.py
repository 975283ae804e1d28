"""Random_search — NP = 100 uniform samples per step, the normaliser of the AEI metric
(reference: src/optimizer/random_search.py:5-58; baseline use src/logger.py:94-120).  The sampling and evaluation run
in the batched kernel (metabox_amd/csrc/mbx_rs.hpp); ``run_episode`` is the B = 1 view, ``run_batch`` steps many
(problem x run) pairs at once."""
from .._abi import ALGO_RANDOM_SEARCH
from .basic_optimizer import Batched_Baseline


class Random_search(Batched_Baseline):
    _ALGO = ALGO_RANDOM_SEARCH
    _NP = 100
    _KEEPS_BATCH = False

    def _n_steps(self):
        return -(-(self._config.maxFEs - self._NP) // self._NP)
