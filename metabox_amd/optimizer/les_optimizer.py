"""LES backbone optimizer — host mirror of the reference class (src/optimizer/les_optimizer.py:42-180).

A learned evolution strategy: NP = 16 samples of a diagonal Gaussian per generation; a 68-parameter attention module weighs the parents by their
costs, a 178-parameter MLP sets the learning rates of mu and sigma per coordinate.  ``update`` is the WHOLE episode in one call (or ``skip_step``
generations of it) and takes the two parameter vectors as its action.  The arithmetic lives in metabox_amd/csrc/mbx_les.hpp; this class is the
B = 1 view of the resident kernel.  ``cost`` can hold more than n_logpoint + 1 entries, as the reference's list can (include/mbx_layout.h §18).
"""
import numpy as np
import torch

from .._abi import ALGO_LES
from .learnable_optimizer import Learnable_Optimizer

N_ATTN, N_PARAM = 68, 246
_CHUNK = 256                            # generations per launch of the budget route


class LES_Optimizer(Learnable_Optimizer):
    def __init__(self, config):
        super().__init__(config)
        config.NP = 16                  # les_optimizer.py:53
        self.__config = config
        self.NP = 16
        self.max_fes = config.maxFEs
        self.sigma_ratio = 0.2
        self.FEs = None
        self.cost = None
        self.log_index = None
        self.log_interval = config.log_interval
        self.evolution_info = None
        self.__batch = None
        self.__seed = None

    @property
    def fes(self):
        return self.FEs

    def make_batch(self, suite, problem_idx, seeds, early_stop=True, flags=0):
        from ..suite import Batch
        c = self.__config
        return Batch(suite, ALGO_LES, problem_idx, seeds, 16, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop, flags=flags)

    def __sync_public(self):
        b = self.__batch
        D = b.cfg.dim
        st = b.read_state(0)
        o = 16 * D + 16
        sc = st[o + 8 * D + 16 * D + 16 + 2 * D:]
        self.FEs = int(sc[1])
        self.log_index = int(sc[2])
        self.cost = [float(v) for v in sc[16:16 + int(sc[3])]]
        self.evolution_info = {'parents': st[:16 * D].reshape(16, D).copy(), 'parents_cost': st[16 * D:o].copy(), 'generation_counter': int(sc[6]),
                               'gbest': float(sc[0]), 'Pc': st[o + 2 * D:o + 5 * D].reshape(3, D).copy(), 'Ps': st[o + 5 * D:o + 8 * D].reshape(3, D).copy(),
                               'mu': st[o:o + D].copy(), 'sigma': st[o + D:o + 2 * D].copy()}

    def init_population(self, problem):
        suite = problem._bound_suite()
        key = (id(suite), problem._suite_index)
        if self.__batch is None or self.__seed != key:
            if self.__batch is not None:
                self.__batch.close()
            seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
            self.__batch = self.make_batch(suite, [problem._suite_index], [seed])
            self.__seed = key
        self.__batch.reset()
        torch.cuda.synchronize()
        self.__sync_public()
        return None

    def update(self, action, problem):
        """action: the reference's dict -- 'attn' (68 values), 'mlp' (178), optional 'skip_step' -> (gbest, reward, is_end, {})."""
        params = np.concatenate([np.asarray(action['attn'], dtype=np.float64).ravel(), np.asarray(action['mlp'], dtype=np.float64).ravel()])
        if params.shape != (N_PARAM,):
            raise ValueError(f"LES takes 68 attention and 178 MLP parameters, not {params.shape[0]} in all")
        b = self.__batch
        b.les_set_params(params)
        skip = action.get('skip_step')
        if skip is not None:
            _, reward, done = b.les_rollout(int(skip), skip=True)
        else:
            while True:
                _, reward, done = b.les_rollout(_CHUNK)
                if bool(done[0].item()):
                    break
        torch.cuda.synchronize()
        self.__sync_public()
        return self.evolution_info['gbest'], float(reward[0].item()), bool(done[0].item()), {}
