"""L2L backbone optimizer — host mirror of the reference class (src/optimizer/l2l_optimizer.py:15-53).

One step = one point: ``update(x_raw, problem)`` maps the LSTM's raw output into the box with a sigmoid, evaluates it once and returns
``(y, 0, done)`` with y = f(x) - optimum (f(x) where the optimum is unknown).  ``cost`` grows by one entry (the best so far) per step; the episode
ends at y <= 1e-8 or after 100 steps -- the reference's literal, maxFEs plays no part.  The arithmetic lives in metabox_amd/csrc/mbx_l2l.hpp
(``k_l2l_step``); this class is the B = 1 view, the agent runs the LSTM on the host as the reference's does.
"""
import numpy as np
import torch

from .._abi import ALGO_L2L
from .learnable_optimizer import Learnable_Optimizer

T = 100                                 # steps per episode (l2l_optimizer.py:51)


class L2L_Optimizer(Learnable_Optimizer):
    def __init__(self, config):
        super().__init__(config)
        self.__config = config
        self.fes = None
        self.cost = None
        self.__batch = None
        self.__key = None

    def make_batch(self, suite, problem_idx, seeds, early_stop=True, flags=0):
        from ..suite import Batch
        c = self.__config
        return Batch(suite, ALGO_L2L, problem_idx, seeds, 1, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop, flags=flags)

    def init_population(self, problem):
        suite = problem._bound_suite()
        key = (id(suite), problem._suite_index)
        if self.__batch is None or self.__key != key:
            if self.__batch is not None:
                self.__batch.close()
            seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
            self.__batch = self.make_batch(suite, [problem._suite_index], [seed])
            self.__key = key
        self.__batch.reset()
        self.fes = 0
        self.cost = []
        return None

    def update(self, action, problem):
        """action: x_raw [dim], the LSTM's output (numpy or tensor) -> (y, 0, is_done)."""
        b = self.__batch
        x = action.detach().cpu().numpy() if torch.is_tensor(action) else np.asarray(action)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(1, -1)
        if x.shape[1] != b.cfg.dim:
            raise ValueError(f'L2L takes x_raw of {b.cfg.dim} values, not {x.shape[1]}')
        state, _, done = b.step(torch.from_numpy(x).to(b.device))
        pub = b.read_public(0)
        self.fes = int(pub[1])
        self.cost.append(float(pub[0]))
        return float(state[0, 0].item()), 0, bool(done[0].item())
