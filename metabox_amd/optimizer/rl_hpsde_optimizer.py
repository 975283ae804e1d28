"""RL-HPSDE backbone optimizer — host mirror of the reference class (src/optimizer/rl_hpsde_optimizer.py:101-287).

SHADE-style DE with a success-history memory of int(0.5 dim) entries and linear population size reduction from 18 dim rows towards 4.  The
action in 0..3 picks the mutation (action & 1: cur_to_rand_1 / cur_to_best_1) and the law of F (action >> 1: Cauchy / Levy); the reward is
the share of improved rows; the state in 0..3 comes from a progressive random walk of 201 points that is drawn, evaluated and billed after
the reset and after every update (fitness-distance correlation bit + 2 x information-entropy bit).  The arithmetic lives in
metabox_amd/csrc/mbx_rlhpsde.hpp; this class is the B = 1 protocol view.
"""
import numpy as np
import torch

from .._abi import ALGO_RLHPSDE
from .learnable_optimizer import Learnable_Optimizer


class RL_HPSDE_Optimizer(Learnable_Optimizer):
    def __init__(self, config):
        super().__init__(config)
        config.F = 0.5                  # rl_hpsde_optimizer.py:104-110
        config.Cr = 0.5
        config.NP_max = 18 * config.dim
        config.NP_min = 4
        config.Hm = 0.5
        config.rw_steps = 200
        config.step_size = 10
        self.__config = config
        self.fes = None
        self.cost = None
        self.log_index = None
        self.log_interval = config.log_interval
        self.__batch = None
        self.__seed = None

    @staticmethod
    def schedule(dim, max_fes):
        """(fes after every update, population size after every update) of an episode that runs to its budget: integers only.  Every update
        bills its NP trials, is cut to max(int(N0 + (4 - N0) fes / maxFEs), 1) rows, tests the budget, and then bills the 201 points of its walk."""
        n0 = 18 * dim
        n, fes, out, done = n0, n0 + 201, [], False
        while not done:
            fes += n
            n = min(n, max(int(n0 + (4 - n0) * fes / max_fes), 1))
            done = fes >= max_fes
            fes += 201
            out.append((fes, n))
        return out

    def make_batch(self, suite, problem_idx, seeds, early_stop=True, flags=0):
        from ..suite import Batch
        c = self.__config
        return Batch(suite, ALGO_RLHPSDE, problem_idx, seeds, c.NP_max, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop, flags=flags)

    def __sync_public(self):
        sc = self.__batch.read_public(0)
        self.fes = int(sc[1])
        self.log_index = int(sc[2])
        self.cost = [float(v) for v in sc[16:16 + int(sc[3])]]

    def init_population(self, problem):
        suite = problem._bound_suite()
        key = (id(suite), problem._suite_index)
        if self.__batch is None or self.__seed != key:
            if self.__batch is not None:
                self.__batch.close()
            seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
            self.__batch = self.make_batch(suite, [problem._suite_index], [seed])
            self.__seed = key
        state = self.__batch.reset()
        torch.cuda.synchronize()
        self.__sync_public()
        return int(state[0, 0].item())

    def update(self, action, problem):
        a = int(np.asarray(action).reshape(-1)[0])
        if not 0 <= a <= 3:
            raise ValueError(f'action error: {a}')
        state, reward, done = self.__batch.step(torch.tensor([a], dtype=torch.int32).cuda())
        torch.cuda.synchronize()
        self.__sync_public()
        return int(state[0, 0].item()), float(reward[0].item()), bool(done[0].item())
