"""NRLPSO backbone optimizer — host mirror of the reference class (src/optimizer/nrlpso_optimizer.py:7-296).

NP = 100, k = 5 neighbours, velocity cap 0.1 (ub - lb), inertia weight from a logistic map once per sweep.  One env step moves ONE
particle with the velocity rule the action names (0 exploration, 1 exploitation, 2 convergence, 3 jumping-out); the reward in
{2, 1, 0, -2} combines "cost improved" with "the particle's normalised mean distance to the swarm grew"; a particle that fails to improve
on its pbest cost twice fires the neighbourhood mutation (two more evaluations); the state is the action the next particle took on its
previous turn.  The arithmetic lives in metabox_amd/csrc/mbx_nrlpso.hpp.  As in the reference, init_population puts the pointer back to 0.
"""
import numpy as np
import torch

from .._abi import ALGO_NRLPSO
from .learnable_optimizer import Learnable_Optimizer


class NRLPSO_Optimizer(Learnable_Optimizer):
    def __init__(self, config):
        super().__init__(config)
        config.NP = 100                 # nrlpso_optimizer.py:12-20
        config.k = 5
        self.__config = config
        self.fes = None
        self.cost = None
        self.log_index = None
        self.log_interval = config.log_interval
        self.__batch = None
        self.__seed = None

    def make_batch(self, suite, problem_idx, seeds, early_stop=True, flags=0):
        from ..suite import Batch
        c = self.__config
        return Batch(suite, ALGO_NRLPSO, problem_idx, seeds, c.NP, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop, flags=flags)

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
        state, reward, done = self.__batch.step(torch.tensor([a], dtype=torch.int32).cuda())
        torch.cuda.synchronize()
        self.__sync_public()
        return int(state[0, 0].item()), float(reward[0].item()), bool(done[0].item())
