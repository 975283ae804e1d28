"""DEDQN backbone optimizer — host mirror of the reference class (src/optimizer/dedqn_optimizer.py:103-206).

NP = 100, F = 0.5, Cr = 0.5, rwsteps = NP.  One env step builds ONE trial vector for the row under the pointer with the DE operator the
action names (0 rand_1, 1 cur_to_rand_1, 2 best_2), selects, and re-evaluates the whole population for the four landscape features of
the next state (fdc, rie, acf, nop); a step bills 2 NP evaluations.  The arithmetic lives in metabox_amd/csrc/mbx_dedqn.hpp.  As in the
reference, the pointer is set when the optimizer object is created and is NOT reset by init_population.
"""
import numpy as np
import torch

from .._abi import ALGO_DEDQN
from .learnable_optimizer import Learnable_Optimizer

NSCALAR, SC_POINTER = 16, 10            # include/mbx_layout.h: MBX_NSCALAR, MBX_SC_DEDQN_POINTER


class DEDQN_Optimizer(Learnable_Optimizer):
    def __init__(self, config):
        super().__init__(config)
        config.NP = 100                 # dedqn_optimizer.py:106-109
        config.F = 0.5
        config.Cr = 0.5
        config.rwsteps = config.NP
        self.__config = config
        self.fes = None
        self.cost = None
        self.log_index = None
        self.log_interval = config.log_interval
        self.__batch = None
        self.__seed = None

    def make_batch(self, suite, problem_idx, seeds, early_stop=True):
        from ..suite import Batch
        c = self.__config
        return Batch(suite, ALGO_DEDQN, problem_idx, seeds, c.NP, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop)

    def __sync_public(self):
        sc = self.__batch.read_public(0)
        self.fes = int(sc[1])
        self.log_index = int(sc[2])
        self.cost = [float(v) for v in sc[16:16 + int(sc[3])]]

    def init_population(self, problem):
        suite = problem._bound_suite()
        key = (id(suite), problem._suite_index)
        if self.__batch is None or self.__seed != key:           # same problem again: keep the batch, and with it the pointer
            pointer = 0.
            if self.__batch is not None:
                pointer = self.__batch.read_public(0)[SC_POINTER]   # the object's pointer moves on to the next problem
                self.__batch.close()
            seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
            self.__batch = self.make_batch(suite, [problem._suite_index], [seed])
            if pointer:
                block = self.__batch.read_state(0)               # the block ends with scalars[NSCALAR] | cost_curve[n_logpoint + 1]
                scalars = len(block) - (NSCALAR + self.__config.n_logpoint + 1)
                block[scalars + SC_POINTER] = pointer
                self.__batch.write_state(0, block)
            self.__seed = key
        state = self.__batch.reset()
        torch.cuda.synchronize()
        self.__sync_public()
        return state[0].cpu().numpy().copy()

    def update(self, action, problem):
        a = int(np.asarray(action).reshape(-1)[0])
        if a not in (0, 1, 2):
            raise ValueError(f'action error: {a}')               # dedqn_optimizer.py:167-168
        state, reward, done = self.__batch.step(torch.tensor([a], dtype=torch.int32).cuda())
        torch.cuda.synchronize()
        self.__sync_public()
        return state[0].cpu().numpy().copy(), float(reward[0].item()), bool(done[0].item())
