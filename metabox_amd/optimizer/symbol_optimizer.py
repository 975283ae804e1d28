"""SYMBOL backbone optimizer -- host mirror of the reference class (src/optimizer/symbol_optimizer.py:52-200), rollout semantics (``is_train = False``).

One action = one update rule applied for ``skip_step`` = 5 sub-steps to a population of 100: ``update(action, problem)`` takes the rule as
``{'tokens': [63] ints, 'consts': [63] float64}`` -- the heap-ordered expression tree the agent wrote and the value of every constant leaf -- and returns
``(state [9], reward, done)``.  The arithmetic lives in metabox_amd/csrc/mbx_symbol.hpp (the kernel walks the tree itself; no string, no lambdify); this
class is the B = 1 view.  The training branch (the MadDE teacher in lock-step, the imitation reward) is not built.
"""
import numpy as np
import torch

from .._abi import ALGO_SYMBOL
from .learnable_optimizer import Learnable_Optimizer

NP = 100                                # symbol_optimizer.py:66
SKIP_STEP = 5


class Symbol_Optimizer(Learnable_Optimizer):
    def __init__(self, config):
        super().__init__(config)
        config.skip_step = config.test_skip_step = SKIP_STEP
        self.__config = config
        self.NP = NP
        self.is_train = False
        self.fes = None
        self.cost = None
        self.__batch = None
        self.__key = None

    def make_batch(self, suite, problem_idx, seeds, early_stop=True, flags=0):
        from ..suite import Batch
        c = self.__config
        return Batch(suite, ALGO_SYMBOL, problem_idx, seeds, self.NP, c.maxFEs, c.log_interval, c.n_logpoint, early_stop=early_stop, flags=flags)

    def init_population(self, problem):
        if self.is_train:
            raise NotImplementedError('Symbol_Optimizer: the training branch (MadDE teacher, imitation reward) is not built; set is_train = False')
        suite = problem._bound_suite()
        key = (id(suite), problem._suite_index)
        if self.__batch is None or self.__key != key:
            if self.__batch is not None:
                self.__batch.close()
            seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
            self.__batch = self.make_batch(suite, [problem._suite_index], [seed])
            self.__key = key
        state = self.__batch.reset()
        pub = self.__batch.read_public(0)
        self.fes = int(pub[1])
        self.cost = [float(pub[16])]
        return state[0].cpu().numpy().copy()

    def observe(self):
        return self.__batch.state[0].cpu().numpy().copy()

    def update(self, action, problem):
        """action: {'tokens': [63], 'consts': [63], 'skip_step': 5} -> (state [9], reward, is_done)."""
        b = self.__batch
        tokens = np.ascontiguousarray(action['tokens'], dtype=np.int32).reshape(1, 63)
        consts = np.ascontiguousarray(action['consts'], dtype=np.float64).reshape(1, 63)
        state, reward, done, bad = b.symbol_rollout(tokens, consts, int(action.get('skip_step', SKIP_STEP)))
        if int(bad[0].item()):
            raise ValueError('Symbol_Optimizer.update: the expression tree is malformed (include/mbx_layout.h section 22)')
        pub = b.read_public(0)
        self.fes = int(pub[1])
        self.cost = [float(v) for v in pub[16:16 + min(int(pub[3]), self.__config.n_logpoint + 1)]]
        return state[0].cpu().numpy().copy(), float(reward[0].item()), bool(done[0].item())
