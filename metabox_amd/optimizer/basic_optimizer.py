"""Classic (non-learnable) optimizers implement ``run_episode(problem) -> {'cost': [...], 'fes': int}``
(reference protocol: src/optimizer/basic_optimizer.py:10-15)."""
import numpy as np
import torch


class Basic_Optimizer:
    def __init__(self, config):
        self.__config = config

    def run_episode(self, problem):
        raise NotImplementedError('run_episode(problem) must be provided by the optimizer')


class Batched_Baseline(Basic_Optimizer):
    """The host loop of an agent-less algorithm whose arithmetic runs in the batched kernels: ``run_batch`` steps many (problem x run) pairs in
    lock step, ``run_episode`` is the B = 1 view.  A subclass declares ``_ALGO``, its population (``_NP``, or ``population_size(dim)``) and its
    step loop (``_n_steps()`` for a fixed count, or ``_run``), and optionally

    ``_KEEPS_BATCH = False``  the B = 1 view builds a fresh batch per episode instead of rebinding the one it has.  A kept batch advances the
                              episode counter, which feeds the Philox stream, so this decides which numbers an episode draws.
    ``_carry_slice``          the slice of the state block that the B = 1 view carries over a reset, as the reference's optimizer object does;
                              ``mbx_batch_rebind`` keeps it in place, and it is copied into the batch made for a problem of another suite.
    """
    _ALGO = None
    _NP = None
    _KEEPS_BATCH = True
    _carry_slice = None

    def __init__(self, config):
        super().__init__(config)
        self._config = config
        self.log_interval = config.log_interval
        self.cost = None
        self.log_index = None
        self._batch = None
        self._batch_key = None

    @classmethod
    def population_size(cls, dim):
        return cls._NP

    def make_batch(self, suite, problem_idx, seeds, early_stop=True):
        from ..suite import Batch
        c = self._config
        return Batch(suite, self._ALGO, problem_idx, seeds, self.population_size(suite.dim), c.maxFEs, c.log_interval, c.n_logpoint,
                     early_stop=early_stop)

    def _n_steps(self):
        raise NotImplementedError

    def _run(self, batch, single=False):
        """The launches of one episode after the reset; done instances stay frozen, so launches past an early stop change nothing.
        single: the batch is the B = 1 view's."""
        for _ in range(self._n_steps()):
            batch.step(None)

    def run_batch(self, suite, problem_idx, seeds):
        """-> dict of device tensors (cost [B, n_logpoint+1] padded, fes [B], cost_len [B], ...)."""
        batch = self.make_batch(suite, problem_idx, seeds)
        batch.reset()
        self._run(batch)
        res = batch.results()
        torch.cuda.synchronize()
        batch.close()
        return res

    def run_episode(self, problem):
        problem.reset()
        suite = problem._bound_suite()
        seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 + int(np.random.randint(0, 2 ** 31 - 1))
        if not self._KEEPS_BATCH:
            res = self.run_batch(suite, [problem._suite_index], [seed])
            n = int(res['cost_len'][0].item())
            self.cost = [float(v) for v in res['cost'][0, :n].cpu().numpy()]
            return {'cost': self.cost, 'fes': int(res['fes'][0].item())}
        if self._batch is not None and self._batch_key == id(suite):
            self._batch.rebind([problem._suite_index], [seed])
        else:
            carried = None
            if self._batch is not None:
                if self._carry_slice is not None:
                    carried = self._batch.read_state(0)[self._carry_slice()].copy()
                self._batch.close()
            self._batch = self.make_batch(suite, [problem._suite_index], [seed])
            self._batch_key = id(suite)
            if carried is not None:
                blk = self._batch.read_state(0)
                blk[self._carry_slice()] = carried
                self._batch.write_state(0, blk)
        self._batch.reset()
        self._run(self._batch, single=True)
        sc = self._batch.read_public(0)
        n = int(sc[3])
        self.log_index = int(sc[2])
        self.cost = [float(v) for v in sc[16:16 + n]]
        return {'cost': self.cost, 'fes': int(sc[1])}
