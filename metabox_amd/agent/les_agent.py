"""LES agent: CMA-ES meta-training of the 246 parameters of the learned evolution strategy (reference: src/agent/les_agent.py).

A meta-generation evaluates meta_pop_size = 16 candidate parameter vectors on every train problem for skip_step = 50 generations; the
meta-cost of a candidate is the median over problems of its z-scored best value, and CMA-ES (``agent/cma.py``) is told the 16 costs.  The
reference does this with 16 deep copies of the environment and a Python loop; ``train_batch`` runs ONE batch of (train problem x candidate)
instances with per-instance parameters through ``mbx_les_rollout``.  ``rollout_batch`` runs whole episodes with ``best_x``.
"""
import numpy as np
import torch

from .basic_agent import Basic_Agent
from .cma import CMA
from .utils import save_class

N_ATTN, N_PARAM = 68, 246


class LES_Agent(Basic_Agent):
    def __init__(self, config):
        super().__init__(config)
        self.__config = config
        self.meta_pop_size = 16
        self.skip_step = 50
        self.optimizer = CMA(mean=np.zeros(N_PARAM), sigma=0.1, population_size=self.meta_pop_size)
        self.x_population = None
        self.meta_performances = None
        self.optimizer_step()
        self.best_x = self.x_population[0]
        self.costs = None
        self.best_les = None
        self.gbest = 1e10
        self.__learning_step = 0
        self.__cur_checkpoint = 0
        self.__checkpoint()

    def __checkpoint(self):
        if getattr(self.__config, 'agent_save_dir', None):
            save_class(self.__config.agent_save_dir, 'checkpoint' + str(self.__cur_checkpoint), self)
        self.__cur_checkpoint += 1

    @property
    def learn_steps(self):
        return self.__learning_step

    def load_exported_weights(self, npz, learn_steps=0):
        self.best_x = np.array(npz['best_x'], dtype=np.float64).reshape(N_PARAM)
        self.__learning_step = int(learn_steps)
        return self

    def to(self, device):
        self.__config.device = device
        return self

    def update_setting(self, config):
        self.__config.max_learning_step = config.max_learning_step
        self.__config.agent_save_dir = config.agent_save_dir
        self.__learning_step = 0
        save_class(self.__config.agent_save_dir, 'checkpoint0', self)
        self.__config.save_interval = config.save_interval
        self.__cur_checkpoint = 1

    def optimizer_step(self):
        """A new population from the meta-optimizer (les_agent.py:46-52)."""
        self.x_population = np.vstack([self.optimizer.ask() for _ in range(self.meta_pop_size)])
        self.meta_performances = [[] for _ in range(self.meta_pop_size)]

    def __after_learning_steps(self):
        c = self.__config
        if self.__learning_step >= c.save_interval * self.__cur_checkpoint:
            self.__checkpoint()
        return self.__learning_step >= c.max_learning_step

    def train_episode(self, env):
        """Every candidate on one problem, one after the other (les_agent.py:55-83)."""
        first = None
        for i in range(self.meta_pop_size):
            env.reset()
            action = {'attn': self.x_population[i][:N_ATTN], 'mlp': self.x_population[i][N_ATTN:], 'skip_step': self.skip_step}
            sub_best, _, _, _ = env.step(action)
            self.meta_performances[i].append(sub_best)
            if i == 0:
                first = (env.optimizer.cost[0], env.optimizer.cost[-1])
        self.__learning_step += 1
        if self.__learning_step % 10 == 0 and self.__config.problem in ['protein', 'protein-torch']:
            self.train_epoch()
        exceed = self.__after_learning_steps()
        return exceed, {'normalizer': first[0], 'gbest': first[1], 'return': 0, 'learn_steps': self.__learning_step}

    def train_epoch(self):
        """The meta-update (les_agent.py:86-100): z-score per problem, median over problems, tell, ask."""
        scores = np.stack(self.meta_performances)
        self.costs = np.median((scores - np.mean(scores, axis=0)[None, :]) / scores.std(axis=0)[None, :], axis=-1)
        if np.min(self.costs) < self.gbest:
            self.gbest = np.min(self.costs)
            self.best_les = np.argmin(self.costs)
            self.best_x = self.x_population[self.best_les]
        self.optimizer.tell(list(zip(self.x_population, self.costs)))
        self.optimizer_step()

    def rollout_episode(self, env):
        env.reset()
        _, r, _, _ = env.step({'attn': self.best_x[:N_ATTN], 'mlp': self.best_x[N_ATTN:]})
        return {'cost': env.optimizer.cost, 'fes': env.optimizer.FEs, 'return': r}

    @torch.no_grad()
    def rollout_batch(self, env, chunk=64):
        """Whole episodes of a BatchedPBO_Env with best_x, `chunk` generations per launch."""
        bc = env.batch.cfg
        env.batch.les_set_params(self.best_x)
        env.reset()
        left = (bc.max_fes - 1) // bc.np                       # generations until FEs >= maxFEs
        while left > 0:
            env.batch.les_rollout(min(chunk, left))
            left -= chunk
        res = env.results()
        return {'cost': res['cost'], 'fes': res['fes'], 'return': res['return'], 'steps': res['steps'], 'cost_len': res['cost_len']}

    @torch.no_grad()
    def train_batch(self, env):
        """One meta-generation in ONE batch: the instances of `env` are (train problem x candidate), problem-major with the candidate as the run index
        of the instance table.  One skip_step call gives scores [16, n_problems]; then train_epoch's tell / ask.  The learning step advances by the
        number of problems, as n_problems calls of train_episode would."""
        import torch.distributed as dist
        P = self.meta_pop_size
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError('LES_Agent.train_batch: the meta-update needs every (problem x candidate) score in one process; run single-process')
        if getattr(self.__config, 'train_batch_size', P) != P:
            raise ValueError(f'LES_Agent.train_batch: --train_batch_size must be {P} (one run per CMA-ES candidate), not {self.__config.train_batch_size}')
        pidx = np.asarray(env.problem_idx)
        if len(pidx) % P or not np.array_equal(pidx.reshape(-1, P), np.repeat(pidx[::P], P).reshape(-1, P)):
            raise ValueError('LES_Agent.train_batch: the batch must hold blocks of 16 instances of one problem each (instance_table order)')
        n_problems = len(pidx) // P
        candidate = np.tile(np.arange(P, dtype=np.int32), n_problems)
        env.batch.les_set_params(self.x_population, candidate)
        env.reset()
        state, _, _ = env.batch.les_rollout(self.skip_step, skip=True)
        scores = state[:, 0].cpu().numpy().reshape(n_problems, P).T      # [candidate, problem]
        for i in range(P):
            self.meta_performances[i].extend(float(v) for v in scores[i])
        res = env.results()
        info = {'normalizer': float(res['cost'][0, 0].item()), 'gbest': float(scores[0, 0]), 'return': 0, 'scores': scores}
        self.train_epoch()
        self.__learning_step += n_problems
        info['learn_steps'] = self.__learning_step
        return self.__after_learning_steps(), info
