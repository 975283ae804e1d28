"""NRLPSO agent: tabular Q-learning over 4 states x 4 actions (reference: src/agent/nrlpso_agent.py).

Policy: softmax over the Q-row of the state, sampled with ``np.random.choice``.  Training: TD(0) with gamma = 0.8 and a learning rate
``1 - 0.9 ls / max_learning_step`` (nrlpso_agent.py:55; QLPSO's schedule ends at 0.1 the same way but is written differently and rounds
differently).  ``rollout_batch`` hands the 4 x 4 table to the step kernel, which then makes the decisions itself, `chunk` env steps per launch
(``mbx_nrlpso_rollout``).
"""
import numpy as np
import torch

from .basic_agent import Basic_Agent
from .utils import save_class


class NRLPSO_Agent(Basic_Agent):
    def __init__(self, config):
        super().__init__(config)
        config.n_states = 4             # nrlpso_agent.py:10-16
        config.n_actions = 4
        config.gamma = 0.8
        self.__config = config
        self.__q_table = np.zeros((config.n_states, config.n_actions))
        self.__max_learning_step = config.max_learning_step
        self.__global_ls = 0
        self.__cur_checkpoint = 0
        self.__checkpoint()

    def __checkpoint(self):
        if getattr(self.__config, 'agent_save_dir', None):
            save_class(self.__config.agent_save_dir, 'checkpoint' + str(self.__cur_checkpoint), self)
        self.__cur_checkpoint += 1

    @property
    def q_table(self):
        return self.__q_table

    @property
    def learn_steps(self):
        return self.__global_ls

    def load_exported_weights(self, npz, learn_steps=0):
        self.__q_table = np.array(npz['q_table'], dtype=np.float64)
        self.__global_ls = int(learn_steps)
        return self

    def to(self, device):
        self.__config.device = device
        return self

    def update_setting(self, config):
        self.__config.max_learning_step = self.__max_learning_step = config.max_learning_step
        self.__config.agent_save_dir = config.agent_save_dir
        self.__global_ls = 0
        save_class(self.__config.agent_save_dir, 'checkpoint0', self)
        self.__config.save_interval = config.save_interval
        self.__cur_checkpoint = 1

    def __get_action(self, state):
        weights = np.exp(self.__q_table[state])
        return np.random.choice(self.__config.n_actions, size=1, p=weights / weights.sum())

    def td_update(self, state, action, reward, next_state):
        """One TD(0) update (nrlpso_agent.py:42-55): Q[s, a] += alpha (r + gamma max Q[s'] - Q[s, a]) with the alpha the reference holds at
        this learning step, 1 - 0.9 ls / max_learning_step; returns the number of learning steps made so far."""
        q = self.__q_table
        alpha = 1 - 0.9 * (self.__global_ls / self.__max_learning_step)
        q[state][action] += alpha * (reward + self.__config.gamma * q[next_state].max() - q[state][action])
        self.__global_ls += 1
        return self.__global_ls

    def train_episode(self, env):
        c = self.__config
        total, state, finished = 0, env.reset(), False
        while not finished:
            action = self.__get_action(state)
            successor, reward, finished = env.step(action)
            total += reward
            self.td_update(state, action, reward, successor)
            if self.__global_ls >= c.save_interval * self.__cur_checkpoint:
                self.__checkpoint()
            if self.__global_ls >= self.__max_learning_step:
                break
            state = successor
        summary = {'normalizer': env.optimizer.cost[0], 'gbest': env.optimizer.cost[-1], 'return': total, 'learn_steps': self.__global_ls}
        return self.__global_ls >= self.__max_learning_step, summary

    def rollout_episode(self, env):
        total, state, finished = 0, env.reset(), False
        while not finished:
            state, reward, finished = env.step(self.__get_action(state))
            total += reward
        return {'cost': env.optimizer.cost, 'fes': env.optimizer.fes, 'return': total}

    @torch.no_grad()
    def rollout_batch(self, env, max_steps=None, chunk=256):
        """Whole episodes of a BatchedPBO_Env with the tabular policy inside the resident step kernel."""
        bc = env.batch.cfg
        if max_steps is None:
            max_steps = bc.max_fes - bc.np                     # every step bills at least one evaluation
        q = torch.from_numpy(np.ascontiguousarray(self.__q_table, dtype=np.float64)).to(env.batch.device)
        env.reset()
        left = max_steps
        while left > 0:
            env.batch.nrlpso_rollout(q, min(chunk, left))
            left -= chunk
        res = env.results()
        return {'cost': res['cost'], 'fes': res['fes'], 'return': res['return'], 'steps': res['steps'], 'cost_len': res['cost_len']}
