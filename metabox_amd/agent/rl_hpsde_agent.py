"""RL-HPSDE agent: tabular Q-learning over 4 landscape states x 4 actions (reference: src/agent/rl_hpsde_agent.py).

Policy: softmax over the Q-row of the state, sampled with ``np.random.choice``.  Training: TD(0) with gamma = 0.5 and a constant learning
rate 0.8 (``alpha_decay`` is False in the reference).  ``rollout_batch`` hands the 4 x 4 table to the step kernel, which then makes the
decisions itself, `chunk` updates per launch (``mbx_rlhpsde_rollout``).
"""
import numpy as np
import torch

from .basic_agent import Basic_Agent
from .utils import save_class


class RL_HPSDE_Agent(Basic_Agent):
    def __init__(self, config):
        super().__init__(config)
        config.n_states = 4             # rl_hpsde_agent.py:8-12
        config.n_actions = 4
        config.alpha_max = 0.8
        config.alpha_decay = False
        config.gamma = 0.5
        self.__config = config
        self.__q_table = np.zeros((config.n_states, config.n_actions))
        self.__alpha = config.alpha_max
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
        """One TD(0) update (rl_hpsde_agent.py:45-47): Q[s, a] += alpha (r + gamma max Q[s'] - Q[s, a]); returns the number of learning steps made
        so far."""
        q = self.__q_table
        td_error = reward + self.__config.gamma * q[next_state].max() - q[state][action]
        q[state][action] += self.__alpha * td_error
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
    def rollout_batch(self, env, max_steps=None, chunk=16):
        """Whole episodes of a BatchedPBO_Env with the tabular policy inside the step kernel."""
        bc = env.batch.cfg
        if max_steps is None:
            max_steps = (bc.max_fes - bc.np - 201) // 202 + 1          # every update bills its walk and at least one trial
        q = torch.from_numpy(np.ascontiguousarray(self.__q_table, dtype=np.float64)).to(env.batch.device)
        env.reset()
        left = max_steps
        while left > 0:
            _, _, done, _ = env.batch.rlhpsde_rollout(q, min(chunk, left))
            left -= chunk
            if bool(done.all()):
                break
        res = env.results()
        return {'cost': res['cost'], 'fes': res['fes'], 'return': res['return'], 'steps': res['steps'], 'cost_len': res['cost_len']}
