"""L2L agent (RNN-OI): an LSTM that proposes the next point from the last point and its value (reference: src/agent/l2l_agent.py).

The net is ``nn.LSTM(input_size=dim + 2, hidden_size=32, proj_size=dim)`` in float64.  An episode is 100 strictly sequential steps: the first input
is all zeros, every later one is (x_raw, y, 1).  ``rollout_episode`` runs the net on the host and the environment through the B = 1 view, as the
reference does; ``rollout_batch`` is ONE launch of ``mbx_l2l_rollout`` with the cell in the kernel.  Only rollout is built: training differentiates
through the objective (the ``*-torch`` problem twins), which this build does not have.
"""
import numpy as np
import torch
from torch import nn

from .basic_agent import Basic_Agent
from .utils import save_class

T = 100
KEYS = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0', 'weight_hr_l0')     # the kernel's order (include/mbx_layout.h section 21)
_NO_TRAINING = ('L2L_Agent.{}: training L2L takes the gradient of the objective (loss = sum of y through problem.eval on the *-torch problem twins), '
                'which this build does not have; rollout_episode / rollout_batch (--test, --rollout) run the trained net (DESIGN.md §7)')


class L2L_Agent(Basic_Agent):
    def __init__(self, config):
        super().__init__(config)
        config.lr = 1e-5
        self.__config = config
        self.hidden_size = 32
        self.proj_size = config.dim
        self.net = nn.LSTM(input_size=config.dim + 2, hidden_size=self.hidden_size, proj_size=config.dim).double()
        self.__learning_step = 0
        self.__cur_checkpoint = 0
        if getattr(config, 'agent_save_dir', None):
            save_class(config.agent_save_dir, 'checkpoint0', self)
        self.__cur_checkpoint = 1

    @property
    def learn_steps(self):
        return self.__learning_step

    def load_exported_weights(self, npz, learn_steps=0):
        """The five arrays of a trained net (tests/golden/l2l_policy.npz holds the shipped bbob_easy checkpoint's)."""
        sd = {k: torch.as_tensor(np.asarray(npz[k]), dtype=torch.float64) for k in KEYS}
        self.net.load_state_dict(sd)
        self.__learning_step = int(learn_steps)
        return self

    def packed_weights(self):
        """-> [128 (D + 2) + 128 D + 256 + 32 D] float64, the layout ``Batch.l2l_set_params`` takes."""
        sd = self.net.state_dict()
        return np.concatenate([sd[k].detach().cpu().numpy().astype(np.float64).ravel() for k in KEYS])

    def to(self, device):
        self.__config.device = device          # the net stays on the host: rollout_batch hands its weights to the kernel
        return self

    def update_setting(self, config):
        self.__config.max_learning_step = config.max_learning_step
        self.__config.agent_save_dir = config.agent_save_dir
        self.__learning_step = 0
        save_class(self.__config.agent_save_dir, 'checkpoint0', self)
        self.__config.save_interval = config.save_interval
        self.__cur_checkpoint = 1

    def train_episode(self, env):
        raise NotImplementedError(_NO_TRAINING.format('train_episode'))

    def train_batch(self, env):
        raise NotImplementedError(_NO_TRAINING.format('train_batch'))

    @torch.no_grad()
    def rollout_episode(self, env):
        """l2l_agent.py:92-135 through the B = 1 view: the cell on the host, box map / evaluation / bookkeeping in ``k_l2l_step``."""
        D = self.__config.dim
        inp = torch.zeros(1, 1, D + 2, dtype=torch.float64)
        h = torch.zeros(1, 1, self.proj_size, dtype=torch.float64)
        c = torch.zeros(1, 1, self.hidden_size, dtype=torch.float64)
        env.reset()
        fes, y_sum, init_y = 0, 0, None
        for t in range(T):
            out, (h, c) = self.net(inp, (h, c))
            x = out[0, 0]
            y, _, is_done = env.step(x.numpy())
            y_sum += y
            if t == 0:
                init_y = y
            fes += 1
            inp = torch.cat((x, torch.tensor([y], dtype=torch.float64), torch.tensor([1.], dtype=torch.float64)))[None, None, :]
            if is_done:
                break
        return {'cost': env.optimizer.cost[::2], 'fes': fes, 'return': y_sum / init_y}

    @torch.no_grad()
    def rollout_batch(self, env):
        """Whole episodes of a BatchedPBO_Env in one launch: 100 steps with the recurrent state on chip."""
        env.batch.l2l_set_params(self.packed_weights())
        env.reset()
        env.batch.l2l_rollout(T)
        res = env.results()
        return {'cost': res['cost'], 'fes': res['fes'], 'return': res['return'], 'steps': res['steps'], 'cost_len': res['cost_len']}
