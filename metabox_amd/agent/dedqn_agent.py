"""DEDQN agent: a small deep Q-network picks one of three DE mutation operators from four landscape features
(reference: src/agent/dedqn_agent.py).

Q-network: MLP 4 -> 10 -> 10 -> 3 with ReLU.  Rollout is greedy (argmax Q); training is epsilon-greedy (eps = 0.1) with a
100-transition replay buffer, a 64-transition warm-up, mini-batches of 64, gamma = 0.8 and AdamW (lr 1e-4).  There is no target
network, and the reference does NOT detach the TD target `r + (1 - done) gamma max_a' Q(s', a')`: the gradient flows through it as
well (dedqn_agent.py:67-73).  ``learn_from_batch`` keeps that; tests/golden/dedqn_train.npz pins it.
``rollout_batch`` hands the packed network to the resident step kernel, which then decides for itself (``mbx_dedqn_rollout``).
"""
import numpy as np
import torch

from .basic_agent import Basic_Agent
from .networks import MLP
from .utils import ReplayBuffer, save_class

_HYPER = dict(state_size=4, n_act=3, lr=1e-4, epsilon=0.1, gamma=0.8, memory_size=100, batch_size=64, warm_up_size=64)


class DEDQN_Agent(Basic_Agent):
    # Under torch.distributed Trainer drives train_batch, whose gradients are averaged over the ranks: every rank holds the same parameters and rank 0
    # alone writes the checkpoints (agent/utils.save_class), `checkpoint0` of __init__ / update_setting included.
    _mbx_replicated = True

    def __init__(self, config):
        super().__init__(config)
        for key, value in _HYPER.items():               # the agent publishes its hyper-parameters on the shared config
            setattr(config, key, value)
        config.mlp_config = [{'in': config.state_size, 'out': 10, 'drop_out': 0, 'activation': 'ReLU'},
                             {'in': 10, 'out': 10, 'drop_out': 0, 'activation': 'ReLU'},
                             {'in': 10, 'out': config.n_act, 'drop_out': 0, 'activation': 'None'}]
        self.__config = config
        self.__device = config.device
        self.__dqn = MLP(config.mlp_config).to(self.__device)
        self.__optimizer = torch.optim.AdamW(self.__dqn.parameters(), lr=config.lr)
        self.__criterion = torch.nn.MSELoss()
        self.__replay_buffer = ReplayBuffer(config.memory_size)
        self.__max_learning_step = config.max_learning_step
        self.__global_ls = 0
        self.__cur_checkpoint = 0
        self.__checkpoint()

    # ---- bookkeeping ---------------------------------------------------------------------------------
    def __checkpoint(self):
        if getattr(self.__config, 'agent_save_dir', None):
            save_class(self.__config.agent_save_dir, f'checkpoint{self.__cur_checkpoint}', self)
        self.__cur_checkpoint += 1

    @property
    def q_net(self):
        return self.__dqn

    def load_exported_weights(self, npz):
        prefix = 'net/'
        self.__dqn.load_state_dict({k[len(prefix):]: torch.as_tensor(np.asarray(npz[k])) for k in npz.files if k.startswith(prefix)})
        return self

    def to(self, device):
        self.__device = self.__config.device = device
        self.__dqn.to(device)
        return self

    def __getstate__(self):
        """Checkpoints carry the network and the host-side replay like the reference's; the device replay of train_batch is rebuilt on demand."""
        return {k: v for k, v in self.__dict__.items() if k != '_dev_replay'}

    def update_setting(self, config):
        self.__max_learning_step = config.max_learning_step
        self.__config.agent_save_dir = config.agent_save_dir
        self.__config.save_interval = config.save_interval
        self.__global_ls = 0
        self.__cur_checkpoint = 0
        self.__checkpoint()

    # ---- acting ---------------------------------------------------------------------------------------
    def __act(self, state, explore):
        with torch.no_grad():
            q = self.__dqn(torch.as_tensor(np.asarray(state), dtype=torch.float32, device=self.__device))
        if explore and np.random.rand() < self.__config.epsilon:
            return int(np.random.randint(low=0, high=self.__config.n_act))
        return int(torch.argmax(q))

    def packed_weights(self):
        """float32 tensor in the layout ``mbx_dedqn_net`` documents (include/mbx.h): per Linear layer the weight transposed, Wt [in][out],
        then the bias: 193 values."""
        parts = []
        for m in self.__dqn.net:
            if isinstance(m, torch.nn.Linear):
                parts += [m.weight.detach().t().contiguous().reshape(-1), m.bias.detach().reshape(-1)]
        return torch.cat(parts).to(torch.float32).contiguous()

    @torch.no_grad()
    def greedy_batch(self, states):
        """Greedy operator choice for a batch of states [B, 4] -> int32 [B] (argmax Q, dedqn_agent.py:44-53)."""
        return self.__dqn(states.to(torch.float32)).argmax(dim=1).to(torch.int32)

    def rollout_episode(self, env):
        state, done, total = env.reset(), False, 0
        while not done:
            state, reward, done = env.step(self.__act(state, explore=False))
            total += reward
        return {'cost': env.optimizer.cost, 'fes': env.optimizer.fes, 'return': total}

    @torch.no_grad()
    def rollout_batch(self, env, max_steps=None, chunk=32, policy='hip'):
        """Whole episodes of a BatchedPBO_Env.  policy = 'hip' (default): the Q-network inside the resident step kernel, `chunk` env steps
        per launch (``mbx_dedqn_rollout``); 'torch': the PyTorch module picks the action for the whole batch, then one step launch.
        The two routes evaluate the same float32 network with different summation orders (one fma chain per unit in ascending k in the
        kernel / torch's GEMMs), so Q values agree to ~1e-6 and the greedy action can differ where two Q values are that close:
        trajectories are route-dependent (both valid); tests/test_dedqn.py bounds the disagreement of the Q values."""
        bc = env.batch.cfg
        if max_steps is None:
            max_steps = -(-(bc.max_fes - 2 * bc.np) // (2 * bc.np))          # a reset and every step bill 2 NP evaluations
        state = env.reset()
        if policy == 'hip':
            packed = self.packed_weights().to(env.batch.device)
            left = max_steps
            while left > 0:
                env.batch.dedqn_rollout(packed, min(chunk, left))
                left -= chunk
        elif policy == 'torch':
            self.__dqn.to(env.batch.device)
            for _ in range(max_steps):
                state, _, _ = env.step(self.greedy_batch(state).contiguous())
        else:
            raise ValueError(f"policy must be 'hip' or 'torch', not {policy!r}")
        res = env.results()
        return {k: res[k] for k in ('cost', 'fes', 'return', 'steps', 'cost_len')}

    # ---- learning -------------------------------------------------------------------------------------
    def learn_from_batch(self, obs, act, rew, nxt, dn, sync_gradients=False, detach_target=False):
        """One DQN update on a mini-batch (dedqn_agent.py:66-75): MSE between Q(s, a) and r + (1 - done) gamma max_a' Q(s', a') of the SAME
        network, AdamW step.  The reference leaves the target attached to the graph, so its gradient is part of the update;
        ``detach_target=True`` is the textbook form (what the parity test shows the fixture does NOT match)."""
        cfg = self.__config
        q_taken = (self.__dqn(obs) * torch.nn.functional.one_hot(act.long(), cfg.n_act)).sum(1)
        target = rew + (1 - dn) * cfg.gamma * self.__dqn(nxt).max(1)[0]
        if detach_target:
            target = target.detach()
        self.__optimizer.zero_grad()
        loss = self.__criterion(q_taken, target)
        loss.backward()
        if sync_gradients:
            from ..distributed import average_gradients
            average_gradients(list(self.__dqn.parameters()))
        self.__optimizer.step()
        self.__global_ls += 1
        if getattr(cfg, 'agent_save_dir', None) and self.__global_ls >= cfg.save_interval * self.__cur_checkpoint:
            self.__checkpoint()
        return loss

    def train_episode(self, env):
        """One episode of epsilon-greedy interaction with a replay update after every step once the buffer holds warm_up_size
        transitions (reference loop: dedqn_agent.py:55-87)."""
        cfg = self.__config
        state, done, total = env.reset(), False, 0
        while not done:
            action = self.__act(state, explore=True)
            nxt, reward, done = env.step(action)
            total += reward
            self.__replay_buffer.append((state, action, reward, nxt, done))
            if len(self.__replay_buffer) >= cfg.warm_up_size:
                obs, act, rew, nx, dn = (t.to(self.__device) for t in self.__replay_buffer.sample(cfg.batch_size))
                self.learn_from_batch(obs, act, rew, nx, dn)
                if self.__global_ls >= self.__max_learning_step:
                    break
            state = nxt
        return self.__global_ls >= self.__max_learning_step, {'normalizer': env.optimizer.cost[0], 'gbest': env.optimizer.cost[-1],
                                                              'return': total, 'learn_steps': self.__global_ls}

    def train_batch(self, env, max_updates=None, updates_per_step=1):
        """DQN training over a lock-step BatchedPBO_Env, built like DE_DDQN_Agent.train_batch: every env step all B instances act
        epsilon-greedily on the device, their transitions go into a device-resident FIFO replay (capacity memory_size rounded to whole
        steps of the batch, at least one), and once it holds warm_up_size transitions `updates_per_step` mini-batch updates follow.
        Gradients are averaged across ranks.  Returns (exceed_max_learning_step, {'normalizer', 'gbest', 'return', 'learn_steps'})."""
        from ..distributed import all_ranks_any
        cfg, dev = self.__config, env.batch.device
        net = self.__dqn.to(dev)
        B, S = env.B, cfg.state_size
        cap = (cfg.memory_size // B) * B if cfg.memory_size >= B else B
        if getattr(self, '_dev_replay', None) is None or self._dev_replay['obs'].shape[0] != cap or self._dev_replay['obs'].device != dev:
            self._dev_replay = dict(obs=torch.empty(cap, S, device=dev), nxt=torch.empty(cap, S, device=dev),
                                    act=torch.empty(cap, dtype=torch.int64, device=dev), rew=torch.empty(cap, device=dev),
                                    done=torch.empty(cap, device=dev), size=0, head=0)
        rb = self._dev_replay
        state = env.reset().to(torch.float32).clone()
        alive = torch.ones(B, dtype=torch.bool, device=dev)
        ret_sum = torch.zeros(B, dtype=torch.float64, device=dev)
        updates, exceed = 0, False
        while all_ranks_any(bool(alive.any()), dev) and not exceed:      # global loop control: every rank issues the same collectives
            with torch.no_grad():
                greedy = net(state).argmax(dim=1)
                explore = torch.rand(B, device=dev) < cfg.epsilon
                action = torch.where(explore, torch.randint(0, cfg.n_act, (B,), device=dev), greedy)
            nstate, reward, done = env.step(action.to(torch.int32).contiguous())
            nstate = nstate.to(torch.float32).clone()
            ret_sum += reward * alive
            live = alive.nonzero(as_tuple=True)[0]                  # finished instances contribute no transitions
            n = int(live.numel())
            if n:
                slots = (rb['head'] + torch.arange(n, device=dev)) % cap
                rb['obs'][slots] = state[live]; rb['nxt'][slots] = nstate[live]; rb['act'][slots] = action[live]
                rb['rew'][slots] = reward[live].to(torch.float32); rb['done'][slots] = (done[live] != 0).to(torch.float32)
                rb['head'] = (rb['head'] + n) % cap
                rb['size'] = min(cap, rb['size'] + n)
            alive = alive & (done == 0)
            state = nstate
            if all_ranks_any(rb['size'] >= min(cfg.warm_up_size, cap), dev) and rb['size'] >= 1:
                for _ in range(updates_per_step):
                    idx = torch.randint(0, rb['size'], (cfg.batch_size,), device=dev)
                    self.learn_from_batch(rb['obs'][idx], rb['act'][idx], rb['rew'][idx], rb['nxt'][idx], rb['done'][idx], sync_gradients=True)
                    updates += 1
                    if self.__global_ls >= self.__max_learning_step or (max_updates is not None and updates >= max_updates):
                        exceed = True
                        break
        res = env.results()
        return self.__global_ls >= self.__max_learning_step, {
            'normalizer': float(res['cost'][:, 0].mean()), 'gbest': float(res['cost'][:, -1].mean()),
            'return': float(ret_sum.mean()), 'learn_steps': self.__global_ls}
