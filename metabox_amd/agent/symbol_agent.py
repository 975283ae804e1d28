"""SYMBOL agent: an LSTM that writes the optimizer's update rule as an expression tree (reference: src/agent/symbol_agent.py,
src/agent/symbol_related/{lstm,utils,expression,tokenizer}.py).

Every action the actor emits a tree over the 11 tokens ``+ * - C-1 C0 x gb gw dx randx pb``, one token at a time in pre-order into a heap array of
63 slots: the input of step t is the 4-bit code of every token written so far (63 x 4 = 252 inputs), the cell state starts at ``x_to_c(state)``, a
grammar mask removes the tokens that would make the tree redundant or ill-formed, and the token is drawn from the masked softmax; a constant token
draws its value from a second head (4 values ``-1 + 0.4 k`` in float32).  The tree and its constants go to the kernel as they are
(``mbx_symbol_rollout``: metabox_amd/csrc/mbx_symbol.hpp walks the tree itself), each instance under its own rule.

``generate`` runs the LSTM in torch over the whole batch, finished rows dropped, as the reference's forward does; the grammar mask is this module's
own restatement of ``get_mask``, memoised on (partial tree, position).  The memo pays where instances share a state (the runs of one problem early in an
episode); 4096 instances on 4096 different states met 115 236 distinct pairs in five actions (docs/EXPERIMENTS.md), so it is bounded -- emptied once it
holds MASK_CACHE_MAX entries -- and never pickled.  ``rollout_checkpoints`` runs the 21 checkpoints of a ``--rollout`` table in ONE batch.  Only rollout
is built: training needs the MadDE teacher episode in lock-step and PPO through the token memory.
"""
import numpy as np
import torch
from torch import nn
from torch.distributions import Categorical

from .basic_agent import Basic_Agent
from .utils import save_class

VOCAB = ('+', '*', '-', 'C-1', 'C0', 'x', 'gb', 'gw', 'dx', 'randx', 'pb')
ADD, MUL, NEG, CM1, C0, X, GB, GW, DX, RANDX, PB = range(11)
N_TOK, N_SLOT, CODE_LEN, MAX_LAYER, FEA_DIM, HIDDEN = 11, 63, 4, 6, 9, 16
MIN_C, MAX_C, C_INTERVAL = -1., 1., 0.4
NUM_C = int((MAX_C - MIN_C) // C_INTERVAL)          # 4, not 5: 2.0 // 0.4 is 4.0 in floating point
SKIP_STEP = 5
MASK_CACHE_MAX = 1 << 16      # entries of the mask memo before it is emptied (about 30 MB)
OPERATORS, CONSTANTS, LEAVES, VARIABLES = (ADD, MUL, NEG), (CM1, C0), tuple(range(CM1, N_TOK)), tuple(range(X, N_TOK))
NON_CONSTANTS = tuple(t for t in range(N_TOK) if t not in CONSTANTS)
KEYS = ('lstm.weight_ih_l0', 'lstm.weight_hh_l0', 'lstm.bias_ih_l0', 'lstm.bias_hh_l0', 'output_net.weight', 'output_net.bias', 'x_to_c.weight',
        'x_to_c.bias', 'constval_net.weight', 'constval_net.bias')
_NO_TRAINING = ('Symbol_Agent.{}: training SYMBOL runs the MadDE teacher episode in lock-step with the student (the imitation part of the reward) and PPO '
                'through the token memory of every generated tree; this build has the rollout side only: rollout_episode / rollout_batch (--test, --rollout)')


# ------------------------------------------------------------------------------------------------ the grammar mask
def _tok(seq, i):
    """The token name the reference decodes slot i to: an empty slot (-1) reads the vocabulary from its end, and so does slot -1 the tree."""
    return VOCAB[seq[i]]


def _prefix(seq, r):
    """Tokens of the subtree at r in pre-order, empty slots skipped."""
    if r >= len(seq) or seq[r] == -1:
        return []
    return [int(seq[r])] + _prefix(seq, 2 * r + 1) + _prefix(seq, 2 * r + 2)


def _nearest(seq, pos, name):
    """The nearest proper ancestor of pos that holds `name`, or -1."""
    while pos > 0:
        pos = (pos - 1) // 2
        if _tok(seq, pos) == name:
            return pos
    return -1


def _plus_chain(seq, begin, seen, out):
    """Walk the maximal chain of '+' nodes through `begin` (up, then left, then right) and collect the roots of its non-'+' operands; True when the chain
    reaches the root."""
    seen.add(begin)
    at_root = begin == 0 and seq[0] == ADD
    up = (begin - 1) // 2
    if begin != 0 and up not in seen and _tok(seq, up) == '+':
        at_root = _plus_chain(seq, up, seen, out) or at_root
    for child in (2 * begin + 1, 2 * begin + 2):
        if child not in seen and seq[child] != -1:
            if seq[child] == ADD:
                at_root = _plus_chain(seq, child, seen, out) or at_root
            else:
                out.append(child)
    return at_root


def _plus_chain_minus(seq, begin, seen, out):
    """The same walk, collecting what stands under the unary minus operands of the chain.  The reference looks at the LEFT child's token when it decides
    about the right child (get_along_continuous_plus_with_minus); kept."""
    seen.add(begin)
    up = (begin - 1) // 2
    if begin != 0 and up not in seen and _tok(seq, up) == '+':
        _plus_chain_minus(seq, up, seen, out)
    left, right = 2 * begin + 1, 2 * begin + 2
    left_tok = None
    if left not in seen and seq[left] != -1:
        left_tok = seq[left]
        if left_tok == ADD:
            _plus_chain_minus(seq, left, seen, out)
        elif left_tok == NEG:
            out.append(2 * left + 1)
    if right not in seen and seq[right] != -1:
        if seq[right] == ADD:
            _plus_chain_minus(seq, right, seen, out)
        elif left_tok == NEG:
            out.append(2 * right + 1)


def _completing(target, operands):
    """Tokens that would complete `target` into one of `operands` (prefix lists); randx and the constants never count as repeats."""
    out = []
    for op in operands:
        if len(op) == len(target) + 1 and op[:-1] == target and op[-1] != RANDX and op[-1] not in CONSTANTS:
            out.append(op[-1])
    return out


def grammar_mask(seq, pos):
    """-> [11] of 0 / 1: the tokens the reference's get_mask allows at slot `pos` of the partial tree `seq` (63 ints, -1 = empty)."""
    m = np.ones(N_TOK)
    if pos == -1:
        return np.zeros(N_TOK)
    if pos == 0:                                             # the root is '+' or '*'
        m[list(LEAVES)] = 0
        m[NEG] = 0
        return m
    fi = (pos - 1) // 2
    f = int(seq[fi])
    right = pos % 2 == 0
    binary, unary = f in (ADD, MUL), f == NEG
    if (binary and right) or unary:
        na = _nearest(seq, pos, '-')
        if na == fi:                                         # right under a minus: no '+', no second minus; at the root's minus no x
            m[ADD] = m[NEG] = 0
            if na == 0:
                m[X] = 0
        if na != -1 and _tok(seq, (na - 1) // 2) == '+':      # a - b next to + b: what would repeat an operand of the enclosing sum
            ops = []
            seen = {na}
            at_root = _plus_chain(seq, (na - 1) // 2, seen, ops)
            operands = [_prefix(seq, r) for r in ops] + ([[X]] if at_root else [])
            m[_completing(_prefix(seq, na)[1:], operands)] = 0
    if f == ADD or (binary and right) or unary:
        pa = _nearest(seq, pos, '+')
        if pa != -1:
            side = 2 * pa + 1 if (f == ADD and not right) else 2 * pa + 2
            ops = []
            _plus_chain_minus(seq, pa, {side}, ops)
            m[_completing(_prefix(seq, side), [_prefix(seq, r) for r in ops])] = 0
    if unary or (binary and right and seq[pos - 1] in CONSTANTS):      # no arithmetic among constants alone
        m[list(CONSTANTS)] = 0
    if f in (ADD, NEG):                                      # no constant right under '+' or '-'
        m[list(CONSTANTS)] = 0
    if f == ADD and right and seq[pos - 1] in LEAVES and seq[pos - 1] != RANDX:
        m[seq[pos - 1]] = 0                                  # x + x
    if f == MUL:
        m[MUL] = m[NEG] = 0
        if right:
            m[list(CONSTANTS if seq[pos - 1] in CONSTANTS else NON_CONSTANTS)] = 0      # exactly one side of '*' is a constant
    if pos <= 6:                                             # the second and third layers (the agent's copy of get_mask: which_layer(pos) <= 3)
        if f == MUL:
            m[list(VARIABLES)] = 0
        elif (binary and right and seq[pos - 1] in LEAVES) or unary:
            m[list(LEAVES)] = 0
    if pos >= 2 ** (MAX_LAYER - 1) - 1:                      # the last layer holds leaves
        m[list(OPERATORS)] = 0
    return m


def next_position(seq, pos):
    """Where the pre-order generation goes after slot `pos` was written: the left child of an operator, else the first open right child on the way up."""
    if seq[pos] in OPERATORS:
        return 2 * pos + 1
    while pos > 0:
        pos = (pos - 1) // 2
        if seq[pos] in (ADD, MUL) and seq[2 * pos + 2] == -1:
            return 2 * pos + 2
    return -1


def constant_value(c32, token):
    """The float64 a constant enters the rule with: the reference prints ``c * 10 ** e`` (a numpy float32 scalar; e = -1 for C-1, 0 for C0) with str()
    and Python parses that string."""
    return float(str(np.float32(c32) * 10 ** (-1 if token == CM1 else 0)))


def rule_constants(tokens, c32):
    """[.., 63] tokens and float32 constants -> float64 values per slot (0 where the slot holds no constant)."""
    tokens, c32 = np.asarray(tokens), np.asarray(c32, dtype=np.float32)
    out = np.zeros(tokens.shape, dtype=np.float64)
    for i in zip(*np.nonzero((tokens == CM1) | (tokens == C0))):
        out[i] = constant_value(c32[i], tokens[i])
    return out


def infix(tokens, c32, p=0):
    """The string the reference hands to its optimizer (construct_action): (left op right), -(child)."""
    t = tokens[p]
    if t in (ADD, MUL):
        return '(' + infix(tokens, c32, 2 * p + 1) + VOCAB[t] + infix(tokens, c32, 2 * p + 2) + ')'
    if t == NEG:
        return '-(' + infix(tokens, c32, 2 * p + 1) + ')'
    return str(np.float32(c32[p]) * 10 ** (-1 if t == CM1 else 0)) if t in CONSTANTS else VOCAB[t]


class Actor(nn.Module):
    """lstm.py:13-31: nn.LSTM(252 -> 16), the token head 16 -> 11, the constant head 16 -> 4, the state encoder 9 -> 16."""

    def __init__(self):
        super().__init__()
        self.lstm = nn.LSTM(N_SLOT * CODE_LEN, HIDDEN, 1, batch_first=True)
        self.output_net = nn.Linear(HIDDEN, N_TOK)
        self.x_to_c = nn.Linear(FEA_DIM, HIDDEN)
        self.constval_net = nn.Linear(HIDDEN, NUM_C)


class Symbol_Agent(Basic_Agent):
    def __init__(self, config):
        super().__init__(config)
        config.skip_step = config.test_skip_step = SKIP_STEP
        config.fea_dim = FEA_DIM
        self.__config = config
        self.actor = Actor()
        self.__masks = {}
        self.__learning_step = 0
        self.__cur_checkpoint = 0
        if getattr(config, 'agent_save_dir', None):
            save_class(config.agent_save_dir, 'checkpoint0', self)
        self.__cur_checkpoint = 1

    @property
    def learn_steps(self):
        return self.__learning_step

    def load_exported_weights(self, npz, prefix='', learn_steps=0):
        """The actor's ten arrays (tests/golden/symbol_policy.npz holds checkpoints 0 and 20 of the shipped bbob_easy run under 'w0/' and 'w20/')."""
        self.actor.load_state_dict({k: torch.as_tensor(np.asarray(npz[prefix + k]), dtype=torch.float32) for k in KEYS})
        self.__learning_step = int(learn_steps)
        return self

    def to(self, device):
        self.__config.device = device          # the actor stays on the host: the grammar mask is host work, token by token
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

    def mask(self, seq, pos):
        key = (np.asarray(seq, dtype=np.int8).tobytes(), int(pos))
        m = self.__masks.get(key)
        if m is None:
            if len(self.__masks) >= MASK_CACHE_MAX:
                self.__masks.clear()
            m = self.__masks[key] = grammar_mask([int(v) for v in seq], int(pos))
        return m

    def mask_cache_size(self):
        return len(self.__masks)

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_Symbol_Agent__masks'] = {}          # a cache, not part of the agent
        return state

    @torch.no_grad()
    def generate(self, state, chooser=None, record=None):
        """state [B, 9] -> (tokens [B, 63] int64, constants [B, 63] float32 as the actor drew them).  lstm.py:34-133 over the whole batch, finished rows
        dropped.  chooser(kind, rows, step, logits) -> choices replaces the Categorical draw ('token': logits [n, 11] before the mask; 'const': [n, 4]);
        record(rows, step, seqs, positions, masks, logits) sees every step."""
        x = torch.as_tensor(np.asarray(state), dtype=torch.float32).reshape(-1, FEA_DIM)
        B = x.shape[0]
        h = torch.zeros(1, B, HIDDEN)
        c = self.actor.x_to_c(x).unsqueeze(0)
        seq = -np.ones((B, N_SLOT), dtype=np.int64)
        c32 = np.zeros((B, N_SLOT), dtype=np.float32)
        x_in = torch.zeros(B, 1, N_SLOT * CODE_LEN)
        pos = np.zeros(B, dtype=np.int64)
        rows = np.arange(B)
        step = 0
        while len(rows):
            out, (h, c) = self.actor.lstm(x_in, (h, c))
            logits = self.actor.output_net(out)[:, 0]
            masks = np.stack([self.mask(seq[r], p) for r, p in zip(rows, pos)])
            if record is not None:
                record(rows, step, seq[rows], pos, masks, logits.numpy().copy())
            if chooser is not None:
                choice = np.asarray(chooser('token', rows, step, logits.numpy()), dtype=np.int64)
            else:
                prob = torch.softmax(logits.masked_fill(torch.from_numpy(masks) == 0, -np.inf), dim=-1)
                choice = Categorical(prob).sample().numpy()
            is_c = np.isin(choice, CONSTANTS)
            if is_c.any():
                lc = self.actor.constval_net(out[torch.from_numpy(is_c)])[:, 0]
                if chooser is not None:
                    kc = torch.as_tensor(np.asarray(chooser('const', rows[is_c], step, lc.numpy()), dtype=np.int64))
                else:
                    kc = Categorical(torch.softmax(lc, dim=-1)).sample()
                c32[rows[is_c], pos[is_c]] = (MIN_C + kc * C_INTERVAL).to(torch.float32).numpy()
            code = ((choice[:, None] + 1) >> np.arange(CODE_LEN - 1, -1, -1)[None, :]) & 1
            x_in = x_in.clone()
            for q in range(CODE_LEN):
                x_in[np.arange(len(rows)), 0, pos * CODE_LEN + q] = torch.from_numpy(code[:, q].astype(np.float32))
            seq[rows, pos] = choice
            pos = np.array([next_position(seq[r], p) for r, p in zip(rows, pos)], dtype=np.int64)
            keep = pos != -1
            kt = torch.from_numpy(keep)
            rows, pos, x_in, h, c = rows[keep], pos[keep], x_in[kt], h[:, kt], c[:, kt]
            step += 1
        return seq, c32

    def act(self, state, chooser=None):
        """state [B, 9] -> (tokens [B, 63] int32, constants [B, 63] float64): what mbx_symbol_rollout takes."""
        seq, c32 = self.generate(state, chooser)
        return seq.astype(np.int32), rule_constants(seq, c32)

    def rollout_episode(self, env, chooser=None):
        """symbol_agent.py:283-296 through the B = 1 view."""
        env.optimizer.is_train = False
        state = env.reset()
        R, done = 0., False
        while not done:
            tokens, consts = self.act(np.asarray(state, dtype=np.float32)[None, :], chooser)
            state, reward, done = env.step({'tokens': tokens[0], 'consts': consts[0], 'skip_step': SKIP_STEP})
            R += reward
        return {'cost': env.optimizer.cost, 'fes': env.optimizer.fes, 'return': R}

    def rollout_batch(self, env):
        """Whole episodes of a BatchedPBO_Env: per action one pass of the actor over the live instances and ONE launch of mbx_symbol_rollout."""
        return Symbol_Agent.rollout_checkpoints([self], env)

    @staticmethod
    def rollout_checkpoints(agents, env):
        """Whole episodes of a BatchedPBO_Env whose instances are len(agents) equal blocks, block k under the policy agents[k] -- the checkpoints of a
        ``--rollout`` table, batched host-side: per action one pass of every actor over the live instances of its block and ONE launch for all of them."""
        bc = env.batch.cfg
        state = env.reset()
        n_actions = -(-(bc.max_fes - bc.np) // (SKIP_STEP * bc.np))      # actions until fes >= maxFEs
        if env.B % len(agents):
            raise ValueError(f'Symbol_Agent.rollout_checkpoints: {env.B} instances are not {len(agents)} equal blocks')
        block = env.B // len(agents)
        tokens = np.zeros((env.B, N_SLOT), dtype=np.int32)
        consts = np.zeros((env.B, N_SLOT), dtype=np.float64)
        tokens[:, 0], tokens[:, 1], tokens[:, 2] = ADD, X, GB            # what a finished instance is handed: never run
        tokens[:, 3:] = -1
        for a in range(n_actions):
            live = np.nonzero(env.batch.done.cpu().numpy() == 0)[0] if a else np.arange(env.B)
            if not len(live):
                break
            feats = state.cpu().numpy().astype(np.float32)
            for k, agent in enumerate(agents):
                mine = live[(live >= k * block) & (live < (k + 1) * block)]
                if len(mine):
                    tokens[mine], consts[mine] = agent.act(feats[mine])
            state, _, _, _ = env.batch.symbol_rollout(tokens, consts, SKIP_STEP)
        res = env.results()
        return {'cost': res['cost'], 'fes': res['fes'], 'return': res['return'], 'steps': res['steps'], 'cost_len': res['cost_len']}
