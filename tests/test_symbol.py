"""SYMBOL (MBX_ALGO_SYMBOL = 27): the update rule as data -- metabox_amd/csrc/mbx_symbol.hpp, tests/symbol_exact.py, Symbol_Optimizer / Symbol_Agent.

CPU: the numpy restatement against the reference's recorded traces (tests/golden/symbol_traces*.npz: candidates, population state, counters, curve, reward,
done bit for bit when fed the reference's costs; features within E_FEAT), the host grammar mask, strings, constants and logits against
tests/golden/symbol_policy.npz, the agent and the ABI.  GPU: the kernel against the restatement fed the kernel's own costs, on every route.
"""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import symbol_exact as sx  # noqa: E402
from oracle import oracle  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
ALGO_SYMBOL = 27
NP_REF, D_REF, NLOG = 100, 10, 50
LB, UB = -5., 5.
# 4 x the largest difference, over the fixtures, between the reference's recorded float64 features and a long-double restatement
# (test_feature_bound_from_the_fixtures measures it: 3.033e-16 -> 1.2133e-15)
E_FEAT = 1.2133e-15
# 4 x the largest difference between the reference's LSTM run on one tree and on all trees of a checkpoint at once (tools/gen_golden.py symbol: 1.9e-6)
E_LOGIT = 7.63e-6


def _load_traces():
    data = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'symbol_traces*.npz'))):
        with np.load(path) as z:
            data.update({k: z[k] for k in z.files})
    return data


@pytest.fixture(scope='module')
def traces():
    return _load_traces()


@pytest.fixture(scope='module')
def policy():
    with np.load(os.path.join(GOLDEN, 'symbol_policy.npz')) as z:
        return {k: z[k] for k in z.files}


def _episode(traces, key):
    pre = key + '/'
    return {k[len(pre):]: v for k, v in traces.items() if k.startswith(pre)}


def _idx_rows(ep):
    """Per action the index rows [5, max(1, nrx), NP] of the flat record."""
    out, off = [], 0
    for nrx in ep['nrx']:
        n = 5 * max(1, int(nrx)) * NP_REF
        out.append(ep['idx'][off:off + n].reshape(5, max(1, int(nrx)), NP_REF))
        off += n
    assert off == len(ep['idx'])
    return out


def _stop_rule(key):
    return True            # every bbob / bbob-noisy problem knows its optimum


def _replay(ep, key, on_sub=None, on_action=None):
    """The restatement over a recorded episode, fed the reference's costs."""
    pop = sx.initial(ep['x0'], ep['cost0'])
    idx = _idx_rows(ep)
    max_fes, log_interval, nlog = int(ep['max_fes']), int(ep['log_interval']), int(ep['n_logpoint'])
    for a in range(len(ep['fes'])):
        tok, cst = ep['tok'][a].astype(np.int64), ep['cval'][a]
        for s in range(5):
            cand = sx.candidates(pop, tok, cst, idx[a][s], LB, UB)
            sx.apply_costs(pop, cand, ep['sub_cost'][a, s])
            if on_sub:
                on_sub(a, s, pop, cand)
        feat = sx.features(pop, LB, UB, max_fes)
        reward, done = sx.end_action(pop, max_fes, log_interval, nlog, _stop_rule(key))
        if on_action:
            on_action(a, pop, feat, reward, done)
    return pop


# ------------------------------------------------------------------------------------------------ CPU: the restatement against the reference
def test_fixture_inventory(traces, policy):
    cases = [str(c) for c in traces['cases']]
    assert len(cases) == 8 and sum(c.startswith('bbob-noisy') for c in cases) == 3
    fids = {c.split('/')[1] for c in cases}
    assert {'1', '10', '15', '16', '101', '102', '103'} <= fids
    hand = {k.split('/')[1] for k in policy if k.startswith('hand/')}
    assert {'three', 'full', 'chain', 'consts'} <= hand
    assert int(np.sum(policy['hand/full/tok'] == sx.RANDX)) == 32 and int(np.sum(policy['hand/full/tok'] >= 0)) == 63
    assert len(policy['tree_tok']) >= 200 and set(policy['tree_ckpt']) == {0, 20}
    for c in cases:
        ep = _episode(traces, c)
        if c != 'bbob/1/2731':
            assert ep['fes'][-1] == 20100 and len(ep['curve']) == 42 and len(ep['fes']) == 40 and ep['done'][-1] == 1 and not ep['done'][:-1].any()


def test_restatement_reproduces_every_recorded_substep_and_action(traces):
    n_sub = n_full = 0
    for key in (str(c) for c in traces['cases']):
        ep = _episode(traces, key)
        keep = set(int(a) for a in ep['full_actions'])
        state = {}

        def on_sub(a, s, pop, cand):
            nonlocal n_sub, n_full
            n_sub += 1
            sc = ep['sub_sc'][a, s]
            assert (pop['gbest'], pop['gworst'], pop['cbest'], pop['cbest_idx'], pop['stag'], pop['fes']) == tuple(sc), (key, a, s)
            if a in keep:
                n_full += 1
                f = lambda k: ep[f'full{a}/sub/{k}'][s]
                assert np.array_equal(cand, f('pos')), (key, a, s, 'before_select_pos')
                prev = ep[f'full{a}/pre/pos'] if s == 0 else ep[f'full{a}/sub/pos'][s - 1]
                assert np.array_equal(pop['dx'], f('pos') - prev), (key, a, s, 'delta_x')
                for k in ('pb', 'pbc', 'gb', 'gw', 'cb'):
                    assert np.array_equal(pop[k], f(k)), (key, a, s, k)
                assert np.array_equal(pop['cost'], ep['sub_cost'][a, s])

        def on_action(a, pop, feat, reward, done):
            assert reward == ep['reward'][a] and done == bool(ep['done'][a]) and pop['fes'] == ep['fes'][a], (key, a)
            assert len(pop['curve']) == ep['cost_len'][a] and pop['gbest'] == ep['gbest'][a]
            if a + 1 in keep:                                        # the state the next recorded action starts from
                state[a + 1] = {k: np.array(pop[k]) for k in ('x', 'dx', 'pb', 'pbc', 'gb', 'gw', 'cb', 'cost')}
        pop = _replay(ep, key, on_sub, on_action)
        assert np.array_equal(np.array(pop['curve']), ep['curve']), key
        for a, st in state.items():
            g = lambda k: ep[f'full{a}/pre/{k}']
            assert np.array_equal(st['x'], g('pos')) and np.array_equal(st['dx'], g('dx')) and np.array_equal(st['pb'], g('pb')), (key, a)
            for k in ('pbc', 'gb', 'gw', 'cb', 'cost'):
                assert np.array_equal(st[k], g(k)), (key, a, k)
    assert n_sub == 5 * (7 * 40 + 12) and n_full >= 5 * (7 * 3 + 2)


def _features_ld(pop, max_fes):
    """feature_encoding in numpy long double (sums by math.fsum-free plain long-double accumulation)."""
    LD = np.longdouble
    x, c = pop['x'].astype(LD), pop['cost'].astype(LD)
    NP, D = x.shape
    gb, gw, cbv = LD(pop['gbest']), LD(pop['gworst']), LD(pop['cbest'])
    den = gw - gb + LD(1e-8)
    maxd = np.sqrt((LD(UB) - LD(LB)) ** 2 * D)
    dist = lambda p: np.sqrt(np.sum((x - p.astype(LD)[None, :]) ** 2, axis=-1))
    diff = x[:, None, :] - x[None, :, :]
    fit = np.where(np.arange(NP) < NP // 2, gw, gb).astype(LD)
    return np.array([np.mean((c - gb) / den), np.mean(np.sqrt(np.sum(diff * diff, axis=-1))) / maxd, np.std(c) / (np.std(fit) + LD(1e-8)),
                     (LD(max_fes) - LD(pop['fes'])) / LD(max_fes), LD(pop['stag']) / LD(max_fes // NP), np.mean(dist(pop['cb']) / maxd),
                     np.mean((c - cbv) / den), np.mean(dist(pop['gb']) / maxd), LD(1. if pop['gbest'] < pop['pre_gbest'] else 0.)], dtype=LD)


def test_feature_bound_from_the_fixtures(traces):
    """E_FEAT = 4 x the largest |recorded feature - long-double restatement| over every recorded action; the kernel-order restatement stays inside it."""
    base = worst = 0.
    for key in (str(c) for c in traces['cases']):
        ep = _episode(traces, key)
        max_fes = int(ep['max_fes'])

        def on_action(a, pop, feat, reward, done, ep=ep, max_fes=max_fes):
            nonlocal base, worst
            ld = _features_ld(dict(pop, sub=5), max_fes)
            base = max(base, float(np.max(np.abs(ep['feat'][a].astype(np.longdouble) - ld))))
            worst = max(worst, float(np.max(np.abs(ep['feat'][a] - feat))))
        _replay(ep, key, None, on_action)
        assert np.max(np.abs(sx.features(sx.initial(ep['x0'], ep['cost0']), LB, UB, max_fes) - ep['state0'])) <= E_FEAT
    print(f'e_feat_base {base:.3e}  4 x = {4 * base:.3e}  kernel-order restatement vs recorded {worst:.3e}')
    assert 4 * base <= E_FEAT <= 4.01 * base, (base, E_FEAT)
    assert worst <= E_FEAT, worst



# ------------------------------------------------------------------------------------------------ CPU: the host policy
def test_host_mask_equals_every_recorded_mask(policy):
    from metabox_amd.agent import symbol_agent as sa
    n = 0
    for seqs, poss, masks in ((policy['tok_seq'], policy['tok_pos'], policy['tok_mask']), (policy['rnd_seq'], policy['rnd_pos'], policy['rnd_mask'])):
        for seq, pos, mask in zip(seqs, poss, masks):
            got = sa.grammar_mask([int(v) for v in seq], int(pos))
            assert np.array_equal(got, mask), (seq[seq >= 0], pos, got, mask)
            n += 1
    assert n == len(policy['tok_pos']) + len(policy['rnd_pos']) and n > 5000
    assert len({(bytes(s), int(p)) for s, p in zip(policy['tok_seq'], policy['tok_pos'])}) < len(policy['tok_pos'])           # what the memo saves
    # the walk after a token: every recorded tree is re-grown slot by slot
    for tree in policy['tree_tok']:
        seq, pos, order = [-1] * 63, 0, []
        while pos != -1:
            seq[pos] = int(tree[pos])
            order.append(pos)
            pos = sa.next_position(seq, pos)
        assert seq == [int(v) for v in tree] and order == _pre_order(tree)


def _pre_order(tok, p=0):
    if p >= 63 or tok[p] == -1:
        return []
    return [p] + _pre_order(tok, 2 * p + 1) + _pre_order(tok, 2 * p + 2)


def test_infix_and_constants_equal_the_recorded_strings(policy):
    """The string the reference built for every recorded tree, and the float64 every constant enters the rule with (the str() round trip of a numpy
    float32 product): the constants the kernel is handed are exactly the numbers in that string."""
    import re
    from metabox_amd.agent import symbol_agent as sa
    assert sa.NUM_C == 4
    seen = set()
    trees = list(zip(policy['tree_tok'], policy['tree_cst'], policy['tree_expr']))
    trees += [(policy[f'hand/{n}/tok'], policy[f'hand/{n}/cst'], policy[f'hand/{n}/expr']) for n in ('three', 'full', 'chain', 'consts', 'de')]
    for tok, c32, expr in trees:
        tok = tok.astype(np.int64)
        assert sa.infix(tok, c32) == str(expr)
        vals = sa.rule_constants(tok, c32)
        assert sx.infix(tok, vals) == str(expr) and sx.well_formed(tok)
        in_string = [float(v) for v in re.findall(r'(?<![a-z0-9.])-?\d+\.\d+(?:e-?\d+)?', str(expr))]
        order = [p for p in _in_order(tok) if tok[p] in (sx.CM1, sx.C0)]
        assert [vals[p] for p in order] == in_string, (expr, vals[order])
        seen.update(str(v) for v in in_string)
    assert {'0.20000005', '-0.02', '-0.6'} <= seen, seen
    assert sa.constant_value(np.float32(-1. + 3 * np.float32(0.4)), sa.C0) == 0.20000005 and sa.constant_value(np.float32(-1.) + np.float32(2) * np.float32(0.4), sa.CM1) == -0.02


def _in_order(tok, p=0):
    if p >= 63 or tok[p] == -1:
        return []
    return _in_order(tok, 2 * p + 1) + [p] + _in_order(tok, 2 * p + 2)


def _agent(policy, ckpt, tmp_path=None):
    from metabox_amd.agent import Symbol_Agent
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--agent_save_dir', str(tmp_path) + '/agents/' if tmp_path else '/nonexistent/'])
    if tmp_path is None:
        cfg.agent_save_dir = None
    return Symbol_Agent(cfg).load_exported_weights(policy, prefix=f'w{ckpt}/'), cfg


def test_logits_within_the_batch_bound(policy):
    """Teacher-forced on the recorded choices, ALL trees of a checkpoint in one batch: the float32 logits before the mask against the recorded ones, which the
    reference computed one tree at a time.  E_LOGIT = 4 x the difference the reference's own LSTM shows between those two ways of running it."""
    assert float(policy['e_logit']) == 4 * float(policy['e_logit_base']) and 4 * float(policy['e_logit_base']) <= E_LOGIT <= 4.1 * float(policy['e_logit_base'])
    first = list(policy['tree_first']) + [len(policy['tok_pos'])]
    worst = 0.
    for ckpt in (0, 20):
        agent, _ = _agent(policy, ckpt)
        ids = [i for i in range(len(policy['tree_tok'])) if policy['tree_ckpt'][i] == ckpt]
        seen = []

        def chooser(kind, rows, step, logits):
            if kind == 'token':
                return [policy['tok_choice'][first[ids[r]] + step] for r in rows]
            return [int(round((float(policy['tok_cval'][first[ids[r]] + step]) + 1.) / 0.4)) for r in rows]

        def record(rows, step, seqs, poss, masks, logits):
            nonlocal worst
            for j, r in enumerate(rows):
                k = first[ids[r]] + step
                assert np.array_equal(seqs[j], policy['tok_seq'][k]) and poss[j] == policy['tok_pos'][k] and np.array_equal(masks[j], policy['tok_mask'][k])
                worst = max(worst, float(np.max(np.abs(logits[j] - policy['tok_logits'][k]))))
                seen.append(k)
        tok, c32 = agent.generate(policy['tree_state'][ids], chooser, record)
        assert np.array_equal(tok, policy['tree_tok'][ids]) and np.array_equal(c32, policy['tree_cst'][ids])
        assert sorted(seen) == [k for i in ids for k in range(first[i], first[i + 1])]
        assert agent.mask_cache_size() < len(seen)
    print(f'logits: batch of many against the recorded batch of one {worst:.3e} (bound {E_LOGIT:.3e})')
    assert worst <= E_LOGIT


def test_agent_by_name_pickles_and_refuses_training(policy, tmp_path):
    import pickle
    import metabox_amd.agent as agents
    import metabox_amd.optimizer as optimizers
    assert hasattr(agents, 'Symbol_Agent') and hasattr(optimizers, 'Symbol_Optimizer')
    agent, cfg = _agent(policy, 20, tmp_path)
    assert os.path.exists(cfg.agent_save_dir + 'checkpoint0.pkl')
    again = pickle.loads(pickle.dumps(agent))
    for k, v in agent.actor.state_dict().items():
        assert np.array_equal(v.numpy(), again.actor.state_dict()[k].numpy()) and np.array_equal(v.numpy(), policy['w20/' + k])
    for call in (agent.train_episode, agent.train_batch):
        with pytest.raises(NotImplementedError, match='MadDE teacher'):
            call(None)
    # sampling: every drawn tree is well formed and respects the mask; two agents under one torch seed draw the same trees
    import torch
    st = policy['tree_state'][:64]
    torch.manual_seed(3)
    tok, c32 = agent.generate(st)
    torch.manual_seed(3)
    tok2, c2 = again.generate(st)
    assert np.array_equal(tok, tok2) and np.array_equal(c32, c2) and all(sx.well_formed(t) for t in tok)
    tokens, consts = agent.act(st[:4], chooser=None)
    assert tokens.dtype == np.int32 and consts.dtype == np.float64 and tokens.shape == consts.shape == (4, 63)


def test_agent_replays_a_recorded_episode(traces, policy):
    """Fed the recorded features, the agent forced to the recorded choices writes the recorded trees and hands over the recorded constants."""
    agent, _ = _agent(policy, 20)
    ep = _episode(traces, 'bbob/1/2701')
    first = list(policy['tree_first']) + [len(policy['tok_pos'])]
    states = np.concatenate([ep['state0'][None, :], ep['feat'][:-1]]).astype(np.float32)
    for a in range(len(ep['fes'])):
        assert np.array_equal(policy['tree_state'][a], states[a])               # the first 40 recorded trees are this episode's
        chooser = lambda kind, rows, step, logits, a=a: ([policy['tok_choice'][first[a] + step]] if kind == 'token' else
                                                         [int(round((float(policy['tok_cval'][first[a] + step]) + 1.) / 0.4))])
        tokens, consts = agent.act(states[a][None, :], chooser)
        assert np.array_equal(tokens[0], ep['tok'][a]) and np.array_equal(consts[0], ep['cval'][a]), a


def test_abi_geometry_of_symbol():
    import re
    from metabox_amd import _abi
    lib = _abi.load_lib()
    lib.mbx_last_error.restype = C.c_char_p
    assert _abi.ALGO_SYMBOL == ALGO_SYMBOL
    for NP, D in ((4, 2), (100, 10), (128, 40)):
        cfg = oracle.make_cfg(ALGO_SYMBOL, NP, D, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(cfg)) == 9 and lib.mbx_action_dim(C.byref(cfg)) == 126
        assert lib.mbx_tape_stride(C.byref(cfg)) == sx.tape_stride(NP, D)
    for NP, D in ((3, 10), (129, 10), (100, 41), (100, 1)):
        cfg = oracle.make_cfg(ALGO_SYMBOL, NP, D, 20000, 400, 50)
        assert lib.mbx_state_dim(C.byref(cfg)) == -3 and b'SYMBOL' in lib.mbx_last_error(), (NP, D)          # MBX_E_UNSUPPORTED, like a protein batch
    root = os.path.dirname(HERE)
    declared = set(re.findall(r'\b(mbx_symbol_[a-z_]+)\s*\(', open(os.path.join(root, 'include', 'mbx_symbol.h')).read()))
    assert declared == set(_abi.SYMBOL_SYMBOLS) == {'mbx_symbol_rollout'} and all(hasattr(lib, n) for n in declared)
    assert not declared & set(_abi.EXPORTED_SYMBOLS) and len(_abi.EXPORTED_SYMBOLS) == 45
    assert sx.offsets(100, 10, 50)['total'] == 3 * 1000 + 2 * 100 + 3 * 10 + 10 + 16 + 51 + 3200 + 1


# ------------------------------------------------------------------------------------------------ GPU
from helpers import problems  # noqa: E402

gpu = pytest.mark.gpu
F_ROLLOUT_PER_GENERATION = 4


@pytest.fixture(scope='module')
def suites():
    from metabox_amd.suite import Suite
    cache = {}

    def get(suite, dim):
        if (suite, dim) not in cache:
            ps = problems(suite, dim)
            ids = sorted(ps)
            cache[(suite, dim)] = (Suite([ps[i] for i in ids]), ids)
        return cache[(suite, dim)]
    return get


def _batch(s, pidx, NP, seeds=None, flags=0, early_stop=True, max_fes=20000):
    from metabox_amd.suite import Batch
    n = len(pidx)
    return Batch(s, ALGO_SYMBOL, pidx, np.arange(n, dtype=np.uint64) + 11 if seeds is None else seeds, NP, max_fes, max_fes // NLOG, NLOG, early_stop=early_stop, flags=flags)


def _set_tape(b, rows):
    import torch
    b.set_tape(torch.from_numpy(np.ascontiguousarray(np.stack(rows))).cuda())


def _kernel_costs(s, k, cand, noise=None):
    """The evaluator every kernel shares, through mbx_eval: cost = f [noisy by the tape's draws] - optimum."""
    p = s.problems[k]
    f = s.eval(k, cand, noisy=noise is not None, noise_draws=noise)
    return f - p.optimum


def _cost_ok(got, want):
    return np.all(np.abs(got - want) <= 1e-10 * np.maximum(np.abs(want), 1.0))       # the bound tests/test_gpu_bbob.py applies to mbx_eval


POP_WORDS = ('x', 'pb', 'dx', 'cost', 'pbc', 'gb', 'gw', 'cb')
POP_SCALARS = ('gbest', 'gworst', 'cbest', 'cbest_idx', 'stag', 'fes', 'gen', 'sub', 'pre_gbest', 'init_cost', 'log_index', 'ret', 'done')


def _same_pop(got, want, who, words=POP_WORDS, scalars=POP_SCALARS):
    for k in words:
        assert np.array_equal(got[k], want[k]), (who, k, np.max(np.abs(got[k] - want[k])))
    for k in scalars:
        assert got[k] == want[k], (who, k, got[k], want[k])
    if 'curve' in scalars or scalars is POP_SCALARS:
        assert np.array_equal(np.array(got['curve']), np.array(want['curve'][:NLOG + 1])), (who, 'curve')


@gpu
@pytest.mark.parametrize('suite', ['bbob', 'bbob-noisy'])
def test_gpu_one_substep_teacher_forced(traces, suites, suite):
    """Every recorded sub-step planted: pre-state, program and tape.  Candidates bit for bit the reference's before_select_pos, costs within the evaluator's
    bound, every other word bit for bit the restatement fed the kernel's own costs."""
    s, ids = suites(suite, D_REF)
    n = 0
    for key in (str(c) for c in traces['cases'] if str(c).split('/')[0] == suite):
        ep = _episode(traces, key)
        k = ids.index(int(key.split('/')[1]))
        idx = _idx_rows(ep)
        b = _batch(s, [k] * 5, NP_REF)
        b.reset()
        blank = b.read_state(0)
        for a in (int(v) for v in ep['full_actions']):
            tok, cst = ep['tok'][a].astype(np.int64), ep['cval'][a]
            nrx = int(ep['nrx'][a])
            pops, tapes = [], []
            for sub in range(5):
                g = (lambda name: ep[f'full{a}/pre/{name}']) if sub == 0 else (lambda name: ep[f'full{a}/sub/{name}'][sub - 1])
                pos = g('pos')
                if sub == 0:
                    dx, cost, sc = g('dx'), g('cost'), g('sc')
                else:
                    prev = ep[f'full{a}/pre/pos'] if sub == 1 else ep[f'full{a}/sub/pos'][sub - 2]
                    dx, cost, sc = pos - prev, ep['sub_cost'][a, sub - 1], ep['sub_sc'][a, sub - 1]
                pop = dict(x=pos.copy(), pb=g('pb').copy(), dx=dx.copy(), cost=cost.copy(), pbc=g('pbc').copy(), gb=g('gb').copy(), gw=g('gw').copy(), cb=g('cb').copy(),
                           gbest=sc[0], gworst=sc[1], cbest=sc[2], cbest_idx=int(sc[3]), gbest_idx=0, stag=int(sc[4]), fes=sc[5], gen=7, sub=0, pre_gbest=sc[0],
                           init_cost=ep['cost0'].min(), log_index=60, curve=[1.], ret=0., done=False)
                pops.append(pop)
                b.write_state(sub, sx.pack(pop, NP_REF, D_REF, NLOG, blank))
                noise = ep['noise'][a, sub] if 'noise' in ep else None
                tapes.append(sx.make_tape(NP_REF, D_REF, subs=[(idx[a][sub][:nrx], noise)]))
            _set_tape(b, tapes)
            b.symbol_rollout(np.tile(tok, (5, 1)), np.tile(cst, (5, 1)), 1)
            for sub in range(5):
                got = sx.unpack(b.read_state(sub), NP_REF, D_REF, NLOG)
                want = pops[sub]
                cand = sx.candidates(want, tok, cst, idx[a][sub], LB, UB)
                assert np.array_equal(got['x'], ep[f'full{a}/sub/pos'][sub]) and np.array_equal(got['x'], cand), (key, a, sub)
                assert _cost_ok(got['cost'], ep['sub_cost'][a, sub]), (key, a, sub, np.max(np.abs(got['cost'] - ep['sub_cost'][a, sub])))
                sx.apply_costs(want, cand, got['cost'])
                _same_pop(got, want, (key, a, sub), scalars=('gbest', 'gworst', 'cbest', 'cbest_idx', 'stag', 'fes', 'gen', 'pre_gbest'))
                assert np.array_equal(got['idx'][0, :nrx], idx[a][sub][:nrx])
                n += 1
        b.close()
    assert n == (5 * (4 * 3 + 3) if suite == 'bbob' else 5 * (3 + 3 + 2))


def _drive(b, s, ks, NP, D, programs, pos_u, idx_of, noise0=None, noise_of=None, max_fes=20000, n_sub=5, check_every=1, who=''):
    """Reset by tape, then len(programs) actions by tape; after every action the whole state block of every instance against the restatement fed the
    evaluator's costs.  programs[a][i] = (tokens, constants); idx_of(a, i, sub) -> index rows; noise_of(a, i, sub) -> [3, NP] or None."""
    B = len(ks)
    lb, ub = s.problems[ks[0]].lb, s.problems[ks[0]].ub
    _set_tape(b, [sx.make_tape(NP, D, pos_u=pos_u[i], noise_init=None if noise0 is None else noise0[i]) for i in range(B)])
    st = b.reset().cpu().numpy().copy()
    pops = []
    for i in range(B):
        x0 = -ub + (ub - -ub) * pos_u[i]
        got = sx.unpack(b.read_state(i), NP, D, NLOG)
        assert np.array_equal(got['x'], x0), (who, i, 'x0')
        c0 = _kernel_costs(s, ks[i], x0, None if noise0 is None else noise0[i])
        assert np.array_equal(got['cost'], c0), (who, i, 'the kernel evaluator and mbx_eval part', np.max(np.abs(got['cost'] - c0)))
        pop = sx.initial(x0, c0)
        _same_pop(got, pop, (who, i, 'reset'))
        f = sx.features(pop, lb, ub, max_fes)
        assert np.max(np.abs(st[i] - f)) <= E_FEAT and np.array_equal(got['feat'], st[i]), (who, i, st[i] - f)
        pops.append(pop)
    done_at = [None] * B
    for a, prog in enumerate(programs):
        tapes = []
        for i in range(B):
            tok, cst = prog[i]
            tapes.append(sx.make_tape(NP, D, subs=[(idx_of(a, i, sub)[:sx.n_randx(tok)], noise_of(a, i, sub) if noise_of else None) for sub in range(n_sub)]))
        _set_tape(b, tapes)
        state, reward, done, bad = b.symbol_rollout(np.stack([p[0] for p in prog]), np.stack([p[1] for p in prog]), n_sub)
        state, reward, done, bad = state.cpu().numpy().copy(), reward.cpu().numpy().copy(), done.cpu().numpy().copy(), bad.cpu().numpy().copy()
        assert not bad.any()
        for i in range(B):
            pop = pops[i]
            if pop['done']:
                assert done[i] == 1 and reward[i] == 0.
                continue
            tok, cst = prog[i]
            for sub in range(n_sub):
                cand = sx.candidates(pop, np.asarray(tok, dtype=np.int64), cst, idx_of(a, i, sub), lb, ub)
                sx.apply_costs(pop, cand, _kernel_costs(s, ks[i], cand, noise_of(a, i, sub) if noise_of else None))
            f = sx.features(pop, lb, ub, max_fes)
            r, d = sx.end_action(pop, max_fes, max_fes // NLOG, NLOG, True)
            assert np.max(np.abs(state[i] - f)) <= E_FEAT, (who, a, i, state[i] - f)
            assert reward[i] == r and bool(done[i]) == d, (who, a, i)
            if d and done_at[i] is None:
                done_at[i] = a
            if a % check_every == 0 or a == len(programs) - 1 or d:
                _same_pop(sx.unpack(b.read_state(i), NP, D, NLOG), pop, (who, a, i))
    return pops, done_at


@gpu
@pytest.mark.parametrize('suite', ['bbob', 'bbob-noisy'])
def test_gpu_recorded_episodes_by_tape(traces, suites, suite):
    """The recorded episodes, one instance each, whole, by tape: fes 20100, 42 curve entries, done at action 40, features within E_FEAT of the restatement
    fed the evaluator's costs and the state block bit for bit."""
    s, ids = suites(suite, D_REF)
    keys = [str(c) for c in traces['cases'] if str(c).split('/')[0] == suite and str(c) != 'bbob/1/2731']
    eps = [_episode(traces, k) for k in keys]
    ks = [ids.index(int(k.split('/')[1])) for k in keys]
    idx = [_idx_rows(ep) for ep in eps]
    noisy = suite == 'bbob-noisy'
    b = _batch(s, ks, NP_REF, max_fes=20000)
    programs = [[(ep['tok'][a].astype(np.int64), ep['cval'][a]) for ep in eps] for a in range(40)]
    pops, done_at = _drive(b, s, ks, NP_REF, D_REF, programs, [ep['pos_u'] for ep in eps], lambda a, i, sub: idx[i][a][sub],
                           noise0=[ep['noise0'] for ep in eps] if noisy else None, noise_of=(lambda a, i, sub: eps[i]['noise'][a, sub]) if noisy else None,
                           check_every=13, who=suite)
    res = b.results()
    for i, ep in enumerate(eps):
        assert pops[i]['fes'] == 20100 and len(pops[i]['curve']) == 42 and done_at[i] == 39, (keys[i], done_at[i])
        assert int(res['cost_len'][i]) == 42 and float(res['fes'][i]) == 20100.
    b.close()


def _tree(spec):
    """{slot: token or (token, constant)} -> (tokens [63] int64, constants [63] float64)."""
    tok, cst = -np.ones(63, dtype=np.int64), np.zeros(63)
    for slot, v in spec.items():
        if isinstance(v, tuple):
            tok[slot], cst[slot] = sx.VOCAB.index(v[0]), v[1]
        else:
            tok[slot] = sx.VOCAB.index(v)
    return tok, cst


def _hand(policy):
    out = {}
    for name in ('three', 'full', 'chain', 'consts', 'de'):
        tok = policy[f'hand/{name}/tok'].astype(np.int64)
        c32 = policy[f'hand/{name}/cst']
        cst = np.array([float(str(np.float32(c32[p]) * 10 ** (-1 if tok[p] == sx.CM1 else 0))) if tok[p] in (sx.CM1, sx.C0) else 0. for p in range(63)])
        out[name] = (tok, cst)
    return out


MORE_TREES = [
    {0: '+', 1: '*', 2: '-', 3: ('C0', 0.5), 4: '+', 9: 'pb', 10: '-', 21: 'x', 5: 'dx'},
    {0: '*', 1: ('C-1', -0.3), 2: '+', 5: 'randx', 6: '+', 13: 'gw', 14: '-', 29: 'randx'},
    {0: '+', 1: 'dx', 2: '*', 5: '+', 11: 'gb', 12: '-', 25: 'x', 6: ('C0', 0.20000005)},
]


@gpu
@pytest.mark.parametrize('NP,D', [(4, 2), (7, 3), (100, 10), (128, 40), (96, 35), (104, 33)])
def test_gpu_edge_geometries(policy, suites, NP, D):
    """B = 1 and B = 3 (three objectives of different cost: a permuted launch order), the hand-built trees and a different tree per instance, by tape,
    against the restatement; (128, 40) keeps pbest_pos and delta_x in the state block, the small ones in LDS.  (96, 35) is the largest geometry that
    still holds them in LDS (162688 B); (104, 33) would take 163696 B with them, which fits 160 KB only without the 256 B of static LDS the sub-step kernels
    carry, so it must run without them (108784 B): every launch leaves 1 KB for static LDS."""
    from helpers import problems as _p
    from metabox_amd.suite import Suite
    ps = _p('bbob', D)
    fids = [1, 16, 10]
    s = Suite([ps[f] for f in fids])
    hand = _hand(policy)
    rs = np.random.RandomState(NP * 100 + D)
    names = ['three', 'full', 'chain', 'consts']
    for ks in ([1], [0, 1, 2]):
        B = len(ks)
        extra = [_tree(t) for t in MORE_TREES]
        programs = [[hand[names[(a + i) % 4]] for i in range(B)] for a in range(4)] + [[extra[(i + a) % 3] for i in range(B)] for a in range(2)]
        idx = rs.randint(0, NP, size=(len(programs), B, 5, 32, NP))
        pos_u = rs.random_sample((B, NP, D))
        b = _batch(s, ks, NP, max_fes=20000)
        info = b.launch_info()
        assert info['lds_bytes'] + 1024 <= 160 * 1024
        assert info['lds_bytes'] == {(100, 10): 49024, (128, 40): 159040, (96, 35): 162688, (104, 33): 108784}.get((NP, D), info['lds_bytes'])
        _drive(b, s, ks, NP, D, programs, pos_u, lambda a, i, sub: idx[a, i, sub], max_fes=20000, who=(NP, D, B))
        b.close()
    s.close()


@gpu
def test_gpu_routes_agree(policy, suites):
    """One resident launch of 5 sub-steps, five one-sub-step launches, mbx_step and a Philox run fed back as its own tape leave bit-identical blocks."""
    import torch
    s, ids = suites('bbob', D_REF)
    ks = [ids.index(1), ids.index(15), ids.index(8)]
    hand = _hand(policy)
    progs = [[hand['de'], hand['full'], _tree(MORE_TREES[1])], [hand['consts'], hand['de'], hand['three']], [_tree(MORE_TREES[0]), hand['chain'], hand['full']]]
    seeds = np.array([5, 6, 7], dtype=np.uint64)
    runs = {}
    for name, flags in (('resident', 0), ('per_substep', F_ROLLOUT_PER_GENERATION), ('step', 0), ('step_per_substep', F_ROLLOUT_PER_GENERATION)):
        b = _batch(s, ks, NP_REF, seeds=seeds, flags=flags)
        out = [b.reset().cpu().numpy().copy()]
        blocks = [[b.read_state(i) for i in range(3)]]
        for prog in progs:
            tok, cst = np.stack([p[0] for p in prog]), np.stack([p[1] for p in prog])
            if name.startswith('step'):
                assert b.action_dim == 126 and b.state_dim == 9
                st, r, d = b.step(torch.from_numpy(np.concatenate([tok.astype(np.float64), cst], axis=1)).cuda())
            else:
                st, r, d, bad = b.symbol_rollout(tok, cst, 5)
                assert not bad.cpu().numpy().any()
            out.append((st.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().copy()))
            blocks.append([b.read_state(i) for i in range(3)])
        runs[name] = (out, blocks)
        b.close()
    ref_out, ref_blocks = runs['resident']
    for name in ('per_substep', 'step', 'step_per_substep'):
        out, blocks = runs[name]
        assert np.array_equal(out[0], ref_out[0])
        for a in range(1, 4):
            for x, y in zip(out[a], ref_out[a]):
                assert np.array_equal(x, y), (name, a)
        for a in range(4):
            for i in range(3):
                assert np.array_equal(blocks[a][i], ref_blocks[a][i]), (name, a, i)
    # the Philox run as a tape: start from the resident run's block after reset, feed the index rows it kept
    b = _batch(s, ks, NP_REF, seeds=seeds + np.uint64(100))
    b.reset()
    for i in range(3):
        b.write_state(i, ref_blocks[0][i])
    for a, prog in enumerate(progs):
        drawn = [sx.unpack(ref_blocks[a + 1][i], NP_REF, D_REF, NLOG)['idx'] for i in range(3)]
        _set_tape(b, [sx.make_tape(NP_REF, D_REF, subs=[(drawn[i][sub, :sx.n_randx(prog[i][0])], None) for sub in range(5)]) for i in range(3)])
        st, r, d, _ = b.symbol_rollout(np.stack([p[0] for p in prog]), np.stack([p[1] for p in prog]), 5)
        for x, y in zip((st, r, d), ref_out[a + 1]):
            assert np.array_equal(x.cpu().numpy(), y), ('tape', a)
        for i in range(3):
            assert np.array_equal(b.read_state(i), ref_blocks[a + 1][i]), ('tape', a, i)
            assert np.all(drawn[i][:5, :sx.n_randx(prog[i][0])] < NP_REF)
    b.close()


BAD_TREES = {
    'empty_child': {0: '+', 1: 'x'},
    'leaf_root': {0: 'x'},
    'empty_root': {},
    'unknown_token': {0: '+', 1: 'x', 2: 'gb'},          # slot 2 is overwritten with 11 below
    'operator_at_the_leaves': {0: '-', 1: '-', 3: '-', 7: '-', 15: '-', 31: '-'},
    'under_a_leaf': {0: '+', 1: 'x', 2: 'gb', 3: 'pb'},
    'right_of_unary': {0: '-', 2: 'x'},
    'orphan': {0: '+', 1: 'x', 2: 'gb', 40: 'randx'},
}


@gpu
def test_gpu_malformed_programs(policy, suites):
    """Counted in d_n_bad, their instances unchanged, their neighbours unaffected -- on both entry points."""
    import torch
    s, ids = suites('bbob', D_REF)
    hand = _hand(policy)
    bad = []
    for name, spec in BAD_TREES.items():
        tok, cst = _tree(spec)
        if name == 'unknown_token':
            tok[2] = 11
        assert not sx.well_formed(tok), name
        bad.append((tok, cst))
    for t in list(hand.values()) + [_tree(t) for t in MORE_TREES]:
        assert sx.well_formed(t[0])
    good = [hand['de'], hand['full'], hand['consts'], hand['three'], _tree(MORE_TREES[0]), _tree(MORE_TREES[1]), _tree(MORE_TREES[2]), hand['chain']]
    ks = [ids.index(f) for f in (1, 2, 3, 5, 8, 10, 15, 16)]
    seeds = np.arange(8, dtype=np.uint64) + 77
    clean = _batch(s, ks, NP_REF, seeds=seeds)
    clean.reset()
    clean.symbol_rollout(np.stack([g[0] for g in good]), np.stack([g[1] for g in good]), 5)
    want = [clean.read_state(i) for i in range(8)]
    clean.close()
    for which in ([1, 3, 4, 6], [0, 2, 5, 7]):
        b = _batch(s, ks, NP_REF, seeds=seeds)
        st0 = b.reset().cpu().numpy().copy()
        before = [b.read_state(i) for i in range(8)]
        prog = [bad[i] if i in which else good[i] for i in range(8)]
        st, r, d, nb = b.symbol_rollout(np.stack([g[0] for g in prog]), np.stack([g[1] for g in prog]), 5)
        assert nb.cpu().numpy().tolist() == [int(i in which) for i in range(8)]
        for i in range(8):
            if i in which:
                assert np.array_equal(b.read_state(i), before[i]) and np.array_equal(st[i].cpu().numpy(), st0[i]) and float(r[i]) == 0. and int(d[i]) == 0
            else:
                assert np.array_equal(b.read_state(i), want[i]), i
        b.close()
    # mbx_step: a token that is no integer, a NaN and an out-of-range one are unknown tokens
    b = _batch(s, ks[:4], NP_REF, seeds=seeds[:4])
    b.reset()
    before = [b.read_state(i) for i in range(4)]
    act = np.stack([np.concatenate([g[0].astype(np.float64), g[1]]) for g in good[:4]])
    act[0, 1], act[1, 0], act[2, 2] = 5.5, np.nan, 1e300
    b.step(torch.from_numpy(act).cuda())
    for i in range(3):
        assert np.array_equal(b.read_state(i), before[i]), i
    assert np.array_equal(b.read_state(3), want[3])
    b.close()


@gpu
def test_gpu_early_stop_freezes_and_noise_by_philox(suites):
    """Sphere, gb planted next to the optimum, the contracting rule x + (gb + -(x)) * 1: every candidate lands on gb, gbest <= 1e-8 ends the episode after
    that action (not inside it), and the instance stays frozen.  Without early_stop the same action does not end it.  A noisy instance runs on Philox."""
    s, ids = suites('bbob', D_REF)
    k = ids.index(1)
    p = s.problems[k]
    rule = _tree({0: '*', 1: '+', 2: ('C0', 1.0), 3: 'gb', 4: '-', 9: 'x'})
    for early in (True, False):
        b = _batch(s, [k, k], NP_REF, early_stop=early)
        b.reset()
        pop = sx.unpack(b.read_state(0), NP_REF, D_REF, NLOG)
        pop['gb'] = np.asarray(p.opt, dtype=np.float64) + 1e-6
        b.write_state(0, sx.pack(pop, NP_REF, D_REF, NLOG, b.read_state(0)))
        tok, cst = np.stack([rule[0]] * 2), np.stack([rule[1]] * 2)
        st, r, d, _ = b.symbol_rollout(tok, cst, 5)
        got = sx.unpack(b.read_state(0), NP_REF, D_REF, NLOG)
        assert got['fes'] == 600 and got['gbest'] <= 1e-8 and got['gen'] == 5          # no end test between the sub-steps
        assert d.cpu().numpy().tolist() == [int(early), 0] and got['done'] == early
        assert len(got['curve']) == (3 if early else 2)                              # [init, the log point at fes 600 >= 400, the closing entry]
        if early:
            frozen, out = b.read_state(0), st[0].cpu().numpy().copy()
            st2, r2, d2, _ = b.symbol_rollout(tok, cst, 5)
            assert np.array_equal(b.read_state(0), frozen) and np.array_equal(st2[0].cpu().numpy(), out) and float(r2[0]) == 0. and int(d2[0]) == 1
            assert sx.unpack(b.read_state(1), NP_REF, D_REF, NLOG)['fes'] == 1100
        b.close()
    sn, idn = suites('bbob-noisy', D_REF)
    kn = [idn.index(f) for f in (101, 102, 103)]
    b = _batch(sn, kn, NP_REF)
    b.reset()
    de = _tree({0: '+', 1: '*', 2: '*', 3: ('C0', 0.5), 4: '+', 9: 'gb', 10: '-', 21: 'x', 5: '+', 11: 'randx', 12: '-', 25: 'randx', 6: ('C0', 0.5)})
    for _ in range(3):
        st, r, d, nb = b.symbol_rollout(np.stack([de[0]] * 3), np.stack([de[1]] * 3), 5)
    for i in range(3):
        got = sx.unpack(b.read_state(i), NP_REF, D_REF, NLOG)
        assert got['fes'] == 1600 and np.all(np.isfinite(got['cost'])) and np.all(got['pbc'] <= got['cost']) and got['gbest'] == got['pbc'].min()
        assert np.all(np.isfinite(st[i].cpu().numpy())) and np.all((got['x'] >= LB) & (got['x'] <= UB))
    b.close()


@gpu
@pytest.mark.parametrize('suite', ['bbob', 'bbob-noisy'])
def test_gpu_symbol_in_the_tester_and_the_b1_view(policy, tmp_path, suite):
    """--test with the pair through the Tester on two problems x two runs: rows 51 long, fes 20100, monotone curves; rollout_episode through the B = 1 view
    runs the same 40 actions."""
    import copy
    from metabox_amd.agent import Symbol_Agent
    from metabox_amd.agent.utils import save_class
    from metabox_amd.config import get_config
    from metabox_amd.environment import PBO_Env
    from metabox_amd.optimizer import Symbol_Optimizer
    from metabox_amd.tester import Tester, _lookup
    import metabox_amd.agent as agents
    import torch
    assert _lookup(agents, 'Symbol_Agent') is Symbol_Agent
    cfg = get_config(['--problem', suite, '--dim', '10', '--log_dir', str(tmp_path / 'out'), '--agent_load_dir', str(tmp_path / 'models') + '/', '--device', 'cuda',
                      '--test', '--agent_for_cp', 'Symbol_Agent', '--l_optimizer_for_cp', 'Symbol_Optimizer', '--test_runs', '2'])
    cfg.t_optimizer_for_cp = []
    acfg = copy.deepcopy(cfg)
    acfg.agent_save_dir = None
    agent = Symbol_Agent(acfg).load_exported_weights(policy, prefix='w20/')
    save_class(cfg.agent_load_dir, 'Symbol_Agent', agent)
    torch.manual_seed(5)
    t = Tester(cfg)
    t.test_set.data = t.test_set.data[:2]
    res = t.test()
    for p in t.test_set.data:
        rows, fes = res['cost'][str(p)]['Symbol_Agent'], res['fes'][str(p)]['Symbol_Agent']
        assert len(rows) == 2 and all(len(r) == 51 for r in rows) and fes == [20100., 20100.], (str(p), fes)
        assert all(np.all(np.diff(r) <= 0) and np.all(np.isfinite(r)) and r[-1] < r[0] for r in rows), str(p)
    p = t.test_set.data[0]
    env = PBO_Env(p, Symbol_Optimizer(copy.deepcopy(cfg)))
    one = agent.rollout_episode(env)
    assert one['fes'] == 20100 and len(one['cost']) == 42 and np.all(np.diff(one['cost']) <= 0) and np.isfinite(one['return'])
    with pytest.raises(ValueError, match='malformed'):
        env.reset()
        env.step({'tokens': [sx.X] + [-1] * 62, 'consts': [0.] * 63})


def _u53(a, b):
    return ((a >> 5) * 67108864.0 + (b >> 6)) * (1.0 / 9007199254740992.0)


@gpu
def test_gpu_philox_noise_and_draws_pinned_by_their_tape(policy, suites):
    """A Philox run on the uniform-noise function (F102: its draws are exact uniforms the host can rebuild) against the same run fed the tape rebuilt from
    the host's Philox under the site map of include/mbx_layout.h section 22: reset uniforms, index rows and noise draws, state blocks bit for bit."""
    SITE_ELEM_R, SITE_NOISE0_A, SITE_NOISE1_A, SITE_SYM_IDX = 4, 5, 7, 84
    s, ids = suites('bbob-noisy', D_REF)
    k = ids.index(102)
    assert s.problems[k].noise[0] == 2
    NP, D, seed = 20, D_REF, 0x1234567890
    de = _hand(policy)['de']
    runs = []
    for by_tape in (False, True):
        b = _batch(s, [k], NP, seeds=np.array([seed], dtype=np.uint64))
        ph = lambda idx, site, gen: oracle.philox(seed, idx, site, gen, 0)      # the first reset of a batch is episode 0

        def noise(site, gen):
            w = [ph(i, site, gen) for i in range(NP)]
            return np.array([[_u53(v[0], v[1]) for v in w], [_u53(v[2], v[3]) for v in w], [0.] * NP])
        if by_tape:
            pos_u = np.array([_u53(*ph(e, SITE_ELEM_R, 0)[:2]) for e in range(NP * D)]).reshape(NP, D)
            _set_tape(b, [sx.make_tape(NP, D, pos_u=pos_u, noise_init=noise(SITE_NOISE1_A, 0))])
        blocks = [b.reset().cpu().numpy().copy(), b.read_state(0)]
        for a in range(2):
            if by_tape:
                subs = []
                for sub in range(5):
                    gen = 5 * a + sub + 1
                    idx = np.array([(ph(q, SITE_SYM_IDX, gen)[0] * NP) >> 32 for q in range(2 * NP)]).reshape(2, NP)
                    subs.append((idx, noise(SITE_NOISE0_A, gen)))
                _set_tape(b, [sx.make_tape(NP, D, subs=subs)])
            st, r, d, _ = b.symbol_rollout(de[0][None, :], de[1][None, :], 5)
            blocks += [st.cpu().numpy().copy(), r.cpu().numpy().copy(), b.read_state(0)]
        runs.append(blocks)
        b.close()
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    got = sx.unpack(runs[0][-1], NP, D, NLOG)
    assert got['fes'] == NP * 11 and len(set(got['cost'])) == NP


@gpu
def test_gpu_rollout_batches_the_checkpoints(policy, tmp_path):
    """rollout() with the pair: the checkpoints of the table are ONE batch (Symbol_Agent.rollout_checkpoints), every block under its own policy; the pickle has
    the reference's schema; a pickled agent carries no mask memo."""
    import copy
    import pickle
    import torch
    from metabox_amd.agent import Symbol_Agent
    from metabox_amd.agent.utils import save_class
    from metabox_amd.config import get_config
    from metabox_amd import tester
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--log_dir', str(tmp_path / 'out'), '--agent_load_dir', str(tmp_path / 'models') + '/', '--device', 'cuda'])
    cfg.agent_for_rollout, cfg.optimizer_for_rollout, cfg.n_checkpoint, cfg.rollout_runs = ['Symbol_Agent'], ['Symbol_Optimizer'], 1, 2
    cfg.rollout_log_dir = str(tmp_path / 'rollout') + '/'
    acfg = copy.deepcopy(cfg)
    acfg.agent_save_dir = None
    for cp, w in ((0, 'w0/'), (1, 'w20/')):
        agent = Symbol_Agent(acfg).load_exported_weights(policy, prefix=w)
        agent.generate(policy['tree_state'][:8])
        assert agent.mask_cache_size() > 0
        save_class(cfg.agent_load_dir + 'Symbol_Agent/', 'checkpoint' + str(cp), agent)
        with open(cfg.agent_load_dir + 'Symbol_Agent/checkpoint' + str(cp) + '.pkl', 'rb') as f:
            assert pickle.load(f).mask_cache_size() == 0
    calls = []
    real = Symbol_Agent.rollout_checkpoints
    Symbol_Agent.rollout_checkpoints = staticmethod(lambda agents, env: (calls.append((len(agents), env.B)), real(agents, env))[1])
    torch.manual_seed(9)
    try:
        res = tester.rollout(cfg)
    finally:
        Symbol_Agent.rollout_checkpoints = staticmethod(real)
    n_prob = len(res['cost'])
    assert calls == [(2, 2 * n_prob * 2)] and os.path.exists(cfg.rollout_log_dir + 'rollout.pkl')
    for p in res['cost']:
        per_cp = res['cost'][p]['Symbol_Agent']
        assert len(per_cp) == 2
        for cp in range(2):
            assert len(per_cp[cp]) == 2 and all(len(r) == 51 and np.all(np.diff(r) <= 0) for r in per_cp[cp])
            assert res['fes'][p]['Symbol_Agent'][cp] == [20100., 20100.] and np.all(np.isfinite(res['return'][p]['Symbol_Agent'][cp]))


def test_mask_memo_is_bounded(policy, monkeypatch):
    from metabox_amd.agent import symbol_agent as sa
    agent, _ = _agent(policy, 20)
    monkeypatch.setattr(sa, 'MASK_CACHE_MAX', 50)
    import torch
    torch.manual_seed(1)
    tok, _ = agent.generate(policy['tree_state'][:100])
    assert agent.mask_cache_size() <= 50 and all(sx.well_formed(t) for t in tok)
