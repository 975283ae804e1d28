"""CPU, world_size 2, gloo: sharded epochs gather to exactly the unsharded table."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from helpers import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_results(lo, hi, nlog=5):
    """Deterministic stand-in for Batch.results(): a pure function of the global instance id (like the kernel)."""
    gid = torch.arange(lo, hi, dtype=torch.float64)
    cost = gid[:, None] * 10 + torch.arange(nlog + 1, dtype=torch.float64)[None, :]
    return {'cost': cost, 'fes': gid * 3 + 1, 'return': -gid, 'steps': (gid % 7).to(torch.int32)}


def _worker(rank, world, port, n_total, q):
    sys.path.insert(0, ROOT)
    from metabox_amd.distributed import gather_rows, pack_rows, shard_range, unpack_rows
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    lo, hi = shard_range(n_total, rank, world)
    rows = pack_rows(_fake_results(lo, hi))
    full = gather_rows(rows, n_total)
    out = unpack_rows(full)
    if rank == 0:
        q.put({k: v.numpy() for k, v in out.items()})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('n_total', [10, 11])
def test_gather_equals_unsharded(n_total):
    from metabox_amd.distributed import pack_rows, unpack_rows
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_total, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    want = unpack_rows(pack_rows(_fake_results(0, n_total)))
    for k in want:
        assert np.array_equal(got[k], want[k].numpy()), k


def _grad_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    from metabox_amd.distributed import average_gradients
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.manual_seed(0)
    net = torch.nn.Linear(3, 2)
    x = torch.full((4, 3), float(rank + 1))
    net(x).sum().backward()
    average_gradients(list(net.parameters()))
    if rank == 0:
        q.put([p.grad.clone().numpy() for p in net.parameters()])
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_averaging_world2():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_grad_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    gw, gb = q.get(timeout=120)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    # rank r sees x = r+1: d/dW sum(Wx+b) = 4*(r+1) per entry, averaged over ranks 1 and 2 -> 6; bias grad 4
    assert np.allclose(gw, 6.0) and np.allclose(gb, 4.0)


class _ScriptedShard:
    """One-instance lock-step environment whose episode lasts `T` steps: stands for a rank's shard that finishes earlier / later than
    the other rank's (the stop rule gbest <= 1e-8 and re-initialisation billing make episode lengths shard-dependent)."""

    def __init__(self, T, seed):
        self.T, self.B, self.t, self.rs = T, 1, 0, np.random.RandomState(seed)

    def reset(self):
        self.t = 0
        return torch.tensor([[0.005]], dtype=torch.float64)

    def step(self, actions):
        self.t += 1
        return (torch.tensor([[0.005 + 0.005 * self.t]], dtype=torch.float64), torch.tensor([float(self.rs.choice([-1., 1.]))], dtype=torch.float64),
                torch.tensor([1 if self.t >= self.T else 0], dtype=torch.uint8))

    def results(self):
        return {'cost': torch.tensor([[1.0, 0.5]], dtype=torch.float64)}


def _train_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    from metabox_amd.agent.rlepso_agent import RLEPSO_Agent
    from metabox_amd.config import get_config
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cpu', '--max_learning_step', '1000'])
    cfg.agent_save_dir = None
    cfg.save_interval = 10 ** 9
    torch.manual_seed(0)                                            # identical initial weights on both ranks
    agent = RLEPSO_Agent(cfg)
    torch.manual_seed(100 + rank)                                   # different action noise per rank
    exceed, info = agent.train_batch(_ScriptedShard(7 if rank == 0 else 23, rank))      # 1 segment vs 3 segments
    flat = torch.cat([p.detach().reshape(-1) for p in list(agent.actor.parameters()) + list(agent.critic.parameters())])
    q.put((rank, info['learn_steps'], flat.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_batched_training_with_unequal_episode_lengths_world2():
    """the number of gradient all-reduces per epoch used to depend on rank-local state (`while alive.any()` over the local
    shard), so ranks whose shards finished at different generations issued different numbers of collectives and hung.  Loop control is
    global now: both ranks run 3 segments x 3 optimizer steps (the finished rank contributes zero gradients) and end with identical weights."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_train_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=300) for _ in range(2)], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    assert outs[0][1] == outs[1][1] == 9
    assert np.array_equal(outs[0][2], outs[1][2])


class _ScriptedInstances:
    """Lock-step environment over the instances `ids` of a global table: per instance a fixed episode length (4 .. 12 steps) and reward sequence that
    depend on the GLOBAL id only, so any partition of the table replays the same instances."""

    def __init__(self, ids):
        self.ids, self.B, self.t = list(ids), len(ids), 0
        self.T = np.array([4 + (3 * i) % 9 for i in self.ids])
        self.rw = np.stack([np.random.RandomState(1000 + i).choice([-1., 1.], size=16) for i in self.ids])

    def reset(self):
        self.t = 0
        return torch.full((self.B, 1), 0.005, dtype=torch.float64)

    def step(self, actions):
        self.t += 1
        state = 0.005 + 0.005 * np.minimum(self.t, self.T)           # a finished instance keeps reporting its terminal state, like the kernels
        return (torch.as_tensor(state[:, None].copy()), torch.as_tensor(self.rw[:, self.t - 1].copy()), torch.as_tensor((self.t >= self.T).astype(np.uint8)))

    def results(self):
        return {'cost': torch.tensor([[1.0, 0.5]] * self.B, dtype=torch.float64)}


def _forced_actions(ids):
    return torch.as_tensor(np.stack([np.random.RandomState(2000 + i).uniform(0, 1, size=(16, 35)) for i in ids], 1).astype(np.float32))     # [T, B, 35]


def _first_ppo_gradient(ids):
    """The gradient RLEPSO_Agent.train_batch hands its optimizers at the first step of a batch over instances `ids` (after average_gradients)."""
    from metabox_amd.agent.rlepso_agent import RLEPSO_Agent
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cpu', '--max_learning_step', '1000'])
    cfg.agent_save_dir = None
    cfg.save_interval = 10 ** 9
    torch.manual_seed(0)
    agent = RLEPSO_Agent(cfg)
    params = list(agent.actor.parameters()) + list(agent.critic.parameters())
    seen = []
    opt = agent._RLEPSO_Agent__optimizer_actor
    orig = opt.step

    def step(*a, **k):
        seen.append(torch.cat([p.grad.detach().reshape(-1).clone() for p in params]))
        return orig(*a, **k)
    opt.step = step
    agent.train_batch(_ScriptedInstances(ids), max_updates=1, forced_actions=_forced_actions(ids))
    return seen[0].numpy()


def _weighted_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    q.put((rank, _first_ppo_gradient([0, 1] if rank == 0 else [2, 3, 4, 5, 6])))         # unequal shards, as cost_partition cuts them
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_of_unequal_shards_equals_the_single_rank_gradient_world2():
    """shards are cost-weighted, so ranks own different numbers of instances and each normalises its loss by its OWN live count.  The
    all-reduce weights every rank's gradient by that count (distributed.average_gradients(weight=...)): two ranks owning 2 and 5 instances must hand
    their optimizers the gradient one rank owning all 7 computes -- the objective does not depend on the world size."""
    want = _first_ppo_gradient(range(7))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_weighted_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=300) for _ in range(2)], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    assert np.array_equal(outs[0][1], outs[1][1])
    scale = np.abs(want).max()
    assert np.abs(outs[0][1] - want).max() <= 2e-6 * scale, np.abs(outs[0][1] - want).max() / scale
    # (the unweighted mean of the two per-rank means is a different vector: the test would fail by ~1e-1 of the gradient's scale)


def _c5_table():
    """BASELINE config 5's instance table: 24 bbob + 30 noisy functions at D = 40, function-sorted, 65 536 instances (problem-major)."""
    from metabox_amd.problem.bbob import BBOB_Dataset
    ps = []
    for suite in ('bbob', 'bbob-noisy'):
        tr, te = BBOB_Dataset.get_datasets(suite, 40, 5.0)
        ps += sorted(tr.data + te.data, key=lambda p: p.func_id)
    n = 65536
    pidx = (np.arange(n) * len(ps) // n).astype(np.int32)           # problem-major, 1213-1214 runs per function
    return ps, pidx


def test_cost_partition_balances_config5_and_keeps_global_order():
    """the equal-count split of the function-sorted table gives some ranks ~2x the work of others; the cost-weighted
    contiguous split keeps every rank's predicted cost within a few instances of the mean for any number of ranks."""
    from metabox_amd.distributed import cost_partition, partition_bounds, relative_cost, shard_range
    ps, pidx = _c5_table()
    cost = np.array([relative_cost(p) for p in ps])[pidx]
    for world in (2, 3, 4, 8, 16):
        b = partition_bounds(ps, pidx, world)
        assert b[0] == 0 and b[-1] == len(pidx) and np.all(np.diff(b) > 0)
        per = np.array([cost[b[r]:b[r + 1]].sum() for r in range(world)])
        assert per.max() / per.mean() <= 1.001, (world, per.max() / per.mean())
    eq = np.array([cost[slice(*shard_range(len(pidx), r, 8))].sum() for r in range(8)])
    assert eq.max() / eq.mean() > 1.15                               # what the equal-count split did (1.23 with the round-4 cost table, 1.7 with round 3's)
    # degenerate inputs: fewer instances than ranks (empty shards are legal), zero ranks' worth of cost, a single rank
    assert list(cost_partition([1., 1.], 4)) in ([0, 0, 1, 1, 2], [0, 1, 1, 2, 2], [0, 0, 1, 2, 2], [0, 1, 1, 1, 2])
    assert list(cost_partition([], 3)) == [0, 0, 0, 0] and list(cost_partition([3., 1.], 1)) == [0, 2]
    assert list(cost_partition(np.ones(10), 5)) == [0, 2, 4, 6, 8, 10]


def _c5_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    from metabox_amd.distributed import gather_rows, pack_rows, partition_bounds, unpack_rows
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    ps, pidx = _c5_table()
    bounds = partition_bounds(ps, pidx, world)
    lo, hi = int(bounds[rank]), int(bounds[rank + 1])
    full = gather_rows(pack_rows(_fake_results(lo, hi)), len(pidx), bounds=bounds)
    if rank == 0:
        q.put({k: v.numpy() for k, v in unpack_rows(full).items()})
    dist.barrier()
    dist.destroy_process_group()


def test_cost_weighted_shards_gather_to_the_unsharded_table_world8():
    """gloo, world size 8, config 5's table: shards of unequal size (cost-weighted) gather to exactly the unsharded table in global-id order."""
    from metabox_amd.distributed import pack_rows, unpack_rows
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_c5_worker, args=(r, 8, port, q)) for r in range(8)]
    for p in procs:
        p.start()
    got = q.get(timeout=300)
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    want = unpack_rows(pack_rows(_fake_results(0, 65536)))
    for k in want:
        assert np.array_equal(got[k], want[k].numpy()), k


def test_train_batched_shards_by_predicted_cost(monkeypatch, tmp_path):
    """Trainer.train_batched cuts the epoch's (problem x run) table with distributed.partition_bounds like Tester.run_pairs:
    the shards of all ranks are contiguous, cover the table once, carry global-id Philox seeds, and balance the predicted cost where the
    equal-count split of the function-sorted table did not.  (The lock-step batch itself needs the GPU: stubbed here, the split is host logic.)"""
    import types
    import metabox_amd.environment as env_mod
    import metabox_amd.suite as suite_mod
    import metabox_amd.tester as tester_mod
    from metabox_amd.distributed import instance_table, philox_seed, relative_cost, shard_range
    from metabox_amd.trainer import Trainer
    ps, _ = _c5_table()
    seen = {}

    class _Env:
        def __init__(self, problems, optimizer, pidx, seeds, suite=None):
            self.pidx, self.seeds = np.asarray(pidx), np.asarray(seeds)

        def close(self):
            pass

    class _Agent:
        def train_batch(self, env):
            seen[self.rank] = (env.pidx, env.seeds)
            return True, {'learn_steps': 1, 'return': 0.0}

    monkeypatch.setattr(env_mod, 'BatchedPBO_Env', _Env)
    monkeypatch.setattr(suite_mod, 'Suite', lambda problems: None)
    world, runs = 8, 16
    for rank in range(world):
        monkeypatch.setattr(tester_mod, '_world', lambda rank=rank: (rank, world))
        t = Trainer.__new__(Trainer)
        t.config = types.SimpleNamespace(train_batch_size=runs, log_dir=str(tmp_path), run_time='t')
        t.optimizer, t.agent = None, _Agent()
        t.agent.rank = rank
        t.train_set = types.SimpleNamespace(data=ps)
        t.train_batched(max_epochs=1)
    pidx, run = instance_table(len(ps), runs)
    seeds = philox_seed(run, np.arange(len(pidx)), epoch_salt=1)
    assert np.array_equal(np.concatenate([seen[r][0] for r in range(world)]), pidx)
    assert np.array_equal(np.concatenate([seen[r][1] for r in range(world)]), seeds)
    cost = np.array([relative_cost(p) for p in ps])
    per = np.array([cost[seen[r][0]].sum() for r in range(world)])
    eq = np.array([cost[pidx[slice(*shard_range(len(pidx), r, world))]].sum() for r in range(world)])
    assert per.max() / per.mean() < 1.05 < eq.max() / eq.mean()


def test_train_batched_falls_back_to_equal_counts_when_a_cost_shard_would_be_empty(monkeypatch, tmp_path):
    """with few instances per rank the cost midpoints can leave a rank without instances although len(table) >= world; such epochs
    used to abort with a misleading message, now they are cut in equal counts.  Fewer instances than ranks still raises, on every rank."""
    import types
    import metabox_amd.environment as env_mod
    import metabox_amd.suite as suite_mod
    import metabox_amd.tester as tester_mod
    import metabox_amd.trainer as trainer_mod
    from metabox_amd.trainer import Trainer
    ps, _ = _c5_table()
    ps = ps[:3]
    seen = {}

    class _Env:
        def __init__(self, problems, optimizer, pidx, seeds, suite=None):
            self.pidx = np.asarray(pidx)

        def close(self):
            pass

    class _Agent:
        def train_batch(self, env):
            seen[self.rank] = env.pidx
            return True, {'learn_steps': 1, 'return': 0.0}

    monkeypatch.setattr(env_mod, 'BatchedPBO_Env', _Env)
    monkeypatch.setattr(suite_mod, 'Suite', lambda problems: None)
    monkeypatch.setattr(trainer_mod, 'partition_bounds', lambda problems, pidx, world: np.array([0, 0, 2, len(pidx)]), raising=False)

    def run(world, runs):
        for rank in range(world):
            monkeypatch.setattr(tester_mod, '_world', lambda rank=rank: (rank, world))
            t = Trainer.__new__(Trainer)
            t.config = types.SimpleNamespace(train_batch_size=runs, log_dir=str(tmp_path), run_time='t')
            t.optimizer, t.agent = None, _Agent()
            t.agent.rank = rank
            t.train_set = types.SimpleNamespace(data=ps)
            t.train_batched(max_epochs=1)
    import metabox_amd.distributed as dmod
    monkeypatch.setattr(dmod, 'partition_bounds', lambda problems, pidx, world: np.array([0, 0, 2, len(pidx)]))
    run(3, 2)                                                   # 6 instances, a partition whose first shard is empty -> equal counts 2 / 2 / 2
    assert [len(seen[r]) for r in range(3)] == [2, 2, 2]
    with pytest.raises(ValueError, match='only 3 instances'):
        run(4, 1)


def test_batched_agents_declare_replication_on_the_class():
    """the flag save_class reads must be true before the first train_batch call (checkpoint0 is written in __init__) and must not travel
    in the pickled instance state."""
    from metabox_amd.agent import DE_DDQN_Agent, GLEET_Agent, LDE_Agent, RLEPSO_Agent
    for cls in (RLEPSO_Agent, LDE_Agent, GLEET_Agent, DE_DDQN_Agent):
        assert cls.__dict__.get('_mbx_replicated') is True, cls


def _save_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    from metabox_amd.agent.utils import save_class
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)

    import types
    save_class(out_dir, 'replicated', {'rank': rank})             # a plain object: per-rank state
    save_class(out_dir, 'agent', types.SimpleNamespace(_mbx_replicated=True, payload=1))
    dist.barrier()
    dist.destroy_process_group()


def test_save_class_writes_replicated_agents_once_and_per_rank_state_per_rank(tmp_path):
    """save_class used to return silently on every rank != 0 whenever a process group was up.  Now only objects that declare themselves
    replicated (the gradient-synchronised train_batch paths set `_mbx_replicated`) are left to rank 0; anything else is written by every rank."""
    ctx = mp.get_context('spawn')
    port = free_port()
    out_dir = str(tmp_path) + '/'
    procs = [ctx.Process(target=_save_worker, args=(r, 2, port, out_dir)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    names = sorted(os.listdir(out_dir))
    assert names == ['agent.pkl', 'replicated.pkl', 'replicated.rank1.pkl'], names


def test_protein_problems_weight_the_partition_by_their_close_pairs():
    """Protein-docking problems tell the inter-rank partition what a step on them costs (Protein_Docking.relative_step_cost: a fixed part + the energy walk over the atom pairs
    that can reach the 9 A cut-off inside the box, the count csrc/mbx.hip: mbx_suite_create stops the walk at); BBOB functions are priced by whole episodes per function id."""
    from metabox_amd import distributed as md
    from metabox_amd.config import get_config
    from metabox_amd.utils import construct_problem_set
    cfg = get_config(['--problem', 'protein'])
    tr, te = construct_problem_set(cfg)
    ps = (tr + te).data
    nc = np.array([p.close_pairs() for p in ps])
    assert len(ps) == 280 and 1500 < nc.min() < nc.max() < 4950 and (nc.min(), nc.max()) == (1771, 3826)
    costs = np.array([md.relative_cost(p) for p in ps])
    assert np.allclose(costs, 1.117 + 1.1715e-4 * nc) and costs.max() / costs.min() > 1.15
    pidx, _ = md.instance_table(len(ps), 64)
    bounds = md.partition_bounds(ps, pidx, 8)
    per_rank = np.array([costs[pidx[bounds[r]:bounds[r + 1]]].sum() for r in range(8)])
    assert per_rank.max() / per_rank.mean() < 1.01 and bounds[0] == 0 and bounds[-1] == 280 * 64
    # a BBOB function: whole-episode cost by function id (Sphere stops early: cheaper than its per-generation cost suggests)
    from helpers import problems
    p1, p21 = problems('bbob', 10)[1], problems('bbob', 10)[21]
    assert md.relative_cost(p1) == md.EPISODE_COST_US[10][1] and md.relative_cost(p21) / md.relative_cost(p1) > 3
