#!/usr/bin/env python
"""Throughput of the other batched paths (BASELINE.json configs 3 and 4, one GPU's share), policy included.
   python tools/kbench_algos.py [lde|ddqn|rs|rlpso|gleet|qlpso|glpso|jde21|madde|dedqn|sdmspso|nrlpso|sahlpso|les|rlhpsde|nlshade|l2l|symbol] """
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metabox_amd.config import get_config
from metabox_amd.environment import BatchedPBO_Env
from metabox_amd.utils import construct_problem_set

def timed(fn, steps):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(steps); torch.cuda.synchronize(); return time.perf_counter() - t0

which = sys.argv[1:] or ['lde', 'ddqn', 'rs', 'rlpso', 'gleet', 'qlpso']
if 'lde' in which:
    from metabox_amd.agent import LDE_Agent
    from metabox_amd.optimizer import LDE_Optimizer
    cfg = get_config(['--problem', 'bbob-noisy', '--dim', '30', '--device', 'cuda']); cfg.agent_save_dir = None
    agent = LDE_Agent(cfg).load_exported_weights(np.load(os.path.join(os.path.dirname(__file__), '..', 'metabox_amd', 'agent_model', 'lde_bbob_easy.npz'))).to('cuda')
    opt = LDE_Optimizer(cfg)
    tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
    B = 16384
    env = BatchedPBO_Env(ps, opt, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1)
    state = env.reset(); h = torch.zeros(1, B, 50, device='cuda'); c = torch.zeros(1, B, 50, device='cuda')
    def run(n):
        global state, h, c
        with torch.no_grad():
            for _ in range(n):
                a, h, c = agent.net.act_batch(state.to(torch.float32), h, c)
                state, _, _ = env.step(a.contiguous())
    run(5); dt = timed(run, 60)
    live = int((env.results()['steps'] > 0).sum())
    print(json.dumps({'path': 'LDE bbob-noisy d=30 NP=50 (reference population), 16384 instances, LSTM policy via PyTorch', 'ms_per_step': dt / 60 * 1e3, 'env_steps_per_s': B * 60 / dt}))
    env.close()
if 'ddqn' in which:
    from metabox_amd.agent import DE_DDQN_Agent
    from metabox_amd.optimizer import DE_DDQN_Optimizer
    cfg = get_config(['--problem', 'protein', '--device', 'cuda']); cfg.agent_save_dir = None
    torch.manual_seed(0)
    agent = DE_DDQN_Agent(cfg).to('cuda'); opt = DE_DDQN_Optimizer(cfg)
    tr, te = construct_problem_set(cfg); ps = (tr + te).data[:35]            # one GPU's share of config 4: 35 problems x 64 runs
    B = 35 * 64
    env = BatchedPBO_Env(ps, opt, np.repeat(np.arange(35), 64), np.arange(B, dtype=np.uint64) + 1)
    state = env.reset()
    print(json.dumps({'ddqn_launch_info': env.batch.launch_info()}))
    def run(n):
        global state
        with torch.no_grad():
            for _ in range(n):
                a = torch.argmax(agent.q_net(state.to(torch.float32)), dim=1).to(torch.int32)
                state, _, _ = env.step(a.contiguous())
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3): torch.argmax(agent.q_net(state.to(torch.float32)), dim=1).to(torch.int32)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        ga = torch.argmax(agent.q_net(state.to(torch.float32)), dim=1).to(torch.int32)
    def run_graph(n):
        for _ in range(n):
            g.replay(); env.step(ga)
    run_graph(5); dg = timed(run_graph, 200)
    print(json.dumps({'path': 'DE-DDQN protein, Q-net replayed as a hipGraph', 'ms_per_step': dg / 200 * 1e3, 'env_steps_per_s': B * 200 / dg}))
    packed = agent.packed_weights()
    def run_hip(n):
        for _ in range(n):
            env.step(env.batch.ddqn_qnet(packed))
    def run_q(n):
        for _ in range(n): env.batch.ddqn_qnet(packed)
    def run_s(n):
        a = env.batch.ddqn_qnet(packed)
        for _ in range(n): env.step(a)
    run_hip(5); dh = timed(run_hip, 200)
    print(json.dumps({'path': 'DE-DDQN protein, Q-net + argmax as one MFMA launch (mbx_ddqn_qnet; rollout_batch default)', 'ms_per_step': dh / 200 * 1e3, 'env_steps_per_s': B * 200 / dh}))
    dq = timed(run_q, 200); ds = timed(run_s, 200)
    print(json.dumps({'path': 'DE-DDQN protein: the two launches alone', 'qnet_us': dq / 200 * 1e6, 'k_dq_step_us': ds / 200 * 1e6}))
    run(5); dt = timed(run, 200)
    print(json.dumps({'path': 'DE-DDQN protein d=12 NP=100, 2240 instances (35 problems x 64 runs), Q-net via PyTorch', 'ms_per_step': dt / 200 * 1e3, 'env_steps_per_s': B * 200 / dt}))
    env.close()
if 'rs' in which:
    from metabox_amd.optimizer import Random_search
    from metabox_amd.suite import Suite
    cfg = get_config(['--problem', 'bbob', '--dim', '10'])
    tr, te = construct_problem_set(cfg); ps = (tr + te).data
    s = Suite(ps); B = 24 * 51
    rs = Random_search(cfg)
    torch.cuda.synchronize(); t0 = time.perf_counter(); rs.run_batch(s, np.repeat(np.arange(24), 51), np.arange(B)); dt = time.perf_counter() - t0
    print(json.dumps({'path': 'Random_search baseline epoch: 24 bbob problems x 51 runs, 199 populations each', 'seconds': dt}))
if 'rlpso' in which:
    from metabox_amd.agent import RL_PSO_Agent
    from metabox_amd.optimizer import RL_PSO_Optimizer
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda']); cfg.agent_save_dir = None
    agent = RL_PSO_Agent(cfg).load_exported_weights(np.load(os.path.join(os.path.dirname(__file__), '..', 'metabox_amd', 'agent_model', 'rlpso_bbob_easy.npz'))).to('cuda')
    tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
    B = 4096
    nets = agent.nets; h1, h2 = nets.hidden_sizes(); net = (nets.packed_weights(), h1, h2, nets.min_sigma, nets.max_sigma)
    for mode, steps in (('fused', 2048), ('fused1', 512), ('hip', 256), ('torch', 128)):
        env = BatchedPBO_Env(ps, RL_PSO_Optimizer(cfg), np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, early_stop=False)
        state = env.reset()
        def run(n):
            global state
            with torch.no_grad():
                if mode == 'fused':
                    for _ in range(n // 256): env.batch.rlpso_rollout(*net, 256)
                elif mode == 'fused1':
                    for _ in range(n): env.batch.rlpso_rollout(*net, 1)
                elif mode == 'hip':
                    for _ in range(n): env.step(env.batch.gauss_policy(*net))
                else:
                    for _ in range(n):
                        a, _ = nets(state.to(torch.float32)); state, _, _ = env.step(a.contiguous())
        run(256 if mode == 'fused' else 5); dt = timed(run, steps)
        print(json.dumps({'path': f'RL-PSO bbob d=10 NP=100, 4096 instances, policy={mode}', 'us_per_step': dt / steps * 1e6, 'env_steps_per_s': B * steps / dt}))
        env.close()
if 'gleet' in which:
    from metabox_amd.agent import GLEET_Agent
    from metabox_amd.optimizer import GLEET_Optimizer
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda']); cfg.agent_save_dir = None
    torch.manual_seed(0)
    agent = GLEET_Agent(cfg).to('cuda')
    tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
    B = 4096
    env = BatchedPBO_Env(ps, GLEET_Optimizer(cfg), np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, early_stop=False)
    state = env.reset()
    const = torch.full((B, 100), 0.5, dtype=torch.float32, device='cuda')
    def run_kernel(n):
        for _ in range(n): env.step(const)
    def run(n):
        global state
        for _ in range(n): state, _, _ = env.step(agent.act_batch(state))
    w = agent.actor.packed_weights()
    def run_hip(n):
        for _ in range(n): env.step(env.batch.gleet_policy(w, agent.actor.min_sigma, agent.actor.max_sigma))
    run_kernel(5); dk = timed(run_kernel, 60)
    run(3); dt = timed(run, 30)
    run_hip(5); dh = timed(run_hip, 60)
    # the resident route (mbx_gleet_rollout, the actor inside the step kernel) against the two-launch route, same batch, a fresh episode (199 steps:
    # 2 x 2 warm-up + 6 x 2 x 15), alternating windows with a device synchronisation around each; the spread of the windows is the noise
    env.batch.gleet_set_params(w, None, agent.actor.min_sigma, agent.actor.max_sigma)
    def run_resident(n):
        env.batch.gleet_rollout(n)
    env.reset(); run_hip(2); run_resident(2)
    alt = {'hip': [], 'resident': []}
    for _ in range(6):
        alt['hip'].append(timed(run_hip, 15) / 15 * 1e6); alt['resident'].append(timed(run_resident, 15) / 15 * 1e6)
    assert int(env.batch.done.sum()) == 0                            # every window ran live instances
    med = {k: float(np.median(v)) for k, v in alt.items()}
    print(json.dumps({'path': 'GLEET bbob d=10 NP=100, 4096 instances', 'kernel_us_per_step': dk / 60 * 1e6,
                      'kernel_env_steps_per_s': B * 60 / dk, 'with_torch_policy_ms_per_step': dt / 30 * 1e3, 'torch_env_steps_per_s': B * 30 / dt,
                      'with_hip_policy_us_per_step': dh / 60 * 1e6, 'hip_env_steps_per_s': B * 60 / dh,
                      'resident_us_per_step': med['resident'], 'resident_env_steps_per_s': B / med['resident'] * 1e6,
                      'alternation': {'windows': 6, 'steps_per_window': 15, 'with_hip_policy_us_per_step': [round(v, 1) for v in alt['hip']],
                                      'resident_us_per_step': [round(v, 1) for v in alt['resident']], 'with_hip_policy_median': med['hip'],
                                      'spread_us': {k: float(max(v) - min(v)) for k, v in alt.items()}}}))
    env.close()
if 'qlpso' in which:
    from metabox_amd.optimizer import QLPSO_Optimizer
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda']); cfg.agent_save_dir = None
    q = torch.from_numpy(np.load(os.path.join(os.path.dirname(__file__), '..', 'metabox_amd', 'agent_model', 'qlpso_bbob_easy.npz'))['q_table']).cuda()
    tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
    B = 4096
    env = BatchedPBO_Env(ps, QLPSO_Optimizer(cfg), np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, early_stop=False)
    env.reset()
    def run(n):
        for _ in range(n // 256): env.batch.qlpso_rollout(q, 256)
    run(256); dt = timed(run, 2048)
    print(json.dumps({'path': 'QLPSO bbob d=10 NP=30, 4096 instances, tabular policy in the kernel, 256 steps per launch', 'us_per_step': dt / 2048 * 1e6,
                      'env_steps_per_s': B * 2048 / dt}))
    env.close()
if 'glpso' in which:
    # GL-PSO (one mbx_step = one generation, two NP = 100 evaluations) next to Random_search's one-population kernel in the same process:
    # 4096 instances, bbob round-robin, fixed horizon so that every instance stays live.  Under rocprofv3 --kernel-trace --stats the
    # per-launch times of k_glpso_generation and k_rs_population come from the trace; the wall times here include the launch gaps.
    from metabox_amd._abi import ALGO_GLPSO, ALGO_RANDOM_SEARCH
    from metabox_amd.suite import Batch, Suite
    for dim in (10, 30):
        cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
        tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
        s = Suite(ps); B = 4096
        for algo, name in ((ALGO_GLPSO, 'k_glpso_generation'), (ALGO_RANDOM_SEARCH, 'k_rs_population')):
            b = Batch(s, algo, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, 100, 10 ** 8, 10 ** 6, 50, early_stop=False)
            b.reset()
            def run(n):
                for _ in range(n): b.step(None)
            run(3); dt = timed(run, 40)
            print(json.dumps({'path': f'{name} bbob d={dim} NP=100, {B} instances, one launch per generation', 'us_per_step': dt / 40 * 1e6,
                              'launch_info': b.launch_info()}))
            b.close()
if 'jde21' in which:
    # JDE21 (one mbx_step = one update: 160 big trials with crowding + 16 x 10 small trials = 320 evaluated rows) next to Random_search's
    # 100-row kernel in the same process: 4096 instances, bbob round-robin, a horizon long enough that no halving is met (bNP stays 160)
    # and every instance stays live.  Under rocprofv3 --kernel-trace --stats the per-launch times of k_jde21_generation and
    # k_rs_population come from the trace; the wall times here include the launch gaps.  A library built with -DMBX_ABLATE_CROWD (MBX_LIB)
    # gives the step without the crowding search.
    from metabox_amd._abi import ALGO_JDE21, ALGO_RANDOM_SEARCH
    from metabox_amd.suite import Batch, Suite
    for dim in (10, 30):
        cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
        tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
        s = Suite(ps); B = 4096
        for algo, name, np_ in ((ALGO_JDE21, 'k_jde21_generation', 170), (ALGO_RANDOM_SEARCH, 'k_rs_population', 100)):
            b = Batch(s, algo, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, np_, 10 ** 8, 10 ** 6, 50, early_stop=False)
            b.reset()
            def run(n):
                for _ in range(n): b.step(None)
            run(3); dt = timed(run, 40)
            print(json.dumps({'path': f'{name} bbob d={dim} NP={np_}, {B} instances, one launch per generation', 'us_per_step': dt / 40 * 1e6,
                              'launch_info': b.launch_info()}))
            b.close()
if 'madde' in which:
    # MadDE (one mbx_step = one update: NP trials, NP = 2 D^2 at the start) next to Random_search's 100-row kernel in the same process: bbob
    # round-robin, 4096 instances at D = 10 and 256 at D = 30 (2.3 MB of state each), a budget so large that NP stays at its start
    # value and every instance stays live.  Under rocprofv3 --kernel-trace --stats the per-launch times of k_madde_generation and
    # k_rs_population come from the trace; the wall times here include the launch gaps.  A library built with -DMBX_ABLATE_MD_SORT /
    # -DMBX_ABLATE_MD_ARC / -DMBX_ABLATE_MD_SUMS (MBX_LIB) gives the step without the sort and row move / the archive update / the pairwise sums
    # (the sort and row move are shared code, mbx_depop.hpp: that switch takes them out of the NL_SHADE_LBC and RL-HPSDE kernels of such a build as well).
    from metabox_amd._abi import ALGO_MADDE, ALGO_RANDOM_SEARCH
    from metabox_amd.suite import Batch, Suite
    for dim, B in ((10, 4096), (30, 256)):
        cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
        tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
        s = Suite(ps)
        for algo, name, np_ in ((ALGO_MADDE, 'k_madde_generation', 2 * dim * dim), (ALGO_RANDOM_SEARCH, 'k_rs_population', 100)):
            b = Batch(s, algo, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, np_, 10 ** 9, 10 ** 7, 50, early_stop=False)
            b.reset()
            def run(n):
                for _ in range(n): b.step(None)
            run(2); dt = timed(run, 10)
            print(json.dumps({'path': f'{name} bbob d={dim} NP={np_}, {B} instances, one launch per update', 'us_per_step': dt / 10 * 1e6,
                              'launch_info': b.launch_info()}))
            b.close()
if 'dedqn' in which:
    # DEDQN (one env step = one trial row + the landscape analysis over a re-evaluation of all NP = 100 rows: 101 row evaluations) next to Random_search's
    # 100-row kernel in the same process: bbob round-robin, 4096 instances at D = 10 and 1024 at D = 30, a budget so large that every instance stays live.
    # k_dedqn_step: one launch per step with the action from the host side; k_dedqn_run: 32 steps per launch with the shipped Q-network in the kernel.
    from metabox_amd._abi import ALGO_DEDQN, ALGO_RANDOM_SEARCH
    from metabox_amd.agent import DEDQN_Agent
    from metabox_amd.suite import Batch, Suite
    acfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda']); acfg.agent_save_dir = None
    agent = DEDQN_Agent(acfg).load_exported_weights(np.load(os.path.join(os.path.dirname(__file__), '..', 'tests', 'golden', 'dedqn_policy.npz')))
    packed = agent.packed_weights().cuda()
    for dim, B in ((10, 4096), (30, 1024)):
        cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
        tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
        s = Suite(ps)
        b = Batch(s, ALGO_RANDOM_SEARCH, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, 100, 10 ** 9, 10 ** 7, 50, early_stop=False)
        b.reset()
        def run(n):
            for _ in range(n): b.step(None)
        run(3); dt = timed(run, 30)
        print(json.dumps({'path': f'k_rs_population bbob d={dim} NP=100, {B} instances', 'us_per_step': dt / 30 * 1e6, 'ns_per_row': dt / 30 / (100 * B) * 1e9}))
        b.close()
        b = Batch(s, ALGO_DEDQN, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, 100, 10 ** 9, 10 ** 7, 50, early_stop=False)
        b.reset()
        acts = torch.full((B,), 2, dtype=torch.int32, device='cuda')
        def run_step(n):
            for _ in range(n): b.step(acts)
        run_step(3); dt = timed(run_step, 30)
        print(json.dumps({'path': f'k_dedqn_step bbob d={dim} NP=100, {B} instances, one launch per env step', 'us_per_step': dt / 30 * 1e6,
                          'ns_per_row': dt / 30 / (101 * B) * 1e9, 'launch_info': b.launch_info()}))
        def run_res(n):
            for _ in range(n): b.dedqn_rollout(packed, 32)
        run_res(1); dt = timed(run_res, 3)
        print(json.dumps({'path': f'k_dedqn_run bbob d={dim} NP=100, {B} instances, 32 env steps per launch, Q-network in the kernel', 'us_per_step': dt / 96 * 1e6,
                          'ns_per_row': dt / 96 / (101 * B) * 1e9}))
        b.close()
if 'nrlpso' in which:
    # NRLPSO (one env step = one particle: the move, two normalised mean distances over the NP x NP distance matrix, one evaluation, now and then the
    # neighbourhood mutation) in its cached form (matrix in LDS, row / column refresh) and its recompute form (MBX_F_NRLPSO_RECOMPUTE), one launch per
    # step (mbx_step, action from the host side) and resident (64 steps per launch, table in the kernel), beside QLPSO's resident step in the same
    # process: bbob round-robin, 4096 instances at D = 10 and 1024 at D = 30, NP = 100, a budget so large that every instance stays live.  Median of
    # 5 windows per path, the paths alternating window by window, each window ended by a device synchronise (wall times, launch gaps included).
    from metabox_amd._abi import ALGO_NRLPSO, ALGO_QLPSO, F_NRLPSO_RECOMPUTE
    from metabox_amd.suite import Batch, Suite
    q = torch.from_numpy(np.load(os.path.join(os.path.dirname(__file__), '..', 'tests', 'golden', 'nrlpso_policy.npz'))['q_table']).cuda()
    for dim, B in ((10, 4096), (30, 1024)):
        cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
        tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
        s = Suite(ps)
        mk = lambda algo, np_, flags=0: Batch(s, algo, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, np_, 10 ** 9, 10 ** 7, 50, early_stop=False, flags=flags)
        bq, bc, br = mk(ALGO_QLPSO, 30), mk(ALGO_NRLPSO, 100), mk(ALGO_NRLPSO, 100, F_NRLPSO_RECOMPUTE)
        acts = torch.full((B,), 2, dtype=torch.int32, device='cuda')
        paths = {'QLPSO resident (NP = 30)': (lambda n: [bq.qlpso_rollout(q, 64) for _ in range(n)], 64),
                 'NRLPSO cached, resident': (lambda n: [bc.nrlpso_rollout(q, 64) for _ in range(n)], 64),
                 'NRLPSO recompute, resident': (lambda n: [br.nrlpso_rollout(q, 64) for _ in range(n)], 64),
                 'NRLPSO cached, one launch per step': (lambda n: [bc.step(acts) for _ in range(n)], 1),
                 'NRLPSO recompute, one launch per step': (lambda n: [br.step(acts) for _ in range(n)], 1)}
        for b in (bq, bc, br): b.reset()
        times = {k: [] for k in paths}
        for w in range(6):
            for k, (fn, per) in paths.items():
                n = 2 if per == 64 else 32
                dt = timed(fn, n)
                if w: times[k].append(dt / (n * per) * 1e6)             # window 0 warms up
        for k, v in times.items():
            print(json.dumps({'path': f'{k}, bbob d={dim}, {B} instances', 'us_per_step_median': float(np.median(v)), 'windows': [round(x, 1) for x in v],
                              'launch_info': (bc if 'cached' in k else br if 'recompute' in k else bq).launch_info()}))
        for b in (bq, bc, br): b.close()
if 'rlhpsde' in which:
    # RL-HPSDE (one update = NP trials, NP = 18 D shrinking towards 4, the memory update, the sort, and the 201-point landscape walk with its evaluations)
    # next to Random_search's 100-row kernel in the same process: bbob round-robin, 4096 instances at D = 10, the reference's budget of 20 000 without the
    # early stop, so that every instance runs the 70 updates of the integer schedule.  k_rlhpsde_run: 10 updates per launch with the shipped Q-table in the
    # kernel, the seven launches of an episode timed one by one (the population shrinks, so the first windows are the dear ones); k_rlhpsde_step: one launch per
    # update with the action from the host side, over the first 10 updates.  Wall times, launch gaps included; each window ends with a device synchronise.
    from metabox_amd._abi import ALGO_RANDOM_SEARCH, ALGO_RLHPSDE
    from metabox_amd.suite import Batch, Suite
    q = torch.from_numpy(np.load(os.path.join(os.path.dirname(__file__), '..', 'tests', 'golden', 'rlhpsde_policy.npz'))['q_table']).cuda()
    dim, B = 10, 4096
    cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
    tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
    s = Suite(ps)
    b = Batch(s, ALGO_RANDOM_SEARCH, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, 100, 10 ** 9, 10 ** 7, 50, early_stop=False)
    b.reset()
    def run(n):
        for _ in range(n): b.step(None)
    run(3); dt = timed(run, 30)
    print(json.dumps({'path': f'k_rs_population bbob d={dim} NP=100, {B} instances', 'us_per_step': dt / 30 * 1e6, 'ns_per_row': dt / 30 / (100 * B) * 1e9}))
    b.close()
    b = Batch(s, ALGO_RLHPSDE, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, 18 * dim, 20000, 400, 50, early_stop=False)
    episodes = []
    for rep in range(3):
        b.reset()
        episodes.append([timed(lambda n: b.rlhpsde_rollout(q, 10), 1) / 10 * 1e3 for _ in range(7)])
    assert bool(b.done.all())
    med = np.median(np.array(episodes), 0)
    print(json.dumps({'path': f'k_rlhpsde_run bbob d={dim} NP=180 -> 3, {B} instances, 10 updates per launch, Q-table in the kernel', 'ms_per_step_by_window': [round(float(x), 3) for x in med],
                      'ms_per_step_episode_mean': float(med.mean()), 'ms_per_episode': float(med.sum() * 10), 'launch_info': b.launch_info()}))
    b.reset()
    acts = torch.full((B,), 1, dtype=torch.int32, device='cuda')
    def run_step(n):
        for _ in range(n): b.step(acts)
    dt = timed(run_step, 10)
    print(json.dumps({'path': f'k_rlhpsde_step bbob d={dim}, {B} instances, one launch per update, the first 10 updates', 'ms_per_step': dt / 10 * 1e3}))
    b.close()
if 'nlshade' in which:
    # NL_SHADE_LBC (one update = NP trials, NP = 23 D collapsing non-linearly to 4, two sorts, the r2 cdf, the memory update): bbob round-robin, 4096 instances at
    # D = 10, the reference's budget of 20 000 without the early stop, so that every instance runs the 919 updates of the integer schedule.  Per-update time over
    # the first 10 updates (NP 230 .. 203) and over updates 700 .. 709 (NP = 4); then the whole episode through 919 single-update launches (mbx_step) against the
    # n-update launch (mbx_nlshade_run, 128 updates per launch, what NL_SHADE_LBC._run does), same batch, same process.  Wall times, launch gaps included; each
    # window ends with a device synchronise.
    from metabox_amd._abi import ALGO_NLSHADE
    from metabox_amd.optimizer import NL_SHADE_LBC
    from metabox_amd.suite import Batch, Suite
    dim, B = 10, 4096
    cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
    tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
    s = Suite(ps)
    total = NL_SHADE_LBC.n_updates(dim, 20000)
    b = Batch(s, ALGO_NLSHADE, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, 23 * dim, 20000, 400, 50, early_stop=False)
    def steps(n):
        for _ in range(n): b.step(None)
    def chunks(n):
        while n > 0:
            b.nlshade_run(min(128, n)); n -= 128
    b.reset(); steps(2)
    first = timed(steps, 10) / 10 * 1e3
    b.nlshade_run(700 - 12)
    late = timed(steps, 10) / 10 * 1e3
    print(json.dumps({'path': f'k_nlshade_step bbob d={dim}, {B} instances, one launch per update', 'ms_per_update_first_10': first, 'ms_per_update_at_NP_4': late,
                      'launch_info': b.launch_info()}))
    res = {}
    for name, fn in (('919 single-update launches', steps), ('n-update launches of 128', chunks)) * 2:
        b.reset(); torch.cuda.synchronize()
        res.setdefault(name, []).append(timed(fn, total) * 1e3)
        assert bool(b.done.all())
    print(json.dumps({'path': f'NL_SHADE_LBC whole episode bbob d={dim}, {B} instances, {total} updates', 'ms_per_episode': {k: [round(x, 2) for x in v] for k, v in res.items()}}))
    b.close()
if 'sdmspso' in which:
    # sDMS_PSO (one mbx_step = one update: 99 evaluated rows) next to GL-PSO (one generation: 200 evaluated rows and the exemplar breeding) in the
    # same process, alternating: bbob round-robin, 4096 instances, every instance live for the whole window (sDMS_PSO has no early stop; its
    # budget of 100 000 keeps it in the local phase, and the window of 3 + 7 x 40 updates meets two regroups).  Median of 7 windows of 40 steps,
    # each ended by a device synchronise; the wall times include the launch gaps.
    from metabox_amd._abi import ALGO_GLPSO, ALGO_SDMSPSO
    from metabox_amd.suite import Batch, Suite
    for dim in (10, 30):
        cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
        tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
        s = Suite(ps); B = 4096
        jobs = {'k_sdmspso_update': (Batch(s, ALGO_SDMSPSO, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, 99, 100000, 2000, 50), 99),
                'k_glpso_generation': (Batch(s, ALGO_GLPSO, np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1, 100, 10 ** 8, 10 ** 6, 50, early_stop=False), 200)}
        times = {k: [] for k in jobs}
        for b, _ in jobs.values():
            b.reset()
            for _ in range(3): b.step(None)
        for rep in range(7):
            for name, (b, _) in jobs.items():
                def run(n):
                    for _ in range(n): b.step(None)
                times[name].append(timed(run, 40) / 40)
        for name, (b, rows) in jobs.items():
            t = float(np.median(times[name]))
            assert int((b.results()['steps'] > 0).sum()) == B and not bool(b.done.any())
            print(json.dumps({'path': f'{name} bbob d={dim}, {B} instances, one launch per step', 'ms_per_step_median': t * 1e3, 'ms_per_step_min_max': [min(times[name]) * 1e3, max(times[name]) * 1e3],
                              'rows_per_step': rows, 'row_evaluations_per_s': rows * B / t, 'launch_info': b.launch_info()}))
            b.close()
if 'sahlpso' in which:
    # SAHLPSO (one mbx_step = one pass over the live particles, each move seeing the one before it: 40 sequential single-row evaluations in ONE launch)
    # beside sDMS_PSO (one update: 99 rows evaluated side by side) and QLPSO (one particle per env step: one launch per step, and resident with 64 steps
    # per launch) in the same process, the paths alternating window by window: bbob round-robin, 4096 instances at D = 10 and 1024 at D = 30.  The
    # budget is so large that SAHLPSO's population stays at 40 and every instance stays live.  Median of 5 windows per path after a warm-up window,
    # each window ended by a device synchronise (wall times, launch gaps included).
    from metabox_amd._abi import ALGO_QLPSO, ALGO_SAHLPSO, ALGO_SDMSPSO
    from metabox_amd.suite import Batch, Suite
    q = torch.from_numpy(np.load(os.path.join(os.path.dirname(__file__), '..', 'metabox_amd', 'agent_model', 'qlpso_bbob_easy.npz'))['q_table']).cuda()
    for dim, B in ((10, 4096), (30, 1024)):
        cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
        tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
        s = Suite(ps)
        pidx, seeds = np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1
        bs = Batch(s, ALGO_SAHLPSO, pidx, seeds, 40, 10 ** 9, 10 ** 7, 50, early_stop=False)
        bd = Batch(s, ALGO_SDMSPSO, pidx, seeds, 99, 100000, 2000, 50)
        bq = Batch(s, ALGO_QLPSO, pidx, seeds, 30, 10 ** 9, 10 ** 7, 50, early_stop=False)
        acts = torch.full((B,), 2, dtype=torch.int32, device='cuda')
        # name: (run n launches, FEs per launch, launches per window)
        paths = {'k_sahlpso_generation (NP = 40)': (lambda n: [bs.step(None) for _ in range(n)], 40, 16),
                 'k_sdmspso_update (NP = 99)': (lambda n: [bd.step(None) for _ in range(n)], 99, 16),
                 'QLPSO one launch per step (NP = 30)': (lambda n: [bq.step(acts) for _ in range(n)], 1, 32),
                 'QLPSO resident, 64 steps per launch': (lambda n: [bq.qlpso_rollout(q, 64) for _ in range(n)], 64, 2)}
        for b in (bs, bd, bq): b.reset()
        times = {k: [] for k in paths}
        for w in range(6):
            for k, (fn, fes, n) in paths.items():
                dt = timed(fn, n)
                if w: times[k].append(dt / n * 1e6)                  # window 0 warms up
        assert not bool(bs.done.any()) and int((bs.results()['steps'] > 0).sum()) == B
        for k, v in times.items():
            fes = paths[k][1]
            print(json.dumps({'path': f'{k}, bbob d={dim}, {B} instances', 'us_per_launch_median': float(np.median(v)), 'us_per_fe_median': float(np.median(v)) / fes,
                              'fes_per_launch': fes, 'windows_us_per_launch': [round(x, 1) for x in v],
                              'launch_info': (bs if 'sahlpso' in k else bd if 'sdmspso' in k else bq).launch_info()}))
        for b in (bs, bd, bq): b.close()
if 'les' in which:
    # LES (one generation = 16 FEs): the resident kernel with 50 generations per launch -- a skip_step = 50 call, what one meta-generation of LES_Agent.train_batch
    # runs -- beside one launch per generation (MBX_F_ROLLOUT_PER_GENERATION: same call, same outputs) and beside SAHLPSO's pass (40 single-row evaluations per launch)
    # in the same process, the paths alternating window by window: bbob round-robin, 4096 instances at D = 10 and 1024 at D = 30, every instance with one of 16
    # parameter sets drawn as CMA-ES draws its first population (N(0, 0.1^2)).  Median of 5 windows per path after a warm-up window, each window ended by a device
    # synchronise (wall times, launch gaps included).
    from metabox_amd._abi import ALGO_LES, ALGO_SAHLPSO, F_ROLLOUT_PER_GENERATION
    from metabox_amd.suite import Batch, Suite
    sets = np.random.RandomState(0).randn(16, 246) * 0.1
    for dim, B in ((10, 4096), (30, 1024)):
        cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
        tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
        s = Suite(ps)
        pidx, seeds = np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1
        br = Batch(s, ALGO_LES, pidx, seeds, 16, 20000, 400, 50)
        bg = Batch(s, ALGO_LES, pidx, seeds, 16, 20000, 400, 50, flags=F_ROLLOUT_PER_GENERATION)
        bs = Batch(s, ALGO_SAHLPSO, pidx, seeds, 40, 10 ** 9, 10 ** 7, 50, early_stop=False)
        for b in (br, bg): b.les_set_params(sets, (np.arange(B) // len(ps)) % 16)
        def les(b):
            def run(n):
                for _ in range(n):
                    b.reset(); b.les_rollout(50, skip=True)
            return run
        # name: (run n launches, generations per launch, FEs per generation, launches per window)
        paths = {'k_les_run resident, 50 generations per launch': (les(br), 50, 16, 4),
                 'k_les_run one launch per generation': (les(bg), 50, 16, 4),
                 'k_sahlpso_generation (NP = 40)': (lambda n: [bs.step(None) for _ in range(n)], 1, 40, 16)}
        bs.reset()
        times = {k: [] for k in paths}
        for w in range(6):
            for k, (fn, gens, fes, n) in paths.items():
                dt = timed(fn, n)
                if w: times[k].append(dt / n / gens * 1e6)           # window 0 warms up
        assert torch.equal(br.state, bg.state) and torch.equal(br.results()['cost'], bg.results()['cost'])
        for k, v in times.items():
            gens, fes = paths[k][1], paths[k][2]
            print(json.dumps({'path': f'{k}, bbob d={dim}, {B} instances', 'us_per_generation_median': float(np.median(v)), 'us_per_fe_median': float(np.median(v)) / fes,
                              'generations_per_call': gens, 'windows_us_per_generation': [round(x, 1) for x in v],
                              'launch_info': (bs if 'sahlpso' in k else br).launch_info()}))
        for b in (br, bg, bs): b.close()
if 'l2l' in which:
    # L2L (one step = one LSTM cell + 1 FE, an episode = 100 steps): whole episodes in ONE launch beside one launch per step (MBX_F_ROLLOUT_PER_GENERATION: same call,
    # same outputs), the paths alternating window by window: bbob round-robin, 4096 instances at D = 10 (the weights in registers) and 1024 at D = 40 (the run-time-D
    # body), every instance with one of 21 weight sets -- the shape of the --rollout table, 21 checkpoints in one batch.  Median of 5 windows per path after a
    # warm-up window, each window ended by a device synchronise (wall times, launch gaps included).
    from metabox_amd._abi import ALGO_L2L, F_ROLLOUT_PER_GENERATION
    from metabox_amd.suite import Batch, Suite
    for dim, B in ((10, 4096), (40, 1024)):
        cfg = get_config(['--problem', 'bbob', '--dim', str(dim)])
        tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
        s = Suite(ps)
        pidx, seeds = np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1
        sets = np.random.RandomState(0).uniform(-0.5, 0.5, (21, 128 * (dim + 2) + 128 * dim + 256 + 32 * dim))
        br = Batch(s, ALGO_L2L, pidx, seeds, 1, 20000, 400, 50, early_stop=False)
        bg = Batch(s, ALGO_L2L, pidx, seeds, 1, 20000, 400, 50, early_stop=False, flags=F_ROLLOUT_PER_GENERATION)
        for b in (br, bg): b.l2l_set_params(sets, (np.arange(B) // len(ps)) % 21)
        def l2l(b):
            def run(n):
                for _ in range(n):
                    b.reset(); b.l2l_rollout(100)
            return run
        paths = {'k_l2l_run resident, 100 steps per launch': (l2l(br), 4), 'k_l2l_run one launch per step': (l2l(bg), 4)}
        times = {k: [] for k in paths}
        for w in range(6):
            for k, (fn, n) in paths.items():
                dt = timed(fn, n)
                if w: times[k].append(dt / n * 1e3)                  # window 0 warms up
        assert torch.equal(br.state, bg.state) and torch.equal(br.results()['cost'], bg.results()['cost']) and bool(br.done.all())
        for k, v in times.items():
            print(json.dumps({'path': f'{k}, bbob d={dim}, {B} instances', 'ms_per_episode_batch_median': float(np.median(v)), 'us_per_step_median': float(np.median(v)) * 10,
                              'windows_ms_per_episode_batch': [round(x, 3) for x in v], 'launch_info': br.launch_info()}))
        for b in (br, bg): b.close()
if 'symbol' in which:
    # SYMBOL (one action = 5 sub-steps under a per-instance expression tree): 4096 instances at D = 10, bbob round-robin, the trees of the shipped policy (checkpoint
    # 20, generated once per window from the batch's own features).  Three figures per action: the resident route (5 sub-steps in ONE launch), the per-sub-step route
    # (MBX_F_ROLLOUT_PER_GENERATION: same call, same outputs) and the host policy (LSTM + grammar mask + constants for 4096 trees).  Median of 5 windows of 8 actions per
    # path after a warm-up window, each window ended by a device synchronise.
    from metabox_amd._abi import ALGO_SYMBOL, F_ROLLOUT_PER_GENERATION
    from metabox_amd.agent import Symbol_Agent
    from metabox_amd.suite import Batch, Suite
    dim, B = 10, 4096
    cfg = get_config(['--problem', 'bbob', '--dim', str(dim)]); cfg.agent_save_dir = None
    agent = Symbol_Agent(cfg).load_exported_weights(np.load(os.path.join(os.path.dirname(__file__), '..', 'tests', 'golden', 'symbol_policy.npz')), prefix='w20/')
    tr, te = construct_problem_set(cfg); ps = sorted(tr.data + te.data, key=lambda p: p.func_id)
    s = Suite(ps)
    pidx, seeds = np.arange(B) % len(ps), np.arange(B, dtype=np.uint64) + 1
    br = Batch(s, ALGO_SYMBOL, pidx, seeds, 100, 20000, 400, 50, early_stop=False)
    bg = Batch(s, ALGO_SYMBOL, pidx, seeds, 100, 20000, 400, 50, early_stop=False, flags=F_ROLLOUT_PER_GENERATION)
    torch.manual_seed(1)
    feats = br.reset().cpu().numpy().astype(np.float32); bg.reset()
    host = []
    def trees():
        t0 = time.perf_counter(); tk, cs = agent.act(feats); host.append((time.perf_counter() - t0) * 1e3)
        return torch.from_numpy(tk).cuda(), torch.from_numpy(cs).cuda()
    tk, cs = trees()
    def sym(b):
        def run(n):
            for _ in range(n):
                b.symbol_rollout(tk, cs, 5)
        return run
    paths = {'k_symbol_run resident, 5 sub-steps per launch': (sym(br), 8), 'k_symbol_step one launch per sub-step': (sym(bg), 8)}
    times = {k: [] for k in paths}
    for w in range(6):
        if w == 1:                                                   # both batches restart side by side so that the windows that count see the same populations
            br.reset(); bg.reset()
        for k, (fn, n) in paths.items():
            dt = timed(fn, n)
            if w: times[k].append(dt / n * 1e3)
        if w < 4: feats = br.state.cpu().numpy().astype(np.float32); tk, cs = trees()
    assert torch.equal(br.state, bg.state) and torch.equal(br.results()['cost'], bg.results()['cost'])
    for k, v in times.items():
        print(json.dumps({'path': f'{k}, bbob d={dim}, {B} instances', 'ms_per_action_median': float(np.median(v)), 'windows_ms_per_action': [round(x, 3) for x in v],
                          'launch_info': br.launch_info()}))
    print(json.dumps({'path': f'Symbol_Agent.act on the host (LSTM, mask, constants), {B} trees', 'ms_per_action_median': float(np.median(host)),
                      'calls_ms': [round(x, 1) for x in host], 'distinct_mask_prefixes': agent.mask_cache_size()}))
    for b in (br, bg): b.close()
