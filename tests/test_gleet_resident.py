"""GLEET's resident rollout (include/mbx_gleet.h: mbx_gleet_set_params, mbx_gleet_rollout): the attention actor inside the step kernel.

CPU: the header / exports / binding, and the LDS walk glr_layout against gl_layout through a host program (tests/lds_sizes_gleet_main.hip).

GPU: one resident launch of 12 steps per geometry, then, from the same reset and seeds,
  * a replay batch -- mbx_step fed the recorded actions -- which the float64 half must equal bit for bit, step by step;
  * the float64 copy of the actor's modules on the states the replay reconstructs, which the recorded (mu, sigma) must meet within the rule
    tests/test_policy_exact.py applies to k_gleet_policy: 4 E_ref + 4 float32 ulp, E_ref = PyTorch's own float32-against-float64 distance on the same inputs;
  * mbx_gleet_policy on the replay batch's states: the same Philox draws;
  * the other routes (one-step calls, a 3 / 1 / 8 split, one launch per step), bit for bit;
then termination inside a launch, per-instance weight sets, the refusals and the host side (rollout_batch(policy='resident'), tester.rollout through
rollout_checkpoints).  Every reference run is computed once (functools.lru_cache) and shared."""
import copy
import functools
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import policy_exact as pe
from helpers import load, problems
from policy_exact import F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ALGO_GLEET = 6
STEPS, NLOG = 12, 50
# name: (NP, D, B, suite, run-time-geometry kernel forced)
GEOMS = {'100x10': (100, 10, 67, 'bbob', False), '100x10-generic': (100, 10, 5, 'bbob', True), '5x3': (5, 3, 7, 'bbob', False),
         '65x10': (65, 10, 3, 'bbob', False), '128x30': (128, 30, 2, 'bbob', False), '4x2': (4, 2, 3, 'bbob', False),
         '63x10-noisy': (63, 10, 3, 'bbob-noisy', False)}
ACTOR_GEOMS = ('4x2', '5x3', '63x10-noisy', '65x10', '100x10', '128x30')          # NP 4, 5, 63, 65, 100, 128


# ================================================================================================ CPU
def _strip_comments(text):
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_header_exports_and_binding():
    from metabox_amd import _abi
    code = _strip_comments(open(os.path.join(ROOT, 'include', 'mbx_gleet.h')).read())
    declared = re.findall(r'\b(mbx_[a-z0-9_]+)\s*\(', code)
    assert sorted(declared) == ['mbx_gleet_rollout', 'mbx_gleet_set_params']
    assert set(_abi.GLEET_SYMBOLS) == set(declared) and not set(declared) & set(_abi.EXPORTED_SYMBOLS) and len(_abi.EXPORTED_SYMBOLS) == 45
    main = open(os.path.join(ROOT, 'include', 'mbx.h')).read()
    assert 'mbx_gleet_set_params' not in main and 'mbx_gleet_rollout' not in main
    lib = _abi.load_lib()
    import ctypes as C
    vp = C.c_void_p
    assert lib.mbx_gleet_set_params.argtypes == [vp, vp, C.c_int, vp, C.c_float, C.c_float] and lib.mbx_gleet_set_params.restype == C.c_int
    assert lib.mbx_gleet_rollout.argtypes == [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp] and lib.mbx_gleet_rollout.restype == C.c_int
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(ROOT, 'metabox_amd', 'csrc', 'libmbx.so')], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if ' T ' in line}
    assert {'mbx_gleet_set_params', 'mbx_gleet_rollout'} <= exported


LDS_GEOMS = ((4, 2), (5, 3), (65, 10), (100, 10), (128, 30))


def test_lds_walk_of_the_resident_kernel(tmp_path):
    """glr_layout: the evaluator prefix (and the generation's own arrays) where gl_layout puts them, the total at least gl's and within the 160 KB a
    workgroup may have, the actor's keys / values inside the evaluator's scratch T | Z, the block-sum slots outside everything else."""
    exe = str(tmp_path / 'lds_sizes_gleet')
    subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-w', '-I', os.path.join(ROOT, 'metabox_amd', 'csrc'), '-o', exe,
                           os.path.join(ROOT, 'tests', 'lds_sizes_gleet_main.hip')])
    args = [str(v) for g in LDS_GEOMS for v in g]
    lines = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    per, cur = {}, None
    for line in lines:
        key, *vals = line.split()
        if key == 'geometry':
            cur = per.setdefault((int(vals[0]), int(vals[1])), {})
        else:
            cur[key] = int(vals[0])
    assert sorted(per) == sorted(LDS_GEOMS)
    for (NP, D), v in per.items():
        names = [k[3:] for k in v if k.startswith('gl_') and k != 'gl_doubles']
        assert names[:9] == ['X', 'T', 'Z', 'M1T', 'M2T', 'DSH', 'V0', 'V1', 'V2'] and len(names) == 16
        for n in names:
            assert v['gl_' + n] == v['glr_' + n], (NP, D, n)
        assert v['gl_X'] == 0 and v['glr_doubles'] >= v['gl_doubles'] and 8 * v['glr_doubles'] <= 160 * 1024, (NP, D)
        assert v['glr_carve_end'] == 8 * v['glr_doubles'], (NP, D)                       # the size and the pointers come from one walk
        assert v['t_begin'] == v['gl_T'] and v['z_end'] <= v['gl_M1T']
        assert v['t_begin'] <= v['kl'] and v['vl'] == v['kl'] + 4 * 16 * NP and v['kv_end'] == v['vl'] + 4 * 16 * NP and v['kv_end'] <= v['z_end'], (NP, D)
        assert 8 * v['gl_doubles'] <= v['pred'] and v['pred'] + 16 <= 8 * v['glr_doubles'], (NP, D)
        print(f'  glr({NP},{D}): {8 * v["glr_doubles"]} bytes (gl {8 * v["gl_doubles"]}), K | V {v["kl"]} .. {v["kv_end"]} inside T | Z {v["t_begin"]} .. {v["z_end"]}')


# ================================================================================================ GPU: shared runs
def _cfg():
    from metabox_amd.config import get_config
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cpu'])
    cfg.agent_save_dir = None
    return cfg


@functools.lru_cache(maxsize=None)
def _actors():
    from metabox_amd.agent import GLEET_Agent
    a32 = GLEET_Agent(_cfg()).load_exported_weights(load('gleet_policy.npz')).actor
    return a32, copy.deepcopy(a32).double()


@functools.lru_cache(maxsize=None)
def _weights():
    return _actors()[0].packed_weights().cuda()


def _problems(suite, D):
    ps = problems(suite, D)
    ids = sorted(ps)
    pick = [i for i in ids if i % 100 in (1, 8, 21)][:3] if suite == 'bbob' else ids[:3]
    assert len(pick) == 3
    return [ps[i] for i in pick]


def _make(name, flags=0, max_fes=None, seeds=None, B=None):
    from metabox_amd import _abi
    from metabox_amd.suite import Batch, Suite
    NP, D, B0, suite, generic = GEOMS[name]
    B = B or B0
    ps = _problems(suite, D)
    max_fes = max_fes or 2000 * D
    seeds = np.arange(B, dtype=np.uint64) * 13 + 5 if seeds is None else seeds
    flags |= _abi.F_GENERIC_GEOMETRY if generic else 0
    return Batch(Suite(ps), ALGO_GLEET, np.arange(B) % 3, seeds, NP, max_fes, max(max_fes // NLOG, 1), NLOG, flags=flags)


def _blocks(b):
    import torch
    torch.cuda.synchronize()
    return np.stack([b.read_state(k) for k in range(b.B)])


def _end(b):
    """everything a route leaves behind: state blocks, the state tensor, curves and counters, done"""
    res = b.results()
    return {'blocks': _blocks(b), 'state': b.state.cpu().numpy().copy(), 'cost': res['cost'].cpu().numpy(), 'cost_len': res['cost_len'].cpu().numpy(),
            'fes': res['fes'].cpu().numpy(), 'return': res['return'].cpu().numpy(), 'done': b.done.cpu().numpy().copy()}


def _rollout(b, calls):
    """reset, then gleet_rollout once per entry of `calls` -> (records of all steps concatenated, summed rewards per call, end)"""
    import torch
    a32 = _actors()[0]
    b.gleet_set_params(_weights(), None, a32.min_sigma, a32.max_sigma)
    s0 = b.reset().cpu().numpy().copy()
    trajs, sums = [], []
    for n in calls:
        _, r, _, t = b.gleet_rollout(n, want_traj=True)
        trajs.append({k: v.cpu().numpy() for k, v in t.items()})
        sums.append(r.cpu().numpy().copy())
    torch.cuda.synchronize()
    return {k: np.concatenate([t[k] for t in trajs]) for k in trajs[0]}, sums, _end(b), s0


@functools.lru_cache(maxsize=None)
def _run(name):
    """The resident launch of STEPS steps with all records, and the replay: mbx_step fed the recorded actions, with mbx_gleet_policy evaluated on the replay
    batch's state before every step (it changes nothing)."""
    import torch
    a32 = _actors()[0]
    b = _make(name)
    traj, sums, end, s0 = _rollout(b, [STEPS])
    b.close()
    r = _make(name)
    s0r = r.reset().cpu().numpy().copy()
    acts = torch.from_numpy(traj['actions']).cuda()
    rep = {'state': [], 'reward': [], 'done': [], 'pol_act': [], 'pol_ms': []}
    for t in range(STEPS):
        pa, pms = r.gleet_policy(_weights(), a32.min_sigma, a32.max_sigma, want_mu_sigma=True)
        rep['pol_act'].append(pa.cpu().numpy().copy()); rep['pol_ms'].append(pms.cpu().numpy().copy())
        st, rw, dn = r.step(acts[t].contiguous())
        rep['state'].append(st.cpu().numpy().copy()); rep['reward'].append(rw.cpu().numpy().copy()); rep['done'].append(dn.cpu().numpy().copy())
    rep = {k: np.stack(v) for k, v in rep.items()}
    rend = _end(r)
    r.close()
    assert np.array_equal(s0, s0r)
    return {'traj': traj, 'sum': sums[0], 'end': end, 's0': s0, 'rep': rep, 'rend': rend}


def _same(a, b):
    import torch
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.from_numpy(a), torch.from_numpy(b))


def _same_end(a, b, who):
    for k in a:
        assert _same(a[k], b[k]), (who, k)


# ================================================================================================ 3. the optimizer half, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize('name', list(GEOMS))
def test_replay_pins_the_optimizer_half(name):
    """mbx_step fed the actions the resident kernel recorded: rewards at every step, the [np, 27] states and done flags at every step (the resident route
    through one-step calls, whose own records must be the 12-step launch's), and at the end the full state blocks and cost curves."""
    run = _run(name)
    NP, D, B, _, generic = GEOMS[name]
    traj, rep = run['traj'], run['rep']
    assert traj['actions'].shape == (STEPS, B, NP) and traj['mu_sigma'].shape == (STEPS, B, 2, NP) and not np.isnan(traj['actions']).any()
    assert not rep['done'].any(), 'the budget of this test ends no instance'
    for t in range(STEPS):
        assert _same(traj['reward'][t], rep['reward'][t]), (name, t)
    total = rep['reward'][0].copy()
    for t in range(1, STEPS):
        total = total + rep['reward'][t]
    assert _same(run['sum'], total), name                          # the SUM of the executed steps' rewards, added in step order
    assert _same(run['end']['state'], rep['state'][-1]) and _same(run['end']['done'], rep['done'][-1])
    _same_end(run['end'], run['rend'], name)
    # one-step calls: the state tensor and the done flags after every step
    import torch
    b = _make(name)
    a32 = _actors()[0]
    b.gleet_set_params(_weights(), None, a32.min_sigma, a32.max_sigma)
    b.reset()
    info = b.launch_info()
    assert info['fixed_geometry'] == (5 if (NP, D) == (100, 10) and not generic else 0)
    for t in range(STEPS):
        st, rw, dn, tj = b.gleet_rollout(1, want_traj=True)
        assert _same(st.cpu().numpy(), rep['state'][t]) and _same(rw.cpu().numpy(), rep['reward'][t]) and _same(dn.cpu().numpy(), rep['done'][t]), (name, t)
        for k in tj:
            assert _same(tj[k][0].cpu().numpy(), traj[k][t]), (name, t, k)
    _same_end(_end(b), run['rend'], name + ' one-step calls')
    b.close()


# ================================================================================================ 4. the actor inside the kernel
def _inputs(run, name):
    """the state every step's actor read: the reset state for step 0, the replay's state after step t - 1 for step t -> [STEPS, B, NP, 27]"""
    NP, _, B, _, _ = GEOMS[name]
    return np.concatenate([run['s0'][None], run['rep']['state'][:-1]]).reshape(STEPS, B, NP, 27)


@functools.lru_cache(maxsize=None)
def _modules(name):
    """(mu, sigma) of PyTorch's float32 modules and of their float64 copy on the inputs of `name`, E_ref per quantity"""
    import torch
    a32, a64 = _actors()
    x = _inputs(_run(name), name)
    m32 = [pe.gleet_forward(a32, torch.from_numpy(x[t].astype(F32))) for t in range(STEPS)]
    m64 = [pe.gleet_forward(a64, torch.from_numpy(np.ascontiguousarray(x[t]))) for t in range(STEPS)]
    m32 = [np.stack([m[q] for m in m32]) for q in (0, 1)]
    m64 = [np.stack([m[q] for m in m64]) for q in (0, 1)]
    return m64, [pe.e_ref(m32[q], m64[q]) for q in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ACTOR_GEOMS)
def test_actor_inside_the_kernel_is_the_reference_actor(name):
    """The recorded (mu, sigma) of every step against the float64 modules on the reconstructed states, within 4 E_ref + 4 float32 ulp."""
    run = _run(name)
    m64, E = _modules(name)
    ms = run['traj']['mu_sigma']
    frac = [pe.rule_fraction(ms[:, :, q], m64[q], E[q]) for q in (0, 1)]
    same = [int((ms[:, :, q] != run['rep']['pol_ms'][:, :, q]).sum()) for q in (0, 1)]
    print(f'GLEET_RESIDENT {name}: E_ref mu {E[0]:.2e} sigma {E[1]:.2e}; worst fraction of 4 E_ref + 4 ulp: mu {frac[0]:.3f} sigma {frac[1]:.3f}; '
          f'values differing from k_gleet_policy bit for bit: mu {same[0]} sigma {same[1]} of {ms[:, :, 0].size}')
    assert all(0 < e < 2e-4 for e in E) and all(f <= 1.0 for f in frac), (E, frac)


@pytest.mark.gpu
def test_resident_draws_are_the_policy_kernels_draws():
    """Both routes draw n = sqrt(-2 ln u1) cos(2 pi u2) from the same Philox counter (i, MBX_SITE_POLICY, gen + 1, episode) with the same float32 operations and
    form a = fl(mu + fl(sigma n)).  For an un-clamped action, 0 < a < 1: a = mu + sigma n (1 + e1) + e2 with |e1| <= 2^-24 and |e2| <= 2^-24 |a| < 2^-24, so
    the float64 quotient z = (a - mu) / sigma of the recorded float32 values is n (1 + e1) + e2 / sigma: |z - n| <= 2^-24 (|z| + 1 / sigma) up to second order,
    whatever mu and sigma the route computed.  Two routes differ by at most twice that; the bound allows 8 x 2^-24 (1 / sigma + |z|), plus what the two
    routes' (mu, sigma) may differ by -- each is within tol = 4 E_ref + 4 ulp of the float64 modules -- carried through the quotient:
    (2 tol_mu + |z| 2 tol_sigma) / sigma."""
    count, worst = 0, 0.0
    for name in ACTOR_GEOMS:
        run = _run(name)
        m64, E = _modules(name)
        a_r, ms_r = run['traj']['actions'].astype(np.float64), run['traj']['mu_sigma'].astype(np.float64)
        a_p, ms_p = run['rep']['pol_act'].astype(np.float64), run['rep']['pol_ms'].astype(np.float64)
        keep = (a_r > 0) & (a_r < 1) & (a_p > 0) & (a_p < 1)
        z_r = (a_r - ms_r[:, :, 0]) / ms_r[:, :, 1]
        z_p = (a_p - ms_p[:, :, 0]) / ms_p[:, :, 1]
        sigma = np.minimum(ms_r[:, :, 1], ms_p[:, :, 1])
        z = np.maximum(np.abs(z_r), np.abs(z_p))
        bound = 8 * 2.0 ** -24 * (1 / sigma + z) + (2 * pe.rule_tol(m64[0], E[0]) + z * 2 * pe.rule_tol(m64[1], E[1])) / sigma
        assert keep.any(), name
        f = float((np.abs(z_r - z_p) / bound)[keep].max())
        print(f'GLEET_RESIDENT draws {name}: {int(keep.sum())} un-clamped of {keep.size}, worst fraction of the bound {f:.3f}, largest |z| {float(z[keep].max()):.2f}')
        assert f <= 1.0 and float(z[keep].max()) < 6.5, (name, f)
        count += int(keep.sum()); worst = max(worst, f)
    assert count >= 1000, count


# ================================================================================================ 5. routes
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['100x10', '5x3'])
def test_every_route_leaves_the_same_bits(name):
    from metabox_amd import _abi
    run = _run(name)
    for who, calls, flags in (('twelve one-step launches', [1] * STEPS, 0), ('3 / 1 / 8', [3, 1, 8], 0),
                              ('one launch per step', [STEPS], _abi.F_ROLLOUT_PER_GENERATION)):
        b = _make(name, flags=flags)
        assert bool(b.flags & _abi.F_ROLLOUT_PER_GENERATION) == bool(flags)
        traj, sums, end, _ = _rollout(b, calls)
        b.close()
        for k in traj:
            assert _same(traj[k], run['traj'][k]), (name, who, k)
        _same_end(end, run['end'], (name, who))
        if len(calls) == 1:
            assert _same(sums[0], run['sum']), (name, who)
        else:                                                      # every call returns the sum over ITS steps
            t0 = 0
            for n, s in zip(calls, sums):
                want = run['traj']['reward'][t0].copy()
                for t in range(t0 + 1, t0 + n):
                    want = want + run['traj']['reward'][t]
                assert _same(s, want), (name, who, t0)
                t0 += n


# ================================================================================================ 6. termination inside a launch
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['5x3', '100x10'])
def test_termination_inside_a_launch(name):
    """max_fes = 7 np + 3 and 20 steps asked for: every instance stops where k_gleet_step stops it, record rows past that keep their NaN, a second call
    changes nothing; a Sphere instance started at its optimum stops after step 1 under the early-stop rule."""
    import torch
    NP, D, _, suite, _ = GEOMS[name]
    B, n_steps, max_fes = 4, 20, 7 * NP + 3
    a32 = _actors()[0]
    sphere = problems(suite, D)[1]
    assert 'Sphere' in str(sphere)

    def make():
        b = _make(name, max_fes=max_fes, B=B)
        b.reset()
        torch.cuda.synchronize()
        blk = b.read_state(3)                                       # instance 3 runs problem 0 = Sphere (F1): the swarm at rest on the optimum
        assert _problems(suite, D)[0] is sphere
        ne = NP * D
        blk[0:ne] = np.tile(sphere.shift, NP); blk[ne:2 * ne] = 0.; blk[2 * ne:3 * ne] = np.tile(sphere.shift, NP)
        blk[3 * ne + 3 * NP:3 * ne + 3 * NP + D] = sphere.shift
        b.write_state(3, blk)
        return b
    b = make()
    b.gleet_set_params(_weights(), None, a32.min_sigma, a32.max_sigma)
    s_in = b.state.clone()
    st, rw, dn, traj = b.gleet_rollout(n_steps, want_traj=True)
    traj = {k: v.cpu().numpy() for k, v in traj.items()}
    rsum, end = rw.cpu().numpy().copy(), _end(b)
    # the replay: mbx_step fed the recorded actions, until every instance is done
    r = make()
    stop, rewards = np.full(B, -1), np.zeros((n_steps, B))
    for t in range(n_steps):
        acts = np.nan_to_num(traj['actions'][t])
        _, rr, dd = r.step(torch.from_numpy(acts).cuda())
        rr, dd = rr.cpu().numpy(), dd.cpu().numpy()
        for k in range(B):
            if stop[k] < 0:
                rewards[t, k] = rr[k]
                if dd[k]:
                    stop[k] = t
    rend = _end(r)
    r.close()
    assert stop[3] == 0 and np.all(stop[:3] == 6), stop               # fes = np (reset) + 7 np >= 7 np + 3 after step 7; the Sphere at once
    for k in range(B):
        live = slice(0, stop[k] + 1)
        assert _same(traj['reward'][live, k], rewards[live, k]) and not np.isnan(traj['actions'][live, k]).any() and not np.isnan(traj['mu_sigma'][live, k]).any()
        assert np.isnan(traj['reward'][stop[k] + 1:, k]).all() and np.isnan(traj['actions'][stop[k] + 1:, k]).all() and np.isnan(traj['mu_sigma'][stop[k] + 1:, k]).all()
        want = rewards[0, k]
        for t in range(1, stop[k] + 1):
            want = want + rewards[t, k]
        assert rsum[k] == want
    assert np.all(end['done'] == 1)
    for k in ('blocks', 'cost', 'cost_len', 'fes', 'return'):
        assert _same(end[k], rend[k]), k
    assert end['cost'][3, end['cost_len'][3] - 1] <= 1e-8 and end['fes'][3] == 2 * NP
    assert not _same(end['state'], s_in.cpu().numpy())
    # frozen: a second call writes no record, leaves the state tensor and the blocks alone, returns reward 0 and done
    st2, rw2, dn2, traj2 = b.gleet_rollout(3, want_traj=True)
    assert all(bool(torch.isnan(v).all()) for v in traj2.values()) and bool((rw2 == 0).all()) and bool((dn2 == 1).all())
    end2 = _end(b)
    for k in end:
        assert _same(end[k], end2[k]), k
    b.close()


# ================================================================================================ 7. per-instance weight sets
@pytest.mark.gpu
def test_per_instance_weight_sets():
    """Three sets (the fixture actor and two seeded perturbations of it), set i % 3 for instance i of 9: every instance's records and final block are those of a
    single-set batch holding that set with the same seed and problem.  An index outside the table is MBX_E_ARG."""
    import torch
    from metabox_amd._abi import MbxError
    a32 = _actors()[0]
    w0 = _weights().cpu()
    rs = np.random.RandomState(77)
    sets = torch.stack([w0] + [w0 * torch.from_numpy(1 + 0.05 * rs.standard_normal(w0.numel()).astype(F32)) for _ in range(2)])
    B = 9
    seeds = np.arange(B, dtype=np.uint64) * 31 + 7
    pidx = np.arange(B) % 3                                          # _make's assignment
    which = np.arange(B) % 3

    def run(weights, set_of_instance):
        b = _make('5x3', B=B, seeds=seeds)
        b.gleet_set_params(weights, set_of_instance, a32.min_sigma, a32.max_sigma)
        b.reset()
        _, rw, _, traj = b.gleet_rollout(STEPS, want_traj=True)
        out = ({k: v.cpu().numpy() for k, v in traj.items()}, _end(b), rw.cpu().numpy().copy())
        b.close()
        return out
    traj, end, rw = run(sets, which)
    assert np.array_equal(pidx, which)
    differ = 0
    for s in range(3):
        t1, e1, r1 = run(sets[s], None)
        mine = which == s
        for k in traj:
            assert _same(traj[k][:, mine], t1[k][:, mine]), (s, k)
            differ += int(not _same(traj[k][:, ~mine], t1[k][:, ~mine]))
        for k in e1:
            assert _same(end[k][mine], e1[k][mine]), (s, k)
        assert _same(rw[mine], r1[mine])
    assert differ > 0, 'the perturbed sets change nothing: the test cannot tell the sets apart'
    b = _make('5x3', B=B, seeds=seeds)
    for bad in (3, -1):
        w = which.copy(); w[4] = bad
        with pytest.raises(MbxError, match='mbx error -1'):          # MBX_E_ARG
            b.gleet_set_params(sets, w, a32.min_sigma, a32.max_sigma)
    b.close()


# ================================================================================================ 8. refusals
@pytest.mark.gpu
def test_refusals_name_their_cause():
    import torch
    from metabox_amd._abi import ALGO_RLPSO, MbxError
    from metabox_amd.suite import Batch, Suite
    a32 = _actors()[0]
    w = _weights()
    ps = _problems('bbob', 2)
    other = Batch(Suite(ps), ALGO_RLPSO, [0], [1], 30, 4000, 80, NLOG)
    other.reset()
    for call in (lambda: other.gleet_set_params(w), lambda: other.gleet_rollout(1)):
        with pytest.raises(MbxError, match=r'mbx error -3: .*not a GLEET batch'):      # MBX_E_UNSUPPORTED
            call()
    other.close()
    big = Batch(Suite(ps), ALGO_GLEET, [0], [1], 129, 4000, 80, NLOG)
    big.reset()
    for call in (lambda: big.gleet_set_params(w), lambda: big.gleet_rollout(1)):
        with pytest.raises(MbxError, match=r'mbx error -3: .*np 129 > 128'):
            call()
    big.close()
    b = _make('4x2')
    b.reset()
    with pytest.raises(MbxError, match=r'mbx error -1: .*mbx_gleet_set_params first'):  # MBX_E_ARG
        b.gleet_rollout(1)
    b.gleet_set_params(w, None, a32.min_sigma, a32.max_sigma)
    for n in (0, -2):
        with pytest.raises(MbxError, match=r'mbx error -1: .*n_steps must be >= 1'):
            b.gleet_rollout(n)
    b.set_tape(torch.zeros(b.B, b.tape_stride, dtype=torch.float64, device='cuda'))
    with pytest.raises(MbxError, match=r'mbx error -3: .*replay tape'):
        b.gleet_rollout(1)
    b.set_tape(None)
    b.gleet_rollout(1)                                               # ... and nothing else stands in the way
    b.close()


# ================================================================================================ 9. host
@pytest.mark.gpu
def test_rollout_batch_resident_route():
    import torch
    from metabox_amd.agent import GLEET_Agent
    from metabox_amd.environment import BatchedPBO_Env
    from metabox_amd.optimizer import GLEET_Optimizer
    cfg = _cfg()
    cfg.device = 'cuda'
    agent = GLEET_Agent(cfg).load_exported_weights(load('gleet_policy.npz'))
    agent.to('cuda')
    small = copy.deepcopy(cfg)
    small.maxFEs, small.log_interval, small.n_logpoint = 1500, 100, 15
    ps = [problems('bbob', 10)[f] for f in (1, 8, 21)]
    B = 12
    outs = {}
    for policy in ('hip', 'resident'):
        env = BatchedPBO_Env(ps, GLEET_Optimizer(small), np.arange(B) % 3, np.arange(B, dtype=np.uint64) + 3)
        outs[policy] = {k: v.cpu().numpy() for k, v in agent.rollout_batch(env, policy=policy).items()}
        env.close()
    hip, res = outs['hip'], outs['resident']
    assert sorted(hip) == sorted(res) and all(hip[k].shape == res[k].shape and hip[k].dtype == res[k].dtype for k in hip)
    assert res['cost'].shape == (B, 16) and np.all(np.diff(res['cost'], axis=1) <= 0) and np.all(res['fes'] == 1500)
    assert np.all(res['steps'] == 14) and np.all(res['cost_len'] == 16) and np.all(res['return'] >= 0)


@pytest.mark.gpu
def test_tester_rollout_goes_through_rollout_checkpoints(tmp_path, monkeypatch):
    """n_checkpoint = 1: two pickled agents, two problems, two runs -- ONE resident batch of 2 x 4 instances.  rollout.pkl has the reference's nesting and
    rows of 51 entries; every checkpoint's rows are, bit for bit, a single-checkpoint resident rollout_batch with the seeds philox_seed(run, arange(n), cp)."""
    import torch
    from metabox_amd import tester
    from metabox_amd.agent import GLEET_Agent
    from metabox_amd.config import get_config
    from metabox_amd.environment import BatchedPBO_Env
    from metabox_amd.optimizer import GLEET_Optimizer
    from metabox_amd.utils import construct_problem_set
    cfg = get_config(['--problem', 'bbob', '--dim', '10', '--device', 'cuda'])
    cfg.agent_save_dir = None
    cfg.maxFEs, cfg.log_interval, cfg.n_logpoint = 1500, 30, 50
    cfg.n_checkpoint, cfg.rollout_runs = 1, 2
    cfg.agent_for_rollout, cfg.optimizer_for_rollout = ['GLEET_Agent'], ['GLEET_Optimizer']
    cfg.agent_load_dir, cfg.rollout_log_dir = str(tmp_path) + '/agents/', str(tmp_path) + '/log/'
    os.makedirs(cfg.agent_load_dir + 'GLEET_Agent')
    rs = np.random.RandomState(5)
    agents = []
    for cp in range(2):
        a = GLEET_Agent(_cfg()).load_exported_weights(load('gleet_policy.npz'))
        if cp:
            with torch.no_grad():
                for p in a.actor.parameters():
                    p.mul_(torch.from_numpy(1 + 0.05 * rs.standard_normal(tuple(p.shape)).astype(F32)))
        with open(cfg.agent_load_dir + f'GLEET_Agent/checkpoint{cp}.pkl', 'wb') as f:
            pickle.dump(a, f, -1)
        agents.append(a)
    train = construct_problem_set(copy.deepcopy(cfg))[0]
    two = train.data[:2]
    monkeypatch.setattr(tester, 'construct_problem_set', lambda config: (type('S', (), {'data': two})(), None))
    calls = []
    real = GLEET_Agent.rollout_checkpoints
    monkeypatch.setattr(GLEET_Agent, 'rollout_checkpoints', staticmethod(lambda ags, env: (calls.append((len(ags), env.B)), real(ags, env))[1]))
    res = tester.rollout(copy.deepcopy(cfg))
    assert calls == [(2, 8)]
    with open(cfg.rollout_log_dir + 'rollout.pkl', 'rb') as f:
        disk = pickle.load(f)
    assert sorted(disk) == ['cost', 'fes', 'return']
    pidx, run = tester.instance_table(2, 2)
    n = len(pidx)
    for cp in range(2):
        agents[cp].to('cuda')
        env = BatchedPBO_Env(two, GLEET_Optimizer(copy.deepcopy(cfg)), pidx, tester.philox_seed(run, np.arange(n), cp))
        one = {k: v.cpu().numpy() for k, v in agents[cp].rollout_batch(env, policy='resident').items()}
        env.close()
        for k, p in enumerate(two):
            rows = slice(k * 2, (k + 1) * 2)
            for key in ('cost', 'fes', 'return'):
                assert sorted(disk[key][str(p)]) == ['GLEET_Agent'] and len(disk[key][str(p)]['GLEET_Agent']) == 2 and len(disk[key][str(p)]['GLEET_Agent'][cp]) == 2
            got = disk['cost'][str(p)]['GLEET_Agent'][cp]
            assert all(len(r) == 51 for r in got)
            assert _same(np.array(got), np.array([tester._pad51(r) for r in one['cost'][rows]])), (cp, str(p))
            assert disk['fes'][str(p)]['GLEET_Agent'][cp] == [float(v) for v in one['fes'][rows]]
            assert disk['return'][str(p)]['GLEET_Agent'][cp] == [float(v) for v in one['return'][rows]]
    assert res['cost'].keys() == disk['cost'].keys()
