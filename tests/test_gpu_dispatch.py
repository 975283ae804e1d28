"""Every algorithm id through mbx_batch_create, mbx_reset, one mbx_step and mbx_read_public, bit for bit against tests/golden/dispatch_step.json.

The file was recorded on an MI355X from the library as it stood before the per-algorithm descriptor table (``AlgoOps`` in metabox_amd/csrc/mbx.hip)
replaced the if-chains over ``cfg.algo``.  The kernels draw from Philox with fixed seeds and use no cross-workgroup atomics, so the same kernel
with the same workgroup size, LDS size and arguments repeats exactly on the same hardware: equality here says that every row of the table still
launches what its branch of the chains launched.  Ids 24 .. 27 were recorded later, from the library as it stood before the own-unit algorithms'
host code moved into their translation units, in a run that reproduced the eighteen earlier records.  Re-record with ``MBX_LIB=<library> python tests/test_gpu_dispatch.py <output.json>`` on the GPU.
"""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
MBX_E_ARG = -1

# id -> (name, np): the smallest valid population, 16 where the algorithm leaves it free
ALGOS = {1: ('RLEPSO', 16), 2: ('LDE', 16), 3: ('DEDDQN', 16), 4: ('RANDOM_SEARCH', 16), 5: ('RLPSO', 16), 6: ('GLEET', 16), 7: ('QLPSO', 16), 8: ('DE', 16),
         9: ('PSO', 16), 10: ('CMAES', 16), 11: ('GLPSO', 16), 13: ('JDE21', 170), 15: ('MADDE', 200), 16: ('DEDQN', 16), 18: ('SDMSPSO', 99),
         19: ('NRLPSO', 16), 20: ('SAHLPSO', 40), 21: ('LES', 16), 24: ('RLHPSDE', 180), 25: ('NLSHADE', 230), 26: ('L2L', 1), 27: ('SYMBOL', 16)}
assert len(ALGOS) == 22              # every id include/mbx.h assigns: 1 .. 27 without 12, 14, 17, 22 and 23
INT_ACTIONS = (3, 7, 16, 19, 24)     # DE-DDQN, QLPSO, DEDQN, NRLPSO, RL-HPSDE choose among discrete actions
F64_ACTIONS = (26, 27)               # L2L takes the point itself, SYMBOL the program: float64 rows
AGENTS = (1, 2, 3, 5, 6, 7, 16, 19, 24, 26, 27)
NEED_STATE_OUT = (2, 3)              # LDE, DE-DDQN
MAX_FES, LOG_INTERVAL, N_LOGPOINT = 2000, 400, 5
# id -> the entry of tests/golden/lds_sizes.json (doubles; recorded before the layouts became walks in metabox_amd/csrc/mbx_lds.hpp) that launch_info's lds_bytes reports at
# this file's geometry (D = 10): the batch's figure, the larger of the reset's and the step's carve-up where both share it (SAHLPSO), or the step kernel's where
# launch_info reports that one (DE-DDQN, NRLPSO with the distance matrix in LDS)
LDS_ENTRY = {1: 'rl(16,10,1)', 2: 'lde(16,10,1)', 3: 'dq(1,16,10)', 4: 'rs(16,10)', 5: 'rp(16,10,0)', 6: 'gl(16,10)', 7: 'ql(16,16,10)', 8: 'cl(16,16,10,0,0)',
             9: 'cl(16,16,10,0,0)', 10: 'cl(16,16,10,0,1)', 11: 'gp(16,10)', 13: 'jd(170,10)', 15: 'md(200,10)', 16: 'dd(16,10)', 18: 'sd(99,10)',
             19: 'nr(1,16,10,1,1)', 20: 'sh(1,10,1)', 21: 'les(10)', 24: 'hp(180,10)', 25: 'nl(230,10)', 26: 'l2l(10)', 27: 'sym(16,10,1)'}
assert sorted(LDS_ENTRY) == sorted(ALGOS)


@functools.lru_cache(maxsize=None)
def _suite():
    from helpers import problems
    from metabox_amd.suite import Suite
    ps = problems('bbob', 10)
    return Suite([ps[1], ps[10]])           # Sphere and the rotated Ellipsoidal


def _batch(algo):
    from metabox_amd.suite import Batch
    b = Batch(_suite(), algo, [0, 1], [1000 + algo, 2000 + algo], ALGOS[algo][1], MAX_FES, LOG_INTERVAL, N_LOGPOINT)
    if algo == 21:
        with np.load(os.path.join(GOLDEN, 'les_policy.npz')) as z:
            b.les_set_params(z['bbob/best_x'])
    return b


def _zero_actions(b, algo):
    import torch
    dtype = torch.int32 if algo in INT_ACTIONS else torch.float64 if algo in F64_ACTIONS else torch.float32
    return torch.zeros(b.B, b.action_dim, dtype=dtype, device='cuda')


def run(algo):
    """-> {'launch_info': {...}, 'public': [[hex, ...] per instance]} after reset and one step with all-zero actions."""
    import torch
    b = _batch(algo)
    b.reset()
    act = None
    if b.action_dim > 0:
        act = _zero_actions(b, algo)
    b.step(act)
    torch.cuda.synchronize()
    out = {'launch_info': {k: int(v) for k, v in b.launch_info().items()}, 'public': [[float(v).hex() for v in b.read_public(i)] for i in range(b.B)]}
    b.close()
    return out


@functools.lru_cache(maxsize=None)
def _want():
    with open(os.path.join(GOLDEN, 'dispatch_step.json')) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _lds_sizes():
    with open(os.path.join(GOLDEN, 'lds_sizes.json')) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize('algo', sorted(ALGOS), ids=lambda a: ALGOS[a][0])
def test_reset_and_one_step_as_recorded(algo):
    got, want = run(algo), _want()[ALGOS[algo][0]]
    assert len(want['public']) == 2 and len(want['public'][0]) == 16 + N_LOGPOINT + 1
    assert float.fromhex(want['public'][0][1]) >= ALGOS[algo][1], 'the record must hold a batch that has evaluated its population'
    assert got['launch_info']['lds_bytes'] == 8 * _lds_sizes()[LDS_ENTRY[algo]]
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize('algo', AGENTS, ids=lambda a: ALGOS[a][0])
def test_step_refuses_null_actions_of_an_agent_algorithm(algo):
    from metabox_amd._abi import load_lib
    from metabox_amd.suite import _ptr, _stream
    lib, b = load_lib(), _batch(algo)
    rc = lib.mbx_step(b._h, C.c_void_p(), _ptr(b.state), _ptr(b.reward), _ptr(b.done), _stream())        # returns before anything is launched
    assert rc == MBX_E_ARG and lib.mbx_last_error() == b'mbx_step: bad arguments'
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize('algo', NEED_STATE_OUT, ids=lambda a: ALGOS[a][0])
def test_reset_and_step_refuse_a_null_state_out_where_the_kernel_writes_features(algo):
    import torch
    from metabox_amd._abi import load_lib
    from metabox_amd.suite import _ptr, _stream
    lib, b = load_lib(), _batch(algo)
    assert lib.mbx_reset(b._h, C.c_void_p(), _stream()) == MBX_E_ARG                                      # returns before anything is launched
    assert lib.mbx_last_error() == b'mbx_reset: this algorithm needs d_state_out'
    act = _zero_actions(b, algo)
    assert lib.mbx_step(b._h, _ptr(act), C.c_void_p(), _ptr(b.reward), _ptr(b.done), _stream()) == MBX_E_ARG
    assert lib.mbx_last_error() == b'mbx_step: this algorithm needs d_state_out'
    b.close()


if __name__ == '__main__':
    rec = {ALGOS[a][0]: run(a) for a in sorted(ALGOS)}
    with open(sys.argv[1], 'w') as f:
        f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in sorted(rec.items())) + '\n}\n')
    print(f'wrote {sys.argv[1]}')
