"""ctypes binding of the C-ABI in include/mbx.h, include/mbx_les.h, include/mbx_l2l.h, include/mbx_gleet.h, include/mbx_symbol.h, include/mbx_rlhpsde.h and include/mbx_nlshade.h (libmbx.so).

This is the stub a maintainer of the reference would add to reach the HIP path (INTEGRATION.md shows it
in isolation).  The library is built in-tree by ``__graft_entry__.build()`` / ``make -C metabox_amd/csrc``;
loading fails loudly when it is missing — there is no CPU fallback in the product.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MBX_LIB') or os.path.join(_HERE, 'csrc', 'libmbx.so')   # MBX_LIB: kernel-ablation builds (tools/kbench.py)

c_double_p = C.POINTER(C.c_double)


class ProblemDesc(C.Structure):
    """mbx_problem_desc"""
    _fields_ = [('func_id', C.c_int32), ('kind', C.c_int32), ('dim', C.c_int32), ('n_peaks', C.c_int32),
                ('noise_kind', C.c_int32), ('reserved', C.c_int32),
                ('bias', C.c_double), ('lb', C.c_double), ('ub', C.c_double), ('pen_coef', C.c_double),
                ('s', C.c_double * 4), ('noise_a', C.c_double), ('noise_b', C.c_double),
                ('dshift', c_double_p), ('m1', c_double_p), ('m2', c_double_p),
                ('v0', c_double_p), ('v1', c_double_p), ('v2', c_double_p),
                ('py', c_double_p), ('pc', c_double_p), ('pw', c_double_p)]


class AlgoCfg(C.Structure):
    """mbx_algo_cfg"""
    _fields_ = [('algo', C.c_int32), ('np', C.c_int32), ('dim', C.c_int32), ('max_fes', C.c_int32),
                ('log_interval', C.c_int32), ('n_logpoint', C.c_int32), ('early_stop', C.c_int32),
                ('n_group', C.c_int32), ('flags', C.c_uint32)]


# mbx_algo_cfg.flags (include/mbx.h)
F_FDR_FAST, F_GENERIC_GEOMETRY, F_ROLLOUT_PER_GENERATION, F_NRLPSO_RECOMPUTE = 1, 2, 4, 8


class GaussMlp(C.Structure):
    """mbx_gauss_mlp"""
    _fields_ = [('d_weights', C.c_void_p), ('in_dim', C.c_int32), ('h1', C.c_int32), ('h2', C.c_int32), ('out_dim', C.c_int32),
                ('min_sigma', C.c_float), ('max_sigma', C.c_float), ('variant', C.c_int32)]


class LstmPolicy(C.Structure):
    _fields_ = [('d_weights', C.c_void_p), ('in_dim', C.c_int32), ('hidden', C.c_int32), ('out_dim', C.c_int32)]


class QNet(C.Structure):
    """mbx_qnet"""
    _fields_ = [('d_weights', C.c_void_p), ('in_dim', C.c_int32), ('width', C.c_int32), ('depth', C.c_int32), ('n_act', C.c_int32)]


class DedqnNet(C.Structure):
    """mbx_dedqn_net"""
    _fields_ = [('d_weights', C.c_void_p), ('in_dim', C.c_int32), ('hidden', C.c_int32), ('n_act', C.c_int32)]


class GleetActor(C.Structure):
    """mbx_gleet_actor"""
    _fields_ = [('d_weights', C.c_void_p), ('n_floats', C.c_int32), ('min_sigma', C.c_float), ('max_sigma', C.c_float)]


ALGO_RLEPSO, ALGO_LDE, ALGO_DEDDQN, ALGO_RANDOM_SEARCH, ALGO_RLPSO, ALGO_GLEET, ALGO_QLPSO, ALGO_DE, ALGO_PSO, ALGO_CMAES = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
ALGO_GLPSO = 11
ALGO_JDE21 = 13      # (12 is not assigned)
ALGO_MADDE = 15      # (14 is not assigned)
ALGO_SDMSPSO = 18    # (17 is not assigned)
ALGO_DEDQN = 16
ALGO_NRLPSO = 19
ALGO_SAHLPSO = 20
ALGO_LES = 21
ALGO_RLHPSDE = 24    # (22 and 23 are not assigned)
ALGO_NLSHADE = 25
ALGO_L2L = 26
ALGO_SYMBOL = 27
POLICY_RLEPSO, POLICY_RLPSO = 0, 1
_ARRAY_FIELDS = ('dshift', 'm1', 'm2', 'v0', 'v1', 'v2', 'py', 'pc', 'pw')


def pack_desc(d):
    """dict from ``problem.desc()`` -> (ProblemDesc, keepalive list of numpy arrays)."""
    st = ProblemDesc()
    keep = []
    for k in ('func_id', 'kind', 'dim', 'n_peaks', 'noise_kind'):
        setattr(st, k, int(d[k]))
    for k in ('bias', 'lb', 'ub', 'pen_coef', 'noise_a', 'noise_b'):
        setattr(st, k, float(d[k]))
    for i in range(4):
        st.s[i] = float(d['s'][i])
    for k in _ARRAY_FIELDS:
        a = d.get(k)
        if a is None:
            setattr(st, k, c_double_p())
        else:
            a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            setattr(st, k, a.ctypes.data_as(c_double_p))
    return st, keep


def pack_descs(descs):
    arr = (ProblemDesc * len(descs))()
    keep = []
    for i, d in enumerate(descs):
        st, k = pack_desc(d)
        arr[i] = st
        keep.extend(k)
    return arr, keep


_lib = None


class MbxError(RuntimeError):
    pass


def load_lib():
    """Load libmbx.so and declare the prototypes of every symbol in include/mbx.h, include/mbx_les.h, include/mbx_l2l.h, include/mbx_gleet.h, include/mbx_symbol.h, include/mbx_rlhpsde.h and include/mbx_nlshade.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH) and not os.environ.get('MBX_LIB'):
        # a fresh checkout (built artefacts are not in git): build in-tree once, exactly like __graft_entry__.build()
        import shutil
        import subprocess
        if shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc'):
            subprocess.call(['make', '-C', os.path.join(_HERE, 'csrc'), '-s'])
    if not os.path.exists(LIB_PATH):
        raise MbxError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                       f'(hipcc --offload-arch=gfx950). metabox_amd has no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    vp, i32, u64, i64 = C.c_void_p, C.c_int32, C.c_uint64, C.c_int64
    proto = {
        'mbx_suite_create': (C.c_int, [C.POINTER(ProblemDesc), C.c_int, c_double_p, C.POINTER(vp)]),
        'mbx_suite_destroy': (C.c_int, [vp]),
        'mbx_suite_size': (C.c_int, [vp]),
        'mbx_suite_optimum': (C.c_int, [vp, c_double_p]),
        'mbx_suite_close_pairs': (C.c_int, [vp, C.c_int]),
        'mbx_eval': (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, u64, vp, vp]),
        'mbx_state_dim': (C.c_int, [C.POINTER(AlgoCfg)]),
        'mbx_action_dim': (C.c_int, [C.POINTER(AlgoCfg)]),
        'mbx_tape_stride': (i64, [C.POINTER(AlgoCfg)]),
        'mbx_batch_create': (C.c_int, [vp, C.POINTER(AlgoCfg), C.POINTER(i32), C.POINTER(u64), C.c_int,
                                       C.POINTER(vp)]),
        'mbx_batch_destroy': (C.c_int, [vp]),
        'mbx_batch_flags': (C.c_int, [vp]),
        'mbx_set_tape': (C.c_int, [vp, vp]),
        'mbx_reset': (C.c_int, [vp, vp, vp]),
        'mbx_step': (C.c_int, [vp, vp, vp, vp, vp, vp]),
        'mbx_results': (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        'mbx_gauss_policy': (C.c_int, [vp, C.POINTER(GaussMlp), vp, vp, vp, vp]),
        'mbx_lde_policy': (C.c_int, [vp, C.POINTER(LstmPolicy), vp, vp, vp, vp, vp, vp]),
        'mbx_ddqn_qnet': (C.c_int, [vp, C.POINTER(QNet), vp, vp, vp, vp]),
        'mbx_rlepso_policy_table_rows': (C.c_int, [vp]),
        'mbx_rlepso_policy_table': (C.c_int, [vp, C.POINTER(GaussMlp), vp, vp]),
        'mbx_rlepso_act_step': (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        'mbx_rlepso_rollout_resident': (C.c_int, [vp]),
        'mbx_rlepso_rollout': (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
        'mbx_lde_rollout_resident': (C.c_int, [vp]),
        'mbx_lde_rollout': (C.c_int, [vp, C.POINTER(LstmPolicy), vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
        'mbx_rlpso_rollout': (C.c_int, [vp, C.POINTER(GaussMlp), C.c_int, vp, vp, vp, vp, vp]),
        'mbx_qlpso_rollout': (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, vp]),
        'mbx_dedqn_rollout': (C.c_int, [vp, C.POINTER(DedqnNet), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
        'mbx_nrlpso_rollout': (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
        'mbx_les_set_params': (C.c_int, [vp, vp, C.c_int, vp]),
        'mbx_les_rollout': (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        'mbx_l2l_set_params': (C.c_int, [vp, vp, C.c_int, vp]),
        'mbx_l2l_rollout': (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
        'mbx_gleet_set_params': (C.c_int, [vp, vp, C.c_int, vp, C.c_float, C.c_float]),
        'mbx_gleet_rollout': (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
        'mbx_symbol_rollout': (C.c_int, [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]),
        'mbx_rlhpsde_rollout': (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
        'mbx_nlshade_run': (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
        'mbx_gleet_policy': (C.c_int, [vp, C.POINTER(GleetActor), vp, vp, vp, vp]),
        'mbx_debug_math': (C.c_int, [C.c_int, vp, vp, vp, C.c_int, vp]),
        'mbx_debug_reduce': (C.c_int, [C.c_int, vp, vp, C.c_int, vp, vp]),
        'mbx_debug_rlepso_draws': (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        'mbx_batch_launch_info': (C.c_int, [vp, C.POINTER(C.c_int32)]),
        'mbx_instance_state_doubles': (i64, [vp]),
        'mbx_debug_read_state': (C.c_int, [vp, C.c_int, c_double_p]),
        'mbx_debug_write_state': (C.c_int, [vp, C.c_int, c_double_p]),
        'mbx_debug_clock_probe': (C.c_int, [vp, C.c_int, C.c_int, vp]),
        'mbx_debug_clock_mark': (C.c_int, [vp, vp]),
        'mbx_debug_clock_slots': (C.c_int, [vp, vp]),
        'mbx_batch_rebind': (C.c_int, [vp, vp, vp]),
        'mbx_read_public': (C.c_int, [vp, C.c_int, c_double_p, vp]),
        'mbx_last_error': (C.c_char_p, []),
        'mbx_version': (C.c_char_p, []),
    }
    for name, (res, args) in proto.items():
        fn = getattr(lib, name)          # AttributeError here = header and library out of sync
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTED_SYMBOLS = ('mbx_suite_create', 'mbx_suite_destroy', 'mbx_suite_size', 'mbx_suite_optimum', 'mbx_suite_close_pairs', 'mbx_eval', 'mbx_state_dim', 'mbx_action_dim',
                    'mbx_tape_stride', 'mbx_batch_create', 'mbx_batch_destroy', 'mbx_batch_flags', 'mbx_set_tape', 'mbx_reset', 'mbx_step', 'mbx_results',
                    'mbx_gauss_policy', 'mbx_lde_policy', 'mbx_ddqn_qnet', 'mbx_rlepso_policy_table_rows', 'mbx_rlepso_policy_table', 'mbx_rlepso_act_step',
                    'mbx_rlepso_rollout_resident', 'mbx_rlepso_rollout', 'mbx_lde_rollout_resident', 'mbx_lde_rollout', 'mbx_rlpso_rollout',
                    'mbx_qlpso_rollout', 'mbx_dedqn_rollout', 'mbx_nrlpso_rollout', 'mbx_gleet_policy', 'mbx_debug_math', 'mbx_debug_reduce', 'mbx_debug_rlepso_draws', 'mbx_batch_launch_info', 'mbx_instance_state_doubles',
                    'mbx_debug_read_state', 'mbx_debug_write_state', 'mbx_debug_clock_probe', 'mbx_debug_clock_mark', 'mbx_debug_clock_slots',
                    'mbx_batch_rebind', 'mbx_read_public', 'mbx_last_error', 'mbx_version')

# the entry points of include/mbx_les.h (LES), beside the 45 of include/mbx.h
LES_SYMBOLS = ('mbx_les_set_params', 'mbx_les_rollout')

# the entry points of include/mbx_l2l.h (L2L)
L2L_SYMBOLS = ('mbx_l2l_set_params', 'mbx_l2l_rollout')

# the entry points of include/mbx_gleet.h (GLEET's resident rollout)
GLEET_SYMBOLS = ('mbx_gleet_set_params', 'mbx_gleet_rollout')

# the entry point of include/mbx_symbol.h (SYMBOL)
SYMBOL_SYMBOLS = ('mbx_symbol_rollout',)

# the entry point of include/mbx_rlhpsde.h (RL-HPSDE)
RLHPSDE_SYMBOLS = ('mbx_rlhpsde_rollout',)

# the entry point of include/mbx_nlshade.h (NL_SHADE_LBC)
NLSHADE_SYMBOLS = ('mbx_nlshade_run',)


def check(rc):
    if rc != 0:
        msg = load_lib().mbx_last_error()
        raise MbxError(f'mbx error {rc}: {msg.decode() if msg else "?"}')
