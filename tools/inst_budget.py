#!/usr/bin/env python
"""Per-phase vector-instruction budget of the headline resident kernel k_rlepso_run<256, 100, 10, 5, true>, by ablation.

  python tools/inst_budget.py build   [--csrc DIR] [--out DIR]       (no GPU needed: hipcc cross-compiles)
  python tools/inst_budget.py measure [--out DIR] [--json FILE] [--only a,b,...]      (on the GPU box)

build: one library per variant of VARIANTS -- mbx_run_rlepso.hip (the translation unit that holds the headline kernel) recompiled with the variant's -D switches and
linked with the objects `make -C metabox_amd/csrc` left behind -- into DIR/libmbx_<variant>.so, and the kernel's registers / scratch bytes from the shipped build's
assembly into DIR/static.json.  The ablation builds compute something else than RLEPSO: they are never shipped and only ever counted.

measure: for every library, ONE `rocprofv3 --pmc SQ_INSTS_VALU` pass (no trace domains) over `bench.py --steps 20 --warmup 5 --repeats 1` (the driver's window: every
instance live, one 20-generation launch) with MBX_LIB pointing at it; SQ_INSTS_VALU of the longest k_rlepso_run dispatch / (instances x 20) = vector wave-instructions per
env-step.  A phase's row is the difference between the full build and the build without it (rows of nested switches are differences of differences, see PHASES); the
differences are not additive to the last instruction -- a phase's absence changes register allocation and, through the swarm's trajectory, the re-initialisation rate --
so the table carries the unattributed remainder as its own row.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPFLAGS = '--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DMBX_NOINLINE_MATH -fPIC -fvisibility=default'.split()


def makefile_objs():
    """Every object of csrc/Makefile but mbx_run_rlepso.o (the translation unit the variants recompile): the list follows the Makefile."""
    text = open(os.path.join(ROOT, 'metabox_amd', 'csrc', 'Makefile')).read()
    objs = re.search(r'^OBJS\s*=\s*(.+)$', text, re.M).group(1).split()
    assert 'mbx_run_rlepso.o' in objs and all(o.endswith('.o') for o in objs), objs
    return [o for o in objs if o != 'mbx_run_rlepso.o']


OBJS = makefile_objs()
SITE_PART, SITE_ELEM_A, SITE_TOURN = 2, 0, 17                 # include/mbx_layout.h
VARIANTS = {
    'full': [],
    'no_policy': ['-DMBX_ABLATE_POLICY'],                      # the action is the table's mu: no Philox, no Box-Muller
    'no_rank': ['-DMBX_ABLATE_RANK'],                          # rank = index: no cost compares
    'no_part_rng': [f'-DMBX_ABLATE_RNG_SITES={1 << SITE_PART}u'],
    'no_stage': ['-DMBX_ABLATE_STAGE'],                        # pbest rows staged in the first generation of a launch only
    'no_fdr_scan': ['-DMBX_ABLATE_FDR_SCAN'],                  # the FDR pass with zero-trip scan loops
    'no_fdr': ['-DMBX_ABLATE_FDR'],                            # no FDR pass at all (KB = 0)
    'no_move_rng': [f'-DMBX_ABLATE_RNG_SITES={(1 << SITE_ELEM_A) | (1 << SITE_TOURN)}u'],
    'no_move': ['-DMBX_ABLATE_MOVE'],
    'no_eval': ['-DMBX_ABLATE_EVAL'],                          # x_0^2 + bias instead of the objective
    'no_commit': ['-DMBX_ABLATE_COMMIT'],
    'no_reinit_draw': ['-DMBX_ABLATE_REINIT_DRAW'],            # no draw, nobody re-initialised
    'no_log': ['-DMBX_ABLATE_LOG'],
    # not ablations but A/B switches of the full kernel (same results): what one trim is worth, as full - variant (TRIMS)
    'per_item_tourn': ['-DMBX_RL_LISTED_TOURN=0'],             # the move with one tournament draw per wave-pass, as k_rlepso_step has it
    'round_bound': ['-DMBX_FDR_ROUND_BOUND'],                  # the scan's bound rounded up to whole unrolled groups (measured and dropped)
    'one_group': ['-DMBX_FDR_GROUPS=1'],                       # the scan's loops as before the third budget: one group per trip, indexed remainder
    'two_groups': ['-DMBX_FDR_GROUPS=2'],                      # two groups (8 candidates) per trip instead of the shipped three
    'no_prio': ['-DMBX_RL_PRIO=0'],                            # no s_setprio around the FDR pass (scalar instructions: the vector count is the same; the A/B is one of time)
    'old_deal': ['-DMBX_FDR_DEAL=0'],                          # the FDR pass dealt from item 0 with the short pass at the top ranks, as before the fourth budget
    'wave_deal': ['-DMBX_FDR_WAVE_DEAL=1'],                    # wave 0 takes the chunks of bounds 10 + 87 (not shipped; same chunks: the A/B is one of time)
    'prio2': ['-DMBX_RL_PRIO=2'],                              # a third priority level around the phases of wave 0 / of the particle waves (not shipped; scalar instructions)
}
TRIMS = [('tournaments compacted per wave', 'full', 'per_item_tourn'), ('scan bound rounded up to whole groups (not shipped)', 'round_bound', 'full'),
         ('scan: three groups per trip from one pair of address registers, straight-line remainder', 'full', 'one_group'),
         ('scan: two groups per trip instead of three (not shipped)', 'two_groups', 'full'), ('wave priority 1 outside the FDR pass, 0 inside (scalar instructions: no vector instruction is saved)', 'full', 'no_prio'),
         ('FDR pass dealt from the top of the table: the short chunk at the low ranks', 'full', 'old_deal'),
         ('chunk-to-wave table: wave 0 takes bounds 10 + 87 (not shipped)', 'wave_deal', 'full'), ('third priority level (not shipped; scalar instructions)', 'prio2', 'full')]
# phase -> (minuend variant, subtrahend variant): instructions of the phase = count(minuend) - count(subtrahend)
PHASES = [
    ('policy draw', 'full', 'no_policy'),
    ('ranking (cost compares)', 'full', 'no_rank'),
    ('per-particle draws (Philox)', 'full', 'no_part_rng'),
    ('pbest staging', 'full', 'no_stage'),
    ('FDR pass: inner loops', 'full', 'no_fdr_scan'),
    ('FDR pass: scaffolding', 'no_fdr_scan', 'no_fdr'),
    ('move: Philox', 'full', 'no_move_rng'),
    ('move: all', 'full', 'no_move'),
    ('objective', 'full', 'no_eval'),
    ('commit', 'full', 'no_commit'),
    ('re-init draw and what it triggers', 'full', 'no_reinit_draw'),
    ('logging, termination, reward', 'full', 'no_log'),
]
KERNEL = '_ZN3mbx12k_rlepso_runILi256ELi100ELi10ELi5ELb1EE'
CAVEATS = ('a row is only as good as its ablation: without the move or with the one-coordinate objective the swarms take another course (re-initialisation storms, early stops), so \'move: the rest\' and \'objective\' are NOT instruction counts of those phases; with zero-trip scan loops the compiler folds most of the scan\'s set-up, so \'FDR pass: scaffolding\' is a lower bound; rows within +-20 of zero are below the method\'s resolution; with rank = index (no_rank) the cost column is not ascending, which the scan\'s near-tie flag (a_0 < 0) relies on: \'ranking\' is not a count of the ranking either')


def build(a):
    csrc = os.path.abspath(a.csrc)
    os.makedirs(a.out, exist_ok=True)
    objdir = os.path.join(ROOT, 'metabox_amd', 'csrc')
    missing = [o for o in OBJS if not os.path.exists(os.path.join(objdir, o))]
    assert not missing, f'run `make -C metabox_amd/csrc` first: {missing}'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    tmp = tempfile.mkdtemp(prefix='mbx_budget_')
    procs = []
    try:
        for name, flags in VARIANTS.items():
            obj = os.path.join(tmp, name + '.o')
            procs.append((name, obj, subprocess.Popen([hipcc, *HIPFLAGS, *flags, '-c', '-o', obj, 'mbx_run_rlepso.hip'], cwd=csrc)))
            if len(procs) % a.jobs == 0:
                for _, _, p in procs[-a.jobs:]:
                    p.wait()
        asm = os.path.join(tmp, 'full.s')
        subprocess.check_call([hipcc, *HIPFLAGS, '--offload-device-only', '-S', '-o', asm, 'mbx_run_rlepso.hip'], cwd=csrc, stderr=subprocess.DEVNULL)
        for name, obj, p in procs:
            assert p.wait() == 0, name
            subprocess.check_call([hipcc, *HIPFLAGS, '-shared', '-o', os.path.join(a.out, f'libmbx_{name}.so'), obj, *[os.path.join(objdir, o) for o in OBJS]])
        text = open(asm).read()
        desc = text[text.index('.amdhsa_kernel ' + KERNEL):]
        desc = desc[:desc.index('.end_amdhsa_kernel')]
        static = {k: int(re.search(r'\.amdhsa_' + k + r'\s+(\d+)', desc).group(1))
                  for k in ('private_segment_fixed_size', 'next_free_vgpr', 'next_free_sgpr', 'group_segment_fixed_size')}
        json.dump({'kernel': 'k_rlepso_run<256, 100, 10, 5, true>', 'scratch_bytes_per_thread': static['private_segment_fixed_size'], 'vgprs': static['next_free_vgpr'],
                   'sgprs': static['next_free_sgpr'], 'static_lds_bytes': static['group_segment_fixed_size']}, open(os.path.join(a.out, 'static.json'), 'w'), indent=1)
        print(open(os.path.join(a.out, 'static.json')).read())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def count(lib, timeout_s):
    """(vector wave-instructions per env-step of the 20-generation launch, instances) with MBX_LIB = lib."""
    exe = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    tmp = tempfile.mkdtemp(prefix='mbx_budget_')
    try:
        env = dict(os.environ, MBX_LIB=os.path.abspath(lib))
        r = subprocess.run([exe, '--pmc', 'SQ_INSTS_VALU', '--output-format', 'csv', '-d', tmp, '-o', 'p', '--', sys.executable, os.path.join(ROOT, 'bench.py'),
                            '--steps', '20', '--warmup', '5', '--repeats', '1'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout_s)
        assert r.returncode == 0, (lib, r.returncode, r.stdout[-400:], r.stderr[-800:])
        line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
        instances = int(json.loads(line)['config']['instances_per_gpu'])
        rows = {}
        for path in glob.glob(os.path.join(tmp, '**', '*counter_collection.csv'), recursive=True):
            for row in csv.DictReader(open(path)):
                if 'k_rlepso_run' in row['Kernel_Name'] and row['Counter_Name'] == 'SQ_INSTS_VALU':
                    rows[row['Dispatch_Id']] = rows.get(row['Dispatch_Id'], 0.) + float(row['Counter_Value'])
        assert rows, (lib, 'no k_rlepso_run dispatch in the counter file')
        return max(rows.values()) / (instances * 20.), instances          # the 20-generation launch issues more than the 5-generation warm-up
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def measure(a):
    only = a.only.split(',') if a.only else list(VARIANTS)
    counts = json.load(open(a.json)).get('variants', {}) if os.path.exists(a.json) else {}
    instances = None
    for name in only:
        lib = os.path.join(a.out, f'libmbx_{name}.so')
        if not os.path.exists(lib):
            print('missing', lib)
            continue
        counts[name], instances = count(lib, a.timeout)
        print(f'{name:16s} {counts[name]:9.1f}', flush=True)
        write(a, counts, instances)


def write(a, counts, instances):
    out = {'command': 'rocprofv3 --pmc SQ_INSTS_VALU -- python bench.py --steps 20 --warmup 5 --repeats 1   (MBX_LIB = one build per variant; tools/inst_budget.py)',
           'unit': 'vector wave-instructions per env-step (instance-generation) of k_rlepso_run<256, 100, 10, 5, true>', 'instances': instances, 'variants': counts}
    st = os.path.join(a.out, 'static.json')
    if os.path.exists(st):
        out['static'] = json.load(open(st))
    out['caveats'] = CAVEATS
    if 'full' in counts:
        ph = {n: counts[p] - counts[m] for n, p, m in PHASES if p in counts and m in counts}
        if 'move: all' in ph and 'move: Philox' in ph:
            ph['move: the rest'] = ph.pop('move: all') - ph['move: Philox']
        out['phases'] = {k: round(v, 1) for k, v in ph.items()}
        out['total'] = round(counts['full'], 1)
        out['trims'] = {n: round(counts[p] - counts[m], 1) for n, p, m in TRIMS if p in counts and m in counts}
        valid = sum(v for k, v in ph.items() if k not in ('objective', 'move: the rest'))      # (see CAVEATS)
        out['not attributed by a valid ablation (objective, the move without its Philox calls, policy coefficients, block set-up, interactions)'] = round(counts['full'] - valid, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(out, open(a.json, 'w'), indent=1)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('cmd', choices=['build', 'measure'])
    ap.add_argument('--csrc', default=os.path.join(ROOT, 'metabox_amd', 'csrc'), help='source directory of the variants (another checkout\'s csrc: a before / after pair)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'build', 'inst_budget'))
    ap.add_argument('--json', default=os.path.join(ROOT, 'build', 'inst_budget', 'headline_inst_budget.json'))
    ap.add_argument('--only', default='')
    ap.add_argument('--jobs', type=int, default=4)
    ap.add_argument('--timeout', type=int, default=240)
    a = ap.parse_args()
    {'build': build, 'measure': measure}[a.cmd](a)
