"""The dynamic-LDS size of every kernel family over a grid of geometries, pinned to tests/golden/lds_sizes.json.

tests/lds_sizes_main.hip is a host-only program around metabox_amd/csrc/mbx_lds.hpp, where each family's layout is one walk that gives both the size the
host launches with and the pointers the kernel carves.  The file was recorded from the tree as it stood BEFORE the walks, when every family had a
hand-written size formula next to a hand-written carve-up in its kernel header: a walk that ends elsewhere than the formula did has either found an
under-allocation of old (it gives more) or lost a deliberate surplus (it gives less), and neither is settled by recording again.

The grid sits where a formula changes branch: rows * D across 2 * kThreads (51 x 10 | 52 x 10, 1 x D), n across 17 and D across 8 (the evaluator's T), odd
NP / D / products (the rounding to 16 bytes), NP across a power of two (the sort's padding), every boolean and rows in {1, NP}, the documented geometries and
the fixed populations.  Re-record with ``MBX_CSRC=<a csrc directory> python tests/test_lds_sizes.py``; a directory without mbx_lds.hpp is read through
its kernel headers.
"""
import functools
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'lds_sizes.json')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def sizes(csrc, workdir, offsets=False):
    """Build the program against the headers in `csrc`, run it -> {'name(args)': doubles}."""
    exe = os.path.join(workdir, 'lds_sizes')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-w', '-I', csrc, '-o', exe, os.path.join(ROOT, 'tests', 'lds_sizes_main.hip')]
    if not os.path.exists(os.path.join(csrc, 'mbx_lds.hpp')):
        cmd.insert(1, '-DMBX_LDS_SIZES_KERNEL_HEADERS')
    subprocess.check_call(cmd)
    if offsets:
        return subprocess.run([exe, 'offsets'], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    got = {}
    for line in out.splitlines():
        key, doubles = line.split()
        assert key not in got, key
        got[key] = int(doubles)
    return got


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_record_holds_the_sizes_checked_by_hand():
    """Three entries a reader can add up from the layouts, so that a re-recorded file cannot drift."""
    want = golden()
    # SAHLPSO reset, 40 rows at D = 10: X 400 | T 400 | Z 512 | 2 maps of 100 | 4 vectors of 10 | NC 40 | RED 32 | 7 int arrays of 40 = 140
    assert want['sh(40,10,0)'] == 400 + 400 + 512 + 200 + 40 + 40 + 32 + 140 == 1764
    # ... a generation, one row: X 10 | T 170 | Z 512 | 200 | 40 | NC 2 | 32 | 140, then 3 x 400 | 4 x 40 | 8 x 16
    assert want['sh(1,10,1)'] == 10 + 170 + 512 + 200 + 40 + 2 + 32 + 140 + 1200 + 160 + 128 == 2594
    # QLPSO step, one row, NP = 30, D = 10: X 10 | T 170 | Z 512 | 200 | 5 vectors of 10 | NC 2 | RED 16 | POP 300 | COST 30 | DIST 30 | SC 16
    assert want['ql(1,30,10)'] == 10 + 170 + 512 + 200 + 50 + 2 + 16 + 300 + 30 + 30 + 16 == 1336
    assert len(want) == 4799 + 227         # the sym and l2l families joined later, recorded from the tree before their host code moved


def test_every_walk_ends_where_the_recorded_formula_did(tmp_path):
    got, want = sizes(os.path.join(ROOT, 'metabox_amd', 'csrc'), str(tmp_path)), golden()
    assert sorted(got) == sorted(want)
    more = {k: (got[k], want[k]) for k in want if got[k] > want[k]}
    less = {k: (got[k], want[k]) for k in want if got[k] < want[k]}
    assert not more, f'the walk asks for MORE than the formula did (an under-allocation of old?): {sorted(more.items())[:20]}'
    assert not less, f'the walk asks for LESS than the formula did (an unnamed surplus?): {sorted(less.items())[:20]}'


def test_every_walk_carves_where_the_hand_written_carve_did(tmp_path):
    """The families whose kernels carve through the walk (rl, lde, lde_run, gl, gp, cl with the CMA-ES matrices, sh, les): every pointer's offset as the
    carve-ups they replaced gave it (tests/golden/lds_offsets.txt, recorded once from those carves' text compiled for the host: they were device-only functions, so
    the MBX_CSRC route cannot record it again).  The families that keep a hand-written carve are held to their walks by the program itself."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'lds_offsets.txt')) as f:
        want = f.read().splitlines()
    got = sizes(os.path.join(ROOT, 'metabox_amd', 'csrc'), str(tmp_path), offsets=True)
    assert len(want) == 356 and got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


if __name__ == '__main__':
    with tempfile.TemporaryDirectory() as tmp:
        rec = sizes(os.environ.get('MBX_CSRC', os.path.join(ROOT, 'metabox_amd', 'csrc')), tmp)
    with open(GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {v}' for k, v in rec.items()) + '\n}\n')
    print(f'wrote {GOLDEN}: {len(rec)} entries')
