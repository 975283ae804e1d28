#!/usr/bin/env python3
"""Compare the device code of two builds, function by function.

    hipcc <the Makefile's flags> --offload-device-only -S -o A/<unit>.s <unit>.hip      (every unit, both trees)
    python tools/asm_same.py A B

For every *.s in both directories: each function's text (from its `.type name,@function` to its `.size`) and each kernel descriptor (`.amdhsa_kernel` ..
`.end_amdhsa_kernel`), with the compiler's local labels renumbered in order of appearance, since their numbers count the functions before them; and the
`amdhsa.kernels` metadata as a whole.  Text is compared, nothing is looked for in it.  Prints one line per unit and the names that differ; exit status 1
if anything does.
"""
import os
import re
import sys

LABEL = re.compile(r'\.L[A-Za-z_]+\d+(?:_\d+)?')


def pieces(path):
    """-> ({name: normalised text} for functions and kernel descriptors, metadata text)"""
    out, meta, name, body, in_meta = {}, [], None, [], False
    with open(path) as f:
        for line in f:
            s = line.strip()
            if in_meta:
                in_meta = s != '.end_amdgpu_metadata'
                if in_meta and not s.startswith('amdhsa.target'):
                    meta.append(s)
                continue
            if s == '.amdgpu_metadata':
                in_meta = True
            elif name is None:
                m = re.match(r'\.type\s+(\S+),@function', s) or re.match(r'\.amdhsa_kernel\s+(\S+)', s)
                if m:
                    name, body = m.group(1) + (' (descriptor)' if s.startswith('.amdhsa') else ''), []
            elif s.startswith('.size') or s == '.end_amdhsa_kernel':
                seen = {}
                out[name] = LABEL.sub(lambda m: seen.setdefault(m.group(0), f'.L{len(seen)}'), '\n'.join(body))
                name = None
            elif s and not s.startswith(';'):
                body.append(s.split(' ; ')[0].rstrip())
    return out, '\n'.join(meta)


def main(a, b):
    units = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = 0
    print(f'{"unit":28} {"functions":>9} {"same":>6} {"differ":>6} {"only one side":>13}  kernel metadata')
    for u in (u for u in units if u.endswith('.s')):
        if not (os.path.exists(os.path.join(a, u)) and os.path.exists(os.path.join(b, u))):
            print(f'{u:28} only in {a if os.path.exists(os.path.join(a, u)) else b}')
            bad += 1
            continue
        (fa, ma), (fb, mb) = pieces(os.path.join(a, u)), pieces(os.path.join(b, u))
        differ = sorted(n for n in fa.keys() & fb.keys() if fa[n] != fb[n])
        lone = sorted(fa.keys() ^ fb.keys())
        print(f'{u:28} {len(fa.keys() | fb.keys()):9} {len(fa.keys() & fb.keys()) - len(differ):6} {len(differ):6} {len(lone):13}  {"equal" if ma == mb else "DIFFERENT"}')
        for n in differ:
            print(f'    differs: {n}')
        for n in lone:
            print(f'    only in {a if n in fa else b}: {n}')
        bad += len(differ) + len(lone) + (ma != mb)
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
