#!/usr/bin/env python3
"""Developer tool: instruction mix of the largest basic block (the 2x-unrolled z-loop body) of kernels in a gfx950 .s file.
Usage: tools/isa_loop_stats.py file.s [--top=K] substring [substring...]   (.s from hipcc -S --cuda-device-only)
--top=K lists the K largest blocks: the one-lane float64 and the packed float32 4-wave kernels hold two z-loops (general and
mirrored).  For the float32 unit:  SRC=psa_rk4_f32.hip OUT=/tmp/f32.s tools/asm_f64.sh  and then
tools/isa_loop_stats.py /tmp/f32.s --top=2 rk4_sweep_pk_kernel  (valu = packed instructions per two-step trip and point pair)."""
import re, sys
from collections import Counter
top = max([int(a[6:]) for a in sys.argv if a.startswith('--top=')] or [1])
sys.argv = [a for a in sys.argv if not a.startswith('--top=')]
s = open(sys.argv[1]).read()
pat = re.compile(r'^(_ZN3psa\S+):\s*; @', re.M)
ms = list(pat.finditer(s))
for k, m in enumerate(ms):
    name = m.group(1)
    if not any(sub in name for sub in sys.argv[2:]):
        continue
    body = s[m.end(): ms[k + 1].start() if k + 1 < len(ms) else len(s)].split('.Lfunc_end')[0]
    blocks = re.split(r'\n(\.LBB\d+_\d+):', body)
    found = []
    for j in range(1, len(blocks), 2):
        ins = [l.strip() for l in blocks[j + 1].splitlines() if l.strip() and not l.strip().startswith((';', '.'))]
        found.append((blocks[j], ins))
    found.sort(key=lambda b: -len(b[1]))
    for best in found[:top]:
        ins = best[1]
        c = Counter(l.split()[0] for l in ins)
        dp = sum(v for kk, v in c.items() if kk.endswith('_f64'))
        valu = sum(v for kk, v in c.items() if kk.startswith('v_'))
        print(name[:80], best[0], 'instrs', len(ins), 'valu', valu, 'f64', dp, 'dpp', sum(1 for l in ins if 'quad_perm' in l))
        print('    non-f64:', {kk: v for kk, v in c.items() if not kk.endswith('_f64')})
