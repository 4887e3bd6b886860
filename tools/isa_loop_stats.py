#!/usr/bin/env python3
"""Developer tool: instruction mix of the largest basic block (the 2x-unrolled z-loop body) of kernels in a gfx950 .s file.
Usage: tools/isa_loop_stats.py file.s [--top=K] substring [substring...]   (.s from hipcc -S --cuda-device-only)
--top=K lists the K largest blocks: the one-lane float64 and the packed float32 4-wave kernels hold two z-loops (general and
mirrored).  For the float32 unit:  SRC=psa_rk4_f32.hip OUT=/tmp/f32.s tools/asm_f64.sh  and then
tools/isa_loop_stats.py /tmp/f32.s --top=2 rk4_sweep_pk_kernel  (valu = packed instructions per two-step trip and point pair).
--row=SE --step=S [--trips=1,2,4] [--via=LABEL,...] walks ONE SAVED ROW of SE steps through the kernel's control flow instead: S the vector
instructions of a step (144 mirrored loop, 288 general), --trips the steps per step block in the order a row runs them, the
largest repeated (the row loop: 1,2,4; the event loop: 2,1; the fixed-row loop, one block of SE steps: --trips=SE).  Prints the instructions executed, those outside the steps, the
branches taken and the path (profiles/row_loop.log)."""
import re, sys
from collections import Counter


def row_walk(name, body, se, step, trips, via=()):
    """One saved row of `se` steps walked through the kernel's control flow: the cheapest closed path (instructions
    executed, then branches taken) that runs the row's step blocks in order and returns to the first.  A step block is a
    block of k * step (+ at most 7 * k) vector instructions, k one of `trips`; the path may pass through no other.  Only labels and
    branch targets are read: an instruction with a block label for operand is a branch, conditional if it falls through.
    `via`: labels the path has to pass, in order, after the row's last step block (the cheapest path is otherwise one on which
    nothing is due: name the block of the row work, read from the assembly)."""
    import heapq
    nodes = []                                   # [label, instructions, valu, taken target or None, falls through]
    cur = ['entry', 0, 0, None, True]
    for line in body.splitlines():
        t = line.strip()
        m = re.match(r'(\.LBB\d+_\d+):', t)
        if m:
            nodes.append(cur)
            cur = [m.group(1), 0, 0, None, True]
            continue
        if not t or t.startswith((';', '.')):
            continue
        op = t.split()[0]
        cur[1] += 1
        cur[2] += op.startswith('v_')
        tgt = re.search(r'\s(\.LBB\d+_\d+)\b', t)
        if tgt or 'endpgm' in op:                # a branch (or the end) closes the node; what follows is reached by falling through
            cur[3] = tgt.group(1) if tgt else None
            cur[4] = bool(tgt) and 'cbranch' in op
            nodes.append(cur)
            cur = [cur[0] + '+', 0, 0, None, True]
    nodes.append(cur)
    first = {}
    for k, nd in enumerate(nodes):
        first.setdefault(nd[0], k)
    big = max(trips)
    seq = []
    for t in trips:
        seq += [t] * (se // big) if t == big else ([t] if se & t else [])
    assert sum(seq) == se, (seq, se)

    def steps_of(nd):                            # how many steps a block runs: 0 = not a step block, -1 = one the row has no use for
        k = (nd[2] + step // 4) // step
        if nd[2] < step:
            return 0
        return k if (k in trips and 0 <= nd[2] - k * step <= 7 * k) else -1

    kinds = [steps_of(nd) for nd in nodes]
    best = None
    for s0, nd0 in enumerate(nodes):
        if kinds[s0] != seq[0]:
            continue
        heap = [(nd0[1], 0, s0, 1, 0, (nd0[0],))]   # cost so far includes the node we are in
        seen = set()
        while heap:
            ins, taken, k, done, v, path = heapq.heappop(heap)
            if (k, done, v) in seen:
                continue
            seen.add((k, done, v))
            nd = nodes[k]
            succ = []
            if nd[3] is not None and nd[3] in first:
                succ.append((first[nd[3]], 1))
            if nd[4] and k + 1 < len(nodes):
                succ.append((k + 1, 0))
            for n, tk in succ:
                # back at the start, not by the trip's own back-edge: a row was passed (a row that is ONE block -- the fixed-row
                # loop, --trips=SE -- closes on that block's own back-edge)
                if n == s0 and done == len(seq) and v == len(via) and (k != s0 or len(seq) == 1):
                    cand = (ins, taken + tk, path)
                    best = min(best, cand) if best else cand
                    continue
                d = done
                if kinds[n]:
                    if d >= len(seq) or kinds[n] != seq[d]:
                        continue
                    d += 1
                w = v + (v < len(via) and d == len(seq) and nodes[n][0] == via[v])
                heapq.heappush(heap, (ins + nodes[n][1], taken + tk, n, d, w, path + ((nodes[n][0],) if nodes[n][0] != path[-1] else ())))
    if not best:
        print(name[:80], f'row of {se} steps: no closed path runs the step blocks {seq}')
        return
    ins, taken, path = best
    print(name[:80], f'row of {se} steps as {seq} x {step} valu: instructions {ins}, outside the steps {ins - se * step}, '
          f'branches taken {taken}')
    print('    path:', ' '.join(path))


opt = {a[2:].split('=')[0]: a.split('=')[1] for a in sys.argv if a.startswith(('--row=', '--step=', '--trips=', '--via='))}
sys.argv = [a for a in sys.argv if not a.startswith(('--row=', '--step=', '--trips=', '--via='))]
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
    if 'row' in opt:
        row_walk(name, body, int(opt['row']), int(opt.get('step', 144)), [int(t) for t in opt.get('trips', '1,2,4').split(',')],
                 tuple(opt['via'].split(',')) if 'via' in opt else ())
        continue
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
