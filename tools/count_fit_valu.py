"""Static instruction counts of the fit kernel's loops from the compiler's assembly.
usage: hipcc <CXXFLAGS of csrc/Makefile> --cuda-device-only -S k2b_fit.hip -o k2b_fit.s
       python3 tools/count_fit_valu.py k2b_fit.s [NBT,MODE[,SCAN64] ...]     (default: 10,3 10,0; SCAN64 0 = the fp32 scans)
For every outermost loop of k2b_fit_world_kernel<NBT, MODE, SCAN64> (`loop@<first block>`: all its blocks) and for every basic block
inside one that holds at least 20 instructions: vector-ALU instructions (mnemonics v_*, without v_mfma*), MFMAs, no-ops, DPP and permlane-swap forms,
LDS and barrier instructions.  A block's role shows in its marks: `f64` = the tree pass of the fp64 instantiation, `mfma` = the row waves'
component block, `bar` = it ends an iteration half."""
import re
import sys
from collections import Counter


def kernel_body(lines, nbt, mode, scan64=0):
    # (assembly from before the SCAN64 parameter has two template arguments: matched for scan64 = 1, which is what it ran)
    sym = re.compile(rf'^_ZN3k2b20k2b_fit_world_kernelILi{nbt}ELi{mode}E(Lb{scan64}E)' + ('?' if scan64 else '') + r'EEvNS_7FitArgsE:')
    start = next(i for i, l in enumerate(lines) if sym.match(l))
    end = next(i for i in range(start, len(lines)) if lines[i].lstrip().startswith('s_endpgm'))
    return lines[start + 1:end + 1]


def blocks_of(body):
    blocks, cur = [], ['entry', []]
    for l in body:
        s = l.split(';')[0].strip()
        if not s or s.startswith('.') and not s.endswith(':'):
            continue
        if s.endswith(':'):
            blocks.append(cur)
            cur = [s[:-1], []]
        else:
            cur[1].append(s)
    blocks.append(cur)
    return blocks


def count(nbt, mode, lines, scan64=0):
    blocks = blocks_of(kernel_body(lines, nbt, mode, scan64))
    index = {name: i for i, (name, _) in enumerate(blocks)}
    in_loop = [False] * len(blocks)
    for i, (_, ins) in enumerate(blocks):
        for s in ins:
            m = re.match(r's_c?branch\S*\s+(\S+)', s)
            if m and m.group(1) in index and index[m.group(1)] <= i:
                for j in range(index[m.group(1)], i + 1):
                    in_loop[j] = True
    rows, total = [], None
    for i, (name, ins) in enumerate(blocks):
        if not in_loop[i]:
            continue
        if i == 0 or not in_loop[i - 1]:                      # a new outermost loop: its total over ALL its blocks, the short ones too
            total = Counter()
            rows.append((f'loop@{name.split("_")[-1]}', total))
        c = Counter()
        for s in ins:
            op = s.split()[0]
            c['all'] += 1
            if op.startswith('v_mfma'):
                c['mfma'] += 1
            elif op.startswith('v_'):
                c['valu'] += 1
                c['dpp'] += 'dpp' in op or ' row_' in s or 'quad_perm' in s
                c['swap'] += op.startswith('v_permlane')
                c['f64'] += op.endswith('_f64')
                c['mov0'] += bool(re.match(r'v_mov_b32(_e32)?\s+v\d+,\s*0$', s))
                c['cndmask'] += op.startswith('v_cndmask')
            elif op == 's_nop':
                c['nop'] += 1
            elif op.startswith('ds_'):
                c['lds'] += 1
            elif op == 's_barrier':
                c['bar'] += 1
        total.update(c)
        if len(ins) >= 20:
            rows.append((name, c))
    return rows


def main():
    lines = open(sys.argv[1]).read().split('\n')
    insts = [(tuple(map(int, a.split(','))) + (0,))[:3] for a in sys.argv[2:]] or [(10, 3, 0), (10, 0, 0)]
    cols = ['all', 'valu', 'mfma', 'nop', 'dpp', 'swap', 'f64', 'mov0', 'cndmask', 'lds', 'bar']
    for nbt, mode, scan64 in insts:
        print(f'k2b_fit_world_kernel<{nbt}, {mode}, {"true" if scan64 else "false"}>')
        print(f'  {"block":<12}' + ''.join(f'{c:>8}' for c in cols))
        for name, c in count(nbt, mode, lines, scan64):
            print(f'  {name:<12}' + ''.join(f'{c[k]:>8}' for k in cols))


if __name__ == '__main__':
    main()
