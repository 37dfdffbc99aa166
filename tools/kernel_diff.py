#!/usr/bin/env python3
"""Compare two `hipcc -S --cuda-device-only` listings of one source file kernel by kernel:  python tools/kernel_diff.py old.s new.s
  identical   the kernel's instructions (comments, .file / .ident and the per-file __hip_cuid symbol stripped) are the same text;
  reordered   same resource line (kernel_regs.py), same count of every opcode, same main-loop string (isa_seq.py) once the VALU
              entries are dropped: instructions moved or registers renamed, nothing added;
  DIFFERENT   anything else; the opcodes whose counts changed are listed.
Exit status 1 if any kernel is DIFFERENT or missing."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_seq import loop_string    # noqa: E402
from kernel_regs import kernels    # noqa: E402


def body(lines, name):
    start = lines.index(name + ':')
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    return lines[start:end]


def clean(path):
    txt = open(path).read()
    lines = []
    for l in txt.split('\n'):
        l = l.split(';')[0].rstrip()
        if l and not re.match(r'\s*\.(file|ident)\b', l) and '__hip_cuid' not in l:
            lines.append(l)
    return txt, lines


def main(old, new):
    (otxt, olines), (ntxt, nlines) = clean(old), clean(new)
    ores = {name: (label, res) for label, name, res in kernels(otxt)}
    bad = 0
    new_kernels = list(kernels(ntxt))
    for label, name, res in new_kernels:
        if name not in ores:
            print('%-44s NEW        %s' % (label, res))
            bad = 1
            continue
        ob, nb = body(olines, name), body(nlines, name)
        if ob == nb and ores[name][1] == res:
            level = 'identical'
        else:
            oh = collections.Counter(l.split()[0] for l in ob[1:] if not l.endswith(':'))
            nh = collections.Counter(l.split()[0] for l in nb[1:] if not l.endswith(':'))
            oseq, nseq = (loop_string(x, name).replace('.', '') for x in (olines, nlines))
            level = 'reordered' if (oh == nh and ores[name][1] == res and oseq == nseq) else 'DIFFERENT'
        print('%-44s %-10s %s' % (label, level, res))
        if level == 'DIFFERENT':
            bad = 1
            if ores[name][1] != res:
                print('    was: %s' % ores[name][1])
            for op in sorted(set(oh) | set(nh)):
                if oh[op] != nh[op]:
                    print('    %-28s %d -> %d' % (op, oh[op], nh[op]))
            if oh == nh and oseq != nseq:
                print('    main loop order (non-VALU) changed')
    for name in set(ores) - {n for _, n, _ in new_kernels}:
        print('%-44s MISSING' % ores[name][0])
        bad = 1
    return bad


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
