#!/usr/bin/env python3
"""Compare two hipcc -S device listings kernel by kernel (listings made as the docstring of isa_count.py says).

    python tools/isa_diff.py before.s after.s

Three verdicts per kernel (the two listings must hold the same set of demangled kernel names):
  identical  the same instruction text (comments and directives stripped, labels renumbered in order of appearance within the kernel,
             because their numbers move with the order of instantiation) and the same VGPR / SGPR count, accum offset, scratch, LDS
             and kernarg size;
  reordered  the same metadata and the same count per opcode (the first token of each instruction; a label counts as one opcode):
             only register names and the order of instructions moved -- what moving a stage into an inlined helper does;
  differs    anything else: the line names the metadata that moved and the opcodes whose counts differ.
Prints one line per kernel that is not identical and the three counts; exit status 1 if a kernel differs or exists on one side only.
"""
import collections
import re
import subprocess
import sys

META = ('.amdhsa_next_free_vgpr', '.amdhsa_next_free_sgpr', '.amdhsa_accum_offset', '.amdhsa_private_segment_fixed_size',
        '.amdhsa_group_segment_fixed_size', '.amdhsa_kernarg_size')
LABEL = re.compile(r'\.L[A-Za-z_]*\d+(?:_\d+)?')


def instructions(text):
    names = {}
    out = []
    for line in text.split('\n')[2:]:          # [0] is empty, [1] the symbol's own label
        t = line.split(';')[0].strip()
        if not t or (t.startswith('.') and not t.endswith(':')):
            continue
        out.append(LABEL.sub(lambda m: names.setdefault(m.group(0), '.L%d' % len(names)), t))
    return out


def kernels(path):
    """{demangled name: (instructions, metadata)} of every kernel of the listing"""
    s = open(path).read()
    blocks = re.findall(r'^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel', s, re.M | re.S)
    demangled = subprocess.run(['c++filt'], input='\n'.join(n for n, _ in blocks), capture_output=True, text=True).stdout.split('\n')
    out = {}
    for (n, body), dn in zip(blocks, demangled):
        a = s.index('\n' + n + ':')
        meta = {k: v for k, v in re.findall(r'^\s*(\.amdhsa_\S+)\s+(\S+)', body, re.M) if k in META}
        out[dn] = (instructions(s[a:s.index('.Lfunc_end', a)]), meta)
    return out


def opcodes(ins):
    return collections.Counter('label:' if i.endswith(':') else i.split()[0] for i in ins)


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for n in sorted(set(a) ^ set(b)):
        bad += 1
        print(('only in %s: ' % sys.argv[1 if n in a else 2]) + n)
    same = reordered = 0
    for n in sorted(set(a) & set(b)):
        if a[n] == b[n]:
            same += 1
            continue
        (ia, ma), (ib, mb) = a[n], b[n]
        ca, cb = opcodes(ia), opcodes(ib)
        if ma == mb and ca == cb:
            reordered += 1
            print('reordered: %s' % n)
            continue
        bad += 1
        what = [k + ' %s -> %s' % (ma.get(k), mb.get(k)) for k in META if ma.get(k) != mb.get(k)]
        if ca != cb:
            what.append('instructions %d -> %d: ' % (len(ia), len(ib)) + ', '.join('%s %d -> %d' % (o, ca[o], cb[o]) for o in sorted(set(ca) | set(cb)) if ca[o] != cb[o]))
        print('differs: %s: %s' % (n, '; '.join(what)))
    print('%d kernels compared, %d identical, %d reordered, %d other' % (len(set(a) | set(b)), same, reordered, bad))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
