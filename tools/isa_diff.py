#!/usr/bin/env python3
"""Compare two hipcc -S device listings kernel by kernel (listings made as the docstring of isa_count.py says).

    python tools/isa_diff.py before.s after.s

Equal means: the same set of demangled kernel names; per kernel the same instruction text (comments and directives stripped, labels
renumbered in order of appearance within the kernel, because their numbers move with the order of instantiation) and the same
VGPR / SGPR count, scratch, LDS and kernarg size.  Prints one line per difference and a count; exit status 1 if anything differs.
"""
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


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for n in sorted(set(a) ^ set(b)):
        bad += 1
        print(('only in %s: ' % sys.argv[1 if n in a else 2]) + n)
    same = 0
    for n in sorted(set(a) & set(b)):
        if a[n] == b[n]:
            same += 1
            continue
        bad += 1
        (ia, ma), (ib, mb) = a[n], b[n]
        what = [k + ' %s -> %s' % (ma.get(k), mb.get(k)) for k in META if ma.get(k) != mb.get(k)]
        if ia != ib:
            first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            what.append('instructions %d -> %d, first difference at %d' % (len(ia), len(ib), first))
        print('differs: %s: %s' % (n, '; '.join(what)))
    print('%d kernels compared, %d identical' % (len(set(a) | set(b)), same))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
