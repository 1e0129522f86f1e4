"""The device assembly of every kernel of some csrc/ files on another checkout (the parent commit) and on this tree, kernel by
kernel -> profiles/<tag>_isa_equality.txt.  No GPU needed.

    python tools/isa_equality.py PARENT_ROOT tag file.hip [file.hip ...] [--rename REGEX=REPL ...]

Each file is compiled on both sides with `hipcc --cuda-device-only -S` and the flags of that side's csrc/Makefile, the per-file ones
included.  A kernel's text is what stands between its label and its .Lfunc_end.  Symbols are demangled in it, the function's index
is taken out of its local labels and of the comments that name them (BB<n>_), and each --rename is applied to THIS tree's symbol
names, so that a kernel which was renamed, got a template argument or takes a renamed struct is matched to the parent's.  Kernels are matched by name over all the
given files together: one that moved to another file is still found.
"""
import hashlib
import os
import re
import subprocess
import sys

SUB = os.path.join('lfd-a-light-and-fast-detector_amd', 'csrc')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assembly(root, base):
    csrc = os.path.join(root, SUB)
    mk = open(os.path.join(csrc, 'Makefile')).read().replace('\\\n', ' ')
    flags = re.search(r'^FLAGS\s*=\s*(.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').replace('$(EXTRA)', '').split()
    per_file = re.search(r'^FLAGS_%s\s*=\s*(.*)$' % base, mk, re.M)
    cmd = ['/opt/rocm/bin/hipcc'] + flags + (per_file.group(1).split() if per_file else []) + \
          ['--cuda-device-only', '-S', os.path.join(csrc, base + '.hip'), '-o', '-']
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def kernels(text, renames):
    """{name as the parent spells it: (lines, sha256)} of one assembly file, in the file's order"""
    syms = sorted(set(re.findall(r'_Z\w+', text)), key=len, reverse=True)
    plain = subprocess.run(['c++filt'], input='\n'.join(syms), capture_output=True, text=True).stdout.split('\n')
    table = {}
    for s, d in zip(syms, plain):
        d = d.replace('(anonymous namespace)::', '')
        for rx, repl in renames:
            d = re.sub(rx, repl, d)
        table[s] = d
    out = {}
    for name in re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M):
        body = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:' % re.escape(name), text, re.M | re.S).group(1)
        body = re.sub(r'_Z\w+', lambda m: table[m.group(0)], body)
        body = re.sub(r'BB\d+_', 'BB_', body)
        out[table[name]] = (body.count('\n'), hashlib.sha256(body.encode()).hexdigest()[:16])
    return out


def main():
    args = sys.argv[1:]
    renames = []
    while '--rename' in args:
        i = args.index('--rename')
        rx, repl = args[i + 1].split('=', 1)
        renames.append((rx, repl))
        del args[i:i + 2]
    parent, tag, files = args[0], args[1], args[2:]
    old, new, where = {}, {}, {}
    for f in files:
        base = os.path.splitext(f)[0]
        if os.path.exists(os.path.join(parent, SUB, f)):
            for k, v in kernels(assembly(parent, base), []).items():
                old[k], where[k] = v, f
        for k, v in kernels(assembly(ROOT, base), renames).items():
            new[k] = v
            where.setdefault(k, f)
    lines = ['# every kernel of %s on the parent commit and on this tree: the device assembly (hipcc --cuda-device-only -S with the flags of'
             % ', '.join('csrc/' + f for f in files),
             '# csrc/Makefile incl. the per-file ones, the text between the kernel\'s label and its .Lfunc_end), symbols demangled, this tree\'s',
             '# names taken back to the parent\'s (tools/isa_equality.py; the renames: %s).' % ('; '.join('%s -> %s' % r for r in renames) or 'none'),
             '# Equal sha256 = the same instructions, registers, labels and LDS symbols, line for line.',
             '# file (the parent\'s) | kernel (the parent\'s name) | lines | sha256 parent (first 16) | sha256 this tree (first 16) | equal']
    differ = 0
    for k, (n, h) in old.items():
        n2, h2 = new.get(k, (0, '-' * 16))
        differ += h != h2
        lines.append('%-15s | %-50s | %5d | %s | %s | %s' % (where[k], k, n, h, h2, 'yes' if h == h2 else 'no'))
    only = [k for k in new if k not in old]
    if only:
        lines.append('# kernels only in this tree: ' + ', '.join(only))
    out = os.path.join(ROOT, 'profiles', '%s_isa_equality.txt' % tag)
    open(out, 'w').write('\n'.join(lines) + '\n')
    print(out, len(old), 'kernels,', differ, 'differ,', len(only), 'only in this tree')
    for l in lines[5:]:
        if l.endswith('| no') or l.startswith('# kernels only'):
            print(l)


if __name__ == '__main__':
    main()
