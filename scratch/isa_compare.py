#!/usr/bin/env python3
"""Do two trees compile to the same gfx950 device code?  Per kernel, for every .hip of bert4clickpath_amd/csrc/.

    python scratch/isa_compare.py REV            # git revision REV against the working tree
    python scratch/isa_compare.py A B            # A, B: each a git revision or the root of a checkout
    options: --files gemm attn_mq ...   --jobs N   --keep DIR (leave the .s files there)

Every file is compiled device-only to assembly with the CXXFLAGS of its own tree's csrc/Makefile (read the way
tests/test_vmcnt_accounting.py reads them).  The assembly is cut per kernel, from the kernel's label to the `.end_amdhsa_kernel`
of its descriptor (so code, register counts and LDS size all count), the per-translation-unit `__hip_cuid_<hash>` name is
normalised, and the texts are compared.  Prints one line per file: kernels identical / total, and the names of the rest.
Exit status 0 iff every kernel of every file is identical and both sides hold the same kernels.

What is compared is the code, not the order in which the compiler emitted it.  A kernel template that is instantiated from
inside a lambda (the launch dispatchers of csrc/common.h) leaves the compiler at another place in the file than one instantiated
from a macro ladder, and local labels carry the number of the function they lie in: `.LBB14_2` for `.LBB0_2`, `.Lfunc_end14`, and
the same names again inside the `; %bb`, loop and register-count comments, whose padding moves with their width.  So per kernel
the comments are dropped, runs of blanks become one, and the local labels (`.L...`) are renumbered in the order in which the
kernel first names them -- two kernels still have to branch to the same places.  Every instruction, directive and descriptor
field (`.amdhsa_next_free_vgpr`, `.amdhsa_group_segment_fixed_size`, ...) is compared as before.
"""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

CSRC = os.path.join('bert4clickpath_amd', 'csrc')


def hipcc():
    for p in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if p and os.path.isfile(p) and os.access(p, os.X_OK):
            return p
    sys.exit('hipcc not found')


def makefile_cxxflags(csrc):
    text = open(os.path.join(csrc, 'Makefile')).read()
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', text, re.M).group(1)
    flags = re.search(r'^CXXFLAGS\s*=\s*(.*)$', text, re.M).group(1)
    flags = flags.replace('$(ARCH)', arch).replace('$(EXTRA)', '')
    assert '$(' not in flags, flags
    return flags.split()


def tree_of(spec, tmp, tag):
    """spec: a directory (the root of a checkout) or a git revision of the repository this script lies in."""
    if os.path.isdir(os.path.join(spec, CSRC)):
        return os.path.abspath(spec)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    root = os.path.join(tmp, 'tree_' + tag)
    os.makedirs(root)
    ar = subprocess.run(['git', '-C', repo, 'archive', spec, CSRC, 'include'], stdout=subprocess.PIPE, check=True)
    subprocess.run(['tar', '-x', '-C', root], input=ar.stdout, check=True)
    return root


def compile_one(cc, flags, csrc, name, out):
    p = subprocess.run([cc] + flags + ['--cuda-device-only', '-S', os.path.join(csrc, name + '.hip'), '-o', out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=csrc)
    if p.returncode != 0:
        sys.exit(f'{csrc}/{name}.hip failed to compile:\n{p.stdout.decode(errors="replace")}')
    return out


_CUID = re.compile(r'__hip_cuid_[0-9a-f]+')
_LABEL = re.compile(r'^([A-Za-z_$][\w$]*):')       # `name:   ; @name`; local labels begin with a dot


_LOCAL = re.compile(r'\.L[\w$.]+')


def normalise(lines):
    """one kernel's lines without comments, blank runs and emission-order label numbers (module docstring)"""
    seen = {}
    out = []
    for l in lines:
        if '"' not in l:                            # (a `;` inside a string is no comment; such lines are kept whole)
            l = l.split(';', 1)[0]
        l = ' '.join(l.split())
        if l:
            out.append(_LOCAL.sub(lambda m: seen.setdefault(m.group(0), '.L%d' % len(seen)), l))
    return '\n'.join(out)


def kernels(path):
    """-> {kernel name: its normalised text, label .. .end_amdhsa_kernel}"""
    lines = [_CUID.sub('__hip_cuid_X', l.rstrip()) for l in open(path, errors='replace')]
    label = {}
    for i, l in enumerate(lines):
        m = _LABEL.match(l)
        if m:
            label.setdefault(m.group(1), i)
    res = {}
    for i, l in enumerate(lines):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == '.end_amdhsa_kernel')
            res[m.group(1)] = normalise(lines[label[m.group(1)]:end + 1])
    return res


def demangle(names):
    if not names or not shutil.which('c++filt'):
        return names
    out = subprocess.run(['c++filt'] + names, stdout=subprocess.PIPE).stdout.decode().splitlines()
    return out if len(out) == len(names) else names


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a')
    ap.add_argument('b', nargs='?', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--files', nargs='*')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--keep')
    args = ap.parse_args()

    cc = hipcc()
    tmp = args.keep or tempfile.mkdtemp(prefix='isa_compare_')
    os.makedirs(tmp, exist_ok=True)
    try:
        roots = [tree_of(args.a, tmp, 'a'), tree_of(args.b, tmp, 'b')]
        names = [sorted(f[:-4] for f in os.listdir(os.path.join(r, CSRC)) if f.endswith('.hip')) for r in roots]
        files = args.files or sorted(set(names[0]) | set(names[1]))
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            for side, r in enumerate(roots):
                csrc = os.path.join(r, CSRC)
                flags = makefile_cxxflags(csrc)
                os.makedirs(os.path.join(tmp, 'ab'[side]), exist_ok=True)
                for f in files:
                    if f in names[side]:
                        jobs[side, f] = pool.submit(compile_one, cc, flags, csrc, f, os.path.join(tmp, 'ab'[side], f + '.s'))
        print(f'a = {args.a}\nb = {args.b}\n')
        print(f'{"file":<16} {"kernels":>7} {"identical":>9}  differing')
        bad = total = same_total = 0
        for f in files:
            if (0, f) not in jobs or (1, f) not in jobs:
                print(f'{f + ".hip":<16} only in {"a" if (0, f) in jobs else "b"}')
                bad += 1
                continue
            ka, kb = kernels(jobs[0, f].result()), kernels(jobs[1, f].result())
            diff = sorted(k for k in set(ka) | set(kb) if ka.get(k) != kb.get(k))
            n = len(set(ka) | set(kb))
            total += n
            same_total += n - len(diff)
            bad += len(diff)
            print(f'{f + ".hip":<16} {n:>7} {n - len(diff):>9}  {"-" if not diff else ""}')
            for k, d in zip(diff, demangle(diff)):
                where = 'differs' if k in ka and k in kb else ('only in a' if k in ka else 'only in b')
                print(f'    {where}: {d}')
        print(f'{"total":<16} {total:>7} {same_total:>9}')
        return 1 if bad else 0
    finally:
        if not args.keep:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
