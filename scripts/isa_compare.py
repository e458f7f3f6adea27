#!/usr/bin/env python3
"""Compare what two source trees compile to, kernel by kernel (host only: hipcc cross-compiles, no GPU is touched).

    python scripts/isa_compare.py OLD_TREE NEW_TREE stem.hip conv3x3_direct.hip ... [-o table.txt]

Each file of rmem_ocu_amd/csrc is compiled for gfx950 to assembly with the Makefile's FLAGS of its own tree plus
--cuda-device-only -S, once plain (bf16) and once with -DRMEM_F16.  Per kernel symbol the table gives the four resource numbers of
the code object's metadata (.vgpr_count, .sgpr_count, .group_segment_fixed_size = LDS, .private_segment_fixed_size = scratch), old
and new, and whether two things are equal:
  hist   the sorted histogram of instruction mnemonics;
  skel   the memory/sync skeleton: the subsequence of lines that are vector-memory instructions (buffer_ / global_ / flat_ /
         scratch_ prefixes), s_waitcnt or s_barrier, register numbers stripped.  The counted vmcnt waits of the strip kernels count
         requests in issue order, so they hold exactly as long as this sequence does.
Where the histogram differs the differing mnemonics are listed with their counts, and whether the MFMA and LDS (ds_) counts hold.
This is a diff of whatever mnemonics come; it looks for no particular instruction.  Exit status 1 if any kernel differs in
resources, skeleton or histogram, or has scratch."""
import argparse
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

KEYS = ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')


def makefile_flags(tree):
    text = open(os.path.join(tree, 'rmem_ocu_amd', 'csrc', 'Makefile')).read()
    flags = re.search(r'^FLAGS\s*=\s*(.*)$', text, re.M).group(1)
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', text, re.M).group(1)
    hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC\s*\?=\s*(\S+)', text, re.M).group(1)
    return hipcc, flags.replace('$(ARCH)', arch).split()


def assembly(tree, name, f16, tmp):
    hipcc, flags = makefile_flags(tree)
    out = os.path.join(tmp, '%s_%d.s' % (re.sub(r'\W', '_', os.path.abspath(tree) + name), f16))
    cmd = [hipcc] + flags + (['-DRMEM_F16'] if f16 else []) + ['--cuda-device-only', '-S', '-Wno-unused-command-line-argument',os.path.join(tree, 'rmem_ocu_amd', 'csrc', name), '-o', out]
    subprocess.run(cmd, check=True)
    return open(out).read()


def kernels(asm):
    """{symbol: (resources, mnemonic histogram, memory/sync skeleton)} of one assembly file"""
    meta = {}
    for block in re.split(r'^  - ', asm.split('amdhsa.kernels:')[1].split('amdhsa.target:')[0], flags=re.M)[1:]:
        sym = re.search(r'^\s+\.name:\s+(\S+)', block, re.M).group(1)
        meta[sym] = tuple(int(re.search(r'^\s+%s:\s+(\d+)' % re.escape(k), block, re.M).group(1)) for k in KEYS)
    found = {}
    for sym, res in meta.items():
        body = asm.split('\n%s:' % sym, 1)[1].split('s_endpgm', 1)[0]
        hist, skel = collections.Counter(), []
        for line in body.split('\n'):
            line = line.split(';')[0].strip()
            if not line or line.startswith('.') or line.endswith(':'):
                continue
            mnemonic = line.split()[0]
            hist[mnemonic] += 1
            if mnemonic.startswith(('buffer_', 'global_', 'flat_', 'scratch_')) or mnemonic in ('s_waitcnt', 's_barrier'):
                skel.append(re.sub(r'\b([vsa])\[?\d+(:\d+)?\]?', r'\1', line))
        found[sym] = (res, hist, skel)
    return found


def short(sym):
    """k_name<template arguments> of a mangled kernel symbol"""
    try:
        name = subprocess.run(['c++filt', sym], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        name = sym
    if name == sym:                             # (a parameter type c++filt does not know, such as _Float16)
        found = re.search(r'\d+(k_[a-z0-9_]+)', sym)
        return found.group(1) if found else sym
    return re.sub(r'^void ', '', name.replace('(anonymous namespace)::', '').split('(')[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('files', nargs='+')
    ap.add_argument('-o', '--out')
    ap.add_argument('--skeleton-lines', type=int, default=12, help='lines of a differing skeleton\'s diff to print')
    args = ap.parse_args()
    lines = ['%-46s %-4s %-13s %-9s %-15s %-8s %-5s %-5s' % ('kernel', 'type', 'vgpr old/new', 'sgpr', 'lds', 'scratch', 'hist', 'skel')]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.files:
            for f16 in (0, 1):
                old, new = kernels(assembly(args.old, name, f16, tmp)), kernels(assembly(args.new, name, f16, tmp))
                for sym in sorted(set(old) | set(new)):
                    label = '%s:%s' % (name.replace('.hip', ''), short(sym))
                    if sym not in old or sym not in new:
                        lines.append('%-46s %-4s only in the %s tree' % (label, 'f16' if f16 else 'bf16', 'old' if sym in old else 'new'))
                        bad += 1
                        continue
                    (ro, ho, so), (rn, hn, sn) = old[sym], new[sym]
                    lines.append('%-46s %-4s %-13s %-9s %-15s %-8s %-5s %-5s' % (
                        label, 'f16' if f16 else 'bf16', *('%d/%d' % (a, b) for a, b in zip(ro, rn)),
                        'same' if ho == hn else 'DIFF', 'same' if so == sn else 'DIFF'))
                    bad += ro != rn or rn[3] != 0 or ho != hn or so != sn
                    if ho != hn:
                        diff = ', '.join('%s %d/%d' % (m, ho[m], hn[m]) for m in sorted(set(ho) | set(hn)) if ho[m] != hn[m])
                        count = lambda h, pre: sum(n for m, n in h.items() if m.startswith(pre))
                        keep = all(count(ho, pre) == count(hn, pre) for pre in ('v_mfma', 'ds_'))
                        lines.append('    histogram: %s; MFMA and LDS counts %s' % (diff, 'equal' if keep else 'DIFFER'))
                    if so != sn:
                        diff = [d for d in difflib.unified_diff(so, sn, 'old', 'new', n=0, lineterm='') if not d.startswith(('---', '+++'))]
                        lines.extend('    skeleton: ' + d for d in diff[:args.skeleton_lines])
                        if len(diff) > args.skeleton_lines:
                            lines.append('    skeleton: ... %d more lines' % (len(diff) - args.skeleton_lines))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        open(args.out, 'w').write(text)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
