#!/usr/bin/env python3
"""Write the gfx950 device assembly of every eve_amd/csrc/*.hip of a source tree into a directory.

    python tools/device_isa.py OUT_DIR [--tree REPO_ROOT]

A host-only change must leave the device code alone.  Run this on a checkout of the parent commit and on the branch and
compare the two directories (`diff -r A B`): the files are compiled with the product's flags (eve_amd/build.py: FLAGS) and
the lines that name `__hip_cuid_`, an identifier hipcc draws at random per compilation, are dropped.

hipcc emits template kernels in the order the host code first names them (each in a section of its own), so a host change that
launches the same kernels from other places reorders the file.  --by-kernel makes the comparison independent of that: comments
and the per-function index in block labels go, and the kernels, their descriptors and their metadata entries are sorted by text.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-inline-asm', '--cuda-device-only', '-S']


def by_kernel(text):
    """the same assembly with everything that depends on the emission order of the kernels normalised away"""
    text = re.sub(r'[ \t]*;.*', '', text)                                   # comments carry function indices and padding
    text = re.sub(r'\.LBB\d+_', '.LBB_', text)
    text = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', text)
    head, sep, meta = text.partition('\t.amdgpu_metadata')
    funcs = re.split(r'(?m)^(?=(?:\t\.section\t\.text\S*\n|\t\.text\n)\t\.protected\t)', head)
    last, mark, tail = funcs[-1].partition('\t.section\t.AMDGPU.gpr_maximums')     # what follows the last kernel belongs to the file
    entries = re.split(r'(?m)^(?=  - \.agpr_count)', meta)
    if len(entries) > 1:
        e_last, e_mark, e_tail = entries[-1].partition('amdhsa.target')
        entries = [entries[0]] + sorted(entries[1:-1] + [e_last]) + [e_mark + e_tail]
    return funcs[0] + ''.join(sorted(funcs[1:-1] + [last])) + mark + tail + sep + ''.join(entries)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('out_dir')
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--by-kernel', action='store_true', help='sort the kernels of each file and drop what only numbers them')
    ap.add_argument('--jobs', type=int, default=min(16, os.cpu_count() or 4))
    args = ap.parse_args()
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    os.makedirs(args.out_dir, exist_ok=True)
    sources = sorted(glob.glob(os.path.join(args.tree, 'eve_amd', 'csrc', '*.hip')))

    def one(src):
        r = subprocess.run([hipcc] + FLAGS + [src, '-o', '-'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            return src, r.stderr
        out = os.path.join(args.out_dir, os.path.basename(src)[:-len('.hip')] + '.s')
        text = ''.join(line for line in r.stdout.splitlines(True) if '__hip_cuid_' not in line)
        with open(out, 'w') as f:
            f.write(by_kernel(text) if args.by_kernel else text)
        return src, None

    failed = 0
    with ThreadPoolExecutor(max_workers=max(1, args.jobs)) as ex:
        for src, err in ex.map(one, sources):
            print(('FAILED ' if err else 'ok     ') + os.path.basename(src))
            if err:
                failed += 1
                sys.stderr.write(err)
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
