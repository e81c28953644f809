#!/usr/bin/env python3
"""Device code of two builds of one source file, kernel by kernel (no GPU): the gfx950 code object inside each object file
(`llvm-objdump --offloading`) is disassembled (`-d --no-show-raw-insn`), split per kernel symbol, addresses and branch-target annotations
stripped, one sha256 per symbol.  For every symbol whose digest differs the instruction count and the resources the code object's
metadata states (VGPR / AGPR / SGPR, scratch and LDS bytes) are printed for both builds.

    scripts/kernel_isa_diff.py LABEL PARENT.o TREE.o [LABEL PARENT.o TREE.o ...]"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')


def code_object(obj, tmp):
    d = tempfile.mkdtemp(dir=tmp)
    local = os.path.join(d, 'o.o')
    os.symlink(os.path.abspath(obj), local)
    subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', 'o.o'], cwd=d, check=True, capture_output=True)
    cos = [f for f in os.listdir(d) if 'gfx950' in f]
    assert len(cos) == 1, (obj, os.listdir(d))
    return os.path.join(d, cos[0])


def kernels(co):
    """{symbol: (sha256, instructions)} of every kernel, {symbol: resources} from the metadata note"""
    note = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], check=True, capture_output=True, text=True).stdout
    meta = {}
    for blk in re.split(r'\n\s*- \.agpr_count:', note)[1:]:
        blk = '.agpr_count:' + blk
        f = {k: v for k, v in re.findall(r'\.(agpr_count|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|name):\s*(\S+)', blk)}
        meta[f['name']] = f
    dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', co], check=True, capture_output=True, text=True).stdout
    out, name, body = {}, None, []

    def close():
        if name in meta:
            out[name] = (hashlib.sha256('\n'.join(body).encode()).hexdigest(), len(body))
    for line in dis.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            close()
            name, body = m.group(1), []
        elif name and line.strip():
            t = re.sub(r'\s*//.*$', '', line).strip()
            t = re.sub(r'<[^>]*>', '', t)                    # branch-target annotations
            if t:
                body.append(t)
    close()
    return out, meta


def main(argv):
    assert len(argv) % 3 == 0 and argv, __doc__
    with tempfile.TemporaryDirectory() as tmp:
        for label, po, to in zip(argv[0::3], argv[1::3], argv[2::3]):
            (pk, pm), (tk, tm) = kernels(code_object(po, tmp)), kernels(code_object(to, tmp))
            both = sorted(set(pk) & set(tk))
            diff = [s for s in both if pk[s][0] != tk[s][0]]
            print(f'{label}: symbols parent / tree / in both {len(pk)} / {len(tk)} / {len(both)}, differing digests {len(diff)}, '
                  f'only in parent {len(set(pk) - set(tk))}, only in tree {len(set(tk) - set(pk))}')
            for s in sorted(set(pk) ^ set(tk)):
                print(f'    only in {"parent" if s in pk else "tree"}: {s}')
            for s in diff:
                def row(k, m):
                    return (f'{k[s][1]:6d} insn  vgpr {m[s]["vgpr_count"]:>3} agpr {m[s]["agpr_count"]:>3} sgpr {m[s]["sgpr_count"]:>3} '
                            f'scratch {m[s]["private_segment_fixed_size"]:>4} lds {m[s]["group_segment_fixed_size"]:>6}')
                filt = shutil.which('llvm-cxxfilt', path=LLVM) or shutil.which('c++filt')
                demangled = subprocess.run([filt, s], capture_output=True, text=True).stdout.strip() if filt else s
                print(f'    {demangled}\n        parent {row(pk, pm)}\n        tree   {row(tk, tm)}')


if __name__ == '__main__':
    main(sys.argv[1:])
