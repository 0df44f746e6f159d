"""Host-side launch log of one HIP source of libamdnuwa, on a machine without a GPU.

    python tools/launch_log/run.py --tree DIR --cases gemm -o LOG [--replace OLD NEW]

Compiles nuwa_pytorch_amd/csrc/<source of the case list> of the tree DIR with `-include launch_log.h` (host pass only: no device code is
needed, nothing is launched) into a scratch library under --scratch, outside the package, then walks the case list of cases_<name>.py through
ctypes with fixed fake operand pointers.  Per case the log holds the tuning keys, the call, its return code and what launch_log.h recorded:
attribute calls, launches (kernel symbol, grid, block, dynamic-LDS bytes, hash of the argument bytes) in order.  Two trees launch the same
if their logs are byte-identical; the summary on stdout carries the sha256 of the log, the counts, and the kernels never reached.

--replace OLD NEW edits the scratch copy of the source first (e.g. to value-initialise an argument block the tree leaves partly unset, so
that its log is deterministic).  Nothing is preloaded; not part of the suite or of build.py."""
import argparse
import ctypes
import hashlib
import importlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def build(tree, source, stubs, scratch, replace):
    os.makedirs(scratch, exist_ok=True)
    csrc = os.path.join(tree, 'nuwa_pytorch_amd', 'csrc')
    text = open(os.path.join(csrc, source)).read()
    for old, new in replace:
        assert old in text, f'--replace: {old!r} does not occur in {source}'
        text = text.replace(old, new)
    src = os.path.join(scratch, 'unit_' + source)
    open(src, 'w').write(text)
    stub = os.path.join(scratch, 'stubs.hip')
    open(stub, 'w').write(stubs)
    lib = os.path.join(scratch, 'liblaunchlog.so')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    # (the device pass cannot be left out: the host object refers to the embedded code object, which the runtime registers but never loads here)
    cmd = [hipcc, '--offload-arch=gfx950', '-O1', '-g0', '-std=c++17', '-fPIC', '-shared', '-I', csrc, '-I', HERE,
           '-include', os.path.join(HERE, 'launch_log.h'), src, stub, '-o', lib, '-ldl']
    subprocess.run(cmd, check=True)
    return lib


def symbols(lib):
    """offset -> kernel name, from the library's own symbol table (the kernels have internal linkage: no dynamic symbol)"""
    out = subprocess.run(['nm', '-C', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
    names = {}
    for line in out.splitlines():
        m = re.match(r'([0-9a-f]+) \w (.*)', line)
        if not m:
            continue
        name = m.group(2).replace('(anonymous namespace)::', '')
        off = int(m.group(1), 16)
        if '__device_stub__' in name:
            names.setdefault(off, name.replace('__device_stub__', ''))
        else:
            names[off] = name
    kernels = {n.replace('__device_stub__', '') for n in (l.split(' ', 2)[2].replace('(anonymous namespace)::', '') for l in out.splitlines() if '__device_stub__' in l)}
    return names, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', required=True)
    ap.add_argument('--cases', required=True, help='case list module: cases_<name>.py next to this file')
    ap.add_argument('--scratch', default='/tmp/launch_log')
    ap.add_argument('--replace', nargs=2, action='append', default=[], metavar=('OLD', 'NEW'))
    ap.add_argument('-o', '--out', required=True)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    cases = importlib.import_module('cases_' + a.cases)
    lib_path = build(os.path.abspath(a.tree), cases.SOURCE, cases.STUBS, a.scratch, a.replace)
    names, kernels = symbols(lib_path)
    L = ctypes.CDLL(lib_path)
    L.launch_log_take.restype = ctypes.c_size_t
    L.launch_log_take.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    tuning = (ctypes.c_int * 32).in_dll(L, 'g_amdnuwa_tuning')
    buf = ctypes.create_string_buffer(1 << 16)
    seen, n_calls, n_launch, n_attr, by_rc = {}, 0, 0, 0, {}
    sha = hashlib.sha256()

    def resolve(m):
        return names.get(int(m.group(1), 16), m.group(0))

    with open(a.out, 'w') as f:
        for name, keys, call in cases.cases(L):
            for k in range(32):
                tuning[k] = keys.get(k, 0)
            rc = call()
            n = L.launch_log_take(buf, len(buf))
            assert n < len(buf)
            body = re.sub(r'\+0x([0-9a-f]+)', resolve, buf.value.decode())
            for line in body.splitlines():
                w = line.split(' ')
                if w[0] == 'launch':
                    n_launch += 1
                    kn = line[len('launch '):line.index(' grid ')]
                    seen[kn] = seen.get(kn, 0) + 1
                elif w[0] == 'attr':
                    n_attr += 1
            n_calls += 1
            by_rc[rc] = by_rc.get(rc, 0) + 1
            text = f'case {name} keys {sorted(keys.items())}\nrc {rc}\n{body}'
            sha.update(text.encode())
            f.write(text)
    for k in range(32):
        tuning[k] = 0
    print(f'{n_calls} calls, {n_launch} launches, {n_attr} attribute calls; return codes {sorted(by_rc.items())}')
    print(f'sha256 of the log: {sha.hexdigest()}')
    print(f'{len(kernels)} kernel instantiations in {cases.SOURCE}, {len(seen)} launched:')
    for kn in sorted(kernels | set(seen)):
        print(f'  {seen.get(kn, 0):7d}  {kn}' + ('' if kn in kernels else '   (not a kernel of this file?)'))
    never = sorted(kernels - set(seen))
    print('never launched: ' + (', '.join(never) if never else 'none'))


if __name__ == '__main__':
    main()
