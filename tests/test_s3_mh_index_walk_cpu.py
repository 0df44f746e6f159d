"""The gate in front of the first launch of the many-head Sparse3DNA kernels (csrc/sparse3dna_mh.hip): every index they form is walked on the
CPU.  The kernels form addresses with the inline functions of csrc/s3mh_index.h and nothing else; tools/s3mh_index_walk.cpp includes the same
header in a plain host compile and, for every case of tests/test_gpu_s3_mh.py (s3_mh_cases_util.all_cases), replays every workgroup, thread,
tap plane, tap and item, asserting that each index lies inside the extent the launcher allocates or the caller passes and that every output
element and every partial is written exactly once.  The program is built with the address and undefined-behaviour sanitizers (host
compiler, no device pass) and run as a child process: nothing is preloaded, nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

import s3_mh_cases_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cxx():
    for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++'):
        if c and shutil.which(c):
            return shutil.which(c)
    pytest.fail('no host C++ compiler found')


@pytest.fixture(scope='module')
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp('s3mh_walk')
    exe = str(d / 'walk')
    cxx = _cxx()
    # the sanitizer runtimes are linked INTO the program (clang's default; gcc needs the flags), so it runs whatever else the process loads
    is_clang = 'clang' in subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout
    static_rt = [] if is_clang else ['-static-libasan', '-static-libubsan']
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static_rt,
           '-I', os.path.join(ROOT, 'nuwa_pytorch_amd', 'csrc'), os.path.join(ROOT, 'tools', 's3mh_index_walk.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f'{" ".join(cmd)}\n{r.stdout}\n{r.stderr}'
    return exe, d


def _run(walk, lines):
    exe, d = walk
    path = str(d / 'cases.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return subprocess.run([exe, path], capture_output=True, text=True)


def test_every_index_of_every_gpu_case_stays_inside_its_extent(walk):
    cases = M.all_cases()
    r = _run(walk, [M.walk_line(c) for c in cases])
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r'cases walked: (\d+), indices checked: (\d+)', r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == len(cases) and int(m.group(2)) > 1_000_000


def test_the_walk_covers_all_instantiations_and_the_shape_that_faulted():
    cases = M.all_cases()
    assert {(c['dim_head'], c['form']) for c in cases} == {(d, f) for d in (32, 64) for f in M.FORMS}
    g222 = [c for c in cases if c['grid'] == (2, 2, 2) and c['heads'] == 16]
    assert {(c['dim_head'], c['form']) for c in g222} == {(d, f) for d in (32, 64) for f in M.FORMS}
    assert {M.threads(c) for c in cases} >= {64, 128, 512}
    assert any(M.tile(c)[1] > 1 and c['grid'][2] % M.tile(c)[0] for c in cases)       # a partial last tile


def test_the_walk_refuses_an_index_outside_its_extent(walk):
    """the checks bite: a geometry outside the envelope of the entry points (17 heads: the padded talking-heads matrix is 16 x 16) fails"""
    c = dict(M.all_cases()[0], heads=17)
    r = _run(walk, [M.walk_line(c)])
    assert r.returncode != 0 and 'FAILED' in r.stderr
