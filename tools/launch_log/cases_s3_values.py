"""Case list of the Sparse3DNA / SparseCross2DNA value tests (tests/s3_cases_util.py) for tools/launch_log/run.py: the same cases and the
same calls (s3_cases_util.call_shape) as tests/test_gpu_s3_every_kernel.py, with fake operand addresses.  sparse3dna_wide.hip is compiled
into the same unit, so the log covers the column-tiled kernels too; the column sums of elementwise.hip are stubs.

    python tools/launch_log/run.py --tree . --cases s3_values -o LOG

prints, per kernel instantiation of the two files, how many launches the case list makes, and `never launched: none`."""
import os
import sys

SOURCE = 'sparse3dna.hip'

STUBS = r'''
#include "launch_log.h"
int g_amdnuwa_tuning[32];
extern "C" size_t amdnuwa_colsum_workspace_bytes(long long R, int D) { return (size_t)(R < 256 ? (R < 1 ? 1 : R) : 256) * D * sizeof(float); }
extern "C" int amdnuwa_colsum(const float* x, float* out, long long R, int D, int accumulate, void* workspace, size_t workspace_bytes, hipStream_t) {
    char buf[128];
    snprintf(buf, sizeof buf, "extern amdnuwa_colsum R %lld D %d accumulate %d\n", R, D, accumulate);
    launch_log::lines() += buf;
    return 0;
}
#include "sparse3dna_wide.hip"
'''

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import s3_cases_util as SC                                   # noqa: E402


def cases(L):
    """one item per (case, entry point): the launch log is taken after every call"""
    SC.declare(L)
    for c in SC.all_cases():
        for entry in c['entries']:
            yield f"{c['name']} :: {entry}", c['keys'], (lambda c=c, entry=entry: SC.call_fake(L, c, entry))
