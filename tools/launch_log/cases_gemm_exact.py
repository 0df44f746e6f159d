"""Case list of the exact-sum GEMM tests (tests/gemm_exact_util.py) for tools/launch_log/run.py: the same cases, the same descriptor
builder and the same C entries as tests/test_gpu_gemm_exact.py, with fake operand addresses, followed by the fused linear + cross-entropy
entries at the smallest shape test_fused_linear_cross_entropy* value-tests (their epilogues are inexact by nature: no exact-sum case).

    python tools/launch_log/run.py --tree . --cases gemm_exact -o LOG

prints, per kernel instantiation of gemm.hip, how many launches the case list makes, and `never launched: none`."""
import ctypes as C
import os
import sys

from cases_gemm import SOURCE, STUBS, P, I, LL, F          # noqa: F401  (SOURCE and STUBS are read by run.py)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import gemm_exact_util as GX                                 # noqa: E402

CE_SHAPE = (300, 192, 64)                                    # (R, C, K)
A, ALO, B, BLO, TGT, RL, LOSS, DL, WS, H16, W16 = (0x30000000 + 0x01000000 * i for i in range(11))


def declare(L):
    L.amdnuwa_gemm_tn_workspace_bytes.restype = C.c_size_t
    L.amdnuwa_gemm_tn.argtypes = [P, P, C.c_size_t, P]
    L.amdnuwa_gemm_nt.argtypes = [P, P]
    L.amdnuwa_linear_ce_workspace_bytes.restype = C.c_size_t
    L.amdnuwa_linear_ce_workspace_bytes.argtypes = [LL, I]
    L.amdnuwa_linear_ce.argtypes = [P, I, P, I, P, LL, I, I, F, P, P, P, I, P, C.c_size_t, P]
    L.amdnuwa_linear_ce_x3.argtypes = [P, P, P, I, P, P, P, I, P, LL, I, I, F, P, P, P, I, P, C.c_size_t, P]


def ce_cases(L):
    R, Cc, K = CE_SHAPE
    nb = L.amdnuwa_linear_ce_workspace_bytes(R, Cc)
    yield f'linear_ce R{R} C{Cc} K{K}', {}, lambda: L.amdnuwa_linear_ce(A, K, B, K, TGT, R, Cc, K, 0.5, RL, LOSS, DL, Cc, WS, nb, None)
    for h16, w16 in ((None, None), (H16, W16)):
        yield (f'linear_ce_x3 R{R} C{Cc} K{K} fp16 copies {h16 is not None}', {},
               lambda h16=h16, w16=w16: L.amdnuwa_linear_ce_x3(A, ALO, h16, K, B, BLO, w16, K, TGT, R, Cc, K, 0.5, RL, LOSS, DL, Cc, WS, nb, None))


def cases(L):
    declare(L)
    for c in GX.all_cases():
        yield c['name'], c['keys'], (lambda c=c: GX.call(L, c, GX.FAKE))
    yield from ce_cases(L)
