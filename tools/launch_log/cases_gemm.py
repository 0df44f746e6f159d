"""Case list of the GEMM entry points (gemm.hip) for tools/launch_log/run.py: amdnuwa_gemm_nt in every descriptor form the wrappers of
kernels.py build, amdnuwa_gemm_tn, amdnuwa_linear_ce / _x3, over the products of the training step, the shapes on both sides of the route
thresholds and the tuning keys that steer a route."""
import ctypes as C

SOURCE = 'gemm.hip'

# what gemm.hip needs from the rest of the library: the tuning table and the stand-alone gate kernels of elementwise.hip (logged as calls)
STUBS = r'''
#include "launch_log.h"
int g_amdnuwa_tuning[32];
static int gate(const char* name, long long R, int FP, int lo_in, int lo_out) {
    char buf[128];
    snprintf(buf, sizeof buf, "extern %s R %lld FP %d lo %d %d\n", name, R, FP, lo_in, lo_out);
    launch_log::lines() += buf;
    return 0;
}
extern "C" int amdnuwa_geglu_il_fwd(const uint16_t* u_hi, const uint16_t* u_lo, uint16_t* o_hi, uint16_t* o_lo, long long R, int FP, hipStream_t) {
    return gate("amdnuwa_geglu_il_fwd", R, FP, u_lo != nullptr, o_lo != nullptr);
}
extern "C" int amdnuwa_geglu_il_bwd(const uint16_t* u_hi, const uint16_t* u_lo, const uint16_t* d_hi, const uint16_t* d_lo, uint16_t* du_hi,
                                    uint16_t* du_lo, long long R, int FP, hipStream_t) {
    return gate("amdnuwa_geglu_il_bwd", R, FP, (u_lo != nullptr) + 2 * (d_lo != nullptr), du_lo != nullptr);
}
'''

P, I, LL, F = C.c_void_p, C.c_int, C.c_longlong, C.c_float


class GemmDesc(C.Structure):                # amdnuwa_gemm_desc of include/amdnuwa.h (ABI 21)
    _fields_ = [('A', P), ('Alo', P), ('strideA', LL), ('lda', I), ('B', P), ('Blo', P), ('strideB', LL), ('ldb', I),
                ('C', P), ('Clo', P), ('strideC', LL), ('ldc', I), ('c_is_bf16', I), ('bias', P), ('alpha', F), ('beta', F),
                ('M', I), ('N', I), ('K', I), ('batch', I), ('shift_ntok', I), ('shift_fmap', I),
                ('batch_inner', I), ('strideA_inner', LL), ('strideB_inner', LL), ('strideC_inner', LL),
                ('C2', P), ('C2lo', P), ('ldc2', I), ('geglu_u', P), ('geglu_u_lo', P), ('ld_u', I), ('c_lo_f16', I), ('ab_f16', I), ('c_f16', I),
                ('alpha_dev', P), ('a_chunk32', I)]


# fake operand addresses: fixed, distinct, 16-byte aligned, never dereferenced
A, ALO, B, BLO, CC, CLO, C2, C2LO, U, ULO, BIAS, WS, ADEV, TGT, RL, LOSS, H16, W16 = (0x10000000 + 0x01000000 * i for i in range(18))

STEP = [(2560 * b, n, k) for b in (1, 128) for n in (1536, 2752, 512, 8192) for k in (512, 1376, 1536, 2752)]
EDGE = ([(m, 512, 512) for m in (32, 33, 128, 129, 384, 385)] + [(256 * 511, 256, 512), (256 * 512, 256, 512), (256 * 511 + 1, 250, 512)] +
        [(m, 512, k) for m in (2560, 327680) for k in (64, 96, 1024, 1056, 2040, 2047, 2048, 36896)] + [(8, 512, 36896), (20, 4096, 512)])
SHORT = [s for s in STEP if s[0] > 2560 and s[1] in (512, 2752)] + EDGE          # the shape list of the non-default key settings

NT_KEYS = ([{}] + [{0: v} for v in (1, 2, 5, 6, 7, 10, 11, 12)] + [{13: 1}, {0: 7, 13: 1}, {20: 1}, {20: 2}, {22: 1}, {22: 2}, {0: 7, 22: 2},
           {14: 3}, {0: 11, 14: 3}, {0: 12, 14: 3}, {7: 1}, {7: 2}, {0: 7, 7: 2}])
TN_KEYS = [{}] + [{6: v} for v in (1, 2, 3, 5)] + [{23: 1}, {25: 1}, {25: 2}, {25: 3}, {1: 512}, {2: 64}, {1: 96, 2: 1024}, {8: 2}, {6: 3, 8: 2}, {6: 2, 25: 1}]


def nt_forms(M, N, K):
    """(name, descriptor fields) of every form the NT wrappers of kernels.py build"""
    out = []
    for x3 in (0, 1):
        ops = dict(Alo=ALO, Blo=BLO) if x3 else {}
        for shift in (0, 1):
            sh = dict(shift_ntok=1 + 16 * 16, shift_fmap=16) if shift else {}
            for bname, bt in (('', {}), (' batch4', dict(batch=4, strideA=M * K, strideB=N * K, strideC=M * N)),
                              (' inner2', dict(batch=4, batch_inner=2, strideA=2 * M * K, strideB=2 * N * K, strideC=2 * M * N,
                                               strideA_inner=M * K, strideB_inner=N * K, strideC_inner=M * N))):
                tag = f"{'hi+lo' if x3 else 'bf16'}{' shift' if shift else ''}{bname}"
                base = {**ops, **sh, **bt}
                out.append((f'nt {tag} -> fp32', base))
                out.append((f'nt {tag} -> fp32 + bias', {**base, 'bias': BIAS}))
                out.append((f'nt {tag} -> bf16', {**base, 'c_is_bf16': 1}))
                out.append((f'nt {tag} -> bf16 + bias', {**base, 'c_is_bf16': 1, 'bias': BIAS}))
                out.append((f'nt {tag} -> bf16 hi+lo', {**base, 'c_is_bf16': 1, 'Clo': CLO}))
                out.append((f'nt {tag} -> fp32 with Clo', {**base, 'Clo': CLO}))
                if x3:
                    out.append((f'nt {tag} -> bf16 + fp16 copy', {**base, 'c_is_bf16': 1, 'Clo': CLO, 'c_lo_f16': 1, 'bias': BIAS}))
                if not bname:
                    gate = dict(c_is_bf16=1, C2=C2, ldc2=N // 2)
                    out.append((f'nt {tag} -> u hi+lo, gate hi+lo', {**base, **gate, 'Clo': CLO, 'C2lo': C2LO}))
                    out.append((f'nt {tag} -> u hi, gate hi+lo', {**base, **gate, 'C2lo': C2LO}))
                    out.append((f'nt {tag} -> u hi, gate hi', {**base, **gate}))
                    out.append((f'nt {tag} -> u fp32, gate', {**base, **gate, 'c_is_bf16': 0}))
                    bwd = dict(c_is_bf16=1, C2=C2, ldc2=2 * N, geglu_u=U, ld_u=2 * N)
                    out.append((f'nt {tag} geglu backward, u hi', {**base, **bwd}))
                    out.append((f'nt {tag} geglu backward, u hi+lo', {**base, **bwd, 'Clo': CLO, 'C2lo': C2LO, 'geglu_u_lo': ULO}))
                    out.append((f'nt {tag} geglu backward, no C2', {**base, 'c_is_bf16': 1, 'geglu_u': U, 'ld_u': 2 * N}))
    f16 = dict(ab_f16=1)
    out += [('nt fp16 -> fp32', f16), ('nt fp16 -> fp32 + bias', {**f16, 'bias': BIAS}), ('nt fp16 -> bf16', {**f16, 'c_is_bf16': 1}),
            ('nt fp16 -> bf16 + fp16 copy', {**f16, 'c_is_bf16': 1, 'Clo': CLO}),
            ('nt fp16 -> u bf16, gate fp16 + bf16', {**f16, 'c_is_bf16': 1, 'C2': C2, 'C2lo': C2LO, 'ldc2': N // 2}),
            ('nt fp16 -> u bf16, gate fp16', {**f16, 'c_is_bf16': 1, 'C2': C2, 'ldc2': N // 2}),
            ('nt fp16 -> fp16', {**f16, 'c_is_bf16': 1, 'c_f16': 1}),
            ('nt fp16 -> fp16, not 16-bit', {**f16, 'c_f16': 1}),
            ('nt fp16 geglu backward', {**f16, 'c_is_bf16': 1, 'c_f16': 1, 'C2': C2, 'ldc2': 2 * N, 'geglu_u': U, 'ld_u': 2 * N}),
            ('nt fp16 geglu backward, bf16 du', {**f16, 'c_is_bf16': 1, 'C2': C2, 'ldc2': 2 * N, 'geglu_u': U, 'ld_u': 2 * N}),
            ('nt fp16 shift', {**f16, 'shift_ntok': 257, 'shift_fmap': 16}), ('nt fp16 batch 2', {**f16, 'batch': 2}),
            ('nt fp16 with Alo', {**f16, 'Alo': ALO})]
    x2 = dict(ab_f16=1, Blo=BLO)
    out += [('nt fp16x2 -> fp32', x2), ('nt fp16x2 -> fp32 + bias', {**x2, 'bias': BIAS}), ('nt fp16x2 -> bf16', {**x2, 'c_is_bf16': 1}),
            ('nt fp16x2 -> bf16 + fp16 copy', {**x2, 'c_is_bf16': 1, 'Clo': CLO}), ('nt fp16x2 -> fp16', {**x2, 'c_is_bf16': 1, 'c_f16': 1}),
            ('nt fp16x2 -> fp32 with Clo', {**x2, 'Clo': CLO}), ('nt fp16x2 gate', {**x2, 'c_is_bf16': 1, 'C2': C2, 'ldc2': N // 2})]
    return out


def tn_forms(M, N, K):
    out = []
    for oname, ops in (('bf16', {}), ('hi+lo', dict(Alo=ALO, Blo=BLO)), ('fp16', dict(ab_f16=1)), ('fp16 device factor', dict(ab_f16=1, alpha_dev=ADEV)),
                       ('bf16 chunked A', dict(a_chunk32=1)), ('fp16 chunked A', dict(ab_f16=1, a_chunk32=1))):
        for shift in (0, 1):
            sh = dict(shift_ntok=257, shift_fmap=16) if shift else {}
            for bname, bt in (('', {}), (' batch2', dict(batch=2, strideA=K * M, strideB=K * N, strideC=M * N)),
                              (' batch1024 inner8', dict(batch=1024, batch_inner=8, strideA=8 * K * M, strideB=8 * K * N, strideC=8 * M * N,
                                                         strideA_inner=M, strideB_inner=N, strideC_inner=M * N))):
                for beta in (0.0, 1.0):
                    out.append((f"tn {oname}{' shift' if shift else ''}{bname} beta {beta:g}", {**ops, **sh, **bt, 'beta': beta}))
    return out


# (M, N, K) of C[M, N] = A[K, M]^T B[K, N]: the weight gradients of the step, the cross attention's dK / dV (264 x 64, batched), the thresholds
TN_SHAPES = ([(n1, n2, 2560 * b) for b in (1, 128) for n1 in (1536, 2752, 512, 8192) for n2 in (512, 1376)] + [(512, 1536, 327680), (2752, 2752, 327680)] +
             [(264, 64, 2560), (264, 64, 2592), (264, 64, 300), (160, 64, 2560), (200, 64, 2560), (200, 64, 300)] + [(m, 64, 2560) for m in (128, 129, 320, 336, 384, 385)] + [(264, 65, 2560), (264, 32, 2560)] +
             [(255, 512, 4096), (256, 256, 4096), (256, 255, 4096), (512, 512, 64), (512, 512, 96), (512, 512, 128), (512, 512, 2080), (64, 64, 4096)])


def desc(M, N, K, fields, tn=False):
    d = GemmDesc()
    d.A, d.B, d.C = A, B, CC
    d.lda, d.ldb, d.ldc = (M, N, N) if tn else (K, K, N)
    d.alpha, d.beta, d.M, d.N, d.K, d.batch = 1.0, 0.0, M, N, K, 1
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def cases(L):
    L.amdnuwa_gemm_tn_workspace_bytes.restype = C.c_size_t
    L.amdnuwa_gemm_tn.argtypes = [P, P, C.c_size_t, P]
    L.amdnuwa_gemm_nt.argtypes = [P, P]
    L.amdnuwa_linear_ce_workspace_bytes.restype = C.c_size_t
    L.amdnuwa_linear_ce_workspace_bytes.argtypes = [LL, I]
    L.amdnuwa_linear_ce.argtypes = [P, I, P, I, P, LL, I, I, F, P, P, P, I, P, C.c_size_t, P]
    L.amdnuwa_linear_ce_x3.argtypes = [P, P, P, I, P, P, P, I, P, LL, I, I, F, P, P, P, I, P, C.c_size_t, P]
    for keys in NT_KEYS:
        for M, N, K in (STEP + EDGE if not keys else SHORT):
            for name, fields in nt_forms(M, N, K):
                d = desc(M, N, K, fields)
                yield f'{name} M {M} N {N} K {K}', keys, (lambda d=d: L.amdnuwa_gemm_nt(C.byref(d), None))
    for keys in TN_KEYS:
        for M, N, K in TN_SHAPES:
            for name, fields in tn_forms(M, N, K):
                d = desc(M, N, K, fields, tn=True)

                def call(d=d):
                    return L.amdnuwa_gemm_tn(C.byref(d), WS, L.amdnuwa_gemm_tn_workspace_bytes(C.byref(d)), None)
                yield f'{name} M {M} N {N} K {K}', keys, call
    for keys in ({}, {0: 7}, {14: 3}, {7: 1}, {20: 2}):
        for R, Cc, K in ((2 * 2559, 8192, 512), (300, 64, 32), (128 * 2559, 8192, 512)):
            nb = L.amdnuwa_linear_ce_workspace_bytes(R, Cc)
            for dl in (None, CC):
                yield (f'linear_ce R {R} C {Cc} K {K} dlogits {dl is not None}', keys,
                       lambda dl=dl, R=R, Cc=Cc, K=K, nb=nb: L.amdnuwa_linear_ce(A, K, B, K, TGT, R, Cc, K, 0.5, RL, LOSS, dl, Cc, WS, nb, None))
                for h16, w16 in ((None, None), (H16, W16), (H16, None)):
                    yield (f'linear_ce_x3 R {R} C {Cc} K {K} dlogits {dl is not None} fp16 copies {h16 is not None} {w16 is not None}', keys,
                           lambda dl=dl, R=R, Cc=Cc, K=K, nb=nb, h16=h16, w16=w16:
                           L.amdnuwa_linear_ce_x3(A, ALO, h16, K, B, BLO, w16, K, TGT, R, Cc, K, 0.5, RL, LOSS, dl, Cc, WS, nb, None))
