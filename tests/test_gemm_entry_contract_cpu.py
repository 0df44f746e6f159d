"""What the GEMM entry points of libamdnuwa (gemm.hip) answer without launching anything, pinned as literal tables.

Return codes: every case of amdnuwa_gemm_nt, amdnuwa_gemm_tn, amdnuwa_linear_ce and amdnuwa_linear_ce_x3 here returns before a launch -- it
has M, N or R = 0, or carries an error that precedes the launch -- so the tables run through ctypes without a device and the operand pointers
are never dereferenced.  The order of the checks shows in the codes.  NT: null pointers (ARG), M / N <= 0 (OK, whatever else is wrong),
geglu_u without C2 (ARG), the gate that cannot ride in an epilogue (its own ARG conditions), the fp16-operand forms (UNSUPPORTED from their
queries), and only then alignment, hi + lo pairing, the shift conditions (ARG) and the fp16 second copy off the hi + lo ring (UNSUPPORTED).
TN: a 16-bit C (ARG), M / N <= 0 (OK), alignment, pairing, shift (ARG), the workspace (WORKSPACE), then the fp16 and chunked-A queries
(UNSUPPORTED).  linear_ce: null pointers (ARG), shape and alignment (UNSUPPORTED), R <= 0 (OK), the workspace.

Queries: amdnuwa_gemm_nt_fused, _f16_fused, _f16ops_supported, _f16x2_supported, amdnuwa_gemm_tn_f16_supported, _chunked_a_supported,
amdnuwa_gemm_tn_workspace_bytes and amdnuwa_linear_ce_workspace_bytes over the products of the training step, the shapes on both sides of
the route thresholds and the tuning keys that steer a route; one value per (query, descriptor form, key setting, shape), key settings with equal rows written once
(193 return codes, 43500 + 7812 + 8 query values).

The expected columns were recorded from the library of the commit BEFORE the host code of gemm.hip was folded into one route choice, one
launcher and one argument builder, and the tables passed there unchanged: they pin the behaviour that commit had."""
import ctypes

import pytest

OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
PTR = 4096                                        # a non-null, 16-byte aligned address that is never dereferenced

# (M, N, K) of C[M, N] = A[M, K] B[N, K]^T: the step's products at batch 1 and 128, M around 32 / 128 / 384, 511 | 512 tiles of 256 x 256, K values
NT_SHAPES = ([(2560 * b, n, k) for b in (1, 128) for n in (1536, 2752, 512, 8192) for k in (512, 1376, 1536, 2752)] +
             [(m, 512, 512) for m in (32, 33, 128, 129, 384, 385)] + [(256 * 511, 256, 512), (256 * 512, 256, 512), (256 * 510 + 1, 250, 512)] +
             [(327680, 512, k) for k in (64, 96, 1024, 1056, 2047, 2048)] + [(2560, 512, 64), (2560, 512, 96), (264, 64, 2560)])
# (M, N, K) of C[M, N] = A[K, M]^T B[K, N]: the step's weight gradients, the cross attention's dK / dV (264 x 64), M and N around the thresholds
TN_SHAPES = ([(n1, n2, 2560 * b) for b in (1, 128) for n1 in (1536, 2752, 512, 8192) for n2 in (512, 1376)] +
             [(m, 64, 2560) for m in (128, 129, 264, 384, 385)] + [(264, 65, 2560), (264, 64, 2592), (264, 64, 300)] +
             [(255, 512, 4096), (256, 256, 4096), (256, 255, 4096), (512, 512, 64), (512, 512, 96), (512, 512, 128), (512, 512, 2080)])
NT_KEYS = [{}] + [{0: v} for v in (1, 2, 5, 6, 7, 10, 11, 12)] + [{13: 1}, {0: 7, 13: 1}, {20: 1}, {20: 2}, {22: 1}, {22: 2}]
TN_KEYS = [{}] + [{6: v} for v in (1, 2, 3)] + [{23: 1}, {25: 1}, {25: 2}, {25: 3}, {1: 512}, {2: 64}, {1: 96, 2: 1024}, {6: 2, 25: 1}]


def _fields():
    from nuwa_pytorch_amd import _lib
    return _lib.GemmDesc


def desc(M, N, K, fields, tn=False):
    """a descriptor with every operand pointer PTR and tight leading dimensions, then the overrides of `fields`: 'N/2' and '2N' stand for
    those multiples of N"""
    d = _fields()()
    d.A, d.B, d.C = PTR, PTR, PTR
    d.lda, d.ldb, d.ldc = (M, N, N) if tn else (K, K, N)
    d.alpha, d.beta, d.M, d.N, d.K, d.batch = 1.0, 0.0, M, N, K, 1
    for k, v in fields.items():
        setattr(d, k, {'N/2': N // 2, '2N': 2 * N}.get(v, v) if isinstance(v, str) else v)
    return d


# ---------------------------------------------------------------------------------------------------
# descriptor forms of the queries (the forms kernels.py asks about, and their neighbours)
# ---------------------------------------------------------------------------------------------------
X3 = dict(Alo=PTR, Blo=PTR)
GATE = dict(c_is_bf16=1, C2=PTR, ldc2='N/2')
GBWD = dict(c_is_bf16=1, C2=PTR, ldc2='2N', geglu_u=PTR, ld_u='2N')
F16 = dict(ab_f16=1)
SHIFT = dict(shift_ntok=257, shift_fmap=16)
FORMS = {
    'amdnuwa_gemm_nt_fused': {
        'bf16 gate': GATE, 'bf16 gate, u hi+lo': {**GATE, 'Clo': PTR}, 'bf16 gate, gate hi+lo': {**GATE, 'C2lo': PTR}, 'bf16 gate, shift': {**GATE, **SHIFT},
        'bf16 gate, batch 2': {**GATE, 'batch': 2}, 'bf16 gate, fp32 u': {**GATE, 'c_is_bf16': 0}, 'bf16 no C2': dict(c_is_bf16=1),
        'hi+lo gate': {**X3, **GATE, 'Clo': PTR, 'C2lo': PTR}, 'hi+lo gate, u hi': {**X3, **GATE, 'C2lo': PTR}, 'hi+lo gate, shift': {**X3, **GATE, **SHIFT},
        'hi+lo gate, Blo NULL': {**GATE, 'Alo': PTR}, 'bf16 gate backward': GBWD, 'bf16 gate backward, u hi+lo': {**GBWD, 'geglu_u_lo': PTR},
        'bf16 gate backward, ld_u 2N+4': {**GBWD, 'ld_u': 1028}, 'hi+lo gate backward': {**X3, **GBWD}, 'fp16 gate': {**F16, **GATE},
        'bf16 gate, ldc2 N/2+4': {**GATE, 'ldc2': 260},
    },
    'amdnuwa_gemm_nt_f16_fused': {
        'hi+lo -> bf16 + fp16': {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, 'hi+lo -> bf16 + fp16, shift': {**X3, **SHIFT, 'c_is_bf16': 1, 'Clo': PTR},
        'hi+lo -> bf16 + fp16, batch 600': {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'batch': 600}, 'hi+lo -> fp32 + Clo': {**X3, 'Clo': PTR},
        'hi+lo -> bf16, no Clo': {**X3, 'c_is_bf16': 1}, 'hi+lo -> bf16 + fp16 + gate': {**X3, **GATE, 'Clo': PTR}, 'Alo only': dict(Alo=PTR, c_is_bf16=1, Clo=PTR),
        'bf16 -> bf16 + Clo': dict(c_is_bf16=1, Clo=PTR), 'hi+lo -> bf16 + fp16, ldc N+4': {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'ldc': 516},
    },
    'amdnuwa_gemm_nt_f16ops_supported': {
        '-> fp32': F16, '-> bf16': {**F16, 'c_is_bf16': 1}, '-> bf16 + fp16 copy': {**F16, 'c_is_bf16': 1, 'Clo': PTR}, '-> bf16 + gate': {**F16, **GATE},
        '-> bf16 + gate + copy': {**F16, **GATE, 'Clo': PTR}, '-> fp16': {**F16, 'c_is_bf16': 1, 'c_f16': 1}, '-> fp16, C not 16-bit': {**F16, 'c_f16': 1},
        '-> fp16 + gate': {**F16, **GATE, 'c_f16': 1}, 'gate backward -> fp16': {**F16, **GBWD, 'c_f16': 1}, 'gate backward -> bf16': {**F16, **GBWD},
        'gate backward, u hi+lo': {**F16, **GBWD, 'c_f16': 1, 'geglu_u_lo': PTR}, '-> fp32 + gate': {**F16, **GATE, 'c_is_bf16': 0},
        '-> fp32 + Clo': {**F16, 'Clo': PTR}, 'shift': {**F16, **SHIFT}, 'batch 2': {**F16, 'batch': 2}, 'Alo': {**F16, 'Alo': PTR}, 'Blo': {**F16, 'Blo': PTR},
        'C NULL': {**F16, 'C': None}, 'lda K+4': {**F16, 'lda': 516}, 'ab_f16 = 0, -> bf16': dict(c_is_bf16=1),
    },
    'amdnuwa_gemm_nt_f16x2_supported': {
        '-> fp32': {**F16, 'Blo': PTR}, '-> bf16': {**F16, 'Blo': PTR, 'c_is_bf16': 1}, '-> bf16 + fp16 copy': {**F16, 'Blo': PTR, 'c_is_bf16': 1, 'Clo': PTR},
        '-> fp16': {**F16, 'Blo': PTR, 'c_is_bf16': 1, 'c_f16': 1}, '-> fp16 + copy': {**F16, 'Blo': PTR, 'c_is_bf16': 1, 'c_f16': 1, 'Clo': PTR},
        '-> fp32 + Clo': {**F16, 'Blo': PTR, 'Clo': PTR}, 'gate': {**F16, **GATE, 'Blo': PTR}, 'Blo NULL': F16, 'Alo': {**F16, **X3}, 'shift': {**F16, **SHIFT, 'Blo': PTR},
        'batch 2': {**F16, 'Blo': PTR, 'batch': 2}, '-> bf16, ldc N+4': {**F16, 'Blo': PTR, 'c_is_bf16': 1, 'ldc': 516},
    },
}
B2 = dict(batch=2)
B1024 = dict(batch=1024, batch_inner=8)
TN_FORMS = {
    'amdnuwa_gemm_tn_f16_supported': {
        'fp16': F16, 'fp16 batch 2': {**F16, **B2}, 'fp16 batch 1024 inner 8': {**F16, **B1024}, 'fp16 shift': {**F16, **SHIFT}, 'fp16 + Alo': {**F16, 'Alo': PTR},
        'fp16 lda M+4': {**F16, 'lda': 268}, 'bf16 batch 2': B2,
    },
    'amdnuwa_gemm_tn_chunked_a_supported': {
        'bf16': {}, 'bf16 batch 2': B2, 'fp16 batch 1024 inner 8': {**F16, **B1024}, 'hi+lo batch 2': {**X3, **B2}, 'shift batch 2': {**SHIFT, **B2}, 'batch 2 ldb N+4': {**B2, 'ldb': 68},
    },
    'amdnuwa_gemm_tn_workspace_bytes': {
        'bf16': {}, 'bf16 batch 2': B2, 'bf16 batch 1024 inner 8': B1024, 'hi+lo': X3, 'hi+lo batch 2': {**X3, **B2}, 'shift': SHIFT, 'shift batch 2': {**SHIFT, **B2}, 'fp16 batch 2': {**F16, **B2},
    },
}
CE_WS = [(0, 64), (5, 0), (5, 96), (1, 64), (300, 64), (2 * 2559, 8192), (128 * 2559, 8192), (1 << 31, 64)]

# ---------------------------------------------------------------------------------------------------
# return-code cases: name -> (shape, descriptor fields, tuning keys).  'NULL d' passes no descriptor.
# ---------------------------------------------------------------------------------------------------
BIG, MID, SMALL = (327680, 512, 512), (2560, 512, 512), (20, 512, 512)
NT_CASES = {
    'NULL d': (BIG, None, {}),
    'A NULL': (BIG, dict(A=None), {}), 'B NULL': (BIG, dict(B=None), {}), 'C NULL': (BIG, dict(C=None), {}),
    'C NULL, M = 0': ((0, 512, 512), dict(C=None), {}),
    'M = 0': ((0, 512, 512), {}, {}), 'N = 0': ((512, 0, 512), {}, {}), 'M = -3': ((-3, 512, 512), {}, {}),
    'M = 0, geglu_u without C2': ((0, 512, 512), dict(geglu_u=PTR), {}),
    'M = 0, K = 12, lda = 3, Alo only, shift without fmap': ((0, 512, 12), dict(lda=3, Alo=PTR, shift_ntok=5), {}),
    'N = 0, fp16 operands with Alo': ((512, 0, 512), {**F16, 'Alo': PTR}, {}),
    'N = 0, fp16 second copy off the ring': ((20, 0, 512), dict(c_is_bf16=1, Clo=PTR, c_lo_f16=1), {}),
    'geglu_u without C2': (BIG, dict(c_is_bf16=1, geglu_u=PTR, ld_u='2N'), {}),
    'geglu_u without C2, fp16 operands': (BIG, {**F16, 'c_is_bf16': 1, 'geglu_u': PTR}, {}),
    'geglu_u without C2, K = 12': ((327680, 512, 12), dict(geglu_u=PTR), {}),
    'gate beside the ring, fp32 u': (MID, {**GATE, 'c_is_bf16': 0}, {}),
    'gate beside the ring, ldc N+8': (MID, {**GATE, 'ldc': 520}, {}),
    'gate beside the ring, batch 2': (MID, {**GATE, 'batch': 2}, {}),
    'gate beside the ring, K = 12': ((2560, 512, 12), GATE, {}),
    'gate beside the ring, lda K+4': (MID, {**GATE, 'lda': 516}, {}),
    'gate beside the ring, Alo only': (MID, {**GATE, 'Alo': PTR}, {}),
    'gate beside the ring, shift without fmap': (MID, {**GATE, 'shift_ntok': 257}, {}),
    'gate beside the ring, fp32 u, K = 12': ((2560, 512, 12), {**GATE, 'c_is_bf16': 0}, {}),
    'gate on the ring shape under key 0 = 2, ldc N+8': (BIG, {**GATE, 'ldc': 520}, {0: 2}),
    'gate on the ring shape under key 0 = 12, fp32 u': (BIG, {**GATE, 'c_is_bf16': 0}, {0: 12}),
    'gate on the ring shape under key 0 = 11, batch 2': (BIG, {**GATE, 'batch': 2}, {0: 11}),
    'hi+lo gate on the ring shape under key 13 = 1, ldc N+8': (BIG, {**X3, **GATE, 'ldc': 520}, {13: 1}),
    'hi+lo gate backward on the ring shape, fp32 u': (BIG, {**X3, **GBWD, 'c_is_bf16': 0}, {}),
    'gate backward with u hi+lo on the ring shape, batch 2': (BIG, {**GBWD, 'geglu_u_lo': PTR, 'batch': 2}, {}),
    'fp16 x2, 20 rows': (SMALL, {**F16, 'Blo': PTR}, {}), 'fp16 x2, 32 rows': ((32, 512, 512), {**F16, 'Blo': PTR}, {}),
    'fp16 x2, Alo': (BIG, {**F16, **X3}, {}), 'fp16 x2, shift': (BIG, {**F16, **SHIFT, 'Blo': PTR}, {}), 'fp16 x2, batch 2': (BIG, {**F16, 'Blo': PTR, 'batch': 2}, {}),
    'fp16 x2, gate': (BIG, {**F16, **GATE, 'Blo': PTR}, {}), 'fp16 x2, K = 520': ((327680, 512, 520), {**F16, 'Blo': PTR}, {}),
    'fp16 x2, fp32 + Clo': (BIG, {**F16, 'Blo': PTR, 'Clo': PTR}, {}), 'fp16 x2, fp16 + copy': (BIG, {**F16, 'Blo': PTR, 'c_is_bf16': 1, 'c_f16': 1, 'Clo': PTR}, {}),
    'fp16 x2, bf16 N = 500': ((327680, 500, 512), {**F16, 'Blo': PTR, 'c_is_bf16': 1}, {}),
    'fp16 x2 under key 0 = 2': (BIG, {**F16, 'Blo': PTR}, {0: 2}), 'fp16 x2 under key 0 = 11': (BIG, {**F16, 'Blo': PTR}, {0: 11}),
    'fp16 x2 under key 0 = 6': (BIG, {**F16, 'Blo': PTR}, {0: 6}), 'fp16 x2 under key 0 = 12': (BIG, {**F16, 'Blo': PTR}, {0: 12}),
    'fp16, 20 rows': (SMALL, F16, {}), 'fp16, 32 rows': ((32, 512, 512), F16, {}), 'fp16, Alo': (BIG, {**F16, 'Alo': PTR}, {}), 'fp16, shift': (BIG, {**F16, **SHIFT}, {}),
    'fp16, batch 2': (BIG, {**F16, 'batch': 2}, {}), 'fp16, K = 520': ((327680, 512, 520), F16, {}), 'fp16, lda K+4': (BIG, {**F16, 'lda': 516}, {}),
    'fp16 -> fp16, C not 16-bit': (BIG, {**F16, 'c_f16': 1}, {}), 'fp16 -> fp16 + gate': (BIG, {**F16, **GATE, 'c_f16': 1}, {}),
    'fp16 gate backward -> bf16': (BIG, {**F16, **GBWD}, {}), 'fp16 gate backward, u hi+lo': (BIG, {**F16, **GBWD, 'c_f16': 1, 'geglu_u_lo': PTR}, {}),
    'fp16 -> fp32 + gate': (BIG, {**F16, **GATE, 'c_is_bf16': 0}, {}), 'fp16 -> fp32 + Clo': (BIG, {**F16, 'Clo': PTR}, {}),
    'fp16 -> bf16 + gate + copy': (BIG, {**F16, **GATE, 'Clo': PTR}, {}), 'fp16 -> bf16, N = 500': ((327680, 500, 512), {**F16, 'c_is_bf16': 1}, {}),
    'fp16 -> fp32, N = 502': ((327680, 502, 512), F16, {}),
    'fp16 under key 0 = 1': (BIG, F16, {0: 1}), 'fp16 under key 0 = 2': (BIG, F16, {0: 2}), 'fp16 under key 0 = 5': (BIG, F16, {0: 5}), 'fp16 under key 0 = 12': (BIG, F16, {0: 12}),
    'K = 12': ((327680, 512, 12), {}, {}), 'K = 2047': ((327680, 512, 2047), {}, {}), 'lda K+4': (BIG, dict(lda=516), {}), 'ldb K+4': (BIG, dict(ldb=516), {}),
    'K = 12, Alo only': ((327680, 512, 12), dict(Alo=PTR), {}),
    'Alo only': (BIG, dict(Alo=PTR), {}), 'Blo only': (BIG, dict(Blo=PTR), {}), 'Alo only, shift without fmap': (BIG, dict(Alo=PTR, shift_ntok=257), {}),
    'shift without fmap': (BIG, dict(shift_ntok=257), {}), 'shift, K = 520': ((327680, 512, 520), SHIFT, {}),
    'shift without fmap, fp16 second copy': (BIG, {**X3, 'shift_ntok': 257, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {}),
    'fp16 second copy, shift': (BIG, {**X3, **SHIFT, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {}),
    'fp16 second copy, 2560 rows': (MID, {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {}),
    'fp16 second copy, 20 rows': (SMALL, {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {}),
    'fp16 second copy, 20 rows, batch 600': (SMALL, {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1, 'batch': 600}, {}),
    'fp16 second copy, bf16 operands': (BIG, dict(c_is_bf16=1, Clo=PTR, c_lo_f16=1), {}),
    'fp16 second copy, fp32 C': (BIG, {**X3, 'Clo': PTR, 'c_lo_f16': 1}, {}),
    'fp16 second copy, no Clo': (BIG, {**X3, 'c_is_bf16': 1, 'c_lo_f16': 1}, {}),
    'fp16 second copy, N = 500': ((327680, 500, 512), {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {}),
    'fp16 second copy, K = 520': ((327680, 512, 520), {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {}),
    'fp16 second copy under key 13 = 1': (BIG, {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {13: 1}),
    'fp16 second copy under key 0 = 2': (BIG, {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {0: 2}),
    'fp16 second copy under key 0 = 12': (BIG, {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {0: 12}),
    'fp16 second copy under key 0 = 11': (BIG, {**X3, 'c_is_bf16': 1, 'Clo': PTR, 'c_lo_f16': 1}, {0: 11}),
    'few rows, fp32 C with Clo': (SMALL, dict(Clo=PTR), {}), 'few rows, fp32 C with Clo, hi+lo': (SMALL, {**X3, 'Clo': PTR}, {}),
    '32 rows, fp32 C with Clo': ((32, 512, 512), dict(Clo=PTR), {}),
}
TN_BIG, TN_KV = (512, 512, 327680), (264, 64, 2560)
TN_CASES = {
    'NULL d': (TN_BIG, None, {}), 'A NULL': (TN_BIG, dict(A=None), {}), 'B NULL': (TN_BIG, dict(B=None), {}), 'C NULL': (TN_BIG, dict(C=None), {}),
    '16-bit C': (TN_BIG, dict(c_is_bf16=1), {}), '16-bit C, M = 0': ((0, 512, 2560), dict(c_is_bf16=1), {}),
    'M = 0': ((0, 512, 2560), {}, {}), 'N = 0': ((512, 0, 2560), {}, {}), 'N = -1, lda M+4, Alo only, no workspace': ((512, -1, 2560), dict(lda=516, Alo=PTR, ws=None), {}),
    'M = 0, fp16 with Alo, chunked A': ((0, 512, 2560), {**F16, 'Alo': PTR, 'a_chunk32': 1}, {}),
    'lda M+4': (TN_BIG, dict(lda=516), {}), 'ldb N+4': (TN_BIG, dict(ldb=516), {}), 'lda M+4, Alo only': (TN_BIG, dict(lda=516, Alo=PTR), {}),
    'Alo only': (TN_BIG, dict(Alo=PTR), {}), 'Blo only': (TN_BIG, dict(Blo=PTR), {}), 'Alo only, shift without fmap': (TN_BIG, dict(Alo=PTR, shift_ntok=257), {}),
    'shift without fmap': (TN_BIG, dict(shift_ntok=257), {}), 'shift, N = 520': ((512, 520, 327680), SHIFT, {}), 'shift without fmap, no workspace': (TN_BIG, dict(shift_ntok=257, ws=None), {}),
    'no workspace': (TN_BIG, dict(ws=None), {}), 'workspace 4 bytes short': (TN_BIG, dict(ws_short=4), {}), 'workspace 4 bytes short, hi+lo': (TN_BIG, {**X3, 'ws_short': 4}, {}),
    'workspace 4 bytes short, dK / dV batch': (TN_KV, {**B2, 'ws_short': 4}, {}), 'workspace 4 bytes short under key 1 = 96': (TN_BIG, dict(ws_short=4), {1: 96}),
    'no workspace, fp16 shift': (TN_BIG, {**F16, **SHIFT, 'ws': None}, {}), 'workspace 4 bytes short, chunked A': (TN_BIG, dict(a_chunk32=1, ws_short=4), {}),
    'fp16, shift': (TN_BIG, {**F16, **SHIFT}, {}), 'fp16, hi+lo': (TN_BIG, {**F16, **X3}, {}), 'fp16, 255 x 512': ((255, 512, 4096), F16, {}), 'fp16, K = 96': ((512, 512, 96), F16, {}),
    'fp16, K = 2080': ((512, 512, 2080), F16, {}), 'fp16 under key 23 = 1': (TN_BIG, F16, {23: 1}), 'fp16 under key 6 = 1': (TN_BIG, F16, {6: 1}), 'fp16 under key 6 = 2': (TN_BIG, F16, {6: 2}),
    'fp16, dK / dV unbatched': (TN_KV, F16, {}), 'fp16, dK / dV batch, 128 rows': ((128, 64, 2560), {**F16, **B2}, {}), 'fp16, dK / dV batch, 385 rows': ((385, 64, 2560), {**F16, **B2}, {}),
    'fp16, dK / dV batch, N = 65': ((264, 65, 2560), {**F16, **B2}, {}), 'fp16, dK / dV batch under key 25 = 1': (TN_KV, {**F16, **B2}, {25: 1}),
    'fp16, dK / dV batch under key 6 = 3': (TN_KV, {**F16, **B2}, {6: 3}), 'fp16, dK / dV batch under key 6 = 1': (TN_KV, {**F16, **B2}, {6: 1}),
    'fp16 chunked A, dK / dV unbatched': (TN_KV, {**F16, 'a_chunk32': 1}, {}),
    'chunked A, big': (TN_BIG, dict(a_chunk32=1), {}), 'chunked A, dK / dV unbatched': (TN_KV, dict(a_chunk32=1), {}), 'chunked A, dK / dV batch, hi+lo': (TN_KV, {**X3, **B2, 'a_chunk32': 1}, {}),
    'chunked A, dK / dV batch, shift': ((264, 64, 2560), {**SHIFT, **B2, 'a_chunk32': 1}, {}), 'chunked A, dK / dV batch under key 25 = 1': (TN_KV, {**B2, 'a_chunk32': 1}, {25: 1}),
    'chunked A, dK / dV batch under key 6 = 1': (TN_KV, {**B2, 'a_chunk32': 1}, {6: 1}), 'chunked A, dK / dV batch under key 6 = 3': (TN_KV, {**B2, 'a_chunk32': 1}, {6: 3}),
}
# linear_ce / linear_ce_x3: overrides of (h w targets row_loss loss dlogits = PTR, ldh = ldw = K, ld_dl = C, R = 300, C = 64, K = 32, exact workspace);
# h_lo / w_lo = PTR and h_f16 / w_f16 = NULL for the x3 entry point
CE_CASES = {
    'h NULL': dict(h=None), 'w NULL': dict(w=None), 'targets NULL': dict(targets=None), 'row_loss NULL': dict(row_loss=None), 'loss NULL': dict(loss=None),
    'loss NULL, C = 96': dict(loss=None, C=96), 'h NULL, R = 0': dict(h=None, R=0),
    'C = 96': dict(C=96), 'K = 48': dict(K=48, ldh=48, ldw=48), 'ldh K+4': dict(ldh=36), 'ldw K+4': dict(ldw=36), 'ld_dl C+4': dict(ld_dl=68), 'ld_dl C+4, no dlogits': dict(ld_dl=68, dlogits=None, R=0),
    'R = 2^31': dict(R=1 << 31), 'R = 2^31, no workspace': dict(R=1 << 31, workspace=None), 'C = 96, R = 0': dict(C=96, R=0),
    'R = 0': dict(R=0), 'R = -1': dict(R=-1), 'R = 0, no workspace': dict(R=0, workspace=None), 'R = 0, no dlogits': dict(R=0, dlogits=None),
    'no workspace': dict(workspace=None), 'workspace 4 bytes short': dict(ws_short=4), 'workspace 4 bytes short, training shape': dict(ws_short=4, R=128 * 2559, C=8192, K=512, ldh=512, ldw=512, ld_dl=8192),
    'h_lo NULL': dict(h_lo=None), 'w_lo NULL': dict(w_lo=None), 'h_f16 only': dict(h_f16=PTR), 'w_f16 only': dict(w_f16=PTR), 'w_f16 only, R = 0': dict(w_f16=PTR, R=0),
    'h_lo NULL, h NULL': dict(h_lo=None, h=None), 'both fp16 copies, R = 0': dict(h_f16=PTR, w_f16=PTR, R=0), 'both fp16 copies, C = 96': dict(h_f16=PTR, w_f16=PTR, C=96),
}
CE_PARAMS = {'amdnuwa_linear_ce': 'h ldh w ldw targets R C K grad_scale row_loss loss dlogits ld_dl workspace workspace_bytes',
             'amdnuwa_linear_ce_x3': 'h h_lo h_f16 ldh w w_lo w_f16 ldw targets R C K grad_scale row_loss loss dlogits ld_dl workspace workspace_bytes'}


def _L():
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    L.amdnuwa_gemm_tn_workspace_bytes.restype = ctypes.c_size_t
    L.amdnuwa_linear_ce_workspace_bytes.restype = ctypes.c_size_t
    L.amdnuwa_linear_ce_workspace_bytes.argtypes = [ctypes.c_longlong, ctypes.c_int]
    return L


class keys_set:
    """sets the tuning keys of a case and puts back what they held"""
    def __init__(self, L, keys):
        self.L, self.keys = L, keys

    def __enter__(self):
        self.old = {k: self.L.amdnuwa_get_tuning(k) for k in self.keys}
        for k, v in self.keys.items():
            self.L.amdnuwa_set_tuning(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.L.amdnuwa_set_tuning(k, v)


def call_gemm(L, entry, case):
    (M, N, K), fields, keys = case
    with keys_set(L, keys):
        if fields is None:
            return L.amdnuwa_gemm_nt(None, None) if entry == 'amdnuwa_gemm_nt' else L.amdnuwa_gemm_tn(None, ctypes.c_void_p(PTR), ctypes.c_size_t(1 << 40), None)
        fields = dict(fields)
        ws, short = fields.pop('ws', PTR), fields.pop('ws_short', 0)
        d = desc(M, N, K, fields, tn=entry == 'amdnuwa_gemm_tn')
        if entry == 'amdnuwa_gemm_nt':
            return L.amdnuwa_gemm_nt(ctypes.byref(d), None)
        nb = L.amdnuwa_gemm_tn_workspace_bytes(ctypes.byref(d)) if M > 0 and N > 0 else 0
        return L.amdnuwa_gemm_tn(ctypes.byref(d), ctypes.c_void_p(ws), ctypes.c_size_t(nb - short), None)


def call_ce(L, entry, over):
    over = dict(over)
    v = dict(h=PTR, w=PTR, targets=PTR, row_loss=PTR, loss=PTR, dlogits=PTR, workspace=PTR, h_lo=PTR, w_lo=PTR, h_f16=None, w_f16=None,
             R=300, C=64, K=32, ldh=32, ldw=32, ld_dl=64, grad_scale=0.5)
    short = over.pop('ws_short', 0)
    v.update(over)
    v['workspace_bytes'] = L.amdnuwa_linear_ce_workspace_bytes(v['R'], v['C']) - short
    conv = {'R': ctypes.c_longlong, 'grad_scale': ctypes.c_float, 'workspace_bytes': ctypes.c_size_t}
    args = [conv[n](v[n]) if n in conv else (v[n] if n in ('C', 'K', 'ldh', 'ldw', 'ld_dl') else ctypes.c_void_p(v[n])) for n in CE_PARAMS[entry].split()]
    return getattr(L, entry)(*args, None)


def ce_applicable(entry, over):
    return all(n in CE_PARAMS[entry].split() or n == 'ws_short' for n in over)


def query_row(L, fn, fields, keys, shapes, tn):
    with keys_set(L, keys):
        return tuple(int(getattr(L, fn)(ctypes.byref(desc(M, N, K, fields, tn=tn)))) for M, N, K in shapes)


# ---------------------------------------------------------------------------------------------------
# recorded return codes, one letter per case in the order of NT_CASES / TN_CASES / the applicable CE_CASES (groups of ten):
# A = ARG, U = UNSUPPORTED, W = WORKSPACE, O = OK
# ---------------------------------------------------------------------------------------------------
WANT = {
    'amdnuwa_gemm_nt': 'AAAAAOOOOO OOAAAAAAAA AAAAAAAAAU UUUUUUUUUU UUUUUUUUUU UUUUUUUUUU UUUAAAAAAA AAAAUUUUUU UUUUUUUAAA',
    'amdnuwa_gemm_tn': 'AAAAAAOOOO AAAAAAAAAW WWWWWWUUAU UUUUUUAAUU UUUUUUUUU',
    'amdnuwa_linear_ce': 'AAAAAAAUUU UUOUUUOOOO WWW',
    'amdnuwa_linear_ce_x3': 'AAAAAAAUUU UUOUUUOOOO WWWAAAAAAO U',
}
# recorded query values: query -> descriptor form -> {one character per shape of NT_SHAPES: the indices into the key list that give it};
# NT_NONE = no shape, NT_ALL = every key setting
NT_NONE, NT_ALL = '0' * 50, tuple(range(15))
NT_QUERIES = {
    'amdnuwa_gemm_nt_fused': {
        'bf16 gate': {'00000000000000001111111111111111000000010111101000': (0, 9, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 4, 6, 7, 8), '11111111111111111111111111111111111111110111101111': (5, 10)},
        'bf16 gate, u hi+lo': {NT_NONE: NT_ALL},
        'bf16 gate, gate hi+lo': {NT_NONE: NT_ALL},
        'bf16 gate, shift': {
            '00000000000000001111111111111111000000010111101000': (0, 9, 11, 12, 13, 14),
            NT_NONE: (1, 2, 3, 4, 6, 7, 8),
            '11111111111111111111111111111111111111110111101111': (5, 10)},
        'bf16 gate, batch 2': {NT_NONE: NT_ALL},
        'bf16 gate, fp32 u': {NT_NONE: NT_ALL},
        'bf16 no C2': {NT_NONE: NT_ALL},
        'hi+lo gate': {'00000000000000001111111111111111000000010111101000': (0, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 4, 6, 7, 8, 9, 10), '11111111111111111111111111111111111111110111101111': (5,)},
        'hi+lo gate, u hi': {
            '00000000000000001111111111111111000000010111101000': (0, 11, 12, 13, 14),
            NT_NONE: (1, 2, 3, 4, 6, 7, 8, 9, 10),
            '11111111111111111111111111111111111111110111101111': (5,)},
        'hi+lo gate, shift': {NT_NONE: NT_ALL},
        'hi+lo gate, Blo NULL': {NT_NONE: NT_ALL},
        'bf16 gate backward': {
            '00000000000000001111111111111111000000010111101000': (0, 9, 11, 12, 13, 14),
            NT_NONE: (1, 2, 3, 4, 6, 7, 8),
            '11111111111111111111111111111111111111110111101111': (5, 10)},
        'bf16 gate backward, u hi+lo': {NT_NONE: NT_ALL},
        'bf16 gate backward, ld_u 2N+4': {NT_NONE: NT_ALL},
        'hi+lo gate backward': {NT_NONE: NT_ALL},
        'fp16 gate': {'00000000000000001111111111111111000000010111101000': (0, 9, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 4, 6, 7, 8), '11111111111111111111111111111111111111110111101111': (5, 10)},
        'bf16 gate, ldc2 N/2+4': {NT_NONE: NT_ALL},
    },
    'amdnuwa_gemm_nt_f16_fused': {
        'hi+lo -> bf16 + fp16': {
            '00000000000000001111111111111111000000010111101000': (0, 11, 12, 13, 14),
            NT_NONE: (1, 2, 3, 4, 6, 7, 8, 9, 10),
            '11111111111111111111111111111111111111110111101111': (5,)},
        'hi+lo -> bf16 + fp16, shift': {NT_NONE: NT_ALL},
        'hi+lo -> bf16 + fp16, batch 600': {
            '11111111111111111111111111111111011111110111101111': (0, 11, 12, 13, 14),
            NT_NONE: (1, 2, 3, 4, 6, 7, 8, 9, 10),
            '11111111111111111111111111111111111111110111101111': (5,)},
        'hi+lo -> fp32 + Clo': {NT_NONE: NT_ALL},
        'hi+lo -> bf16, no Clo': {NT_NONE: NT_ALL},
        'hi+lo -> bf16 + fp16 + gate': {NT_NONE: NT_ALL},
        'Alo only': {NT_NONE: NT_ALL},
        'bf16 -> bf16 + Clo': {NT_NONE: NT_ALL},
        'hi+lo -> bf16 + fp16, ldc N+4': {NT_NONE: NT_ALL},
    },
    'amdnuwa_gemm_nt_f16ops_supported': {
        '-> fp32': {'11111111111111111111111111111111011111110111101111': (0, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 8)},
        '-> bf16': {'11111111111111111111111111111111011111110111101111': (0, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 8)},
        '-> bf16 + fp16 copy': {'11111111111111111111111111111111011111110111101111': (0, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 8)},
        '-> bf16 + gate': {'11111111111111111111111111111111011111110111101111': (0, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 8)},
        '-> bf16 + gate + copy': {NT_NONE: NT_ALL},
        '-> fp16': {'11111111111111111111111111111111011111110111101111': (0, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 8)},
        '-> fp16, C not 16-bit': {NT_NONE: NT_ALL},
        '-> fp16 + gate': {NT_NONE: NT_ALL},
        'gate backward -> fp16': {'11111111111111111111111111111111011111110111101111': (0, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 8)},
        'gate backward -> bf16': {NT_NONE: NT_ALL},
        'gate backward, u hi+lo': {NT_NONE: NT_ALL},
        '-> fp32 + gate': {NT_NONE: NT_ALL},
        '-> fp32 + Clo': {NT_NONE: NT_ALL},
        'shift': {NT_NONE: NT_ALL},
        'batch 2': {NT_NONE: NT_ALL},
        'Alo': {NT_NONE: NT_ALL},
        'Blo': {NT_NONE: NT_ALL},
        'C NULL': {NT_NONE: NT_ALL},
        'lda K+4': {NT_NONE: NT_ALL},
        'ab_f16 = 0, -> bf16': {'11111111111111111111111111111111011111110111101111': (0, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 8)},
    },
    'amdnuwa_gemm_nt_f16x2_supported': {
        '-> fp32': {'11111111111111111111111111111111011111111111101111': (0, 5, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 4, 6, 7, 8)},
        '-> bf16': {'11111111111111111111111111111111011111110111101111': (0, 5, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 4, 6, 7, 8)},
        '-> bf16 + fp16 copy': {'11111111111111111111111111111111011111110111101111': (0, 5, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 4, 6, 7, 8)},
        '-> fp16': {'11111111111111111111111111111111011111110111101111': (0, 5, 9, 10, 11, 12, 13, 14), NT_NONE: (1, 2, 3, 4, 6, 7, 8)},
        '-> fp16 + copy': {NT_NONE: NT_ALL},
        '-> fp32 + Clo': {NT_NONE: NT_ALL},
        'gate': {NT_NONE: NT_ALL},
        'Blo NULL': {NT_NONE: NT_ALL},
        'Alo': {NT_NONE: NT_ALL},
        'shift': {NT_NONE: NT_ALL},
        'batch 2': {NT_NONE: NT_ALL},
        '-> bf16, ldc N+4': {NT_NONE: NT_ALL},
    },
}
# recorded query values: query -> descriptor form -> {one character per shape of TN_SHAPES: the indices into the key list that give it};
# TN_NONE = no shape, TN_ALL = every key setting; amdnuwa_gemm_tn_workspace_bytes is recorded as its number of split-K slabs per shape,
# bytes / (batch * M * N * 4), space-separated
TN_NONE, TN_ALL = '0' * 31, tuple(range(12))
TN_QUERIES = {
    'amdnuwa_gemm_tn_f16_supported': {
        'fp16': {'1111111111111111000000000100010': (0, 3, 5, 6, 7, 8, 9, 10), TN_NONE: (1, 2, 4, 11)},
        'fp16 batch 2': {'1111111111111111001100110100010': (0, 6, 7, 8, 9, 10), TN_NONE: (1, 11), '0000000000000000001100110000000': (2, 4), '1111111111111111000000000100010': (3, 5)},
        'fp16 batch 1024 inner 8': {'1111111111111111001100110100010': (0, 6, 7, 8, 9, 10), TN_NONE: (1, 11), '0000000000000000001100110000000': (2, 4), '1111111111111111000000000100010': (3, 5)},
        'fp16 shift': {TN_NONE: TN_ALL},
        'fp16 + Alo': {TN_NONE: TN_ALL},
        'fp16 lda M+4': {TN_NONE: TN_ALL},
        'bf16 batch 2': {'1111111111111111001100110100010': (0, 6, 7, 8, 9, 10), TN_NONE: (1, 11), '0000000000000000001100110000000': (2, 4), '1111111111111111000000000100010': (3, 5)},
    },
    'amdnuwa_gemm_tn_chunked_a_supported': {
        'bf16': {TN_NONE: TN_ALL},
        'bf16 batch 2': {'0000000000000000001100110000000': (0, 2, 4, 6, 7, 8, 9, 10), TN_NONE: (1, 3, 5, 11)},
        'fp16 batch 1024 inner 8': {'0000000000000000001100110000000': (0, 2, 4, 6, 7, 8, 9, 10), TN_NONE: (1, 3, 5, 11)},
        'hi+lo batch 2': {TN_NONE: TN_ALL},
        'shift batch 2': {TN_NONE: TN_ALL},
        'batch 2 ldb N+4': {TN_NONE: TN_ALL},
    },
    'amdnuwa_gemm_tn_workspace_bytes': {
        'bf16': {
            '10 7 10 3 10 10 4 1 21 7 11 3 64 21 4 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (0, 3, 4, 5, 6, 7),
            '10 7 10 4 10 10 4 1 21 7 11 4 64 23 4 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (1, 2, 11),
            '10 10 10 7 10 10 8 2 42 14 23 7 128 42 8 2 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (8,),
            '21 7 11 3 40 21 4 1 21 7 11 3 64 21 4 1 40 40 40 40 40 40 41 5 64 64 64 1 2 2 33': (9,),
            '3 2 3 1 3 3 1 1 8 2 4 1 24 8 1 1 3 3 3 3 3 3 3 1 4 4 4 1 1 1 3': (10,)},
        'bf16 batch 2': {
            '10 3 5 1 10 10 2 1 10 3 5 1 32 10 2 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (0, 3, 4, 5, 6, 7),
            '10 3 5 2 10 10 2 1 10 3 5 2 32 11 2 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (1, 2, 11),
            '10 7 10 3 10 10 4 1 21 7 11 3 64 21 4 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (8,),
            '10 3 5 1 32 10 2 1 10 3 5 1 32 10 2 1 40 40 40 40 40 40 41 5 64 64 64 1 2 2 32': (9,),
            '3 1 2 1 3 3 1 1 4 1 2 1 12 4 1 1 3 3 3 3 3 3 3 1 4 4 4 1 1 1 3': (10,)},
        'bf16 batch 1024 inner 8': {'1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1': TN_ALL},
        'hi+lo': {
            '10 7 10 4 10 10 4 1 21 7 11 4 64 23 4 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (0, 1, 2, 3, 4, 5, 6, 7, 11),
            '10 3 5 2 10 10 2 1 10 3 5 2 32 11 2 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (8,),
            '21 7 11 4 40 23 4 1 21 7 11 4 64 23 4 1 40 40 40 40 40 40 41 5 64 64 64 1 2 2 33': (9,),
            '2 1 1 1 3 2 1 1 2 1 1 1 6 2 1 1 3 3 3 3 3 3 3 1 4 4 4 1 1 1 3': (10,)},
        'hi+lo batch 2': {
            '10 3 5 2 10 10 2 1 10 3 5 2 32 11 2 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (0, 1, 2, 3, 4, 5, 6, 7, 11),
            '5 1 2 1 10 5 1 1 5 1 2 1 16 5 1 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (8,),
            '10 3 5 2 32 11 2 1 10 3 5 2 32 11 2 1 40 40 40 40 40 40 41 5 64 64 64 1 2 2 32': (9,),
            '1 1 1 1 3 1 1 1 1 1 1 1 3 1 1 1 3 3 3 3 3 3 3 1 4 4 4 1 1 1 3': (10,)},
        'shift': {
            '10 7 10 3 10 10 4 1 21 7 11 3 64 21 4 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (0, 3, 4, 5, 6, 7),
            '10 7 10 4 10 10 4 1 21 7 11 4 64 23 4 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (1, 2, 11),
            '10 10 10 7 10 10 8 2 42 14 23 7 128 42 8 2 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (8,),
            '21 7 11 3 40 21 4 1 21 7 11 3 64 21 4 1 40 40 40 40 40 40 41 5 64 64 64 1 2 2 33': (9,),
            '3 2 3 1 3 3 1 1 8 2 4 1 24 8 1 1 3 3 3 3 3 3 3 1 4 4 4 1 1 1 3': (10,)},
        'shift batch 2': {
            '10 3 5 1 10 10 2 1 10 3 5 1 32 10 2 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (0, 3, 4, 5, 6, 7),
            '10 3 5 2 10 10 2 1 10 3 5 2 32 11 2 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (1, 2, 11),
            '10 7 10 3 10 10 4 1 21 7 11 3 64 21 4 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (8,),
            '10 3 5 1 32 10 2 1 10 3 5 1 32 10 2 1 40 40 40 40 40 40 41 5 64 64 64 1 2 2 32': (9,),
            '3 1 2 1 3 3 1 1 4 1 2 1 12 4 1 1 3 3 3 3 3 3 3 1 4 4 4 1 1 1 3': (10,)},
        'fp16 batch 2': {
            '10 3 5 1 10 10 2 1 10 3 5 1 32 10 2 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (0, 3, 4, 5, 6, 7),
            '10 3 5 2 10 10 2 1 10 3 5 2 32 11 2 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (1, 2, 11),
            '10 7 10 3 10 10 4 1 21 7 11 3 64 21 4 1 10 10 10 10 10 10 11 2 16 16 16 1 1 1 9': (8,),
            '10 3 5 1 32 10 2 1 10 3 5 1 32 10 2 1 40 40 40 40 40 40 41 5 64 64 64 1 2 2 32': (9,),
            '3 1 2 1 3 3 1 1 4 1 2 1 12 4 1 1 3 3 3 3 3 3 3 1 4 4 4 1 1 1 3': (10,)},
    },
}
CE_WS_BYTES = [0, 0, 0, 16, 4800, 5281776, 338033664, 34359738368]


def cases_of(entry):
    if entry.startswith('amdnuwa_linear_ce'):
        return {c: v for c, v in CE_CASES.items() if ce_applicable(entry, v)}
    return NT_CASES if entry == 'amdnuwa_gemm_nt' else TN_CASES


@pytest.mark.parametrize('entry', sorted(WANT))
def test_return_codes_before_any_launch(entry):
    L = _L()
    cases = cases_of(entry)
    want = [{'O': OK, 'A': ARG, 'U': UNSUPPORTED, 'W': WORKSPACE}[ch] for ch in WANT[entry].replace(' ', '')]
    assert len(want) == len(cases) >= 20
    got = []
    for (name, case), w in zip(cases.items(), want):
        if entry.startswith('amdnuwa_linear_ce'):
            assert w != OK or case.get('R', 300) <= 0, 'a case may not reach a launch'
            got.append((name, call_ce(L, entry, case)))
        else:
            assert w != OK or min(case[0][:2]) <= 0, 'a case may not reach a launch'
            got.append((name, call_gemm(L, entry, case)))
    assert got == list(zip(cases, want))


def check_queries(L, table, forms, keys, shapes, tn):
    """every form of every query under every key setting against the recorded row; returns the number of values compared"""
    assert {f: list(v) for f, v in table.items()} == {f: list(v) for f, v in forms.items()}
    bad, n = [], 0
    for fn, rows in table.items():
        for name, by_value in rows.items():
            assert sorted(k for ks in by_value.values() for k in ks) == list(range(len(keys))), (fn, name)
            for want, ks in by_value.items():
                for k in ks:
                    got = query_row(L, fn, forms[fn][name], keys[k], shapes, tn)
                    if fn.endswith('workspace_bytes'):          # recorded as slabs: bytes / (batch * M * N * 4)
                        b = forms[fn][name].get('batch', 1)
                        exp = tuple(int(s) * b * M * N * 4 for s, (M, N, K) in zip(want.split(), shapes))
                    else:
                        exp = tuple(int(ch) for ch in want)
                    assert len(exp) == len(shapes)
                    n += len(exp)
                    if got != exp:
                        bad.append((fn, name, keys[k], got, exp))
    assert not bad, bad[:5]
    assert all(L.amdnuwa_get_tuning(k) == 0 for k in range(32))
    return n


def test_nt_queries():
    L = _L()
    assert check_queries(L, NT_QUERIES, FORMS, NT_KEYS, NT_SHAPES, False) == 43500
    assert [int(getattr(L, fn)(None)) for fn in FORMS] == [0, 0, 0, 0]


def test_tn_queries_and_workspace_bytes():
    L = _L()
    assert check_queries(L, TN_QUERIES, TN_FORMS, TN_KEYS, TN_SHAPES, True) == 7812
    assert [int(getattr(L, fn)(None)) for fn in TN_FORMS] == [0, 0, 0]
    assert [L.amdnuwa_linear_ce_workspace_bytes(R, Cc) for R, Cc in CE_WS] == CE_WS_BYTES
