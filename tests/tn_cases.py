"""The committed cases of the weight-gradient GEMMs (b4c_gemm_tn, b4c_gemm_tn_seg, b4c_gemm_tn_group; csrc/gemm.hip, the TN part),
each with the form of the family it is there to reach.  No tests here: tests/test_tn_plan_cpu.py asks the library for the split
count of every case and asserts the class below (so a change of the split rule that empties a class fails there, without a GPU),
tests/test_gpu_weight_grad.py runs them.

How a launch is shaped (tn_plan / tn_group_plan): the M token rows are cut into `nsplit` chunks, every 128 x 128 output tile gets one
workgroup per chunk.  The class of a case is its nsplit:

    'one'     nsplit == 1         the workgroup adds its tile to dW itself (TN_DIRECT), no workspace, no reduction
    'narrow'  2 <= nsplit <= 16   partial tiles through the workspace (TN_WS) or float atomics (TN_ATOMIC); the reduction runs in its
                                  64-blocks-per-tile shape (16 partitions of the splits)
    'wide'    17 <= nsplit <= 64  the 256-blocks-per-tile shape (64 partitions), one trip of its split loop
    'trips'   nsplit > 64         the same with more than one trip of the split loop (and of the column sums' loop)

A grouped launch orders its workgroups by XCD ('swizzled') when nsplit % 8 == 0 and linearly otherwise.
"""
CLASSES = ('one', 'narrow', 'wide', 'trips')


def split_class(nsplit):
    return 'one' if nsplit == 1 else 'narrow' if nsplit <= 16 else 'wide' if nsplit <= 64 else 'trips'


# (M, K, N, dtype, pitch, class, what the case reaches).  pitch 'pad8': operand pitches rounded up to a multiple of 8 (for bf16 the
# 16-byte kernel); 'tight': pitches K and N (here even and no multiple of 8: for bf16 the generic kernel).
SINGLE = [
    (256, 128, 128, 'bf16', 'pad8', 'one', 'TN_DIRECT, one full tile'),
    (257, 128, 128, 'bf16', 'pad8', 'narrow', 'the smallest split: 2 chunks, the second holds one row'),
    (128, 104, 312, 'f32', 'pad8', 'one', 'fp32 TN_DIRECT, 3 x 104 segments'),
    (129, 104, 312, 'f32', 'pad8', 'narrow', 'fp32, narrow reduction'),
    (1000, 104, 312, 'bf16', 'pad8', 'narrow', 'narrow reduction, segments that straddle the 128-column tiles'),
    (4200, 104, 312, 'bf16', 'pad8', 'wide', 'wide reduction, straddling segments'),
    (2100, 104, 312, 'f32', 'pad8', 'wide', 'fp32, wide reduction'),
    (16448, 128, 128, 'bf16', 'pad8', 'trips', '65 splits: the second trip of the split loop holds one element'),
    (70001, 104, 128, 'bf16', 'pad8', 'trips', 'several trips, ragged last chunk'),
    (33000, 128, 128, 'f32', 'pad8', 'trips', 'fp32, several trips'),
    (9000, 256, 768, 'bf16', 'pad8', 'wide', 'two row tiles (the second carries no column sums), six column tiles'),
    (300, 128, 24576, 'bf16', 'pad8', 'one', '192 tiles: one split whatever M is'),
    (50, 8, 264, 'bf16', 'pad8', 'one', 'tiny K, N past two tiles'),
    (50, 8, 264, 'f32', 'pad8', 'one', 'tiny K, N past two tiles'),
    (37, 6, 10, 'f32', 'tight', 'one', 'K, N no multiples of 8'),
    (37, 6, 10, 'bf16', 'tight', 'one', 'K, N no multiples of 8, pitches 6 / 10: even only, the generic bf16 kernel'),
    (37, 6, 10, 'bf16', 'pad8', 'one', 'K, N no multiples of 8 under 16-byte loads (pitches 8 / 16)'),
]
# number of column segments the segmented variants use (N -> n_seg); 4 x 192 straddles every other tile edge
SEGMENTS = {312: 3, 768: 4}
# the cases of the real-valued test
REAL = [(257, 128, 128, 'bf16'), (4200, 104, 312, 'bf16'), (16448, 128, 128, 'bf16'), (70001, 104, 128, 'bf16'), (33000, 128, 128, 'f32'),
        (9000, 256, 768, 'bf16')]

_LAYER = [(104, 128, 1), (128, 104, 1), (128, 128, 1), (128, 384, 3)]
# (M, [(K, N, n_seg)], class, tile order, what the case reaches)
GROUP = [
    (200, _LAYER, 'one', 'linear', 'TN_DIRECT in the group'),
    (1500, _LAYER, 'narrow', 'linear', 'linear tile order (nsplit % 8 != 0), narrow reduction'),
    (1800, _LAYER, 'narrow', 'swizzled', 'XCD tile order, narrow reduction'),
    (2049, _LAYER, 'narrow', 'linear', 'the t == 8 fallback of tn_group_plan, whose chunk rounding leaves 7 splits'),
    (40000, [(128, 128, 1), (104, 104, 1)], 'wide', 'swizzled', 'XCD order, wide reduction behind the group block walk'),
    (70001, _LAYER, 'wide', 'swizzled', 'wide, ragged last chunk'),
    (6144, [(256, 768, 3), (256, 256, 1), (256, 256, 1)], 'wide', 'swizzled', 'more than 8 tiles (target 512), two row tiles'),
    (8192, [(104, 104, 1)] * 8, 'wide', 'swizzled', 'eight problems (TN_GROUP_MAX)'),
    (4100, [(104, 312, 3), (104, 104, 1)], 'narrow', 'swizzled', 'segments that straddle the tiles, in the group'),
]
GROUP_REAL = GROUP[8]


def dt_code(L, dtype):
    return {'bf16': L.BF16, 'f32': L.F32}[dtype]


def single_tiles(K, N):
    return (K + 127) // 128, (N + 127) // 128


def single_nsplit(L, M, K, N, dtype):
    """The split count of b4c_gemm_tn(_seg) for this shape, from the library's own workspace size: nsplit * (tk tn 16384 + tn 128)
    floats, 0 bytes for one split.  L: bert4clickpath_amd._lib."""
    tk, tn = single_tiles(K, N)
    need = int(L.lib().b4c_gemm_tn_workspace_bytes(M, K, N, dt_code(L, dtype)))
    per = (tk * tn * 16384 + tn * 128) * 4
    assert need % per == 0, (need, per)
    return need // per if need else 1


def group_descs(L, probs):
    """A TNDesc array that carries the shapes only (what the workspace size looks at)."""
    descs = (L.TNDesc * len(probs))()
    for d, (K, N, n_seg) in zip(descs, probs):
        d.K, d.n_seg, d.seg_width = K, n_seg, N // n_seg
    return descs


def group_tiles(probs):
    return sum(tk * tn for tk, tn in (single_tiles(K, N) for K, N, _ in probs))


def group_nsplit(L, M, probs):
    """The split count of b4c_gemm_tn_group (which always goes through the workspace, also with one split)."""
    need = int(L.lib().b4c_gemm_tn_group_workspace_bytes(group_descs(L, probs), len(probs), M))
    per = sum(tk * tn * 16384 + tn * 128 for tk, tn in (single_tiles(K, N) for K, N, _ in probs)) * 4
    assert need > 0 and need % per == 0, (need, per)
    return need // per


def case_id(c):
    return '%dx%dx%d-%s-%s' % c[:5]


def group_id(c):
    return '%d-%dprob-%dtiles' % (c[0], len(c[1]), group_tiles(c[1]))

