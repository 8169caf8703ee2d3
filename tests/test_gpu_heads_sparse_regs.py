"""Sparse heads with the neighbourhoods in registers (csrc/heads.hip heads_sparse_kernel, the default path of h3d_heads_sparse_lists):
every wave of a workgroup computes 32 positions whose 3x3 x 64-channel neighbourhood it holds as B fragments, and a workgroup runs ONE
head of its list.  Every value is the dense launch's of the same op, bit for bit, on all three paths: the default (8 waves, 256
positions per workgroup), TUNE_HEADS_SPARSE_WAVES4 (128 positions) and TUNE_HEADS_SPARSE_LDS_PATCH (the older kernel: 64 positions,
a list's heads in series).  Op level on two small maps with a feature map of the test's own (tests/heads_sparse_op.py), so nothing
here has a tolerance."""
import ctypes
import functools

import pytest
import torch
import numpy as np

from h3d_amd import _lib
from heads_sparse_op import CENTRE, DEV, NPOS, PATHS, PEAK, SPARSE, Op

pytestmark = pytest.mark.gpu
B0 = 2
MAPS = {"16x32": (16, 32, 64), "20x24": (20, 24, 72)}        # H, W, pixel stride of the feature map (20 x 24: no multiple of any tile)
# list lengths K (entries per image; a launch has B0 K = 2 K entries): 1, around the 32-position N-tile, and for every path's
# workgroup of P = 64 / 128 / 256 positions P - 1, P, P + 1 and 2 P + 1 -- which are also P / 2 - 1 ... P / 2 + 1 of the next P, the
# launches of P - 2, P and P + 2 entries; with the last entry outside the map those have P - 3, P - 1 and P + 1 live entries
LENGTHS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513]


@functools.lru_cache(maxsize=None)
def _op(dtype, name):
    return Op(dtype, B0, *MAPS[name])


def _list(op, K, seed):
    """[B0][K] entries: the four corners, points on each edge, interior, duplicates, and (from 8
    entries per image on) entries below 0 and at or above H W -- as much as fits, each image starting at another part of the border."""
    H, W = op.H, op.W
    HW = H * W
    rs = np.random.RandomState(seed)
    corners = [0, W - 1, (H - 1) * W, HW - 1]
    top, bottom = list(range(1, W - 1, 3)), list(range((H - 1) * W + 2, HW - 1, 3))
    left, right = [y * W for y in range(1, H - 1, 2)], [y * W + W - 1 for y in range(2, H - 1, 2)]
    outside = [-1, HW, HW + 7, -(1 << 40), 1 << 40]
    rows = []
    for b, border in enumerate((corners + top + right + bottom + left, bottom + left + corners[::-1] + right + top)):
        pool = border[:6] + outside[b:b + 2] + border[6:] + [border[0], border[3]] + outside[2:] + list(rs.randint(0, HW, K))
        if K < 8:
            pool = [p for p in pool if 0 <= p < HW]
        rows.append(pool[:K])
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def _bits(maps):
    return {h: t.view(torch.int32) for h, t in maps.items()}


@pytest.mark.parametrize("last", ["inside", "outside"])
@pytest.mark.parametrize("K", LENGTHS)
@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_path_writes_the_dense_bits_at_each_list_s_positions_and_nothing_else(dtype, name, K, last):
    op = _op(dtype, name)
    # a six-head list of 2 K entries in front of a one-head list of another length: the first list's last workgroup is partly empty
    # (or full, or one entry over), its workgroups straddle the two images wherever K is no multiple of the workgroup
    inds, peak_inds = _list(op, K, K), _list(op, LENGTHS[-1 - LENGTHS.index(K)], 1000 + K)
    assert inds.shape == (B0, K)
    peak_inds[:, -1] = inds[:, 0]                                                     # a position in both lists gets both
    if last == "outside":                                                             # the launch's last entry stores nothing: the last LIVE lane is an even one
        inds[-1, -1] = op.H * op.W
        peak_inds[-1, -1] = -1
    lists = [(inds, CENTRE), (peak_inds, PEAK)]
    if K >= 32:
        both = op.written(inds) | op.written(peak_inds)
        for y, x in ((0, 0), (0, op.W - 1), (op.H - 1, 0), (op.H - 1, op.W - 1), (0, 4), (op.H - 1, 5), (3, 0), (4, op.W - 1)):
            assert bool(both[:, 0, y, x].any()), (y, x)                               # corners and every edge are listed
        assert int((inds < 0).sum()) > 0 and int((inds >= op.H * op.W).sum()) > 0
    got = {}
    for path in PATHS:
        got[path] = op.sparse(path, *lists)
        op.check(got[path], lists, (dtype, name, K, last, path))
    # the old path against the new ones, NaN for NaN
    for path in ("regs8", "regs4"):
        for h in SPARSE:
            assert torch.equal(_bits(got[path])[h], _bits(got["lds_patch"])[h]), (path, h)
    # the lists the other way round: the same launch order (most heads first), the same bits
    swapped = op.sparse("regs8", *lists[::-1])
    for h in SPARSE:
        assert torch.equal(_bits(swapped)[h], _bits(got["regs8"])[h]), h


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_how_the_heads_are_split_over_lists_and_workgroups_does_not_change_the_bits(dtype, path):
    op = _op(dtype, "20x24")
    P = NPOS[path]
    a, b, c = _list(op, 2 * P + 1, 1), _list(op, P - 1, 2), _list(op, 33, 3)         # K: launches of 4 P + 2, 2 P - 2 and 66 entries
    b[-1, -1] = -1                                                                    # ... of which b's last is not live
    for lists in ([(a, CENTRE | PEAK)],                                               # one list, all seven heads
                  [(a, 0x15), (b, 0x6a)],                                             # 1 + 3 + 34 channels | 2 + 10 + 72 + 2
                  [(b, 0x20), (a, 0x1f), (c, PEAK)],                                  # the widest head alone, given first
                  [(c, 0x01), (c, 0x02), (b, 0x04), (a, 0x78)]):                      # four lists, two of them the same positions
        op.check(op.sparse(path, *lists), lists, (dtype, path, [hex(m) for _, m in lists]))
    # h3d_heads_sparse: one list, every head
    for t in op.out.values():
        t.fill_(float("nan"))
    op.op.reserved = PATHS[path]
    try:
        _lib.check(_lib.lib().h3d_heads_sparse(ctypes.byref(op.op), a.data_ptr(), a.shape[1], _lib.stream_ptr()), "h3d_heads_sparse")
    finally:
        op.op.reserved = 0
    torch.cuda.synchronize()
    op.check(op.out, [(a, CENTRE | PEAK)], (dtype, path, "h3d_heads_sparse"))


def test_tuning_words():
    op = _op("bf16", "16x32")
    inds = _list(op, 33, 5)
    arr = (_lib.H3dHeadsList * 1)()
    arr[0].inds, arr[0].K, arr[0].head_mask = inds.data_ptr(), inds.shape[1], CENTRE
    L = _lib.lib()
    for word in (_lib.TUNE_HEADS_SEPARATE_BIAS, 1, 0x1000, _lib.TUNE_HEADS_SPARSE_LDS_PATCH | 0x2000):
        op.op.reserved = word
        try:
            assert L.h3d_heads_sparse_lists(ctypes.byref(op.op), 1, arr, _lib.stream_ptr()) == -4, hex(word)      # H3D_ERR_UNSUPPORTED
            assert b"tuning word" in L.h3d_last_error()
        finally:
            op.op.reserved = 0
    # the LDS-patch path wins over the wave count of the register path
    lists = [(inds, CENTRE)]
    op.op.reserved = 0
    for t in op.out.values():
        t.fill_(float("nan"))
    op.op.reserved = _lib.TUNE_HEADS_SPARSE_LDS_PATCH | _lib.TUNE_HEADS_SPARSE_WAVES4
    try:
        _lib.check(L.h3d_heads_sparse_lists(ctypes.byref(op.op), 1, arr, _lib.stream_ptr()), "h3d_heads_sparse_lists")
    finally:
        op.op.reserved = 0
    torch.cuda.synchronize()
    op.check(op.out, lists, "lds_patch | waves4")
