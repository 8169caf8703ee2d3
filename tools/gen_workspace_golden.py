"""Writes tests/golden/workspace_bytes.json: what every workspace-size entry point of libh3d_hip.so answers for a table of shapes.
tests/test_cpu_host.py asserts the table, so a change of a workspace layout shows up as a diff of this file.  Needs no GPU.

    python tools/gen_workspace_golden.py
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import h3d_amd  # noqa: E402,F401
from h3d_amd import _lib, losses  # noqa: E402

# (B, C, H, W, Cout): the DeformConv layers of DLA-34 at 512 x 512 (batch 1 and 64), small maps, C % 16 != 0, Cout % 128 != 0
DCN = [(1, 64, 128, 128, 64), (64, 64, 128, 128, 64), (1, 128, 64, 64, 64), (64, 128, 64, 64, 128), (1, 256, 32, 32, 128),
       (64, 256, 32, 32, 256), (1, 512, 16, 16, 256), (64, 512, 16, 16, 256), (2, 64, 10, 12, 64), (1, 16, 32, 32, 8),
       (1, 4, 23, 23, 4), (1, 64, 23, 23, 200), (3, 32, 17, 19, 130)]
MODEL_GEO = (3, 3, 1, 1, 1, 1, 1, 1, 1)       # kernel, stride, pad, dilation (h, w each), deformable_group
# other configurations: the general kernels (5 x 5 stride 2, dilation 2, two deformable groups, 1 x 1)
DCN_BWD = [s + MODEL_GEO for s in DCN] + [(2, 8, 20, 24, 12, 5, 5, 2, 2, 2, 2, 1, 1, 1), (1, 16, 32, 32, 8, 3, 3, 1, 1, 2, 2, 2, 2, 1),
                                          (2, 32, 15, 15, 40, 3, 3, 1, 1, 1, 1, 1, 1, 2), (1, 64, 64, 64, 1100, 3, 3, 1, 1, 1, 1, 1, 1, 1),
                                          (4, 64, 9, 9, 64, 1, 1, 1, 1, 0, 0, 1, 1, 1)]
POSE_HEADS = [1, 2, 34, 2, 17, 2]
# (B, H, W, head_conv, channels per head): 1 split (64 pixels), 2 unequal splits (529), the model's maps, the split maximum
HEADS = [(1, 8, 8, 64, [2]), (1, 23, 23, 64, [2]), (1, 16, 32, 64, [1, 96]), (2, 20, 24, 128, [3]), (1, 128, 128, 256, POSE_HEADS),
         (64, 128, 128, 256, POSE_HEADS), (1, 128, 128, 64, [80, 2, 2]), (3, 33, 31, 192, [17]), (1, 1, 1, 64, []), (16, 128, 128, 256, [1]),
         (1, 64, 64, 256, POSE_HEADS), (1, 23, 22, 256, [5, 7])]
# (P, V, Vpad, nnz, want_verts): the SMPL body (6890 vertices) and the tests' small bodies
SMPL = [(1, 6890, 6912, 4, 1), (4, 6890, 6912, 4, 1), (64, 6890, 6912, 4, 1), (2048, 6890, 6912, 4, 1), (3, 100, 128, 4, 1),
        (3, 100, 128, 4, 0), (0, 100, 128, 4, 1), (5, 128, 128, 1, 1), (33, 300, 384, 2, 1), (257, 6890, 6912, 4, 1), (1, 1, 128, 1, 1),
        (100, 6890, 7040, 4, 1)]
# (B, C, H, W, K): one band, two bands (the 320 x 184 map of a 1280 x 736 frame), many bands
NMS = [(1, 1, 128, 128, 100), (64, 17, 128, 128, 100), (1, 1, 320, 184, 100), (2, 17, 320, 184, 100), (1, 80, 320, 184, 100),
       (1, 1, 512, 512, 20), (4, 3, 1000, 36, 7), (1, 1, 193, 192, 1024), (1, 2, 2000, 1000, 50), (1, 1, 3, 12288, 5),
       (1, 1, 4, 4, 2), (3, 5, 600, 600, 128)]
# (B, max_objs, num_joints)
TARGETS = [(1, 32, 17), (64, 32, 17), (1, 128, 0), (64, 128, 0), (0, 32, 17), (2, 1, 1), (16, 32, 17), (3, 7, 5), (1, 0, 17), (128, 128, 17),
           (1, 1, 0), (5, 100, 17)]
# terms (kind, flags, n | B, C, HW, M): the multi_pose and ctdet losses at batch 1 and 64, single terms around the block caps
F, R, G8 = losses.FOCAL, losses.REG_L1, losses.TUNE_GRID8


def _pose_terms(B, HW=128 * 128, M=32):
    return [(F, 1, B * HW), (F, 1, B * 17 * HW), (losses.REG_WEIGHTED_L1, 0, B, 34, HW, M), (R, 0, B, 2, HW, M), (R, 0, B, 2, HW, M),
            (R, 0, B, 2, HW, M * 17)]


LOSS = [_pose_terms(1), _pose_terms(64), [(F, 1, 80 * 128 * 128), (R, 0, 1, 2, 128 * 128, 128), (R, 0, 1, 2, 128 * 128, 128)],
        [(F, 1, 64 * 80 * 128 * 128), (losses.NORM_REG_L1, 0, 64, 2, 128 * 128, 128), (losses.REG_SL1, 0, 64, 2, 128 * 128, 128)],
        [], [(F, 0, 1)], [(F, 0, 1024)], [(F, 0, 1025)], [(F, G8, 1 << 24)], [(R, 0, 1, 1, 16, 1)], [(R, G8, 8, 34, 1024, 4096)],
        [(F, 0, 1 << 30)] * 16]


def loss_term_array(terms):
    arr = (losses.H3dLossTerm * max(len(terms), 1))()
    for c, t in zip(arr, terms):
        c.kind, c.flags = t[0], t[1]
        c.x = c.gt = c.ind = c.mask = 256                     # (sizes only: nothing is read through the pointers)
        if t[0] == F:
            c.n = t[2]
        else:
            c.B, c.C, c.HW, c.M = t[2:]
    return arr


def by_pointer(fn, *args):
    n = ctypes.c_size_t(0)
    _lib.check(fn(*args, ctypes.byref(n)), fn.__name__)
    return n.value


def table():
    L = _lib.lib()
    t = {}
    t["h3d_dcn_v2_workspace_bytes"] = [[list(s), L.h3d_dcn_v2_workspace_bytes(*s)] for s in DCN]
    t["h3d_dcn_v2_packed_workspace_bytes"] = [[list(s[:4]) + [f], L.h3d_dcn_v2_packed_workspace_bytes(*s[:4], f)]
                                              for s in DCN for f in (0, _lib.DCN_INPUT_NHWC)]
    t["h3d_dcn_v2_packed_weight_bytes"] = [[[s[4], s[1], d], L.h3d_dcn_v2_packed_weight_bytes(s[4], s[1], d)]
                                           for s in DCN for d in (_lib.H3D_F32, _lib.H3D_BF16)]
    t["h3d_dcn_v2_backward_workspace_bytes"] = [[list(s), by_pointer(L.h3d_dcn_v2_backward_workspace_bytes, *s)] for s in DCN_BWD]
    t["h3d_heads_backward_workspace_bytes"] = [
        [list(s), by_pointer(L.h3d_heads_backward_workspace_bytes, *s[:4], len(s[4]), (ctypes.c_int * max(len(s[4]), 1))(*s[4]))] for s in HEADS]
    t["h3d_smpl_backward_workspace_bytes"] = [[list(s), by_pointer(L.h3d_smpl_backward_workspace_bytes, *s)] for s in SMPL]
    t["h3d_nms_topk_large_workspace_bytes"] = [[list(s), L.h3d_nms_topk_large_workspace_bytes(*s)] for s in NMS]
    t["h3d_targets_workspace_bytes"] = [[list(s), by_pointer(L.h3d_targets_workspace_bytes, *s)] for s in TARGETS]
    t["h3d_loss_workspace_bytes"] = [[[list(x) for x in s], by_pointer(L.h3d_loss_workspace_bytes, loss_term_array(s), len(s))] for s in LOSS]
    return t


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": [\n%s\n ]' % (k, ",\n".join("  " + json.dumps(r) for r in rows)) for k, rows in table().items()) + "\n}\n")
    print(path)
