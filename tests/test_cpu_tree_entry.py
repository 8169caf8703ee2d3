"""Plan.FLAGS fold_tree_entry on the CPU (the lowering is host code): which ops carry H3D_OPF_TREE_ENTRY -- the max-pool, the `project` conv and the
stride-2 conv1 at the entry of levels 2 to 5, next to each other and in this order, with the pointer identities the run loop asks for --, that
level 2's pooled map is private and its conv1 moves to the one-slot 64-channel tile of csrc/conv2.hip, that the flag off is the default plan, that
share_pool=False flags nothing, and that every flagged triple dispatches to a tile tests/test_gpu_tree_entry.py covers."""
import ctypes
import importlib.util
import os

import pytest

from h3d_amd import _lib
from h3d_amd.engine import Plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location("dump_plans", os.path.join(ROOT, "tools", "dump_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dump_plans = _load_tool()
SHAPES = [(2, 64, 96), (64, 512, 512)]
FLAG, PRIVATE = _lib.OPF_TREE_ENTRY, _lib.OPF_TREE_ENTRY_PRIVATE_POOL
LEVELS = [(32, 64, 4), (64, 128, 8), (128, 256, 16), (256, 512, 32)]       # (Cin, Cout, down-sampling of the output) of levels 2, 3, 4, 5
ONE_SLOT_64 = _lib.TUNE_CONV_STREAM_TILE(4, 2, 4)


@pytest.fixture(scope="module")
def builder():
    return dump_plans.Builder()


def _flagged(ops):
    return [i for i, op in enumerate(ops) if op.kind in (_lib.OP_MAXPOOL, _lib.OP_CONV, _lib.OP_CONV_STREAM) and op.reserved & (FLAG | PRIVATE)]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_four_flagged_triples_with_the_pointer_identities(builder, dtype, B, H, W):
    pw, _ = builder.packer("dla34", dtype)
    plan = Plan(pw, B, H, W, fold_tree_entry=True)
    ops = list(plan.op_array)
    flagged = _flagged(ops)
    pools = [i for i in flagged if ops[i].kind == _lib.OP_MAXPOOL]
    assert len(pools) == 4 and flagged == sorted(j for i in pools for j in (i, i + 1, i + 2))
    assert sum(op.kind == _lib.OP_MAXPOOL for op in ops) == 4
    buf = ctypes.create_string_buffer(256)
    for i, (cin, cout, f) in zip(pools, LEVELS):
        pool, proj, conv = ops[i:i + 3]
        assert (pool.kind, proj.kind, conv.kind) == (_lib.OP_MAXPOOL, _lib.OP_CONV, _lib.OP_CONV_STREAM)
        private = cout == 64                    # level 2: nothing but `project` reads the pooled map; from level 3 on Root reads it too
        assert pool.reserved == (FLAG | PRIVATE if private else FLAG) and proj.reserved == FLAG
        assert conv.reserved == (FLAG | ONE_SLOT_64 if cout < 128 else FLAG)
        # the 1x1 conv reads exactly what the pool writes, the 3x3 conv exactly what the pool reads
        assert (proj.in_, proj.in_cs, proj.Cin) == (pool.out, pool.out_cs, pool.Cout) and pool.out
        assert (conv.in_, conv.in_cs, conv.Cin) == (pool.in_, pool.in_cs, pool.Cin) and pool.in_
        assert (pool.Cin, conv.Cout, proj.Cout) == (cin, cout, cout)
        assert (pool.H, pool.W) == (conv.H, conv.W) == (2 * H // f, 2 * W // f) and pool.H % 2 == 0 and pool.W % 2 == 0
        assert (pool.Ho, pool.Wo) == (conv.Ho, conv.Wo) == (proj.H, proj.W) == (proj.Ho, proj.Wo) == (H // f, W // f)
        assert (conv.ksize, conv.stride, proj.ksize, proj.stride) == (3, 2, 1, 1)
        assert not proj.in2 and proj.relu == 0 and conv.relu == 1 and proj.out_mode == conv.out_mode == _lib.OUT_NHWC
        # the pooled map lives in Root's concat buffer, or is private: then no other op of the plan touches its buffer
        if private:
            lo, n = pool.out, B * pool.Ho * pool.Wo * pool.out_cs * 2
            assert pool.out_cs == pool.Cout
            for j, op in enumerate(ops):
                ptrs = [op.in_, op.out] + ([op.in2] if op.kind in (_lib.OP_CONV, _lib.OP_CONV_STREAM, _lib.OP_UPADD, _lib.OP_STEM3) else [])
                assert j in (i, i + 1) or not any(p and lo <= p < lo + n for p in ptrs), "op %d also touches the private pooled map" % j
        else:
            assert pool.out_cs > pool.Cout
        # the project result is the residual of the block's second conv
        assert ops[i + 3].kind == _lib.OP_CONV_STREAM and ops[i + 3].in_ == conv.out and ops[i + 3].in2 == proj.out
        # a single op still names the kernel it is without the fold
        names = []
        for op in (pool, proj, conv):
            assert _lib.lib().h3d_op_kernel_name(ctypes.byref(op), buf, 256) == 0
            names.append(buf.value.decode())
        assert names[0].startswith("maxpool_kernel<") and (names[1].startswith("conv_kernel<") or names[1].startswith("gemm1_kernel<"))
        t = "f16_t" if dtype == "f16" else "unsigned short"
        assert names[2] == "conv2_kernel<%s, %d, 4, 2, 2, 1, 1>" % (t, 4 if cout >= 128 else 2), names[2]     # a one-slot tile, LDS-transposed epilogue: the tiles with the fused twin


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_flag_off_is_the_default_plan_and_on_changes_the_flag_words_and_level_2s_conv1(builder, B, H, W):
    off = builder.plan("dla34", "bf16", B, H, W, fold_tree_entry=False)
    assert off == builder.plan("dla34", "bf16", B, H, W)
    on = builder.plan("dla34", "bf16", B, H, W, fold_tree_entry=True)
    assert len(on["ops"]) == len(off["ops"]) and on["outputs"] == off["outputs"]
    changed = [i for i, (a, b) in enumerate(zip(on["ops"], off["ops"])) if a != b]
    assert len(changed) == 12
    moved = []
    for i in changed:
        a, b = dict(on["ops"][i]), dict(off["ops"][i])
        assert a.pop("reserved") & FLAG and b.pop("reserved") == 0
        if a != b:              # level 2's conv1: from csrc/conv.hip to csrc/conv2.hip (another filter pack, another kernel), the same maps
            moved.append(i)
            assert (b["kind"], a["kind"], a["Cin"], a["Cout"]) == (_lib.OP_CONV, _lib.OP_CONV_STREAM, 32, 64)
            assert b["kernel"].startswith("conv_kernel<unsigned short, 3, 2,") and a["kernel"] == "conv2_kernel<unsigned short, 2, 4, 2, 2, 1, 1>"
            for k in a:
                assert a[k] == b[k] or k in ("kind", "kernel", "w", "bias"), k
    assert len(moved) == 1


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_share_pool_off_flags_nothing(builder, dtype):
    pw, _ = builder.packer("dla34", dtype)
    assert not _flagged(list(Plan(pw, 2, 64, 96, fold_tree_entry=True, share_pool=False).op_array))


@pytest.mark.parametrize("dtype", ["f32", "f16x3"])
def test_other_arithmetics_flag_nothing(builder, dtype):
    pw, _ = builder.packer("dla34", dtype)
    assert not _flagged(list(Plan(pw, 2, 64, 96, fold_tree_entry=True).op_array))


def test_other_backbones_are_untouched(builder):
    for arch_name, shape in (("hourglass", (1, 128, 128)), ("resdcn101", (1, 64, 64))):
        assert builder.plan(arch_name, "bf16", *shape, fold_tree_entry=True) == builder.plan(arch_name, "bf16", *shape)
