"""Plan.FLAGS fold_upadd on the CPU (the lowering is host code): which H3D_OP_UPADD ops carry H3D_OPF_UPADD_FOLDED, that each stands where
the run loop can take it together with the DeformConv that writes its skip, that nothing else reads that skip, that the flag off is
the default plan, and that every folded pair of the plans the product runs has an exact lattice case in tests/test_gpu_upadd_fold.py."""
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


@pytest.fixture(scope="module")
def builder():
    return dump_plans.Builder()


def _span(plan, ptr):
    """(start, bytes) of the plan buffer that holds `ptr`."""
    for t in plan.keep:
        if hasattr(t, "data_ptr") and t.data_ptr() <= ptr < t.data_ptr() + t.numel() * t.element_size():
            return t.data_ptr(), t.numel() * t.element_size()
    raise AssertionError("pointer 0x%x is in no buffer of the plan" % ptr)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_four_folded_pairs_and_private_skips(builder, B, H, W):
    pw, _ = builder.packer("dla34", "bf16")
    plan = Plan(pw, B, H, W, fold_upadd=True)
    ops = list(plan.op_array)
    folded = [i for i, op in enumerate(ops) if op.kind == _lib.OP_UPADD and op.reserved & _lib.OPF_UPADD_FOLDED]
    assert len(folded) == 4
    assert sum(op.kind == _lib.OP_UPADD for op in ops) == 8
    for i in folded:
        up, node = ops[i], ops[i - 1]
        assert node.kind == _lib.OP_DCN_FUSED_STREAM and node.out == up.in2 and up.in2_cs == node.out_cs
        assert (up.Ho, up.Wo, up.Cin) == (node.H, node.W, node.Cout) == (H // 4, W // 4, 64)
        assert up.out_mode == _lib.OUT_NHWC_F16 and up.reserved == _lib.OPF_UPADD_FOLDED
        # nothing else reads the skip buffer
        lo, n = _span(plan, up.in2)
        assert lo == up.in2
        for j, op in enumerate(ops):
            if op.kind == _lib.OP_HEADS:
                readers = [op.in_]
            else:
                readers = [op.in_] + ([op.in2] if op.kind in (_lib.OP_CONV, _lib.OP_CONV_STREAM, _lib.OP_UPADD, _lib.OP_STEM3) else [])
            for p in readers:
                assert j == i or not (p and lo <= p < lo + n), "op %d also reads the skip of the folded op %d" % (j, i)
            assert j == i - 1 or not (op.out and lo <= op.out < lo + n), "op %d also writes the skip of the folded op %d" % (j, i)
        # the low-resolution map is written by an earlier op (the hoisted proj DeformConv)
        writers = [j for j, op in enumerate(ops) if op.out == up.in_]
        assert len(writers) == 1 and writers[0] < i - 1 and ops[writers[0]].kind == _lib.OP_DCN_FUSED_STREAM
    assert sorted(ops[i].stride for i in folded) == [2, 2, 2, 4]
    # every op still names its kernel; a flagged op answers with the up-sample + add kernel it is without the fold
    buf = ctypes.create_string_buffer(256)
    for i, op in enumerate(ops):
        assert _lib.lib().h3d_op_kernel_name(ctypes.byref(op), buf, 256) == 0, i
        assert buf.value, i
        if i in folded:
            assert buf.value.decode().startswith("upadd_kernel<unsigned short, true"), buf.value
            assert "dcn3_kernel<" in dump_plans.kernel_name(ops[i - 1])


def test_f16_plan_folds_the_same_four(builder):
    pw, _ = builder.packer("dla34", "f16")
    ops = list(Plan(pw, 2, 64, 96, fold_upadd=True).op_array)
    folded = [i for i, op in enumerate(ops) if op.kind == _lib.OP_UPADD and op.reserved & _lib.OPF_UPADD_FOLDED]
    assert len(folded) == 4 and all(ops[i - 1].kind == _lib.OP_DCN_FUSED_STREAM and ops[i - 1].out == ops[i].in2 and ops[i].out_mode == _lib.OUT_NHWC
                                    for i in folded)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("B,H,W", [(64, 512, 512), (32, 512, 512), (16, 512, 512), (8, 512, 512), (2, 64, 96)])
def test_every_folded_pair_of_the_plans_has_a_lattice_case(builder, dtype, B, H, W):
    """What decides the code a folded pair runs -- the producer's kernel, the plan's dtype, f, Cout, the UPADD's out_mode and whether the
    low-resolution map is exactly C wide -- is among the tuples tests/test_gpu_upadd_fold.py's FOLD_CASES dispatch to (the folding twins
    have no name of their own in h3d_op_kernel_name, so the kernel-name coverage tests cannot see them)."""
    import test_gpu_upadd_fold as G
    tested = G.folded_dispatches()
    pw, _ = builder.packer("dla34", dtype)
    ops = list(Plan(pw, B, H, W, fold_upadd=True).op_array)
    folded = [i for i, op in enumerate(ops) if op.kind == _lib.OP_UPADD and op.reserved & _lib.OPF_UPADD_FOLDED]
    assert len(folded) == 4
    for i in folded:
        up = ops[i]
        key = (dump_plans.kernel_name(ops[i - 1]), dtype, up.stride, up.Cout, up.out_mode, up.in_cs == up.Cin)
        assert key in tested, "no lattice case dispatches to the folded pair %s" % (key,)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_flag_off_is_the_default_plan(builder, B, H, W):
    off = builder.plan("dla34", "bf16", B, H, W, fold_upadd=False)
    assert off == builder.plan("dla34", "bf16", B, H, W)
    on = builder.plan("dla34", "bf16", B, H, W, fold_upadd=True)
    # the fold reorders ops and flags four of them, nothing more: the same multiset of ops up to the flag
    key = lambda r: sorted((op["kind"], op["kernel"], op["Cin"], op["Cout"], op["H"], op["W"], op["reserved"] & ~_lib.OPF_UPADD_FOLDED) for op in r["ops"])
    assert key(on) == key(off) and on["outputs"] == off["outputs"]
