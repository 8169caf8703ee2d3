"""The up-sample + skip add folded into the epilogue of the DeformConv that writes its skip (H3D_OPF_UPADD_FOLDED, Plan.FLAGS fold_upadd):
the same bits as the two launches, so nothing here has a tolerance.  Op pair through h3d_run_ops on a 24 x 40 map (partial 16 x 16 tiles in
both directions, border taps on all four sides), the fallback on a tile without the fold, whole plans and the detector."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
from gpu_helpers import DEV, TD, dcn_fused_op, kernel_name, mk, rnd, run
from h3d_amd import _lib, arch, synth
from h3d_amd.detector import MultiPoseDetector, Opt
from h3d_amd.engine import Plan
from h3d_amd.model import create_model

pytestmark = pytest.mark.gpu
B, C, H, W = 2, 64, 24, 40
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def _producer(dtype, reserved, kind=None):
    """A 64 -> 64 fused DeformConv stream op on a [B, 24, 40] map with synthetic filters (offsets of a pixel or two: samples inside the
    apron and in patch slots), as the node DeformConvs of a plan are: fp16 input in a bf16 plan."""
    x = rnd("fold.x", (B, C, H, W), -1.0, 1.0)
    w, b = rnd("fold.w", (C, C, 3, 3), -0.06, 0.06), rnd("fold.b", (C,), -0.2, 0.2)
    wo, bo = rnd("fold.wo", (27, C, 3, 3), -0.03, 0.03), rnd("fold.bo", (27,), -1.0, 1.0)
    return dcn_fused_op(kind or ("stream16" if dtype == "bf16" else "stream"), x, w, b, wo, bo, dtype=dtype, reserved=reserved)


def _pair(dtype, f, reserved_dcn, flag, kind=None):
    """(ops, node output buffer, sum buffer): the producer followed by the H3D_OP_UPADD that adds the f-times up-sampled [B, H/f, W/f] map."""
    built = _producer(dtype, reserved_dcn, kind)
    k = 2 * f
    lo = rnd("fold.lo%d" % f, (B, C, H // f, W // f), -1.0, 1.0).permute(0, 2, 3, 1).contiguous().to(TD[dtype]).to(DEV)
    wup = rnd("fold.up%d" % f, (C, k * k), -0.5, 0.5).t().contiguous().float().to(DEV)          # fp32 [k*k][C]
    node = torch.full((B, H, W, C), SENTINEL, dtype=TD[dtype], device=DEV)
    out = torch.full((B, H, W, C), SENTINEL, dtype=TD[dtype], device=DEV)       # (bf16 plans: holds fp16 bits, compared as bits)
    dcn = mk(built.op.kind, dtype, **{n: getattr(built.op, n) for n, _ in _lib.H3dOp._fields_ if n not in ("kind", "dtype")})
    dcn.out = node.data_ptr()
    up = mk(_lib.OP_UPADD, dtype, in_=lo.data_ptr(), in2=node.data_ptr(), w=wup.data_ptr(), out=out.data_ptr(), B=B, H=H // f, W=W // f, Cin=C,
            in_cs=C, in2_cs=C, Ho=H, Wo=W, Cout=C, out_cs=C, ksize=k, stride=f, out_mode=_lib.OUT_NHWC_F16 if dtype == "bf16" else _lib.OUT_NHWC,
            reserved=_lib.OPF_UPADD_FOLDED if flag else 0)
    return [dcn, up], node, out, (built, lo, wup)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("f", [2, 4])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_folded_pair_gives_the_bits_of_the_two_launches(dtype, f):
    ops, node, want, keep = _pair(dtype, f, 0, False)
    run(ops)
    assert not bool((node == SENTINEL).all()) and bool(torch.isfinite(node.float()).all())
    ops2, node2, got, keep2 = _pair(dtype, f, 0, True)
    name = kernel_name(ops2[0])
    assert name.startswith("dcn3_kernel<") and ", 2, 16, 2, 2, true, 256" in name, name          # the 64-channel patch-slot tile, LDS-transposed epilogue
    assert kernel_name(ops2[1]).startswith("upadd_kernel<")
    run(ops2)
    assert torch.equal(_bits(got), _bits(want)), "%s f=%d: %d vectors differ" % (dtype, f, int((_bits(got) != _bits(want)).any(-1).sum()))
    assert bool((node2 == SENTINEL).all()), "the pair ran as two launches: the DeformConv's own output was written"
    # the timed run loop folds the same pair: its time under the DeformConv op, 0 under the folded one
    got.fill_(SENTINEL)
    arr, ms = (_lib.H3dOp * 2)(*ops2), (ctypes.c_float * 2)()
    _lib.check(_lib.lib().h3d_run_ops_timed(arr, 2, _lib.stream_ptr(), ms), "h3d_run_ops_timed")
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and ms[0] > 0.0 and ms[1] == 0.0


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_flag_is_ignored_on_a_tile_without_the_fold(dtype):
    # H3D_OPF_DCN_STREAM_NO_SLOTS: round 1's tiles have no folding twin (and, in a bf16 plan, no fp16-input option) -- two launches, the same bits
    ops, node, want, keep = _pair(dtype, 2, _lib.OPF_DCN_STREAM_NO_SLOTS, False, kind="stream")
    run(ops)
    ops2, node2, got, keep2 = _pair(dtype, 2, _lib.OPF_DCN_STREAM_NO_SLOTS, True, kind="stream")
    assert ", true, 256" not in kernel_name(ops2[0]), kernel_name(ops2[0])
    run(ops2)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(node2), _bits(node)) and not bool((node2 == SENTINEL).all())


HEADS = Opt(smpl=True).heads


def _sd():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0).items()}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_plan_with_the_fold_gives_the_default_plans_maps(dtype):
    m = create_model("dla_34", HEADS, 256, False, dtype=dtype)
    m.load_state_dict(_sd(), strict=True)
    m.to(DEV).eval()
    pw = m.engine(torch.device(DEV)).pw
    x = torch.from_numpy(synth.synth_images(2, 64, 96, seed=5)).to(DEV)
    res = []
    for flags in ({}, {"fold_upadd": True}):
        plan = Plan(pw, 2, 64, 96, **flags)
        plan.images.copy_(x)
        plan.run()
        torch.cuda.synchronize()
        res.append((plan.feat.buf.clone(), {h: t.clone() for h, t in plan.outputs.items()}, plan))
    assert sum(bool(op.reserved & _lib.OPF_UPADD_FOLDED) for op in res[1][2].ops if op.kind == _lib.OP_UPADD) == 4
    assert bool(torch.isfinite(res[0][0].float()).all()) and float(res[0][0].float().abs().max()) > 0
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])), "feat"
    for h in HEADS:
        assert torch.equal(res[0][1][h], res[1][1][h]), h


def test_detector_with_and_without_the_fold():
    sd = _sd()
    x = torch.from_numpy(synth.synth_images(2, 64, 96, seed=7)).to(DEV)
    out = []
    for fold in (True, False):
        det = MultiPoseDetector(Opt(input_h=64, input_w=96, smpl=True, smpl_people=4, dtype="bf16", K=20), sd, device=torch.device(DEV))
        assert det.model.engine_flags["fold_upadd"] is True
        det.model.engine_flags["fold_upadd"] = fold
        r = det.run(x)
        torch.cuda.synchronize()
        plan = det.model.engine(torch.device(DEV)).plan(2, 64, 96)
        assert sum(bool(op.reserved & _lib.OPF_UPADD_FOLDED) for op in plan.ops if op.kind == _lib.OP_UPADD) == (4 if fold else 0)
        out.append({k: r[k].clone() for k in ("dets", "inds", "verts")})
    for k in ("dets", "inds", "verts"):
        assert torch.equal(out[0][k], out[1][k]), k
