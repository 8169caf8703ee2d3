"""The up-sample + skip add folded into the epilogue of the DeformConv that writes its skip (H3D_OPF_UPADD_FOLDED, Plan.FLAGS fold_upadd):
the same bits as the two launches, so nothing here has a tolerance.  Op pair through h3d_run_ops on a 24 x 40 map (partial 16 x 16 tiles in
both directions, border taps on all four sides), the fallback on a tile without the fold, whole plans and the detector.

The second half compares the fold with an INDEPENDENT reference: integer-lattice operands (tests/lattice_ref.py `fold_operands`), the fp64
result rounded where the kernel rounds (`exact_fold`), over what h3d_launch_dcn3_fold admits -- FOLD_CASES, exported as data for
tests/test_oracle_upadd_fold.py (the conditions of a zero tolerance) and tests/test_cpu_upadd_fold.py (the plans' folded pairs all
dispatch to a tuple of this table) --, the pairs that must NOT fold, and the run loop's pairing."""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
import lattice_ref as L
from gpu_helpers import DEV, TD, dcn_fused_op, from_nhwc, kernel_name, mk, rnd, run
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


# ---- exact lattice tests over what h3d_launch_dcn3_fold admits ------------------------------------------------------------------------
# mode -> (plan dtype, dcn_fused_op kind, the UPADD's out_mode, type the node value is rounded to, type the sum is stored in)
MODES = {"b16": ("bf16", "stream16", _lib.OUT_NHWC_F16, torch.bfloat16, torch.float16),        # as the bf16 plan has it: fp16 in, fp16 out
         "bb": ("bf16", "stream", _lib.OUT_NHWC, torch.bfloat16, torch.bfloat16),
         "f16": ("f16", "stream", _lib.OUT_NHWC, torch.float16, torch.float16)}
# name, producer (B, Ci, Co, H, W), f, producer's reserved, (channel stride, channel offset) of the low-resolution map and of the output
# inside wider buffers (None: exactly C wide), modes, and whether the launcher must take the pair as one launch
FoldCase = collections.namedtuple("FoldCase", "name shape f reserved lo out modes folds")
ROW_16MIB = 1 << 20            # channel stride at which an 8-pixel row of 2-byte values is 16 MiB: the bound of the tail's 24-bit multiplies
FOLD_CASES = [
    FoldCase("f2", (2, 64, 64, 24, 40), 2, 0, None, None, ("b16", "bb", "f16"), True),
    FoldCase("f4", (2, 64, 64, 24, 40), 4, 0, None, None, ("b16", "bb", "f16"), True),
    FoldCase("f8", (2, 64, 64, 24, 40), 8, 0, None, None, ("b16", "bb", "f16"), True),
    FoldCase("lo_1x3", (1, 64, 64, 8, 24), 8, 0, None, None, ("b16", "f16"), True),                 # a map below one tile, one low-resolution row
    FoldCase("lo_1x1", (1, 64, 64, 4, 4), 4, 0, None, None, ("b16", "f16"), True),                  # one low-resolution pixel: three of four taps invalid everywhere
    FoldCase("lo_1x8", (3, 64, 64, 2, 16), 2, 0, None, None, ("b16", "f16"), True),
    FoldCase("co128", (2, 64, 128, 24, 40), 4, 0, None, None, ("b16", "f16"), True),                # small grid: 64-channel workgroups, grid.y = 2, cout0 = 64
    FoldCase("co256", (1, 64, 256, 16, 16), 2, 0, None, None, ("b16", "f16"), True),                # grid.y = 4
    FoldCase("co48", (2, 64, 48, 24, 40), 2, 0, None, None, ("bb", "f16"), True),                   # the last two 16-byte slots of a pixel are dead
    FoldCase("wide_margin", (2, 64, 64, 40, 24), 2, _lib.OPF_DCN_STREAM_WIDE_MARGIN, None, None, ("b16", "f16"), True),      # the packed-apron tiles
    FoldCase("slots512", (2, 64, 64, 40, 24), 2, _lib.OPF_DCN_STREAM_SLOTS512, None, None, ("b16", "f16"), True),
    FoldCase("strided", (2, 64, 64, 24, 40), 4, 0, (80, 8), (96, 16), ("b16",), True),
    FoldCase("row_below_16MiB", (1, 64, 64, 6, 16), 2, 0, (ROW_16MIB - 8, 0), None, ("b16",), True),      # iy0 * row bytes > 2^24, row bytes < 2^24
    FoldCase("row_16MiB", (1, 64, 64, 6, 16), 2, 0, (ROW_16MIB, 0), None, ("b16",), False),          # the launcher's bound: two launches
    # producers whose tile has no folding twin: the flag is ignored
    FoldCase("co32", (1, 64, 32, 8, 24), 2, 0, None, None, ("bb", "f16"), False),                    # MT = 1
    FoldCase("wide_wg", (1, 128, 128, 24, 40), 2, _lib.TUNE_DCN_STREAM_FORCE_WIDE_WG, None, None, ("b16", "f16"), False),    # MT = 4
    FoldCase("ci48", (1, 48, 64, 8, 24), 2, 0, None, None, ("bb", "f16"), False),                    # Cin % 32: the tiles without patch slots
]
FOLD_BY_NAME = {c.name: c for c in FOLD_CASES}
SAME_BITS_CASES = ("f8", "co128", "wide_margin", "slots512", "strided")       # ... also with real-valued operands against the two launches
_PTR = 0x10000                  # a non-null, 16-byte aligned stand-in for a dry run (h3d_op_kernel_name launches nothing)


def fold_case_params():
    return [pytest.param(c.name, m, id="%s-%s" % (c.name, m)) for c in FOLD_CASES for m in c.modes]


def producer_name(case, mode):
    """The kernel the case's producer dispatches to, from the op's integer fields alone (no device needed)."""
    plan, kind = MODES[mode][:2]
    Bn, Ci, Co, Hn, Wn = case.shape
    op = mk(_lib.OP_DCN_FUSED_STREAM, plan, in_=_PTR, in2=_PTR, w=_PTR, bias=_PTR, out=_PTR, B=Bn, H=Hn, W=Wn, Cin=Ci, in_cs=Ci, Ho=Hn, Wo=Wn, Cout=Co,
            out_cs=Co, ksize=3, stride=1, relu=1, out_mode=_lib.OUT_NHWC, wrows=(Co + 127) // 128 * 128,
            reserved=case.reserved | (_lib.OPF_DCN_STREAM_F16_INPUT if kind == "stream16" else 0))
    return kernel_name(op)


def fold_dispatch(case, mode):
    """What decides the code a folded pair runs: (producer kernel, plan dtype, f, Cout, the UPADD's out_mode, low-resolution map exactly C wide)."""
    return (producer_name(case, mode), MODES[mode][0], case.f, case.shape[2], MODES[mode][2], case.lo is None)


def folded_dispatches():
    return {fold_dispatch(c, m) for c in FOLD_CASES if c.folds for m in c.modes}


@functools.lru_cache(maxsize=None)
def _rnd_operands(shape, f):
    Bn, Ci, Co, Hn, Wn = shape
    return (rnd("fold.x", (Bn, Ci, Hn, Wn), -1.0, 1.0), rnd("fold.w", (Co, Ci, 3, 3), -0.06, 0.06), rnd("fold.b", (Co,), -0.2, 0.2),
            rnd("fold.wo", (27, Ci, 3, 3), -0.03, 0.03), rnd("fold.bo", (27,), -1.0, 1.0),
            rnd("fold.lo%d" % f, (Bn, Co, Hn // f, Wn // f), -1.0, 1.0), rnd("fold.up%d" % f, (Co, 1, 2 * f, 2 * f), -0.5, 0.5))


@functools.lru_cache(maxsize=None)
def _built_producer(shape, kind, plan, reserved, real):
    x, w, b, wo, bo = (_rnd_operands(shape, 2) if real else L.dcn_operands(*shape))[:5]
    return dcn_fused_op(kind, x, w, b, wo, bo, dtype=plan, reserved=reserved)


class Pair:
    """The producer and the H3D_OP_UPADD that adds the f-times up-sampled low-resolution map to its output, on sentinel-filled buffers."""

    def __init__(self, case, mode, real=False):
        plan, kind, out_mode, node_t, out_t = MODES[mode]
        Bn, Ci, Co, Hn, Wn = case.shape
        f = case.f
        k, h, w = 2 * f, Hn // f, Wn // f
        self.case, self.mode, self.C = case, mode, Co
        x_lo, w_up = (_rnd_operands(case.shape, f) if real else L.fold_operands(*case.shape, f))[5:]
        built = _built_producer(case.shape, kind, plan, case.reserved, real)
        assert built.op.out_cs == Co and built.name == producer_name(case, mode), (built.name, producer_name(case, mode))
        in_cs, in_off = case.lo or (Co, 0)
        self.out_cs, self.out_off = case.out or (Co, 0)
        self.lo = torch.zeros(Bn, h, w, in_cs, dtype=TD[plan], device=DEV)
        self.lo[..., in_off:in_off + Co] = x_lo.permute(0, 2, 3, 1).to(TD[plan]).to(DEV)
        self.wup = w_up.reshape(Co, k * k).t().contiguous().float().to(DEV)                                  # fp32 [k*k][C]
        self.node = torch.empty(Bn, Hn, Wn, Co, dtype=node_t, device=DEV)
        self.out = torch.empty(Bn, Hn, Wn, self.out_cs, dtype=out_t, device=DEV)
        self.dcn = mk(built.op.kind, plan, **{n: getattr(built.op, n) for n, _ in _lib.H3dOp._fields_ if n not in ("kind", "dtype")})
        self.dcn.out = self.node.data_ptr()
        self.up = mk(_lib.OP_UPADD, plan, in_=self.lo.data_ptr() + 2 * in_off, in2=self.node.data_ptr(), w=self.wup.data_ptr(),
                     out=self.out.data_ptr() + 2 * self.out_off, B=Bn, H=h, W=w, Cin=Co, in_cs=in_cs, in2_cs=Co, Ho=Hn, Wo=Wn, Cout=Co,
                     out_cs=self.out_cs, ksize=k, stride=f, out_mode=out_mode, reserved=_lib.OPF_UPADD_FOLDED)
        self.keep = built
        self.reset()

    def reset(self):
        self.node.fill_(SENTINEL)
        self.out.fill_(SENTINEL)

    def ops(self, flag=True):
        self.up.reserved = _lib.OPF_UPADD_FOLDED if flag else 0
        return [self.dcn, self.up]

    def result(self):
        """The sum as NCHW fp32 on the host; every element of the output buffer outside the C live channels of a pixel is still the sentinel."""
        live = torch.zeros(self.out_cs, dtype=torch.bool, device=DEV)
        live[self.out_off:self.out_off + self.C] = True
        assert bool((self.out[..., ~live] == SENTINEL).all()), "%s %s: written outside the output's channels" % (self.case.name, self.mode)
        return from_nhwc(self.out, self.C, self.out_off)

    def node_result(self):
        return from_nhwc(self.node, self.C)

    def node_untouched(self):
        return bool((self.node == SENTINEL).all())


def run_timed(ops):
    arr, ms = (_lib.H3dOp * len(ops))(*ops), (ctypes.c_float * len(ops))()
    _lib.check(_lib.lib().h3d_run_ops_timed(arr, len(ops), _lib.stream_ptr(), ms), "h3d_run_ops_timed")
    torch.cuda.synchronize()
    return list(ms)


def _exact(case, mode):
    """(the pair's exact output, the exact node value), NCHW fp32."""
    node_t, out_t = MODES[mode][3:]
    x_lo, w_up = L.fold_operands(*case.shape, case.f)[5:]
    pre = L.fold_pre(*case.shape)
    return L.exact_fold(x_lo, w_up, pre, case.f, node_t, out_t), L.fold_node(pre, node_t)


@pytest.mark.parametrize("name,mode", fold_case_params())
def test_fold_lattice(name, mode):
    """With the flag: one launch where the case must fold (node buffer untouched, 0 ms under the folded op), two where it must not (node
    written, a time under both ops); without the flag two launches.  Every output equals the fp64 reference rounded where the kernels round."""
    from test_gpu_lattice import assert_exact
    case = FOLD_BY_NAME[name]
    want, node_want = _exact(case, mode)
    pair = Pair(case, mode)
    what = "%s %s (%s)" % (name, mode, pair.keep.name)
    for timed in (False, True):
        pair.reset()
        ms = run_timed(pair.ops(True)) if timed else run(pair.ops(True))
        assert_exact(pair.result(), want, what + (", flagged, timed loop" if timed else ", flagged"))
        if case.folds:
            assert pair.node_untouched(), what + ": the pair ran as two launches"
            assert ms is None or (ms[0] > 0.0 and ms[1] == 0.0), ms
        else:
            assert_exact(pair.node_result(), node_want, what + ": node of the fallback")
            assert ms is None or (ms[0] > 0.0 and ms[1] > 0.0), ms
    pair.reset()
    run(pair.ops(False))
    assert_exact(pair.result(), want, what + ", two launches")
    assert_exact(pair.node_result(), node_want, what + ": node")


@pytest.mark.parametrize("name,mode", [(n, m) for n in SAME_BITS_CASES for m in FOLD_BY_NAME[n].modes])
def test_fold_same_bits_as_the_two_launches_on_real_operands(name, mode):
    """Real-valued operands round in every fma: a fold whose tap order or contraction differs from upadd_kernel's shows here, not on the lattice."""
    pair = Pair(FOLD_BY_NAME[name], mode, real=True)
    run(pair.ops(False))
    want, node = pair.out.clone(), pair.node.clone()
    assert not pair.node_untouched() and bool(torch.isfinite(node.float()).all()) and bool(torch.isfinite(pair.result()).all())
    pair.reset()
    run(pair.ops(True))
    assert pair.node_untouched()
    assert torch.equal(_bits(pair.out), _bits(want)), "%s %s: %d vectors differ" % (name, mode, int((_bits(pair.out) != _bits(want)).any(-1).sum()))


# ---- the run loop's pairing ---------------------------------------------------------------------------------------------------------------
def _skip_buffer(pair, node_want):
    """A skip filled by the host with the exact node value: what a flagged UPADD reads when its `in2` is not the producer's `out`."""
    skip = node_want.permute(0, 2, 3, 1).contiguous().to(pair.node.dtype).to(DEV)
    pair.up.in2 = skip.data_ptr()
    return skip


@pytest.mark.parametrize("mode", ["b16", "f16"])
@pytest.mark.parametrize("layout", ["copy_between", "other_skip", "upadd_first"])
def test_flagged_upadd_that_the_run_loop_must_not_pair(layout, mode):
    from test_gpu_lattice import assert_exact
    case = FOLD_BY_NAME["f2"]
    want, node_want = _exact(case, mode)
    pair = Pair(case, mode)
    dcn, up = pair.ops(True)
    keep = None
    if layout == "copy_between":                   # an op of an unrelated buffer between the two
        src = torch.arange(2 * 4 * 4 * 8, dtype=torch.float32).view(2, 4, 4, 8).to(TD[MODES[mode][0]]).to(DEV)
        dst = torch.zeros_like(src)
        keep = (src, dst)
        copy = mk(_lib.OP_COPY, MODES[mode][0], in_=src.data_ptr(), out=dst.data_ptr(), B=2, H=4, W=4, Cin=8, in_cs=8, Ho=4, Wo=4, Cout=8, out_cs=8,
                  ksize=1, stride=1)
        ops, i_dcn, i_up = [dcn, copy, up], 0, 2
    elif layout == "other_skip":                   # in2 is a separately filled skip, not the producer's out
        keep = _skip_buffer(pair, node_want)
        ops, i_dcn, i_up = [dcn, up], 0, 1
    else:                                          # the flagged op at index 0: nothing in front of it to pair with
        keep = _skip_buffer(pair, node_want)
        ops, i_dcn, i_up = [up, dcn], 1, 0
    for timed in (False, True):
        pair.reset()
        ms = run_timed(ops) if timed else run(ops)
        assert_exact(pair.result(), want, "%s %s%s" % (layout, mode, ", timed loop" if timed else ""))
        assert_exact(pair.node_result(), node_want, "%s %s: node" % (layout, mode))
        assert ms is None or all(t > 0.0 for t in ms), ms
    if layout == "copy_between":
        assert torch.equal(keep[0], keep[1])


@pytest.mark.parametrize("what", ["f16_plan_f16out", "Ho_not_H_times_f"])
def test_pair_its_own_launcher_refuses_fails_the_same_with_and_without_the_flag(what):
    """What the UPADD asks beyond the fold is left to its own launcher, which owns the message: same return code, same text, `out` untouched."""
    pair = Pair(FOLD_BY_NAME["f2"], "f16")
    if what == "f16_plan_f16out":
        pair.up.out_mode = _lib.OUT_NHWC_F16       # an option of bf16 plans only
    else:
        pair.up.H -= 1                             # Ho = 24 is no longer H * f
    seen = []
    for flag in (True, False):
        for timed in (False, True):
            pair.reset()
            ops = pair.ops(flag)
            arr, ms = (_lib.H3dOp * 2)(*ops), (ctypes.c_float * 2)()
            rc = (_lib.lib().h3d_run_ops_timed(arr, 2, _lib.stream_ptr(), ms) if timed else _lib.lib().h3d_run_ops(arr, 2, _lib.stream_ptr()))
            torch.cuda.synchronize()
            seen.append((rc, _lib.lib().h3d_last_error().decode()))
            assert rc != 0 and bool((pair.out == SENTINEL).all()), (what, flag, timed, rc)
    assert len(set(seen)) == 1 and "op 1 (kind %d): upadd: " % _lib.OP_UPADD in seen[0][1], seen


@pytest.mark.parametrize("mode", ["b16", "bb", "f16"])
def test_two_folded_pairs_back_to_back(mode):
    """[dcnA, upA, dcnB, upB] with dcnB reading upA's output: two launches, the chain of references, ms = [> 0, 0, > 0, 0]."""
    from test_gpu_lattice import assert_exact
    plan, kind, out_mode, node_t, out_t = MODES[mode]
    case_a, case_b = FOLD_BY_NAME["f2"], FOLD_BY_NAME["f4"]
    Bn, Ci, Co, Hn, Wn = case_a.shape
    assert case_b.shape == case_a.shape and Ci == Co
    a, b = Pair(case_a, mode), Pair(case_b, mode)
    wb, bb, wob, bob = L.fold_chain_operands(Co, Co)
    built = dcn_fused_op(kind, torch.zeros(Bn, Co, Hn, Wn), wb, bb, wob, bob, dtype=plan)
    assert built.name == producer_name(case_b, mode)
    for n, _ in _lib.H3dOp._fields_:
        if n not in ("kind", "dtype", "in_", "out"):
            setattr(b.dcn, n, getattr(built.op, n))
    b.dcn.in_ = a.out.data_ptr()                   # (the stored type of upA's sum is the input type of this mode's producer)
    want_a = _exact(case_a, mode)[0]
    pre_b = L.dcn_pre(want_a, wb, bb, wob, bob)
    assert torch.equal(pre_b * 8, (pre_b * 8).round()) and float(pre_b.abs().max()) < 2.0 ** 18
    x_lo, w_up = L.fold_operands(*case_b.shape, case_b.f)[5:]
    want_b = L.exact_fold(x_lo, w_up, pre_b, case_b.f, node_t, out_t)
    ops = a.ops(True) + b.ops(True)
    for timed in (False, True):
        a.reset(), b.reset()
        ms = run_timed(ops) if timed else run(ops)
        assert_exact(a.result(), want_a, "first pair, " + mode)
        assert_exact(b.result(), want_b, "second pair, " + mode)
        assert a.node_untouched() and b.node_untouched()
        assert ms is None or (ms[0] > 0.0 and ms[1] == 0.0 and ms[2] > 0.0 and ms[3] == 0.0), ms
