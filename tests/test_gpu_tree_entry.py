"""The entry of a DLA Tree as one launch (H3D_OPF_TREE_ENTRY, Plan.FLAGS fold_tree_entry): the 2x2 max-pool of x, the 1x1 `project` conv of the
pooled map and the 3x3 stride-2 conv of x, through h3d_run_ops, against the same three ops with the flag cleared.  The MFMA chains, the
maximum and the fp32 epilogues are the same sequences, so every comparison is torch.equal on the stored bits: nothing here has a tolerance.
B = 2 on a 24 x 40 input: a 12 x 20 output with partial 8 x 16 tiles in both directions.  Integer-lattice operands (tests/lattice_ref.py)
are also compared with the fp64 reference rounded where the kernels round."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import h3d_amd  # noqa: F401
import lattice_ref as L
from gpu_helpers import DEV, TD, fake_pw, from_nhwc, kernel_name, mk, pack_conv, rnd, run
from h3d_amd import _lib, arch, synth
from h3d_amd.detector import MultiPoseDetector, Opt
from h3d_amd.engine import Plan
from h3d_amd.model import create_model

pytestmark = pytest.mark.gpu
B, H, W = 2, 24, 40
SENTINEL = 7.0
FLAG, PRIVATE = _lib.OPF_TREE_ENTRY, _lib.OPF_TREE_ENTRY_PRIVATE_POOL
CHANNELS = [(64, 128), (128, 256), (32, 64)]   # one channel block; two: the pooled map is written once, project computed per block; level 2: the 64-channel tile
ONE_SLOT_64 = _lib.TUNE_CONV_STREAM_TILE(4, 2, 4)      # ... which the conv op asks for by its tuning code (the launcher's own choice below 128 channels has two slots)
LAYOUTS = ["slice", "private"]              # the pooled map in a channel slice of a wider buffer (offset 8, stride C + 24) | marked private


def _bits(t):
    return t.view(torch.int16)


@functools.lru_cache(maxsize=None)
def _operands(ci, co, h, real):
    """(x, w3, b3, w1, b1), NCHW fp32 on the host.  real: values that round in every product, with negative values, both zeros in one pool
    window (in both orders), one NaN and one Inf."""
    if not real:
        x, w3, b3 = L.lattice_x((B, ci, h, W), key="te.x"), L.lattice_w((co, ci, 3, 3), key="te.w3"), L.lattice_bias(co, key="te.b3")
        return x, w3, b3, L.lattice_w((co, ci, 1, 1), key="te.w1"), L.lattice_bias(co, key="te.b1")
    x = rnd("te.rx", (B, ci, h, W), -1.0, 1.0).clone()
    x[0, 7, 8:10, 8:10] = torch.tensor([[-0.0, 0.0], [-0.5, -0.25]])
    x[0, 9, 8:10, 8:10] = torch.tensor([[0.0, -0.0], [-0.5, -0.25]])
    x[1, 11, 2:4, 30:32] = torch.tensor([[-0.75, -0.0], [-0.0, -1.0]])
    x[0, 3, 4, 6] = float("nan")
    x[1, 5, 11, 33] = float("inf")
    return (x, rnd("te.rw3", (co, ci, 3, 3), -0.06, 0.06), rnd("te.rb3", (co,), -0.2, 0.2), rnd("te.rw1", (co, ci, 1, 1), -0.12, 0.12),
            rnd("te.rb1", (co,), -0.2, 0.2))


class Triple:
    """[H3D_OP_MAXPOOL, 1x1 H3D_OP_CONV, 3x3 stride-2 H3D_OP_CONV_STREAM] over one input, on sentinel-filled output buffers."""

    def __init__(self, dtype, ci, co, layout="slice", h=H, real=False):
        x, w3, b3, w1, b1 = _operands(ci, co, h, real)
        self.dtype, self.ci, self.co, self.layout = dtype, ci, co, layout
        ho, wo = h // 2, W // 2
        self.x = x.permute(0, 2, 3, 1).contiguous().to(TD[dtype]).to(DEV)
        pw = fake_pw({"w": w3, "b": b3}, dtype)
        wimg, bp3, cout, cin, rows3 = pw.conv_stream("w", "b")
        wp1, bp1, _, rows1 = pack_conv(w1, b1, dtype)
        self.pool_cs, self.pool_off = ci + 24, 8
        self.pooled = torch.empty(B, ho, wo, self.pool_cs, dtype=TD[dtype], device=DEV)
        self.res = torch.empty(B, ho, wo, co, dtype=TD[dtype], device=DEV)
        self.t = torch.empty(B, (h - 1) // 2 + 1, wo, co, dtype=TD[dtype], device=DEV)
        self.keep = (pw, wimg, bp3, wp1, bp1)
        pptr = self.pooled.data_ptr() + 2 * self.pool_off
        self.pool = mk(_lib.OP_MAXPOOL, dtype, in_=self.x.data_ptr(), out=pptr, B=B, H=h, W=W, Cin=ci, in_cs=ci, Ho=ho, Wo=wo, Cout=ci,
                       out_cs=self.pool_cs, ksize=2, stride=2)
        self.proj = mk(_lib.OP_CONV, dtype, in_=pptr, w=wp1.data_ptr(), bias=bp1.data_ptr(), out=self.res.data_ptr(), B=B, H=ho, W=wo, Cin=ci,
                       in_cs=self.pool_cs, Ho=ho, Wo=wo, Cout=co, out_cs=co, ksize=1, stride=1, relu=0, out_mode=_lib.OUT_NHWC, wrows=rows1)
        self.conv = mk(_lib.OP_CONV_STREAM, dtype, in_=self.x.data_ptr(), w=wimg.data_ptr(), bias=bp3.data_ptr(), out=self.t.data_ptr(), B=B, H=h, W=W,
                       Cin=ci, in_cs=ci, Ho=(h - 1) // 2 + 1, Wo=wo, Cout=co, out_cs=co, ksize=3, stride=2, relu=1, out_mode=_lib.OUT_NHWC, wrows=rows3)
        self.reset()

    def reset(self):
        for t in (self.pooled, self.res, self.t):
            t.fill_(SENTINEL)

    def ops(self, flag=True):
        self.pool.reserved = (FLAG | (PRIVATE if self.layout == "private" else 0)) if flag else 0
        self.proj.reserved = FLAG if flag else 0
        self.conv.reserved = (FLAG if flag else 0) | (ONE_SLOT_64 if self.co < 128 else 0)
        return [self.pool, self.proj, self.conv]

    def outputs(self):
        return {"pooled": self.pooled.clone(), "project": self.res.clone(), "conv": self.t.clone()}

    def pooled_untouched(self):
        return bool((self.pooled == SENTINEL).all())

    def pooled_outside_untouched(self):
        live = torch.zeros(self.pool_cs, dtype=torch.bool, device=DEV)
        live[self.pool_off:self.pool_off + self.ci] = True
        return bool((self.pooled[..., ~live] == SENTINEL).all())


def run_timed(ops):
    arr, ms = (_lib.H3dOp * len(ops))(*ops), (ctypes.c_float * len(ops))()
    _lib.check(_lib.lib().h3d_run_ops_timed(arr, len(ops), _lib.stream_ptr(), ms), "h3d_run_ops_timed")
    torch.cuda.synchronize()
    return list(ms)


def _same_bits(got, want, what, skip=()):
    for k in want:
        if k not in skip:
            n = int((_bits(got[k]) != _bits(want[k])).any(-1).sum())
            assert n == 0, "%s: %d pixels of `%s` differ from the three launches" % (what, n, k)


def _check_fused(tr, want, what):
    """The flagged triple through both run loops: one launch (0 ms under the two convs), the bits of the three launches in every output."""
    for timed in (False, True):
        tr.reset()
        ms = run_timed(tr.ops(True)) if timed else run(tr.ops(True))
        got = tr.outputs()
        assert ms is None or (ms[0] > 0.0 and ms[1] == 0.0 and ms[2] == 0.0), (what, ms)
        if tr.layout == "private":
            assert tr.pooled_untouched(), what + ": a pooled map marked private was written"
            _same_bits(got, want, what, skip=("pooled",))
        else:
            assert tr.pooled_outside_untouched(), what + ": written outside the pooled map's channel slice"
            _same_bits(got, want, what)
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ci,co", CHANNELS)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fused_triple_on_the_lattice(dtype, ci, co, layout):
    from test_gpu_lattice import assert_exact
    tr = Triple(dtype, ci, co, layout)
    t = "f16_t" if dtype == "f16" else "unsigned short"
    tr.ops(True)
    assert kernel_name(tr.conv) == "conv2_kernel<%s, %d, 4, 2, 2, 1, 1>" % (t, 4 if co >= 128 else 2) and kernel_name(tr.pool).startswith("maxpool_kernel<")
    what = "%s %d -> %d %s" % (dtype, ci, co, layout)
    run(tr.ops(False))
    want = tr.outputs()
    assert not tr.pooled_untouched() and tr.pooled_outside_untouched()
    # the three launches against the fp64 reference, rounded once where the kernels round
    x, w3, b3, w1, b1 = _operands(ci, co, H, False)
    pooled = F.max_pool2d(x, 2)
    assert_exact(from_nhwc(want["pooled"], ci, tr.pool_off), pooled, what + ": pooled map")
    assert_exact(from_nhwc(want["conv"], co), L.exact_conv(x, w3, b3, 2, 1, True, None, dtype), what + ": conv")
    assert_exact(from_nhwc(want["project"], co), L.exact_conv(pooled, w1, b1, 1, 0, False, None, dtype), what + ": project")
    _check_fused(tr, want, what)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ci,co", CHANNELS)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fused_triple_on_real_operands_with_zeros_nan_and_inf(dtype, ci, co, layout):
    tr = Triple(dtype, ci, co, layout, real=True)
    run(tr.ops(False))
    want = tr.outputs()
    pooled = want["pooled"][..., tr.pool_off:tr.pool_off + ci].float()
    # the operands do what they are there for: fmaxf drops the NaN (the window's other three decide), the Inf is pooled (fp16 stores
    # saturate), both zeros meet in a window
    x = _operands(ci, co, H, True)[0]
    assert not bool(torch.isnan(pooled).any())
    assert float(pooled[0, 2, 3, 3]) == float(torch.stack([x[0, 3, 4, 7], x[0, 3, 5, 6], x[0, 3, 5, 7]]).max().to(TD[dtype]))
    assert float(pooled[1, 5, 16, 5]) == (65504.0 if dtype == "f16" else float("inf"))
    assert float(pooled[0, 4, 4, 7]) == 0.0 and float(pooled[0, 4, 4, 9]) == 0.0 and float(pooled[1, 1, 15, 11]) == 0.0
    assert float(pooled.min()) < -0.5
    _check_fused(tr, want, "%s %d -> %d %s, real operands" % (dtype, ci, co, layout))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_odd_height_is_not_admitted_and_gives_the_three_launches(dtype):
    tr = Triple(dtype, 64, 128, "slice", h=23, real=True)         # the pool drops the last row, the conv does not: 11 and 12 output rows
    assert tr.pool.Ho == 11 and tr.conv.Ho == 12
    run(tr.ops(False))
    want = tr.outputs()
    for timed in (False, True):
        tr.reset()
        ms = run_timed(tr.ops(True)) if timed else run(tr.ops(True))
        _same_bits(tr.outputs(), want, "odd H, " + dtype)
        assert ms is None or all(t > 0.0 for t in ms), ms


@pytest.mark.parametrize("case", ["unflagged_conv", "other_pooled_map", "relu_on_project", "pool_last", "two_ops", "two_slot_64"])
def test_flagged_triples_the_run_loop_must_not_fuse(case):
    """Whatever breaks the structure runs as separate launches (a time under every op) and gives their bits."""
    tr = Triple("bf16", 32, 64, "slice", real=True) if case == "two_slot_64" else Triple("bf16", 64, 128, "slice", real=True)
    keep = None
    if case in ("other_pooled_map", "pool_last"):  # the 1x1 conv reads a copy of the pooled map, not the pool's `out`
        run(tr.ops(False))
        keep = tr.pooled.clone()
        tr.proj.in_ = keep.data_ptr() + 2 * tr.pool_off
    if case == "relu_on_project":
        tr.proj.relu = 1

    def ops(flag):
        pool, proj, conv = tr.ops(flag)
        if case == "unflagged_conv":
            conv.reserved = 0
        if case == "two_slot_64":                  # 64 channels without the one-slot code: the launcher's two-slot tile has no fused twin
            conv.reserved &= ~ONE_SLOT_64
        return [proj, conv, pool] if case == "pool_last" else [pool, proj] if case == "two_ops" else [pool, proj, conv]

    tr.reset()
    run(ops(False))
    want = tr.outputs()
    tr.reset()
    ms = run_timed(ops(True))
    _same_bits(tr.outputs(), want, case)
    assert all(t > 0.0 for t in ms), (case, ms)


HEADS = Opt(smpl=True).heads


def _sd():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0).items()}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_plan_with_the_fused_entries_gives_the_default_plans_maps(dtype):
    m = create_model("dla_34", HEADS, 256, False, dtype=dtype)
    m.load_state_dict(_sd(), strict=True)
    m.to(DEV).eval()
    pw = m.engine(torch.device(DEV)).pw
    x = torch.from_numpy(synth.synth_images(2, 64, 96, seed=5)).to(DEV)
    res = []
    for flags in ({}, {"fold_tree_entry": True}):
        plan = Plan(pw, 2, 64, 96, **flags)
        plan.images.copy_(x)
        plan.run()
        torch.cuda.synchronize()
        res.append((plan.feat.buf.clone(), {h: t.clone() for h, t in plan.outputs.items()}, plan))
    on = res[1][2]
    assert sum(bool(op.reserved & FLAG) for op in on.ops) == 12
    # the flagged triples ran as one launch each: the timed loop books nothing under their convs
    ms = run_timed(list(on.op_array))
    pools = [i for i, op in enumerate(on.ops) if op.kind == _lib.OP_MAXPOOL and op.reserved & FLAG]
    assert len(pools) == 4 and all(ms[i] > 0.0 and ms[i + 1] == 0.0 and ms[i + 2] == 0.0 for i in pools), [ms[i:i + 3] for i in pools]
    assert bool(torch.isfinite(res[0][0].float()).all()) and float(res[0][0].float().abs().max()) > 0
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])), "feat"
    for h in HEADS:
        assert torch.equal(res[0][1][h], res[1][1][h]), h


def test_detector_with_and_without_the_fused_entries():
    sd = _sd()
    x = torch.from_numpy(synth.synth_images(2, 64, 96, seed=7)).to(DEV)
    out = []
    for fold in (True, False):
        det = MultiPoseDetector(Opt(input_h=64, input_w=96, smpl=True, smpl_people=4, dtype="bf16", K=20), sd, device=torch.device(DEV))
        assert det.model.engine_flags["fold_tree_entry"] is True
        det.model.engine_flags["fold_tree_entry"] = fold
        r = det.run(x)
        torch.cuda.synchronize()
        plan = det.model.engine(torch.device(DEV)).plan(2, 64, 96)
        assert sum(bool(op.reserved & FLAG) for op in plan.ops) == (12 if fold else 0)
        out.append({k: r[k].clone() for k in ("dets", "inds", "verts")})
    for k in ("dets", "inds", "verts"):
        assert torch.equal(out[0][k], out[1][k]), k
