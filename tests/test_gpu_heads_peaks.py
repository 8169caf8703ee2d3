"""Peak heads (csrc/heads.hip h3d_heads_sparse_lists, Plan.FLAGS peak_heads): `hp_offset`, which multi_pose_decode reads at the 17 x K
key-point peaks only, is computed there only, in the same launch as the heads read at the K centres.  Every value is the dense
launch's, bit for bit, so nothing here has a tolerance.  Op level on the 24 x 16 map of tests/test_gpu_heads_sparse.py, the lowering
of each flag setting, and end to end against a detector on the dense path of the default lowering."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
from h3d_amd import _lib, arch, synth
from h3d_amd.detector import PEAK_HEADS, WHOLE_MAP_HEADS, LazyHeads, MultiPoseDetector, Opt
from h3d_amd.model import create_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B0, H0, W0 = 3, 24, 16            # the op-level map: a 96 x 64 input
HW = H0 * W0
CENTRE = ["cam", "hps", "pose", "reg", "shape", "wh"]


def _sd(heads):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(arch.state_dict_shapes(heads, True), seed=0).items()}


def _model(heads, sd, dtype, flags):
    m = create_model("dla_34", heads, 256, False, dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).eval()
    m.engine_flags.update(flags)
    return m


def _desc(op):
    return ctypes.cast(op.in2, ctypes.POINTER(_lib.H3dHeadsDesc)).contents


def _signature(plan):
    """Everything of a plan's op array but the addresses: per op the integer fields, for a heads op the widths of its heads."""
    sig = []
    for op in plan.ops:
        row = [getattr(op, f) for f, t in _lib.H3dOp._fields_ if t is ctypes.c_int32]
        if op.kind == _lib.OP_HEADS:
            d = _desc(op)
            row.append([d.head[i].C for i in range(d.nheads)])
        sig.append(row)
    return sig


def _head_names(plan, op):
    """Names of the heads of a heads op, by the output maps its descriptor points at."""
    at = {t.data_ptr(): h for h, t in plan.outputs.items()}
    d = _desc(op)
    return [at[d.head[i].out] for i in range(d.nheads)]


@functools.lru_cache(maxsize=None)
def _plans(dtype):
    """-> (the plan lowered with split_heads + peak_heads after a dense run, clones of the DEFAULT lowering's maps).  The lowering of
    every flag setting is asserted here, once per dtype."""
    heads = Opt(smpl=True, smpl_cam=True).heads                     # nine heads: widths 1, 2, 34, 2, 17, 2, 72, 10 and cam (3)
    assert len(heads) == 9
    sd = _sd(heads)
    x = torch.from_numpy(synth.synth_images(B0, 4 * H0, 4 * W0)).to(DEV)
    settings = ({}, {"peak_heads": PEAK_HEADS}, {"split_heads": WHOLE_MAP_HEADS}, {"split_heads": WHOLE_MAP_HEADS, "peak_heads": PEAK_HEADS})
    maps, plans = [], []
    for flags in settings:
        m = _model(heads, sd, dtype, flags)
        maps.append({h: t.clone() for h, t in m(x)[-1].items()})
        plans.append(m.engine(torch.device(DEV)).plan(B0, 4 * H0, 4 * W0))
    torch.cuda.synchronize()
    default, peak_only, split, both = plans
    # peak_heads alone: today's lowering
    assert peak_only.n_eager is None and peak_only.sparse_op is None and peak_only.sparse_masks == (0, 0)
    assert _signature(peak_only) == _signature(default)
    # split_heads alone: today's split lowering -- three whole maps in the eager launch, a sparse op without hp_offset
    assert split.sparse_op is not None and split.n_eager == len(split.ops) - 3 and len(split.ops) == len(default.ops) + 1
    assert _head_names(split, split.ops[split.n_eager - 1]) == ["hm", "hm_hp", "hp_offset"]
    assert _head_names(split, split.sparse_op) == ["wh", "hps", "reg", "pose", "shape", "cam"] and split.sparse_masks == (0x3f, 0)
    assert [_head_names(split, op) for op in split.ops[split.n_eager:]] == [["wh", "reg", "shape", "cam"], ["hps"], ["pose"]]
    # both: hp_offset leaves the eager launch for the narrow deferred group and joins the sparse op
    assert both.sparse_op is not None and both.n_eager == len(both.ops) - 3 and len(both.ops) == len(split.ops)
    assert _head_names(both, both.ops[both.n_eager - 1]) == ["hm", "hm_hp"]
    assert _head_names(both, both.sparse_op) == ["wh", "hps", "reg", "hp_offset", "pose", "shape", "cam"] and both.sparse_masks == (0x77, 0x08)
    assert [_head_names(both, op) for op in both.ops[both.n_eager:]] == [["wh", "reg", "hp_offset", "shape", "cam"], ["hps"], ["pose"]]
    assert _signature(both)[:both.n_eager - 1] == _signature(default)[:both.n_eager - 1]       # the backbone
    # run() of every lowering: the default lowering's nine maps
    for got in maps[1:]:
        assert list(got) == list(maps[0])
        for h in heads:
            assert torch.equal(got[h], maps[0][h]), h
    for h in heads:
        assert bool(torch.isfinite(maps[0][h]).all()), h
    return both, maps[0]


def _list(n, seed):
    """[B0][n] positions on the 24 x 16 map: corners, full border rows and columns, interior -- as much as fits n, each image starting
    at another part of the border -- then random positions (repeats: n may exceed the 384 positions of the map)."""
    rs = np.random.RandomState(seed)
    corners = [0, W0 - 1, (H0 - 1) * W0, HW - 1]
    top, bottom = list(range(W0)), list(range((H0 - 1) * W0, HW))
    left, right = [y * W0 for y in range(H0)], [y * W0 + W0 - 1 for y in range(H0)]
    interior = [y * W0 + x for y in range(1, H0 - 1) for x in range(1, W0 - 1)]
    rows = []
    for b, border in enumerate((corners + top + bottom + left + right, bottom + right + corners + top + left, left + corners[::-1] + right + bottom + top)):
        pool = border + list(rs.permutation(interior)[:40]) + list(rs.randint(0, HW, max(n, 1)))
        rows.append(pool[:n])
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def _written(inds):
    m = torch.zeros(B0, HW, dtype=torch.bool, device=DEV)
    m.scatter_(1, inds, True)
    return m.view(B0, 1, H0, W0)


def _check_maps(plan, dense, inds, peak_inds, tag):
    centre, peaks = _written(inds), _written(peak_inds)
    for h, t in plan.outputs.items():
        if h in ("hm", "hm_hp"):                                  # not in the sparse op's descriptor
            assert bool(torch.isnan(t).all()), (tag, h)
            continue
        m = (peaks if h == "hp_offset" else centre).expand_as(t)
        assert torch.equal(t[m], dense[h][m]), (tag, h, int((t[m] != dense[h][m]).sum()))
        assert bool(torch.isnan(t[~m]).all()), (tag, h, "an element outside the list was written")
    assert sorted(set(plan.outputs) - {"hm", "hm_hp", "hp_offset"}) == CENTRE


@pytest.mark.parametrize("K,PK", [(1, 17), (7, 119), (33, 561), (100, 1700)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_list_launch_writes_each_list_s_heads_at_its_positions_and_nothing_else(dtype, K, PK):
    plan, dense = _plans(dtype)
    inds, peak_inds = _list(K, K), _list(PK, 1000 + PK)
    peak_inds[:, -1] = inds[:, 0]                                 # a position in both lists gets both
    if K >= 7:
        both = (_written(inds) & _written(peak_inds)).view(B0, HW)
        for p in (0, W0 - 1, (H0 - 1) * W0, HW - 1):              # the corners are in both lists (of some image)
            assert bool(both[:, p].any()), p
    if K >= 33:
        assert bool(_written(inds).view(B0, H0, W0)[0, 0].all()) and bool(_written(peak_inds).view(B0, H0, W0)[2, :, 0].all())    # a full border row | column
    for t in plan.outputs.values():
        t.fill_(float("nan"))
    plan.run_sparse_lists(inds, K, peak_inds, PK)
    torch.cuda.synchronize()
    _check_maps(plan, dense, inds, peak_inds, (dtype, K, PK))
    for b in range(B0):                                           # ... both: the centre heads AND hp_offset at inds[b, 0]
        p = int(inds[b, 0])
        for h in ("wh", "pose", "hp_offset"):
            assert torch.equal(plan.outputs[h].view(B0, -1, HW)[b, :, p], dense[h].view(B0, -1, HW)[b, :, p]), (h, b)
    # run_sparse keeps its meaning: the centre heads only
    for t in plan.outputs.values():
        t.fill_(float("nan"))
    plan.run_sparse(inds, K)
    torch.cuda.synchronize()
    assert bool(torch.isnan(plan.outputs["hp_offset"]).all())
    _check_maps(plan, dense, inds, torch.zeros(B0, 0, dtype=torch.int64, device=DEV), (dtype, K, "run_sparse"))


def _raw_lists(plan, *lists):
    arr = (_lib.H3dHeadsList * max(len(lists), 1))()
    for e, (inds, K, mask) in zip(arr, lists):
        e.inds, e.K, e.head_mask = inds.data_ptr(), K, mask
    return _lib.lib().h3d_heads_sparse_lists(ctypes.byref(plan.sparse_op), len(lists), arr, _lib.stream_ptr())


def test_entries_outside_the_map_store_nothing_and_the_order_of_the_lists_does_not_matter():
    plan, dense = _plans("bf16")
    inds = torch.tensor([[5, -1, HW], [HW + 7, 9, 1 << 40], [-(1 << 40), 0, 383]], dtype=torch.int64, device=DEV)
    peak_inds = torch.tensor([[-1, 17, HW, 1 << 40, 383], [-(1 << 40), HW, -1, HW + 1, -2], [0, 1 << 40, 5, -(1 << 40), HW]], dtype=torch.int64, device=DEV)
    valid = {"wh": {0: [5], 1: [9], 2: [0, 383]}, "pose": {0: [5], 1: [9], 2: [0, 383]}, "hp_offset": {0: [17, 383], 1: [], 2: [0, 5]}}
    cm, pm = plan.sparse_masks
    for order in (0, 1):
        for t in plan.outputs.values():
            t.fill_(float("nan"))
        if order == 0:
            plan.run_sparse_lists(inds, 3, peak_inds, 5)
        else:                                                     # the peak list first: same launch order (most heads first), same result
            _lib.check(_raw_lists(plan, (peak_inds, 5, pm), (inds, 3, cm)), "h3d_heads_sparse_lists")
        torch.cuda.synchronize()
        for h, per in valid.items():
            t = plan.outputs[h].view(B0, -1, HW)
            for b, pos in per.items():
                assert torch.equal(t[b][:, pos], dense[h].view(B0, -1, HW)[b][:, pos]), (h, b)
            assert int((~torch.isnan(t)).sum()) == sum(len(p) for p in per.values()) * t.shape[1], h
        assert bool(torch.isnan(plan.outputs["hm"]).all()) and bool(torch.isnan(plan.outputs["hm_hp"]).all())


def test_error_returns():
    plan, _ = _plans("bf16")
    inds, peak_inds = _list(7, 7), _list(119, 119)
    cm, pm = plan.sparse_masks
    L = _lib.lib()

    def fails(rc, word):
        assert rc == -5, rc                                       # H3D_ERR_ARG
        assert word in L.h3d_last_error().decode(), L.h3d_last_error()
        with pytest.raises(RuntimeError, match="argument error"):
            _lib.check(rc, "h3d_heads_sparse_lists")

    fails(_raw_lists(plan, (inds, 7, cm), (peak_inds, 119, pm | 1)), "earlier list")          # a head in two masks
    fails(_raw_lists(plan, (inds, 7, cm), (peak_inds, 119, 1 << 7)), "head mask")             # a bit beyond the descriptor's seven heads
    fails(_raw_lists(plan, (inds, 7, cm), (peak_inds, 119, 0)), "head mask")                  # no head at all
    fails(_raw_lists(plan, *[(inds, 7, 1 << i) for i in range(_lib.HEADS_LISTS_MAX + 1)]), "position lists")
    fails(_raw_lists(plan), "position lists")
    assert _raw_lists(plan, (inds, 0, cm)) == -1 and _raw_lists(plan, (inds, (1 << 24) // B0 + 1, cm)) == -1       # H3D_ERR_SHAPE, per list
    with pytest.raises(RuntimeError, match="int64"):
        plan.run_sparse_lists(inds, 7, peak_inds.int(), 119)
    with pytest.raises(RuntimeError, match="int64"):
        plan.run_sparse_lists(inds.int(), 7, peak_inds, 119)
    with pytest.raises(RuntimeError, match="contiguous"):
        plan.run_sparse_lists(inds, 7, _list(238, 1)[:, ::2], 119)
    with pytest.raises(RuntimeError, match="contiguous"):
        plan.run_sparse_lists(inds, 7, peak_inds, 118)             # a shape other than [B, PK]
    # an f32 plan has neither a split nor a sparse op
    heads = Opt(smpl=False).heads
    m32 = _model(heads, _sd(heads), "f32", {"split_heads": WHOLE_MAP_HEADS, "peak_heads": PEAK_HEADS})
    p32 = m32.engine(torch.device(DEV)).plan(B0, 4 * H0, 4 * W0)
    assert p32.sparse_op is None and p32.n_eager is None
    with pytest.raises(RuntimeError, match="peak_heads"):
        p32.run_sparse_lists(inds, 7, peak_inds, 119)
    torch.cuda.synchronize()


CONFIGS = [dict(smpl=True), dict(smpl=False), dict(smpl=True, hm_hp=False, reg_hp_offset=False, reg_offset=False),
           dict(smpl=True, hm_hp=True, reg_hp_offset=False), dict(smpl=True, hm_hp=False, reg_hp_offset=True), dict(smpl=True, dtype="f16", K=20)]


@functools.lru_cache(maxsize=None)
def _detectors(i):
    """-> (a detector as constructed: sparse heads + peak heads; one with the default lowering on the dense path)."""
    kw = dict(dict(dtype="bf16", K=100), **CONFIGS[i])
    sd = _sd(Opt(**kw).heads)
    on, off = MultiPoseDetector(Opt(**kw), sd, device=DEV), MultiPoseDetector(Opt(**kw), sd, device=DEV)
    off.sparse_heads = False
    off.model.engine_flags.clear()
    off.model._engine = None
    return on, off, kw


def _clone(res):
    return {k: (v.clone() if torch.is_tensor(v) else {h: t.clone() for h, t in v.items()}) for k, v in res.items()}


def _same(a, b, smpl):
    for k in ("dets", "inds") + (("verts", "joints") if smpl else ()):
        assert torch.equal(a[k], b[k]), k
    got = dict(a["heads"])
    assert list(got) == list(b["heads"])
    for h, t in b["heads"].items():
        assert torch.equal(got[h], t), h


@pytest.mark.parametrize("size", [(64, 64), (96, 64)])
@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
def test_detector_equals_the_dense_path(cfg, size):
    on, off, kw = _detectors(cfg)
    opt = on.opt
    x = torch.from_numpy(synth.synth_images(2, *size)).to(DEV)
    ref = off.run(x)
    assert type(ref["heads"]) is dict and off.model.engine(torch.device(DEV)).plan(2, *size).sparse_op is None
    plan = on.model.engine(torch.device(DEV)).plan(2, *size)
    assert (plan.sparse_masks[1] != 0) == bool(opt.reg_hp_offset)
    names = [h for h in opt.heads if h not in ("hm", "hm_hp")]
    assert plan.sparse_masks[1] == (1 << names.index("hp_offset") if opt.reg_hp_offset else 0)
    if opt.reg_hp_offset and not opt.hm_hp:
        plan.outputs["hp_offset"].fill_(float("nan"))
    res = on.run(x)
    assert isinstance(res["heads"], LazyHeads) and not res["heads"].complete
    if opt.reg_hp_offset and not opt.hm_hp:                       # no peaks, nothing reads it: the run computed it nowhere
        torch.cuda.synchronize()
        assert bool(torch.isnan(plan.outputs["hp_offset"]).all())
    _same(res, ref, kw["smpl"])
    assert res["heads"].complete
    res = on.run(x)                                               # armed again by the next run
    assert not res["heads"].complete
    _same(res, ref, kw["smpl"])
    torch.cuda.synchronize()


def test_detector_graph_capture_and_two_replays_equal_the_dense_path():
    on, off, kw = _detectors(0)
    x = torch.from_numpy(synth.synth_images(2, 96, 64)).to(DEV)
    xs = [x, torch.flip(x, [0]).contiguous(), torch.flip(x, [3]).contiguous()]
    refs = [_clone(off.run(xi)) for xi in xs]
    for xi, ref in zip(xs, refs):                                 # capture + first replay, then two replays on other batches
        res = on.run(xi, graph=True)
        assert isinstance(res["heads"], LazyHeads) and not res["heads"].complete
        _same(res, ref, True)
        assert res["heads"].complete
    torch.cuda.synchronize()


def test_large_map_fallback_of_the_top_k_yields_the_same_peak_list(monkeypatch):
    """decode._multi_pose_topk takes one `_map_topk` call per tensor instead of the two-tensor launch for maps beyond decode.MAX_LDS_MAP:
    the same hm_inds [B,17,K], the same run."""
    from h3d_amd import decode
    on, off, kw = _detectors(0)
    x = torch.from_numpy(synth.synth_images(2, 96, 64)).to(DEV)
    ref = _clone(off.run(x))
    limit, one_map, two_maps, calls = decode.MAX_LDS_MAP, decode._map_topk, decode._map_topk2, []

    def map_topk(scores, K, flags):                               # (the 24 x 16 map itself still fits the one-workgroup kernel)
        calls.append(1)
        monkeypatch.setattr(decode, "MAX_LDS_MAP", limit)
        try:
            return one_map(scores, K, flags)
        finally:
            monkeypatch.setattr(decode, "MAX_LDS_MAP", 16)

    monkeypatch.setattr(decode, "_map_topk2", lambda *a: calls.append(2) or two_maps(*a))
    monkeypatch.setattr(decode, "_map_topk", map_topk)
    _same(on.run(x), ref, True)
    assert calls == [2]
    monkeypatch.setattr(decode, "MAX_LDS_MAP", 16)                # `_multi_pose_topk` now takes the path of a large map
    _same(on.run(x), ref, True)
    assert calls == [2, 1, 1]
    torch.cuda.synchronize()
