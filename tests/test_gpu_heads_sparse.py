"""Sparse heads (csrc/heads.hip h3d_heads_sparse, detector.MultiPoseDetector.sparse_heads): the heads that decode and the SMPL stage read
at the K detection centres only are computed there only -- and every value is the dense launch's, bit for bit, so nothing here has
a tolerance.  Op level on a 24 x 16 map (edges, corners, list lengths around the 32-position N-tile and the 64-position workgroup),
end to end against a detector on the dense path of the default lowering, and the cases that must stay dense."""
import functools

import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
from h3d_amd import arch, decode, synth
from h3d_amd.detector import WHOLE_MAP_HEADS, CtdetDetector, LazyHeads, MultiPoseDetector, Opt
from h3d_amd.model import create_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B0, H0, W0 = 3, 24, 16            # the op-level map: a 96 x 64 input


def _sd(heads):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(arch.state_dict_shapes(heads, True), seed=0).items()}


@functools.lru_cache(maxsize=None)
def _dense_plan(dtype):
    """-> (split plan after a dense run, clones of its maps).  The maps equal the default lowering's (asserted here, once)."""
    heads = Opt(smpl=True, smpl_cam=True).heads                     # widths 1, 2, 34, 2, 17, 2, 72, 10 and cam (3)
    sd = _sd(heads)
    x = torch.from_numpy(synth.synth_images(B0, 4 * H0, 4 * W0)).to(DEV)
    maps = []
    for flags in ({}, {"split_heads": WHOLE_MAP_HEADS}):
        m = create_model("dla_34", heads, 256, False, dtype=dtype)
        m.load_state_dict(sd, strict=True)
        m.to(DEV).eval()
        m.engine_flags.update(flags)
        out = m(x)[-1]
        maps.append({h: t.clone() for h, t in out.items()})
    torch.cuda.synchronize()
    plan = m.engine(torch.device(DEV)).plan(B0, 4 * H0, 4 * W0)
    assert plan.sparse_op is not None and plan.n_eager == len(plan.ops) - 3
    for h in heads:
        assert torch.equal(maps[0][h], maps[1][h]), h
        assert bool(torch.isfinite(maps[1][h]).all()), h
    return plan, maps[1], m


def _lists(K):
    """[B0][K] positions on the 24 x 16 map: corners, edges, interior, repeats -- whatever fits K."""
    rs = np.random.RandomState(K)
    corners = [0, W0 - 1, (H0 - 1) * W0, H0 * W0 - 1]
    top, bottom = list(range(W0)), list(range((H0 - 1) * W0, H0 * W0))
    left, right = [y * W0 for y in range(H0)], [y * W0 + W0 - 1 for y in range(H0)]
    interior = [y * W0 + x for y in range(1, H0 - 1) for x in range(1, W0 - 1)]
    if K == 1:
        rows = [[corners[0]], [corners[3]], [interior[77]]]
    elif K == 7:
        rows = [corners + [200, 200, 37], [37, 37, 5, 16, 31, 383, 368], corners[::-1] + [100, 101, 116]]     # an index listed twice
    elif K == 32:
        rows = [top + bottom, left + interior[:8], right + interior[-8:]]                # full edge rows / columns
    elif K == 33:
        rows = [left + corners + interior[50:55], top + bottom + [0], right + list(rs.choice(interior, 9, replace=False))]
    else:
        rows = [list(rs.permutation(H0 * W0)[:K]), list(rs.randint(0, H0 * W0, K)), (top + left + bottom + right + interior)[:K]]
    assert all(len(r) == K for r in rows)
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("K", [1, 7, 32, 33, 100])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_sparse_op_writes_the_dense_bits_at_the_listed_positions_and_nothing_else(dtype, K):
    plan, dense, _ = _dense_plan(dtype)
    inds = _lists(K)
    for t in plan.outputs.values():
        t.fill_(float("nan"))
    plan.run_sparse(inds, K)
    torch.cuda.synchronize()
    listed = torch.zeros(B0, H0 * W0, dtype=torch.bool, device=DEV)
    listed.scatter_(1, inds, True)
    listed = listed.view(B0, 1, H0, W0)
    for h, t in plan.outputs.items():
        if h in WHOLE_MAP_HEADS:                                  # not in the sparse op's descriptor
            assert bool(torch.isnan(t).all()), h
            continue
        m = listed.expand_as(t)
        assert torch.equal(t[m], dense[h][m]), (dtype, K, h, int((t[m] != dense[h][m]).sum()))
        assert bool(torch.isnan(t[~m]).all()), (dtype, K, h, "an element outside the list was written")
    assert sorted(set(plan.outputs) - set(WHOLE_MAP_HEADS)) == ["cam", "hps", "pose", "reg", "shape", "wh"]


def test_sparse_op_skips_entries_outside_the_map_and_rejects_other_plans():
    plan, dense, m = _dense_plan("bf16")
    inds = torch.tensor([[5, -1, H0 * W0], [H0 * W0 + 7, 9, 1 << 40], [-(1 << 40), 0, 383]], dtype=torch.int64, device=DEV)
    for t in plan.outputs.values():
        t.fill_(float("nan"))
    plan.run_sparse(inds, 3)
    torch.cuda.synchronize()
    valid = {0: [5], 1: [9], 2: [0, 383]}
    for h in ("wh", "pose"):
        t = plan.outputs[h].view(B0, -1, H0 * W0)
        for b, pos in valid.items():
            assert torch.equal(t[b][:, pos], dense[h].view(B0, -1, H0 * W0)[b][:, pos]), (h, b)
        assert int((~torch.isnan(t)).sum()) == 4 * t.shape[1], h
    with pytest.raises(RuntimeError, match="int64"):
        plan.run_sparse(inds.int(), 3)


@functools.lru_cache(maxsize=None)
def _detectors():
    """-> (a detector as constructed: sparse heads, one with the default lowering on the dense path: what the parent of this change ran)."""
    opt = Opt(smpl=True, dtype="bf16", K=100)
    sd = _sd(opt.heads)
    on = MultiPoseDetector(opt, sd, device=DEV)
    off = MultiPoseDetector(Opt(smpl=True, dtype="bf16", K=100), sd, device=DEV)
    off.sparse_heads = False
    off.model.engine_flags.clear()
    off.model._engine = None
    return on, off


def _same(a, b, heads=True):
    for k in ("dets", "inds", "verts", "joints"):
        assert torch.equal(a[k], b[k]), k
    if heads:
        got = dict(a["heads"])
        assert list(got) == list(b["heads"])
        for h, t in b["heads"].items():
            assert torch.equal(got[h], t), h


@pytest.mark.parametrize("people", [100, 5])
@pytest.mark.parametrize("size", [(64, 64), (96, 64)])
def test_detector_results_and_lazy_heads_equal_the_dense_path(size, people):
    on, off = _detectors()
    on.opt.smpl_people = off.opt.smpl_people = people
    x = torch.from_numpy(synth.synth_images(2, *size)).to(DEV)
    ref = off.run(x)
    assert type(ref["heads"]) is dict and off.model.engine(torch.device(DEV)).plan(2, *size).sparse_op is None
    res = on.run(x)
    assert isinstance(res["heads"], LazyHeads) and not res["heads"].complete
    _same(res, ref, heads=False)                   # before anybody asked for the maps
    _same(res, ref)
    assert res["heads"].complete
    # the same detector with the switch off: dense launches of the split lowering
    on.sparse_heads = False
    try:
        mid = on.run(x)
    finally:
        on.sparse_heads = True
    assert type(mid["heads"]) is dict
    _same(mid, ref)
    # side stream, second plan slot; the maps are completed from the default stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = on.run(x, slot=1)
    got = dict(side["heads"])                      # completed HERE, on the default stream, behind the event the run recorded on its own
    for h, t in ref["heads"].items():
        assert torch.equal(got[h], t), h
    torch.cuda.current_stream().wait_stream(st)    # (the run's other results are ordinary tensors of the side stream)
    _same(side, ref, heads=False)
    torch.cuda.synchronize()


def test_detector_graph_replay_equals_the_dense_path_and_completes_outside_the_graph():
    on, off = _detectors()
    on.opt.smpl_people = off.opt.smpl_people = 100
    x = torch.from_numpy(synth.synth_images(2, 96, 64)).to(DEV)
    x2 = torch.flip(x, [0]).contiguous()
    ref, ref2 = None, None
    ref = {k: (v.clone() if torch.is_tensor(v) else {h: t.clone() for h, t in v.items()}) for k, v in off.run(x).items()}
    ref2 = {k: (v.clone() if torch.is_tensor(v) else {h: t.clone() for h, t in v.items()}) for k, v in off.run(x2).items()}
    res = on.run(x, graph=True)                    # capture + first replay
    assert isinstance(res["heads"], LazyHeads) and not res["heads"].complete
    _same(res, ref)
    res = on.run(x2, graph=True)                   # replay on another batch: the maps are incomplete again
    assert not res["heads"].complete
    _same(res, ref2)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kw", [dict(smpl=False), dict(smpl=False, hm_hp=False, reg_hp_offset=False, reg_offset=False), dict(smpl=True, dtype="f16", K=20)])
def test_detector_with_other_head_sets_equals_the_dense_path(kw):
    """No SMPL heads; `hm` the only map read whole (no key-point maps, no offsets); the f16 plan with K = 20."""
    kw = dict(dict(dtype="bf16", K=100), **kw)
    sd = _sd(Opt(**kw).heads)
    on, off = MultiPoseDetector(Opt(**kw), sd, device=DEV), MultiPoseDetector(Opt(**kw), sd, device=DEV)
    off.sparse_heads = False
    off.model.engine_flags.clear()
    x = torch.from_numpy(synth.synth_images(2, 96, 64)).to(DEV)
    res, ref = on.run(x), off.run(x)
    assert isinstance(res["heads"], LazyHeads) and type(ref["heads"]) is dict
    for k in ("dets", "inds") + (("verts", "joints") if kw["smpl"] else ()):
        assert torch.equal(res[k], ref[k]), k
    for h, t in ref["heads"].items():
        assert torch.equal(res["heads"][h], t), h


def test_flip_test_f32_and_ctdet_stay_on_the_dense_path():
    on, off = _detectors()
    on.opt.smpl_people = off.opt.smpl_people = 5
    x = torch.from_numpy(synth.synth_images(2, 64, 64)).to(DEV)
    on.opt.flip_test = off.opt.flip_test = True
    try:
        a, b = on.run(x), off.run(x)
    finally:
        on.opt.flip_test = off.opt.flip_test = False
    assert type(a["heads"]) is dict
    _same(a, b)
    # f32: the default lowering, the model's own forward + the public decode
    o32 = Opt(smpl=False, dtype="f32", K=100)
    d32 = MultiPoseDetector(o32, _sd(o32.heads), device=DEV)
    r = d32.run(x)
    assert type(r["heads"]) is dict and not d32.model.engine_flags
    assert d32.model.engine(torch.device(DEV)).plan(2, 64, 64).n_eager is None
    out = {h: t.clone() for h, t in d32.model(x)[-1].items()}
    dets = decode.multi_pose_decode_logits(out["hm"], out["wh"], out["hps"], reg=out["reg"], hm_hp=out["hm_hp"], hp_offset=out["hp_offset"], K=100)
    assert torch.equal(r["dets"], dets) and all(torch.equal(r["heads"][h], out[h]) for h in out)
    # ctdet
    oc = Opt(task="ctdet", dtype="bf16", K=100)
    dc = CtdetDetector(oc, _sd(oc.heads), device=DEV)
    rc = dc.run(x)
    assert type(rc["heads"]) is dict and dc.model.engine(torch.device(DEV)).plan(2, 64, 64).n_eager is None
    outc = {h: t.clone() for h, t in dc.model(x)[-1].items()}
    from h3d_amd.utils import _sigmoid
    assert torch.equal(rc["dets"], decode.ctdet_decode(_sigmoid(outc["hm"].clone()), outc["wh"], reg=outc["reg"], K=100))
