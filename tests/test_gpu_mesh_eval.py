"""GPU: csrc/mesh_eval.hip (`h3d_pointset_errors`, `h3d_metric_means`) and h3d_amd/mesh_eval.py against the numpy mirror
mesh_eval.evaluate_numpy, which tests/test_oracle_mesh_eval.py holds to the loop restatement of include/h3d.h section 8b and to LAPACK.

Bit-equal, nothing excluded: err, count and transform, compared as the int64 views of the doubles.  That rests on fp64 + - * / and sqrt
being correctly rounded on the device and on -ffp-contract=off, as csrc/targets.hip and csrc/eval.hip already do."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import mesh_eval_cases as cases
from gpu_helpers import DEV
from h3d_amd import arch, coco_eval as C, decode, mesh_eval as ME, model, smpl, synth, trainer
from h3d_amd.detector import multi_pose_post_process

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def run(c, root, want_transform=True):
    return ME.pointset_errors(dev(c["pred"]), dev(c["gt"]), dev(c["pred_idx"]), dev(c["gt_idx"]), dev(c["weight"]), dev(c["pred_root"]),
                              dev(c["gt_root"]), root, want_transform=want_transform)


def check(c, root):
    """One case on the device against the mirror, twice (two calls, the same bits) -> the mirror's (err, count, transform)."""
    want = ME.evaluate_numpy(c["pred"], c["gt"], c["pred_idx"], c["gt_idx"], c["weight"], c["pred_root"], c["gt_root"], root)
    first, second = run(c, root), run(c, root)
    torch.cuda.synchronize()
    for got in (first, second):
        err, count, tr = (t.cpu().numpy() for t in got)
        assert np.array_equal(count, want[1])
        assert np.isfinite(err).all() and np.isfinite(tr).all()
        assert np.array_equal(bits(err), bits(want[0])), np.abs(err - want[0]).max()
        assert np.array_equal(bits(tr), bits(want[2])), np.abs(tr - want[2]).max()
    return want


# the lane, wave and workgroup edges of the sum order
@pytest.mark.parametrize("n", [1, 2, 3, 24, 63, 64, 65, 255, 256, 257, 1000])
def test_pointset_errors_bit_equal_to_the_mirror(n):
    for P in (1, 5, 130):
        for with_root, root in ((False, (0, 0)), (True, (1, 2)), (True, (2, 2))):
            c = cases.device_case(n, P, 7 * n + P + root[0], with_root, root)
            _, count, _ = check(c, root)
            if P >= 5:
                pi, gi = c["pred_idx"], c["gt_idx"]
                assert (pi == -1).any() and (pi >= 4).any() and (gi == 3).any() and (gi == 4).any() and len(set(pi.tolist())) < P
                assert count[1] == 0 and count[2] == 1 and count[3] == 0 and count[4] == 0 and count[0] > 1 or n == 1


def test_pointset_errors_on_meshes_of_6890_vertices():
    for with_root, root in ((False, (0, 0)), (True, (1, 2))):
        check(cases.device_case(6890, 3, 11, with_root, root), root)         # a repeat, the all-zero row, the one-valid-point row
        check(cases.device_case(6890, 6, 12, with_root, root), root)         # ... and -1, an index out of range


def test_degenerate_families_are_bit_equal_and_finite():
    xs, ys = zip(*[cases.family_pair(f, 24, s) for f in cases.FAMILIES + ("near_collinear_source",) for s in range(4)])
    c = dict(pred=np.stack(xs), gt=np.stack(ys), pred_idx=np.arange(len(xs), dtype=np.int32), gt_idx=np.arange(len(xs), dtype=np.int32),
             weight=None, pred_root=None, gt_root=None)
    err, count, tr = check(c, (0, 0))
    assert (count == 24).all()
    R = tr[:, 1:10].reshape(-1, 3, 3)
    assert np.abs(np.linalg.det(R) - 1).max() <= 64 * 2.0 ** -53 and np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 64 * 2.0 ** -53
    # two points (rank 1 by construction), one point and the same point twice
    two = np.array([[[0.25, 0.5, -1.0], [1.0, -0.5, 0.75]], [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]], np.float32)
    c = dict(pred=two, gt=two[::-1].copy(), pred_idx=np.array([0, 1, 0, 1], np.int32), gt_idx=np.array([0, 0, 1, 1], np.int32), weight=None,
             pred_root=None, gt_root=None)
    check(c, (0, 0))


def test_known_answer_on_a_lattice():
    for n in (3, 14, 65, 6890):
        x, y, R0, t0 = cases.lattice_case(n, n % 5)
        err, count, tr = (t.cpu().numpy() for t in ME.pointset_errors(dev(x[None]), dev(y[None]), dev([0], np.int32), dev([0], np.int32),
                                                                      want_transform=True))
        ext = cases.extent("general", y)
        print("lattice n = %d: aligned %.3g of extent %.3g, s - 0.5 = %.3g" % (n, err[0, 1], ext, tr[0, 0] - 0.5))
        assert count[0] == n and err[0, 1] <= 1e-13 * ext and abs(tr[0, 0] - 0.5) <= 1e-13
        assert np.abs(tr[0, 1:10].reshape(3, 3) - R0).max() <= 1e-13 and np.abs(tr[0, 10:] - t0).max() <= 1e-13
        d = x.astype(np.float64) - y.astype(np.float64)
        want = float(np.mean(np.sqrt((d * d).sum(1))))
        assert abs(err[0, 0] - want) <= 1e-14 * want


@pytest.mark.parametrize("P", [0, 1, 64, 65, 1000])
def test_metric_means_bit_equal_to_the_mirror(P):
    rs = np.random.RandomState(P)
    err, count = rs.uniform(0, 0.2, (P, 2)), rs.randint(0, 3, P).astype(np.int32)
    for cnt in (count, np.zeros(P, np.int32)):
        want, pairs = ME.metric_means_numpy(err, cnt)
        a, b = ME.metric_means(dev(err), dev(cnt)), ME.metric_means(dev(err), dev(cnt))
        for means, n in (a, b):
            assert int(n.cpu()) == pairs and np.array_equal(bits(means.cpu().numpy()), bits(want))
        if not cnt.any():
            assert pairs == 0 and not want.any()


def test_wrong_operands_are_refused():
    x = torch.zeros(2, 5, 3, device=DEV)
    i = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="float32"):
        ME.pointset_errors(x.double(), x, i, i)
    with pytest.raises(RuntimeError, match="argument error.*roots"):
        ME.pointset_errors(x, x, i, i, None, x, x, (1, 5))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ME.pointset_errors(x.cpu(), x.cpu(), i.cpu(), i.cpu())


# ---- the trainer's val() -------------------------------------------------------------------------------------------------------------------
HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}
HEADS9 = dict(HEADS, pose=72, shape=10, cam=3)
K = 20


def test_heads_trainer_val_with_planted_meshes():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(arch.state_dict_shapes(HEADS9, True, 64), seed=0).items()}
    # (a net with synthetic weights may put x2 left of x1, and such a box overlaps nothing: the size head gets a small weight and a
    # positive bias, so every detection is an upright box of about 12 x 20 map pixels)
    sd["wh.2.weight"] = sd["wh.2.weight"] * 0.01
    sd["wh.2.bias"] = torch.tensor([12.0, 20.0])
    net = model.dla_net(HEADS9, head_conv=64, dtype="f32")
    net.load_state_dict(sd)
    net = net.to(DEV)
    body = smpl.SMPLModel.synthetic(seed=0)
    x = torch.from_numpy(synth.synth_images(3, 128, 128)).to(DEV)
    c, s = np.full((3, 2), 64.0, np.float32), np.full(3, 128.0, np.float32)
    loader = [{"input": x[:2], "meta": {"c": c[:2], "s": s[:2], "index": [0, 1]}}, {"input": x[2:], "meta": {"c": c[2:], "s": s[2:], "index": [2]}}]
    # what val() computes, batch by batch: the records and the meshes of all K slots
    net.eval()
    results, joints, verts = [], [], []
    with torch.no_grad():
        for b in loader:
            out = net(b["input"])[-1]
            dets, aux = decode.multi_pose_decode_logits(out["hm"], out["wh"], out["hps"], reg=out["reg"], hm_hp=out["hm_hp"],
                                                        hp_offset=out["hp_offset"], K=K, return_aux=True)
            results.append(multi_pose_post_process(dets, b["meta"]["c"], b["meta"]["s"], out["hm"].shape[2], out["hm"].shape[3]))
            v, j = smpl.lbs_from_heads(body, out["pose"], out["shape"], aux["inds"], K, return_joints=True, exact=True)
            joints.append(j)
            verts.append(v)
    results, joints, verts = torch.cat(results), torch.cat(joints).cpu().numpy(), torch.cat(verts).cpu().numpy()
    assert results.shape == (3, K, 39) and joints.shape == (3 * K, 24, 3) and verts.shape == (3 * K, 6890, 3)
    # ground truth boxes: in images 0 and 1 up to three upright detections, to two decimals; in image 2 one box no detection comes near
    r = C.round2(results.cpu().numpy().astype(np.float64))
    G = 3
    boxes, num = np.zeros((3, G, 4)), np.zeros(3, np.int32)
    for i in range(2):
        up = [d for d in range(K) if r[i, d, 2] - r[i, d, 0] > 1 and r[i, d, 3] - r[i, d, 1] > 1][:G]
        for g, d in enumerate(up):
            boxes[i, g] = (r[i, d, 0], r[i, d, 1], r[i, d, 2] - r[i, d, 0], r[i, d, 3] - r[i, d, 1])
        num[i] = len(up)
    boxes[2, 0], num[2] = (5000.0, 5000.0, 40.0, 80.0), 1
    assert num[0] > 0 and num[1] > 0, "the synthetic net gives no upright box to plant a person on"
    gt = C.GroundTruth(boxes, None, boxes[..., 2] * boxes[..., 3] + 1.0, np.zeros((3, G)), None, num, 1)
    dm = C.match(results, gt, "bbox")["dt_match"][:, 0, 0, :].cpu().numpy()                     # [3,K]: area 'all', IoU 0.5
    assert (dm[:2] >= 0).sum() >= 2 and (dm[2] == -1).all()
    # the persons: the model's own mesh at the matched detection under a known similarity, rounded to float32
    R0, shift = cases.rotation(np.random.RandomState(3)), np.array([0.3, -0.2, 0.5])
    gj, gv, valid = np.zeros((3, G, 24, 3), np.float32), np.zeros((3, G, 6890, 3), np.float32), np.zeros((3, G), np.uint8)
    gt_idx = np.full(3 * K, -1, np.int32)
    for i, d in zip(*np.nonzero(dm >= 0)):
        g = dm[i, d]
        gj[i, g] = 1.25 * joints[i * K + d].astype(np.float64) @ R0.T + shift
        gv[i, g] = 1.25 * verts[i * K + d].astype(np.float64) @ R0.T + shift
        valid[i, g] = 1
        gt_idx[i * K + d] = i * G + g
    gt3d = ME.GroundTruth3D(gj, gv, valid)
    tr = trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-4, K=K), net)
    # 1. without gt3d nothing changes
    kp_stats, bb_stats = tr.val(loader, gt)
    kp, bb = C.evaluate(results, gt, "keypoints"), C.evaluate(results, gt, "bbox")
    assert np.array_equal(bits(kp_stats), bits(kp.stats)) and np.array_equal(bits(bb_stats), bits(bb.stats)) and set(tr.last_val) == {"keypoints", "bbox"}
    # 2. with the planted persons
    kp2, bb2 = tr.val(loader, gt, gt3d, body)
    assert np.array_equal(bits(kp2), bits(kp_stats)) and np.array_equal(bits(bb2), bits(bb_stats)) and set(tr.last_val) == {"keypoints", "bbox", "mesh"}
    res = tr.last_val["mesh"]
    n_planted = int(valid.sum())
    assert res.extra == {"n_gt3d": n_planted, "n_matched": n_planted} and res.n_pairs == n_planted
    biggest = max(np.abs(gj).max(), np.abs(gv).max())
    bound = np.sqrt(3.0) * 2.0 ** -24 * biggest + 1e-13 * biggest        # float32 rounding of the planted coordinates + the fp64 arithmetic
    print("planted: pa_mpjpe %.3g pa_pve %.3g (bound %.3g), mpjpe %.6g pve %.6g, %d pairs" % (res.pa_mpjpe, res.pa_pve, bound, res.mpjpe, res.pve, res.n_pairs))
    assert 0 <= res.pa_mpjpe <= bound and 0 <= res.pa_pve <= bound
    pidx = np.arange(3 * K, dtype=np.int32)
    flat_j, flat_v = gj.reshape(-1, 24, 3), gv.reshape(-1, 6890, 3)
    want_j = ME.evaluate_numpy(joints, flat_j, pidx, gt_idx, None, joints, flat_j, (1, 2))
    want_v = ME.evaluate_numpy(verts, flat_v, pidx, gt_idx, None, joints, flat_j, (1, 2))
    assert np.array_equal(res.joint_count, want_j[1]) and np.array_equal(bits(res.joint_err), bits(want_j[0]))
    assert np.array_equal(res.vert_count, want_v[1]) and np.array_equal(bits(res.vert_err), bits(want_v[0]))
    mj, mv = ME.metric_means_numpy(*want_j[:2])[0], ME.metric_means_numpy(*want_v[:2])[0]
    assert np.array_equal(bits([res.mpjpe, res.pa_mpjpe]), bits(mj)) and np.array_equal(bits([res.pve, res.pa_pve]), bits(mv))
    assert res.mpjpe > 0.01 and res.pve > 0.01 and len(res.summarize()) == 4                # a scale of 1.25 and a rotation: far from aligned
    # 3. a person nobody detects: the coverage drops, the means stay
    valid[2, 0] = 1
    tr.val(loader, gt, ME.GroundTruth3D(gj, gv, valid), body)
    res3 = tr.last_val["mesh"]
    assert res3.extra == {"n_gt3d": n_planted + 1, "n_matched": n_planted} and res3.n_pairs == n_planted
    assert np.array_equal(bits([res3.mpjpe, res3.pa_mpjpe, res3.pve, res3.pa_pve]), bits([res.mpjpe, res.pa_mpjpe, res.pve, res.pa_pve]))
    # the evaluator through evaluate_pairs on the same pairs
    direct = ME.evaluate_pairs(dev(joints), dev(verts), gt3d.flat(DEV), dev(pidx), dev(gt_idx))
    assert np.array_equal(bits([direct.mpjpe, direct.pa_mpjpe, direct.pve, direct.pa_pve]), bits([res.mpjpe, res.pa_mpjpe, res.pve, res.pa_pve]))


def test_val_with_gt3d_needs_the_pose_and_shape_heads():
    net = model.dla_net(HEADS, head_conv=64, dtype="f32").to(DEV)
    tr = trainer.HeadsTrainer(NS(task="multi_pose", lr=1e-4, K=K), net)
    gt = C.GroundTruth(np.zeros((1, 1, 4)), None, [[0]], [[0]], None, [0], 1)
    gt3d = ME.GroundTruth3D(np.zeros((1, 1, 24, 3), np.float32), None, [[0]])
    with pytest.raises(ValueError, match="pose"):
        tr.val([], gt, gt3d, smpl.SMPLModel.synthetic(seed=0, num_verts=100))
