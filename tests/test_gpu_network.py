"""GPU parity of the whole DLA-34 forward through the reference-named factory `dla_net`:
  * plain-conv variant, f32 mode, against the golden vectors = the REFERENCE's own model output
    (tests/golden/dla34_plain.npz) and against the oracle restatement;
  * DCN variant, f32 mode, against the oracle (the reference cannot run DCN on a CPU);
  * bf16 throughput mode against the f32 oracle with the bf16 tolerance stated here;
  * end-to-end detector (model -> sigmoid -> decode -> SMPL) index agreement."""
import os

import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
from h3d_amd import arch, model, synth
from h3d_amd._lib import OPF_DCN_STREAM_F16_INPUT, OPF_DCN_STREAM_SLOTS512, OPF_DCN_STREAM_WIDE_MARGIN, TUNE_DCN_F16_ONE_WG_PER_CU
from h3d_amd.detector import MultiPoseDetector, Opt
from oracle import decode as odec
from oracle import dla as odla

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}
F32_TOL = 2e-4      # abs, heads are O(1): f32 MFMA = exact fmaf chain, BN folding + summation order only
BF16_TOL = 0.06     # abs, 2x the measured worst (0.03): ~50 layers of bf16 activations/weights (2^-9 relative per rounding);
                    # tests/test_gpu_fullsize.py has the 512x512 check against a bf16-emulating oracle and the index statistics


def _net(use_dcn, dtype, heads=HEADS):
    sd = synth.synth_state_dict(arch.state_dict_shapes(heads, use_dcn), seed=0)
    m = model.dla_net(heads, not_use_dcn=not use_dcn, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval(), sd


@pytest.mark.parametrize("dtype", ["f32", "f16x3"])     # f16x3: the same fp32 parity bound on split-operand fp16 MFMAs (csrc/common.h ET<x3_t>)
def test_plain_f32_matches_reference_golden(golden_dir, dtype):
    g = np.load(os.path.join(golden_dir, "dla34_plain.npz"))
    m, _ = _net(False, dtype)
    x = torch.from_numpy(synth.synth_images(2, 96, 128, seed=317)).to(DEV)
    out = m(x)[0]
    assert set(out) == set(HEADS)
    for k in HEADS:
        got = out[k].cpu().numpy()
        assert got.shape == g[k].shape
        np.testing.assert_allclose(got, g[k], rtol=0, atol=F32_TOL, err_msg=k)


@pytest.mark.parametrize("dtype", ["f32", "f16x3"])
def test_dcn_f32_matches_oracle(dtype):
    m, sd = _net(True, dtype)
    xs = synth.synth_images(2, 64, 96, seed=5)
    out = m(torch.from_numpy(xs).to(DEV))[0]
    with torch.no_grad():
        ref = odla.DLAOracle(sd, HEADS, use_dcn=True)(torch.from_numpy(xs))[0]
    for k in HEADS:
        np.testing.assert_allclose(out[k].cpu().numpy(), ref[k].numpy(), rtol=0, atol=5e-4, err_msg=k)


@pytest.mark.parametrize("use_dcn", [False, True])
def test_bf16_mode_within_stated_tolerance(use_dcn):
    m, sd = _net(use_dcn, "bf16")
    xs = synth.synth_images(2, 128, 128, seed=7)
    out = m(torch.from_numpy(xs).to(DEV))[0]
    with torch.no_grad():
        ref = odla.DLAOracle(sd, HEADS, use_dcn=use_dcn)(torch.from_numpy(xs))[0]
    worst = 0.0
    for k in HEADS:
        e = float(np.abs(out[k].cpu().numpy() - ref[k].numpy()).max())
        worst = max(worst, e)
        assert e < BF16_TOL, (k, e)
    print("bf16 max abs head error (dcn=%s): %.4f" % (use_dcn, worst))


F16_TOL = 0.012    # abs: 1/8 of bf16's step (3 more mantissa bits per stored activation), same 2x margin (measured worst below)


def test_f16x3_plan_saturates_beyond_its_contract_instead_of_producing_nan():
    """CONTRACT of the f16x3 plans: |activation| <= 65504 (the split's hi term is an fp16).  Beyond it every split clamps (x3_split4:
    the staging of conv / heads / DeformConv tiles, the blended DeformConv sample, the heads' slab), so a wildly scaled input gives
    finite, saturated heads -- never inf * 0 = NaN."""
    m, sd = _net(True, "f16x3")
    xs = synth.synth_images(1, 64, 96, seed=5) * 3e4
    out = m(torch.from_numpy(xs).to(DEV))[0]
    for k in HEADS:
        assert bool(torch.isfinite(out[k]).all()), k


@pytest.mark.parametrize("use_dcn", [False, True])
def test_f16_mode_within_stated_tolerance(use_dcn):
    """fp16 plans (H3D_F16: the arithmetic BASELINE configs[4] names; also `dla_net(..., dtype="f16")`): same kernels with
    v_mfma_f32_32x32x16_f16 and fp16 epilogues.  Heads vs the fp32 oracle, and no worse than 1.5x an independent fp16
    evaluation of the same graph on the CPU."""
    m, sd = _net(use_dcn, "f16")
    xs = synth.synth_images(2, 128, 128, seed=7)
    out = m(torch.from_numpy(xs).to(DEV))[0]
    eng = m.engine(torch.device(DEV))
    from gpu_helpers import kernel_name
    names = {kernel_name(op) for op in eng.plan(2, 128, 128).ops}
    # no bf16 kernel sneaks into an fp16 plan (csrc/dcn5.hip exists for fp16 only: no type in its name)
    assert all("f16_t" in n or n.startswith("dcn5_kernel<") for n in names), sorted(n for n in names if "f16_t" not in n)
    with torch.no_grad():
        ref = odla.DLAOracle(sd, HEADS, use_dcn=use_dcn)(torch.from_numpy(xs))[0]
        emu = odla.DLAOracle(sd, HEADS, use_dcn=use_dcn, emulate="f16")(torch.from_numpy(xs))[0]
    worst = 0.0
    for k in HEADS:
        e = float(np.abs(out[k].cpu().numpy() - ref[k].numpy()).max())
        t = float((emu[k] - ref[k]).abs().max())
        worst = max(worst, e)
        assert e < F16_TOL and e <= 1.5 * t + 1e-3, (k, e, t)
    print("f16 max abs head error (dcn=%s): %.5f" % (use_dcn, worst))
    again = m(torch.from_numpy(xs).to(DEV))[0]
    for k in HEADS:
        assert torch.equal(out[k], again[k]), k


def test_f16_plan_saturates_instead_of_overflowing():
    # stored activations of an fp16 plan saturate at +-65504 (v_med3_f32 in the epilogues); an input scaled far beyond
    # the fp16 range must give finite heads, not inf / nan
    m, _ = _net(False, "f16")
    xs = torch.from_numpy(synth.synth_images(1, 64, 64, seed=3) * 3.0e4).to(DEV)
    out = m(xs)[0]
    for k in HEADS:
        assert bool(torch.isfinite(out[k]).all()), k


def test_dcn_wide_margin_flag_and_calibration():
    # engine.dcn_wide_margin = 1: every <= 64-channel-workgroup DeformConv on the margin-4 packed apron -- bit-identical heads while
    # no tile overflows its patch slots (small offsets).  calibrate_dcn_margins: with weights of LARGE offsets (offset_scale 2:
    # mean |offset| 6 px) the rule on the kernels' own far-sample counts moves the layers whose tiles overflow to the 512-slot or the
    # wide-margin variant; the choice is a pure function of (weights, images) -- asserted by recomputing it from the returned
    # statistics and by a second calibration -- the network then still matches the oracle within the bf16 tolerance, and the plan
    # runs the packed-apron kernels for exactly those layers.
    from gpu_helpers import kernel_name
    m, _ = _net(True, "bf16")
    xs = torch.from_numpy(synth.synth_images(2, 128, 128, seed=7)).to(DEV)
    on, off = _ab(m, xs, "dcn_wide_margin")
    m.engine(xs.device).dcn_wide_margin = 0
    m.engine(xs.device).plans.clear()
    for k in HEADS:
        assert torch.equal(on[k], off[k]), k
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0, offset_scale=2.0, gain=1.25)
    m2 = model.dla_net(HEADS, dtype="bf16")
    m2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m2.to(DEV).eval()
    x2 = synth.synth_images(2, 256, 256, seed=7)
    eng = m2.engine(torch.device(DEV))
    before = {k: v.clone() for k, v in m2(torch.from_numpy(x2).to(DEV))[0].items()}
    rep = eng.calibrate_dcn_margins(torch.from_numpy(x2).to(DEV))
    assert len(rep) == 16 and all(set(r["cost"]) == {"narrow", "slots512", "wide"} for r in rep.values()), rep
    chosen = dict(eng.pw.dcn_variant)
    assert chosen and set(chosen.values()) <= {OPF_DCN_STREAM_WIDE_MARGIN, OPF_DCN_STREAM_SLOTS512}, (chosen, rep)
    R = eng.DCN_RULE
    for p_, r in rep.items():                            # the choice IS the rule applied to the reported tile shares
        def over(f):
            return max(R["pass2"] * f, min(R["pass2"], R["tail"] / r["rounds"]) if f > 0 else 0.0)
        c = {"narrow": 1 + over(r["tiles_over_256"]),
             "slots512": 1 + R["slots512"] + R["round2"] * (r["tiles_over_256"] - r["tiles_over_512"]) + over(r["tiles_over_512"]),
             "wide": 1 + R["wide"] + over(r["tiles_over_256_wide"])}
        best = min(c, key=c.get)
        want = best if best != "narrow" and c[best] < (1 - R["min_gain"]) * c["narrow"] - 1e-3 else None
        got = {OPF_DCN_STREAM_WIDE_MARGIN: "wide", OPF_DCN_STREAM_SLOTS512: "slots512"}.get(chosen.get(p_))
        assert want is None or got == want, (p_, r, c)
        assert r["choice"] == (got or "narrow")
    # streams = 2 (forward() would run sub-plans and leave plan(B, H, W) untouched: ADVICE r3) and a repeat: the same choice
    eng.streams = 2
    rep2 = eng.calibrate_dcn_margins(torch.from_numpy(x2).to(DEV))
    eng.streams = 1
    assert eng.pw.dcn_variant == chosen and rep2 == rep
    after = m2(torch.from_numpy(x2).to(DEV))[0]
    plan = eng.plan(2, 256, 256)
    assert {p_: plan.ops[i].reserved & ~OPF_DCN_STREAM_F16_INPUT for p_, i in plan.dcn_layers if plan.ops[i].reserved & ~OPF_DCN_STREAM_F16_INPUT} == eng.pw.dcn_variant    # (F16_INPUT: fp16 input of the node layers)
    names = {p_: kernel_name(plan.ops[i]) for p_, i in plan.dcn_layers}
    for p_, bits in eng.pw.dcn_variant.items():
        assert ("512" in names[p_].split("<")[1]) == (bits == OPF_DCN_STREAM_SLOTS512) and (names[p_].endswith(", true>") or ", 4, 16, 4," in names[p_]), names[p_]
    # the stopwatch (tools/fit_dcn_rule.py's yardstick) leaves the plan as it found it
    times = eng.time_dcn_variants(torch.from_numpy(x2).to(DEV), reps=1)
    assert len(times) == 16 and all(set(t) == {"narrow", "slots512", "wide"} and min(t.values()) > 0 for t in times.values()), times
    again = m2(torch.from_numpy(x2).to(DEV))[0]
    for k in HEADS:
        assert torch.equal(after[k], again[k]), k
    with torch.no_grad():
        ref = odla.DLAOracle(sd, HEADS, use_dcn=True)(torch.from_numpy(x2))[0]
        emu = odla.DLAOracle(sd, HEADS, use_dcn=True, emulate_bf16=True)(torch.from_numpy(x2))[0]
    for k in HEADS:
        e_b = float((before[k].cpu() - ref[k]).abs().max())
        e_a = float((after[k].cpu() - ref[k]).abs().max())
        t = float((emu[k] - ref[k]).abs().max())
        assert e_a <= 1.5 * t + 1e-3 and e_b <= 1.5 * t + 1e-3, (k, e_b, e_a, t)


def test_dcn_far_sample_counts_match_the_offsets():
    # h3d_dcn_far_samples (the kernels' own count, what the variant rule and bench.py's dcn_apron read) against the same test
    # evaluated in torch on the offsets of an UNFUSED twin of the plan (engine._tiles_over_slots' arithmetic): equal per tile up to
    # the samples whose position sits within rounding of an apron edge (the twin's offset conv accumulates in another order)
    from h3d_amd.engine import Plan
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0, offset_scale=1.0, gain=1.25)
    m2 = model.dla_net(HEADS, dtype="bf16")
    m2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m2.to(DEV).eval()
    x = torch.from_numpy(synth.synth_images(2, 256, 256, seed=9)).to(DEV)
    eng = m2.engine(torch.device(DEV))
    stats = eng.dcn_far_samples(x)
    twin = Plan(eng.pw, 2, 256, 256, **dict(eng._flags(), fuse_offsets=False))
    twin.op_array[0].in_ = x.data_ptr()
    twin.run()
    torch.cuda.synchronize()
    from h3d_amd import _lib
    from gpu_helpers import kernel_name
    plan = eng.plan(2, 256, 256)
    dcn_ops = [op for op in twin.ops if op.kind == _lib.OP_DCN]
    assert len(dcn_ops) == len(plan.dcn_layers) == 16
    total = 0
    for (p_, i), op in zip(plan.dcn_layers, dcn_ops):
        om = [t for t in twin.keep if torch.is_tensor(t) and t.data_ptr() == op.in2][0]
        h, w = om.shape[1], om.shape[2]
        name = kernel_name(plan.ops[i])
        margin = int(name.split(",")[3])
        ys = torch.arange(h, device=DEV, dtype=torch.float32).view(1, h, 1)
        xs_ = torch.arange(w, device=DEV, dtype=torch.float32).view(1, 1, w)
        y0, x0 = ys - ys % 16 - 1 - margin, xs_ - xs_ % 16 - 1 - margin
        HH = 18 + 2 * margin
        miss = torch.zeros(om.shape[:3], device=DEV)
        for t in range(9):
            ti, tj = divmod(t, 3)
            h_im, w_im = ys - 1 + ti + om[..., 2 * t], xs_ - 1 + tj + om[..., 2 * t + 1]
            inside = (h_im > -1) & (w_im > -1) & (h_im < h) & (w_im < w)
            ry, rx = torch.floor(h_im) - y0, torch.floor(w_im) - x0
            ok = (ry >= 0) & (ry + 1 < HH) & (rx >= 0) & (rx + 1 < HH)
            miss += (inside & ~ok).float()
        th, tw = -(-h // 16), -(-w // 16)
        pad = torch.zeros(2, th * 16, tw * 16, device=DEV)
        pad[:, :h, :w] = miss
        per_tile = pad.view(2, th, 16, tw, 16).sum(dim=(2, 4)).reshape(-1)
        got = stats[p_]["narrow"].float()
        assert got.shape == per_tile.shape, (p_, got.shape, per_tile.shape)
        d = (got - per_tile).abs()
        # (the twin's stand-alone offset conv runs bf16 filters, the fused kernels fp16 ones: offsets differ by ~1e-2 px)
        assert float(d.max()) <= 8 and float(d.sum()) <= 0.03 * float(per_tile.sum()) + 4, (p_, float(d.max()), float(d.sum()), float(per_tile.sum()))
        total += float(per_tile.sum())
        assert bool((stats[p_]["wide"] <= stats[p_]["narrow"]).all()), p_
    assert total > 1000


def test_keep_res_frame_larger_than_the_lds_map_end_to_end():
    # `--keep_res` pads a frame to (h | 31) + 1 (datasets/coco.py:160-163): 1280 x 720 -> 1280 x 736 -> a 320 x 184 output map,
    # 58880 pixels > the 36864 the one-workgroup top-k holds in LDS.  Network (f32 plan) vs the oracle, and the detector's decode
    # (banded top-k + merge) bit-exact against the oracle's decode of the GPU's own heads.
    from h3d_amd import utils
    opt = Opt(input_h=736, input_w=1280, dtype="f32", K=100)
    sd = synth.synth_state_dict(arch.state_dict_shapes(opt.heads, True), seed=0, gain=1.25)
    det = MultiPoseDetector(opt, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, device=DEV)
    xs = synth.synth_images(1, 736, 1280, seed=11)
    res = det.run(torch.from_numpy(xs).to(DEV))
    assert res["heads"]["hm"].shape == (1, 1, 184, 320) and res["dets"].shape == (1, 100, 40)
    with torch.no_grad():
        ref = odla.DLAOracle(sd, opt.heads, use_dcn=True)(torch.from_numpy(xs))[0]
    for k in opt.heads:
        e = float(np.abs(res["heads"][k].cpu().numpy() - ref[k].numpy()).max())
        assert e <= 2e-3, (k, e)
    h = {k: v.cpu().numpy() for k, v in res["heads"].items()}
    dref, aux = odec.multi_pose_decode(utils._sigmoid(res["heads"]["hm"].clone()).cpu().numpy(), h["wh"], h["hps"], h["reg"],
                                       utils._sigmoid(res["heads"]["hm_hp"].clone()).cpu().numpy(), h["hp_offset"], K=100, return_aux=True)
    np.testing.assert_array_equal(res["inds"].cpu().numpy(), aux["inds"])
    np.testing.assert_array_equal(res["dets"].cpu().numpy(), dref)


def test_batch_position_invariance_and_determinism():
    m, _ = _net(True, "bf16")
    xs = torch.from_numpy(synth.synth_images(3, 64, 64, seed=3)).to(DEV)
    a = {k: v.clone() for k, v in m(xs)[0].items()}
    b = {k: v.clone() for k, v in m(xs)[0].items()}
    one = {k: v.clone() for k, v in m(xs[1:2].contiguous())[0].items()}
    for k in HEADS:
        assert torch.equal(a[k], b[k])
        assert torch.equal(a[k][1:2], one[k])


def test_state_dict_keys_and_reference_checkpoint_format(tmp_path):
    m = model.dla_net(HEADS, not_use_dcn=False)
    keys = set(m.state_dict())
    assert keys == set(arch.state_dict_shapes(HEADS, True))
    # reference checkpoint format (trains/trainer.py:530-539): {'epoch', 'state_dict'}, 'module.' prefix
    ck = {"epoch": 3, "state_dict": {"module." + k: v for k, v in m.state_dict().items()}}
    path = os.path.join(tmp_path, "model_last.pth")
    torch.save(ck, path)
    from h3d_amd.checkpoint import load_model
    m2 = model.dla_net(HEADS, not_use_dcn=False)
    load_model(m2, path)
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k])
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train()(torch.zeros(1, 3, 32, 32, device=DEV))
    with pytest.raises(RuntimeError, match="CPU"):
        m.eval()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="multiples of 32"):
        m.to(DEV).eval()(torch.zeros(1, 3, 48, 40, device=DEV))


def test_detector_end_to_end_f32_indices_match_oracle():
    opt = Opt(input_h=128, input_w=128, dtype="f32", K=50)
    sd = synth.synth_state_dict(arch.state_dict_shapes(opt.heads, True), seed=0)
    det = MultiPoseDetector(opt, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, device=DEV)
    xs = synth.synth_images(2, 128, 128, seed=317)
    res = det.run(torch.from_numpy(xs).to(DEV), meta={"c": np.array([[64, 64], [64, 64]], np.float32),
                                                      "s": np.array([128.0, 128.0], np.float32)})
    heads = {k: v.cpu().numpy() for k, v in res["heads"].items()}
    # decode of the GPU's own heads by the oracle: identical inputs -> bit-exact indices
    from h3d_amd import utils
    hm = utils._sigmoid(res["heads"]["hm"]).cpu().numpy()
    hp = utils._sigmoid(res["heads"]["hm_hp"]).cpu().numpy()
    ref, aux = odec.multi_pose_decode(hm, heads["wh"], heads["hps"], heads["reg"], hp, heads["hp_offset"], K=50,
                                      return_aux=True)
    np.testing.assert_array_equal(res["inds"].cpu().numpy(), aux["inds"])
    np.testing.assert_array_equal(res["dets"].cpu().numpy(), ref)
    # network heads vs the fp32 oracle network, then indices wherever the score gap allows
    with torch.no_grad():
        oref = odla.DLAOracle(sd, opt.heads, use_dcn=True)(torch.from_numpy(xs))[0]
    ohm = odec.sigmoid_clamp(oref["hm"].numpy())
    _, oaux = odec.multi_pose_decode(ohm, oref["wh"].numpy(), oref["hps"].numpy(), oref["reg"].numpy(),
                                     odec.sigmoid_clamp(oref["hm_hp"].numpy()), oref["hp_offset"].numpy(), K=50,
                                     return_aux=True)
    agree = (res["inds"].cpu().numpy() == oaux["inds"]).mean()
    assert agree > 0.9, agree
    assert res["results"].shape == (2, 50, 39)


@pytest.mark.parametrize("dtype,tol", [("f32", 2e-4), ("bf16", 6e-2)])
def test_fused_heads_match_per_head_convs(dtype, tol):
    # fused heads kernel (csrc/heads.hip) vs one conv3x3 + conv1x1 launch pair per head, incl. the
    # 72- and 10-channel SMPL heads and a map whose width is not a multiple of the 32-pixel tile
    heads = dict(HEADS, pose=72, shape=10)
    m, sd = _net(True, dtype, heads)
    xs = torch.from_numpy(synth.synth_images(2, 96, 160, seed=11)).to(DEV)
    fused = {k: v.clone() for k, v in m(xs)[0].items()}
    eng = m.engine(xs.device)
    eng.fuse_heads = False
    eng.plans.clear()
    plain = {k: v.clone() for k, v in m(xs)[0].items()}
    eng.fuse_heads = True
    eng.plans.clear()
    for k in heads:
        assert fused[k].shape == (2, heads[k], 24, 40)
        e = float((fused[k] - plain[k]).abs().max())
        assert e <= tol, (k, e)
    if dtype == "f32":
        with torch.no_grad():
            ref = odla.DLAOracle(sd, heads, use_dcn=True)(xs.cpu())[0]
        for k in heads:
            np.testing.assert_allclose(fused[k].cpu().numpy(), ref[k].numpy(), rtol=0, atol=5e-4, err_msg=k)


@pytest.mark.parametrize("dtype,tol", [("f32", 3e-4), ("bf16", 6e-2)])
def test_fused_offset_dcn_matches_two_launch_path(dtype, tol):
    # DeformConv with conv_offset_mask fused (csrc/dcn3.hip) vs offset conv + dcn2 launches, and vs the oracle
    m, sd = _net(True, dtype)
    xs = torch.from_numpy(synth.synth_images(2, 96, 160, seed=13)).to(DEV)
    eng = m.engine(xs.device)
    assert eng.fuse_offsets
    fused = {k: v.clone() for k, v in m(xs)[0].items()}
    eng.fuse_offsets = False
    eng.plans.clear()
    plain = {k: v.clone() for k, v in m(xs)[0].items()}
    eng.fuse_offsets = True
    eng.plans.clear()
    for k in HEADS:
        e = float((fused[k] - plain[k]).abs().max())
        assert e <= tol, (k, e)
    if dtype == "f32":
        with torch.no_grad():
            ref = odla.DLAOracle(sd, HEADS, use_dcn=True)(xs.cpu())[0]
        for k in HEADS:
            np.testing.assert_allclose(fused[k].cpu().numpy(), ref[k].numpy(), rtol=0, atol=5e-4, err_msg=k)


def test_fused_offset_dcn_large_offsets_take_the_global_path():
    # offset filters scaled up so many samples leave the 2-pixel apron: pass 2 must add them back exactly
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0, offset_scale=12.0)
    m = model.dla_net(HEADS, not_use_dcn=False, dtype="f32")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    xs = synth.synth_images(1, 64, 96, seed=17)
    out = m(torch.from_numpy(xs).to(DEV))[0]
    with torch.no_grad():
        ref = odla.DLAOracle(sd, HEADS, use_dcn=True)(torch.from_numpy(xs))[0]
    for k in HEADS:
        np.testing.assert_allclose(out[k].cpu().numpy(), ref[k].numpy(), rtol=0, atol=1e-3, err_msg=k)


def test_stream_split_matches_single_stream():
    m, _ = _net(True, "bf16")
    xs = torch.from_numpy(synth.synth_images(16, 64, 64, seed=19)).to(DEV)
    one = {k: v.clone() for k, v in m(xs)[0].items()}
    eng = m.engine(xs.device)
    eng.streams = 2
    two = {k: v.clone() for k, v in m(xs)[0].items()}
    torch.cuda.synchronize()
    eng.streams = 1
    for k in HEADS:
        assert torch.equal(one[k], two[k]), k


def _ab(m, xs, flag, **first):
    """heads with engine flag `flag` on and off, plans rebuilt in between; `first`: flags to set before (e.g. the
    csrc/dcn4.hip path is off by default since round 2)."""
    eng = m.engine(xs.device)
    for k, v in first.items():
        setattr(eng, k, v)
    setattr(eng, flag, True)
    eng.plans.clear()
    on = {k: v.clone() for k, v in m(xs)[0].items()}
    setattr(eng, flag, False)
    eng.plans.clear()
    off = {k: v.clone() for k, v in m(xs)[0].items()}
    setattr(eng, flag, True)
    eng.plans.clear()
    return on, off


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_all_heads_in_one_launch_is_bit_identical_to_one_launch_per_width(dtype):
    # engine.mixed_heads = 1 (off by default: faster kernel, slower step with three steps in flight): ONE heads launch for the whole model, the kernel picking the 1 / 2 / 3-row-tile body per
    # head, against one launch per width (heads <= 32 channels | hps | the SMPL pose head): the same instruction stream per head
    from gpu_helpers import kernel_name
    m, _ = _net(True, dtype)
    xs = torch.from_numpy(synth.synth_images(2, 96, 160, seed=29)).to(DEV)      # ragged 16 x 32 tiles
    eng = m.engine(xs.device)
    on, off = _ab(m, xs, "mixed_heads")                 # (leaves the flag on)
    names = [kernel_name(op) for op in eng.plan(2, 96, 160).ops if op.kind == _lib_mod().OP_HEADS]
    assert len(names) == 1 and names[0].endswith(", true, true>"), names
    eng.mixed_heads = 0
    eng.plans.clear()
    m(xs)
    assert len([op for op in eng.plan(2, 96, 160).ops if op.kind == _lib_mod().OP_HEADS]) >= 2
    for k in HEADS:
        assert torch.equal(on[k], off[k]), k


def _lib_mod():
    from h3d_amd import _lib
    return _lib


def test_streamed_conv_matches_register_staged_kernel():
    # csrc/conv2.hip (LDS-DMA operands, LDS-transposed stores) vs csrc/conv.hip on every 3x3 s1 layer:
    # same bf16 operands, same fp32 accumulation -> only the summation order inside an MFMA chain differs
    m, _ = _net(False, "bf16")
    xs = torch.from_numpy(synth.synth_images(3, 96, 160, seed=23)).to(DEV)     # ragged tiles on both axes
    on, off = _ab(m, xs, "stream_convs")
    kinds = [op.kind for op in m.engine(xs.device).plan(3, 96, 160).ops]
    from h3d_amd import _lib
    assert _lib.OP_CONV_STREAM in kinds
    for k in HEADS:
        e = float((on[k] - off[k]).abs().max())
        assert e <= 3e-2, (k, e)


@pytest.mark.extra      # csrc/dcn4.hip: a superseded generation, `make EXTRA=1` (engine.stream_dcn)
@pytest.mark.parametrize("offset_scale,tol", [(0.5, 6e-2), (12.0, 0.25)])
def test_streamed_dcn_matches_dcn3(offset_scale, tol):
    # csrc/dcn4.hip (fp16 input written by the up-sample kernel, all operands by LDS-DMA) vs csrc/dcn3.hip;
    # offset_scale 12 drives many samples out of the apron so the global-gather pass 2 is exercised too.
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0, offset_scale=offset_scale)
    m = model.dla_net(HEADS, not_use_dcn=False, dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    xs = torch.from_numpy(synth.synth_images(2, 96, 160, seed=29)).to(DEV)
    on, off = _ab(m, xs, "stream_dcn")
    from h3d_amd import _lib
    kinds = [op.kind for op in m.engine(xs.device).plan(2, 96, 160).ops]
    assert _lib.OP_UPDCN_F16 in kinds           # (dcn4 with the up-sample + add folded in)
    with torch.no_grad():
        ref = odla.DLAOracle(sd, HEADS, use_dcn=True)(xs.cpu())[0]
    for k in HEADS:
        e = float((on[k] - off[k]).abs().max())
        assert e <= tol, (k, e)
        # and the streamed path is no further from the fp32 oracle than the bf16 tolerance of this file
        e_ref = float((on[k].cpu() - ref[k]).abs().max())
        e_off = float((off[k].cpu() - ref[k]).abs().max())
        assert e_ref <= max(BF16_TOL, 1.5 * e_off), (k, e_ref, e_off)


@pytest.mark.extra      # csrc/dcn4.hip: a superseded generation, `make EXTRA=1` (engine.stream_dcn)
@pytest.mark.parametrize("offset_scale", [0.5, 3.0, 12.0])
def test_dcn4_two_workgroups_per_cu_matches_one(offset_scale):
    # csrc/dcn4.hip DENSE = 1 (margin-1 apron, single filter slot, the default) vs DENSE = 0 (margin 2, 3-slot ring;
    # h3d_op.reserved = TUNE_DCN_F16_ONE_WG_PER_CU): same arithmetic per sample, only the split between the apron pass and the
    # global-gather pass 2 differs (offset_scale 3 puts samples between the two margins), i.e. fp32 summation order
    from h3d_amd import _lib
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0, offset_scale=offset_scale)
    m = model.dla_net(HEADS, not_use_dcn=False, dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    xs = torch.from_numpy(synth.synth_images(2, 96, 160, seed=31)).to(DEV)
    m.engine(xs.device).fuse_upnode = False     # the one-workgroup variant exists for the fp16-input op only
    m.engine(xs.device).stream_dcn = True       # csrc/dcn4.hip is an option since round 2, not the default
    dense = {k: v.clone() for k, v in m(xs)[0].items()}
    plan = m.engine(xs.device).plan(2, 96, 160)
    idx = [i for i, op in enumerate(plan.ops) if op.kind == _lib.OP_DCN_FUSED_F16]
    assert idx
    try:
        for i in idx:
            plan.op_array[i].reserved = TUNE_DCN_F16_ONE_WG_PER_CU
        one = {k: v.clone() for k, v in m(xs)[0].items()}
    finally:
        for i in idx:
            plan.op_array[i].reserved = 0
    for k in HEADS:
        e = float((dense[k] - one[k]).abs().max())
        assert e <= 2e-2, (k, e)


@pytest.mark.extra      # csrc/dcn4.hip: a superseded generation, `make EXTRA=1` (engine.stream_dcn)
@pytest.mark.parametrize("offset_scale", [0.5, 12.0])
def test_fused_upsample_node_is_bit_identical(offset_scale):
    # H3D_OP_UPDCN_F16 (csrc/dcn4.hip UP = 1: skip + depthwise ConvTranspose2d evaluated while the apron is filled, and
    # again from global memory for pass-2 samples) vs H3D_OP_UPADD writing fp16 + H3D_OP_DCN_FUSED_F16: the same
    # arithmetic in the same order with the same single rounding to fp16, so every head must match bit for bit
    # (2x up-sampling on four levels, 4x on the last; ragged tiles; offset_scale 12 exercises pass 2)
    from h3d_amd import _lib
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0, offset_scale=offset_scale)
    m = model.dla_net(HEADS, not_use_dcn=False, dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    xs = torch.from_numpy(synth.synth_images(3, 96, 160, seed=43)).to(DEV)
    on, off = _ab(m, xs, "fuse_upnode", stream_dcn=True)
    kinds = [op.kind for op in m.engine(xs.device).plan(3, 96, 160).ops]
    assert _lib.OP_UPDCN_F16 in kinds and _lib.OP_DCN_FUSED_F16 not in kinds
    for k in HEADS:
        assert torch.equal(on[k], off[k]), (k, float((on[k] - off[k]).abs().max()))


@pytest.mark.parametrize("offset_scale,tol", [(0.5, 6e-2), (12.0, 0.25)])
def test_dma_filter_dcn3_matches_register_staged(offset_scale, tol):
    # csrc/dcn3.hip with the filters as stage-major images copied by LDS-DMA (H3D_OP_DCN_FUSED_STREAM) vs the
    # register-staged filters (H3D_OP_DCN_FUSED): identical arithmetic, so the outputs agree to bf16 noise
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0, offset_scale=offset_scale)
    m = model.dla_net(HEADS, not_use_dcn=False, dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    xs = torch.from_numpy(synth.synth_images(2, 96, 160, seed=31)).to(DEV)
    eng = m.engine(xs.device)
    eng.dense_dcn3 = False            # so that "off" is the register-staged kernel on every layer
    eng.plans.clear()
    on, off = _ab(m, xs, "stream_dcn3")
    from h3d_amd import _lib
    assert _lib.OP_DCN_FUSED_STREAM in [op.kind for op in eng.plan(2, 96, 160).ops]
    for k in HEADS:
        e = float((on[k] - off[k]).abs().max())
        assert e <= tol, (k, e)


def test_node_f16_plan_error_is_not_above_the_bf16_node_plan():
    # engine.node_f16 (default on, bf16 plans): the up-sample + add launches write the `node` DeformConvs' inputs as fp16 instead of
    # bf16 (three more mantissa bits on the tensors whose rounding the heads see most directly).  Whole network, both settings against
    # the fp32 oracle: the flag must not cost precision on any head (it had a kernel-level case only)
    from h3d_amd import _lib
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0)
    m = model.dla_net(HEADS, not_use_dcn=False, dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    x = synth.synth_images(2, 96, 160, seed=37)
    xs = torch.from_numpy(x).to(DEV)
    eng = m.engine(xs.device)
    on, off = _ab(m, xs, "node_f16")
    assert _lib.OUT_NHWC_F16 in [op.out_mode for op in eng.plan(2, 96, 160).ops]      # the flag is live in this plan
    with torch.no_grad():
        ref = odla.DLAOracle(sd, HEADS, use_dcn=True)(torch.from_numpy(x))[0]
    for k in HEADS:
        e_on = float(((on[k].cpu() - ref[k]) ** 2).mean().sqrt())
        e_off = float(((off[k].cpu() - ref[k]) ** 2).mean().sqrt())
        assert e_on <= 1.1 * e_off + 1e-4, (k, e_on, e_off)


@pytest.mark.parametrize("offset_scale,tol", [(0.5, 6e-2), (3.0, 0.1), (12.0, 0.25)])
def test_dense_dcn3_matches_register_staged(offset_scale, tol):
    # the default for DeformConvs with <= 64 output channels: csrc/dcn3.hip with DMA'd filters, a margin-1 apron and
    # two workgroups per CU, vs the register-staged margin-2 kernel; offset_scale 3 puts samples between the two
    # margins (apron pass on one side, global-gather pass 2 on the other), 12 drives most of them into pass 2
    from h3d_amd import _lib
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0, offset_scale=offset_scale)
    m = model.dla_net(HEADS, not_use_dcn=False, dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    xs = torch.from_numpy(synth.synth_images(2, 96, 160, seed=41)).to(DEV)
    m.engine(xs.device).dense_dcn3_min_tiles = 0      # (the default engages it from 512 tiles per layer)
    on, off = _ab(m, xs, "dense_dcn3", stream_dcn3=False)
    kinds = [op.kind for op in m.engine(xs.device).plan(2, 96, 160).ops]
    assert _lib.OP_DCN_FUSED_STREAM in kinds and _lib.OP_DCN_FUSED in kinds
    with torch.no_grad():
        ref = odla.DLAOracle(sd, HEADS, use_dcn=True)(xs.cpu())[0]
    for k in HEADS:
        e = float((on[k] - off[k]).abs().max())
        assert e <= tol, (k, e)
        e_ref = float((on[k].cpu() - ref[k]).abs().max())
        e_off = float((off[k].cpu() - ref[k]).abs().max())
        assert e_ref <= max(BF16_TOL, 1.5 * e_off), (k, e_ref, e_off)


@pytest.mark.parametrize("dtype,tol", [("bf16", 3e-2), ("f16x3", 2e-4)])
def test_fused_stem_levels_match_three_launches(dtype, tol):
    # csrc/stem3.hip (base_layer + level0 + level1 in one kernel, intermediates in LDS) vs the three separate
    # launches: the same bf16 rounding points, only the fp32 summation order inside the MFMA chains differs.
    # f16x3 (csrc/stem3x.hip): the intermediates are split by the lane that produced them exactly as the consumer's staging would split
    # the stored fp32 value -- the same numbers, another accumulation order: fp32-level agreement
    m, _ = _net(False, dtype)
    xs = torch.from_numpy(synth.synth_images(3, 96, 160, seed=37)).to(DEV)      # ragged 8x16 tiles on both axes
    on, off = _ab(m, xs, "fuse_stem")
    from h3d_amd import _lib
    assert _lib.OP_STEM3 in [op.kind for op in m.engine(xs.device).plan(3, 96, 160).ops]
    for k in HEADS:
        e = float((on[k] - off[k]).abs().max())
        assert e <= tol, (k, e)
    # a single tile row / narrow image
    xs = torch.from_numpy(synth.synth_images(1, 32, 224, seed=41)).to(DEV)
    on, off = _ab(m, xs, "fuse_stem")
    for k in HEADS:
        e = float((on[k] - off[k]).abs().max())
        assert e <= tol, (k, e)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [(3, 96, 160), (1, 32, 224), (2, 128, 128)])
def test_stem_launch_with_pool_and_project_is_bit_identical(dtype, shape):
    # engine.fuse_stem_proj (round 4): the fused stem launch also max-pools its level1 tile and applies level2's `project` 1x1 conv
    # (model.py:200-207, 211-212) -- against the plan with the max-pool and the 1x1 conv as their own launches: every head bit for
    # bit (max of packed non-negative values == float max; the 1x1 conv uses the stand-alone kernel's MFMA shape and K order)
    from h3d_amd import _lib
    m, _ = _net(True, dtype)
    B, H, W = shape
    xs = torch.from_numpy(synth.synth_images(B, H, W, seed=43)).to(DEV)
    on, off = _ab(m, xs, "fuse_stem_proj")          # (leaves the flag on: the plan below is the fused one; off by default, see engine.Plan.FLAGS)
    ops = m.engine(xs.device).plan(B, H, W).ops
    assert ops[0].kind == _lib.OP_STEM3 and ops[0].in2 and sum(op.kind == _lib.OP_MAXPOOL for op in ops) == 3
    for k in HEADS:
        assert torch.equal(on[k], off[k]), k


@pytest.mark.parametrize("offset_scale", [0.5, 6.0])
def test_forward_is_deterministic_and_batch_position_independent(offset_scale):
    # a race in one of the LDS pipelines (counted vmcnt / lgkmcnt waits, DMA rings, wave-private staging areas) shows up
    # as run-to-run or image-to-image differences: the same two images repeated four times through the default bf16
    # plan must give the same bits for every repeat and for every run (offset_scale 6 sends samples through pass 2)
    sd = synth.synth_state_dict(arch.state_dict_shapes(HEADS, True), seed=0, offset_scale=offset_scale)
    m = model.dla_net(HEADS, not_use_dcn=False, dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    xs = torch.from_numpy(synth.synth_images(2, 128, 192, seed=47)).to(DEV).repeat(4, 1, 1, 1).contiguous()
    first = {k: v.clone() for k, v in m(xs)[0].items()}
    for k, v in first.items():
        r = v.view(4, 2, *v.shape[1:])
        assert torch.equal(r, r[:1].expand_as(r)), k
    for _ in range(4):
        again = m(xs)[0]
        for k in first:
            assert torch.equal(first[k], again[k]), k


def test_plan_slots_on_two_streams_give_identical_results():
    # bench.py --pipeline 2: consecutive batches alternate between two HIP streams, each with its own copy of the plan's
    # buffers (engine.plan(..., slot)); interleaved launches of both slots must not disturb each other
    opt = Opt(input_h=128, input_w=192, dtype="bf16", K=40, smpl=True, smpl_people=8)
    sd = synth.synth_state_dict(arch.state_dict_shapes(opt.heads, True), seed=0, gain=1.25)
    det = MultiPoseDetector(opt, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, device=DEV)
    xa = torch.from_numpy(synth.synth_images(4, 128, 192, seed=1)).to(DEV)
    xb = torch.from_numpy(synth.synth_images(4, 128, 192, seed=2)).to(DEV)
    ra = {k: v.clone() for k, v in det.run(xa).items() if k in ("dets", "verts")}
    rb = {k: v.clone() for k, v in det.run(xb).items() if k in ("dets", "verts")}
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for i in range(6):
        with torch.cuda.stream(streams[i % 2]):
            r = det.run(xa if i % 2 == 0 else xb, slot=i % 2)
            outs.append((r["dets"].clone(), r["verts"].clone()))
    torch.cuda.synchronize()
    for i, (d, v) in enumerate(outs):
        ref = ra if i % 2 == 0 else rb
        assert torch.equal(d, ref["dets"]) and torch.equal(v, ref["verts"]), i
    eng = det.model.engine(torch.device(DEV))
    assert eng.plan(4, 128, 192, 0) is not eng.plan(4, 128, 192, 1)


def test_plan_slots_combined_with_sub_batch_streams():
    # engine.streams > 1 (sub-batches on internal HIP streams) used to ignore `slot`: two batches in flight on
    # different slots shared one set of sub-plans, output tensors and internal streams (a silent race).  Now every slot
    # owns its own: interleaving both slots with the split on must reproduce the one-stream, one-slot results bit for bit.
    opt = Opt(input_h=128, input_w=128, dtype="bf16", K=40, smpl=True, smpl_people=8)
    sd = synth.synth_state_dict(arch.state_dict_shapes(opt.heads, True), seed=0, gain=1.25)
    det = MultiPoseDetector(opt, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, device=DEV)
    xa = torch.from_numpy(synth.synth_images(16, 128, 128, seed=1)).to(DEV)
    xb = torch.from_numpy(synth.synth_images(16, 128, 128, seed=2)).to(DEV)
    ra = {k: v.clone() for k, v in det.run(xa).items() if k in ("dets", "verts")}
    rb = {k: v.clone() for k, v in det.run(xb).items() if k in ("dets", "verts")}
    torch.cuda.synchronize()
    eng = det.model.engine(torch.device(DEV))
    eng.streams = 2
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for i in range(6):
        with torch.cuda.stream(streams[i % 2]):
            r = det.run(xa if i % 2 == 0 else xb, slot=i % 2)
            outs.append((r["dets"].clone(), r["verts"].clone()))
    torch.cuda.synchronize()
    eng.streams = 1
    assert ("split", 16, 128, 128, 0) in eng.plans and ("split", 16, 128, 128, 1) in eng.plans
    assert eng.plans[("split", 16, 128, 128, 0)][1]["hm"].data_ptr() != eng.plans[("split", 16, 128, 128, 1)][1]["hm"].data_ptr()
    for i, (d, v) in enumerate(outs):
        ref = ra if i % 2 == 0 else rb
        assert torch.equal(d, ref["dets"]) and torch.equal(v, ref["verts"]), i


def test_flip_test_on_a_mirror_symmetric_input_keeps_symmetry_and_runs_both_passes():
    # --flip_test (opts.py:89): heads of the batch and of its mirror image averaged with the reference's flip helpers.
    # For every head the recipe must equal the explicit two-pass computation done here with the same helpers.
    from h3d_amd import utils
    opt = Opt(input_h=128, input_w=128, dtype="f32", K=30, flip_test=True)
    sd = synth.synth_state_dict(arch.state_dict_shapes(opt.heads, True), seed=0, gain=1.25)
    det = MultiPoseDetector(opt, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, device=DEV)
    x = torch.from_numpy(synth.synth_images(2, 128, 128, seed=9)).to(DEV)
    res = det.run(x)
    a = {k: v.clone() for k, v in det.model(x)[0].items()}
    b = {k: v.clone() for k, v in det.model(torch.flip(x, [3]).contiguous())[0].items()}
    wh = (a["wh"] + utils.flip_tensor(b["wh"])) / 2
    hps = (a["hps"] + utils.flip_lr_off(b["hps"], opt.flip_idx)) / 2
    np.testing.assert_allclose(res["heads"]["wh"].cpu().numpy(), wh.cpu().numpy(), atol=1e-5)
    np.testing.assert_allclose(res["heads"]["hps"].cpu().numpy(), hps.cpu().numpy(), atol=1e-5)
    p = (utils._sigmoid(a["hm"].clone()) + utils.flip_tensor(utils._sigmoid(b["hm"].clone()))) / 2
    np.testing.assert_allclose(utils._sigmoid(res["heads"]["hm"].clone()).cpu().numpy(), p.cpu().numpy(), atol=1e-6)
    assert torch.equal(res["heads"]["reg"], a["reg"]) and res["dets"].shape == (2, 30, 40)


@pytest.mark.parametrize("arch_args", [[], ["--arch", "resdcn_101"], ["--arch", "hourglass"], ["--dtype", "f16x3"]])
def test_bench_cli_prints_one_contract_line(arch_args):
    """bench.py --full end to end as the driver starts it (a child process; small batch and image): ONE JSON line with the contract's
    keys, `roofline` with a live per-launch figure, and a value that is a rate of the K timed steps."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--size", "128",
           "--full", "--no-cpu-baseline"] + arch_args
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert d["dtype"] == ("f16x3" if "f16x3" in arch_args else "bf16") and d["data"] == "synthetic" and "workload" in d["config"] and d["vs_baseline"] is None
    for k in ("shader_clock_mhz", "value_long"):          # (round 5; value_long is null for the other backbones, the clock where sysfs hides it)
        assert k in d, k
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms", "frac_rocprof", "mfma_util", "shader_clock_mhz_timed_region",
              "peak_assumes_mhz"):
        assert k in rf, k
    assert rf["avg_launch_ms"] > 0 and 0 < rf["frac"] < 1


def test_bench_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """bench.py without --full: the line holds the headline fields and none of the --full records, `--steps` sets the timed steps,
    and --dump-outputs writes the last timed step's result as float32 / float64 .npy files within 64 MB: dets and inds whole,
    the SMPL vertices as the seeded sample, all equal to what the same detector computes on the same inputs in this process."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
                        "--size", "128", "--dump-outputs", out], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "bf16" and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    for k in ("roofline", "kernels", "cpu_baseline", "index_match", "value_long", "shader_clock_mhz", "shard_sweep", "parity_mode"):
        assert k not in d, k
    files = sorted(os.listdir(out))
    assert {"dets.npy", "inds.npy", "verts.npy", "joints.npy", "heads_hm.npy", "heads_pose.npy"} <= set(files), files
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64e6
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    # the same detector and images as bench.py's defaults, in this process
    opt = Opt(input_h=128, input_w=128, smpl=True, smpl_people=100, dtype="bf16", K=100)
    sd = synth.synth_state_dict(arch.state_dict_shapes(opt.heads, True), seed=0, offset_scale=0.5, gain=1.25)
    det = MultiPoseDetector(opt, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, device=DEV)
    x = torch.from_numpy(synth.synth_image_batch(4, 128, 128, seed=317)).to(DEV)
    det.model.engine(DEV).calibrate_dcn_margins(x)
    res = det.run(x)
    torch.cuda.synchronize()
    assert got["inds"].dtype == np.float64 and np.array_equal(got["inds"], res["inds"].cpu().numpy().astype(np.float64))
    assert got["dets"].shape == (4, 100, 40)
    np.testing.assert_allclose(got["dets"], res["dets"].cpu().numpy(), rtol=0, atol=1e-5)
    verts = res["verts"].cpu().numpy().reshape(-1)
    n = got["verts"].size
    assert got["verts"].ndim == 1 and n < verts.size
    pos = np.sort(np.random.default_rng(0).choice(verts.size, n, replace=False))
    np.testing.assert_allclose(got["verts"], verts[pos], rtol=0, atol=1e-5)


@pytest.mark.parametrize("scale", [0.5, 2.0])
def test_two_processes_return_identical_bits(scale):
    """Plan selection is deterministic ACROSS processes (the timed choice of round 3 could differ from run to run,
    and with it the accumulation order of overflowing DeformConv tiles): two fresh processes -- own library load, own
    calibration on the same weights and images -- print the same digest of dets, indices and every head, at small and at large
    offsets (at scale 2.0 most layers leave the default variant and many tiles overflow).  The reference operator is
    deterministic by construction (dcn_v2_cuda.cu:43-173)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for _ in range(2):                                        # one after the other: never more than one child on the GPU
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "dets_digest.py"), str(scale), "4", "256"], cwd=root,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
        assert len(line) == 1, r.stdout[-2000:]
        outs.append(line[0])
    assert outs[0] == outs[1], outs
    if scale >= 2.0:
        assert "[]" not in outs[0], outs[0]                  # some layer did leave the default variant


def test_fused_tail_is_bit_identical_to_the_separate_launches():
    # detector.fused_tail (round 4): no topk_merge launch for the single multi_pose class, the pose / shape gathers and the
    # blend-shape operand pack inside the SMPL pose kernel -- against round 3's tail (nine launches) on the same heads
    from h3d_amd import decode as dec
    opt = Opt(input_h=128, input_w=128, smpl=True, smpl_people=40, dtype="bf16", K=100)
    sd = synth.synth_state_dict(arch.state_dict_shapes(opt.heads, True), seed=0, gain=1.25)
    det = MultiPoseDetector(opt, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, device=DEV)
    x = torch.from_numpy(synth.synth_images(4, 128, 128, seed=11)).to(DEV)
    a = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in det.run(x).items() if k != "heads"}
    det.fused_tail, dec.SINGLE_CLASS_SHORTCUT = False, False
    try:
        b = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in det.run(x).items() if k != "heads"}
    finally:
        det.fused_tail, dec.SINGLE_CLASS_SHORTCUT = True, True
    assert set(a) == set(b) == {"dets", "inds", "verts", "joints"}
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_bench_step_with_the_rccl_collective_on_one_gpu():
    """`bench.py --rehearse-collective`: the multi-GPU rank's code path on the one GPU a test box has -- `init_process_group("nccl")`
    (RCCL, a group of one rank), every step's `all_gather_into_tensor` of `dets` issued from the default stream behind an event of
    the slot stream, barrier + all-reduce(MAX) timing.  The N > 1 path is otherwise covered by gloo on the CPU only
    (tests/test_cpu_host.py); here the same calls meet RCCL and the device (trainer.py:176 is the reference's scatter)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--rehearse-collective", "--batch", "8", "--steps", "6", "--warmup", "2",
                        "--no-extras", "--no-cpu-baseline", "--no-roofline"], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0 and any(k in r.stderr for k in ("ncclSystemError", "ncclUnhandledCudaError", "NCCL WARN", "Bootstrap", "bootstrap")) \
            and "h3d" not in r.stderr.split("Traceback")[-1]:
        pytest.skip("RCCL could not bootstrap on this box (environment, not the step): %s" % r.stderr[-400:])
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["rccl_ranks"] == 1 and line["config"]["collective"].startswith("rehearsed"), line["config"]
    assert line["value"] > 100 and line["config"]["steps_in_flight"] == 4
