"""CPU (-m "not gpu"): host logic, the C-ABI library's exports, sharding + the world_size-2 gloo
path of the one collective.  No compute calls (there is no GPU here and no CPU fallback)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import h3d_amd  # noqa: F401
from h3d_amd import _lib, arch, detector, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}


def test_library_loads_and_exports_every_declared_symbol():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "h3d.h")).read()
    declared = set(re.findall(r"\b(h3d_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(L, name), name
    size_t_fns = {"h3d_dcn_v2_workspace_bytes", "h3d_dcn_v2_packed_weight_bytes", "h3d_dcn_v2_packed_workspace_bytes",
                  "h3d_nms_topk_large_workspace_bytes"}     # (size_t results: bound separately)
    assert declared - {"h3d_last_error", "h3d_abi_version"} - size_t_fns == set(_lib.SIGNATURES)
    assert L.h3d_dcn_v2_workspace_bytes(2, 64, 10, 12, 64) >= 2 * 10 * 12 * (64 + 32) * 4 + 128 * 9 * 64 * 4
    assert L.h3d_dcn_v2_workspace_bytes(0, 64, 10, 12, 64) == 0
    assert L.h3d_abi_version() == _lib.ABI_VERSION


def test_abi4_operator_workspaces_hold_the_activation_maxima():
    # ABI 4: behind the [B*H*W, 32] offset / mask rows both operator workspaces keep 16 bytes for max |x| and max |mask|
    L = _lib.lib()
    B, C, H, W, Co = 2, 64, 10, 12, 64
    px = B * H * W
    om = (px * 32 * 4 + 16 + 255) // 256 * 256
    assert L.h3d_dcn_v2_packed_workspace_bytes(B, C, H, W, _lib.DCN_INPUT_NHWC) == om
    assert L.h3d_dcn_v2_packed_workspace_bytes(B, C, H, W, 0) == om + px * C * 4
    assert L.h3d_dcn_v2_workspace_bytes(B, C, H, W, Co) == px * C * 4 + om + 128 * 9 * C * 4 + 128 * 4 + 256
    assert L.h3d_dcn_nchw_to_nhwc_scaled(None, None, 1, 16, 4, 4, None, None) == -5 and b"null pointer" in L.h3d_last_error()


def _ctype_of(param):
    """ctypes classes a C parameter declaration of include/h3d.h may be bound as."""
    if "*" in param:
        if re.match(r"(const )?size_t \*", param):
            return (ctypes.POINTER(ctypes.c_size_t),)
        return (ctypes.c_void_p, ctypes.c_char_p, ctypes._Pointer)
    return {"int": (ctypes.c_int,), "int32_t": (ctypes.c_int,), "size_t": (ctypes.c_size_t,), "float": (ctypes.c_float,)}[param.rsplit(" ", 1)[0]]


def test_every_ctypes_signature_matches_its_declaration():
    L = _lib.lib()
    hdr = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(ROOT, "include", "h3d.h")).read(), flags=re.S)
    decls = {name: (ret, [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")])
             for ret, name, params in re.findall(r"^(int|size_t|const char \*) ?(h3d_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)}
    assert set(decls) == set(re.findall(r"\b(h3d_[a-z0-9_]+)\s*\(", hdr)) and len(decls) == len(_lib.SIGNATURES) + 6
    bound = dict(_lib.SIGNATURES)
    for name, (ret, _) in decls.items():
        if ret == "size_t":
            fn = getattr(L, name)
            assert name not in bound and fn.restype is ctypes.c_size_t, name
            bound[name] = fn.argtypes
    for name, args in bound.items():
        params = decls[name][1]
        assert len(args) == len(params), (name, len(args), len(params))
        for k, (a, p) in enumerate(zip(args, params)):
            assert a in _ctype_of(p) or issubclass(a, ctypes._Pointer) and ctypes._Pointer in _ctype_of(p), (name, k, p, a)


def test_workspace_sizes_are_the_recorded_ones():
    # tests/golden/workspace_bytes.json: written by tools/gen_workspace_golden.py (which holds the shapes) before the layouts moved
    # onto h3d_ws_layout; region order, sizes and alignment of every workspace are part of what a caller may have sized buffers by
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("gen_workspace_golden", os.path.join(ROOT, "tools", "gen_workspace_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")))
    got = json.loads(json.dumps(gen.table()))
    assert set(got) == set(want) and all(len(rows) >= 12 for rows in want.values())
    for name in want:
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)
        assert len(got[name]) == len(want[name]), name


def test_op_struct_matches_header_layout():
    # 2 int32, 5 pointers, 18 int32 (ABI 2: + wexp, wexp2) -> 8 + 40 + 72 = 120 bytes on LP64
    assert ctypes.sizeof(_lib.H3dOp) == 120 and _lib.H3dOp.wexp.offset == 112
    assert _lib.H3dOp.in_.offset == 8 and _lib.H3dOp.B.offset == 48


def test_null_and_bad_arguments_return_error_codes_without_a_gpu():
    L = _lib.lib()
    rc = L.h3d_run_ops(None, 0, None)
    assert rc == -5 and b"null plan" in L.h3d_last_error()
    rc = L.h3d_nms_topk(None, 1, 1, 4, 4, 2, 0, None, None, None, None, None)
    assert rc == -5
    with pytest.raises(RuntimeError, match="argument error"):
        _lib.check(rc, "nms_topk")


def test_product_has_no_cpu_fallback():
    m = model.dla_net(HEADS, not_use_dcn=True)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        m(torch.zeros(1, 3, 64, 64))
    from h3d_amd import decode
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        decode.multi_pose_decode(torch.zeros(1, 1, 8, 8), torch.zeros(1, 2, 8, 8), torch.zeros(1, 34, 8, 8), K=4)
    src = "".join(open(os.path.join(ROOT, "human-3d-reconstruction_amd", f)).read()
                  for f in os.listdir(os.path.join(ROOT, "human-3d-reconstruction_amd")) if f.endswith(".py"))
    assert "import oracle" not in src and "from oracle" not in src


def test_flop_table_matches_survey():
    # 80.48 / 75.83 GFLOP per image incl. two dead 1x1 `project` convs (0.134 GFLOP) we skip
    assert abs(arch.conv_flops(HEADS, True) / 1e9 - (80.48 - 0.134)) < 0.02
    assert abs(arch.conv_flops(HEADS, False) / 1e9 - (75.83 - 0.134)) < 0.02


def test_default_init_follows_reference_rules():
    torch.manual_seed(0)
    m = model.dla_net(HEADS)
    sd = m.state_dict()
    assert float(sd["hm.2.bias"]) == pytest.approx(-2.19) and float(sd["hm_hp.2.bias"][3]) == pytest.approx(-2.19)
    assert sd["wh.0.bias"].abs().max() == 0 and sd["reg.2.bias"].abs().max() == 0
    assert sd["hm.0.bias"].abs().max() > 0
    assert sd["dla_up.ida_0.proj_1.conv.conv_offset_mask.weight"].abs().max() == 0
    assert sd["dla_up.ida_0.proj_1.conv.bias"].abs().max() == 0
    w = sd["ida_up.up_2.weight"]
    assert w.shape == (64, 1, 8, 8) and torch.equal(w[0], w[5])
    assert float(w[0, 0, 3, 3]) == pytest.approx((1 - abs(3 / 4 - 0.875)) ** 2)
    assert float(sd["base.level2.root.bn.running_var"][0]) == 1.0


def test_shard_batch_partitions():
    for n, world in [(64, 8), (10, 4), (3, 8), (128, 8)]:
        spans = [detector.shard_batch(n, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
        assert max(b - a for a, b in spans) - min(b - a for a, b in spans) <= 1


@pytest.mark.parametrize("world,port", [(2, 29531), (4, 29537)])
def test_gather_detections_gloo(world, port):
    # even and uneven shards (n = 8, 9, 10, ...), see tests/dist_worker.py
    script = os.path.join(ROOT, "tests", "dist_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % world,
                        "--master-addr", "127.0.0.1", "--master-port", str(port), script],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "DIST_OK" in r.stdout


def test_bench_launches_its_own_ranks_gloo_dry_run():
    # `python bench.py --gpus 2` without torchrun must start 2 ranks itself and relay rank 0's JSON line; --dry-run
    # replaces the GPU step by the collective on CPU tensors over gloo (no HIP call anywhere), everything else --
    # launcher, rendezvous on 127.0.0.1, barriers, max-over-ranks timing, the line's contract fields -- is the real code
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--dry-run", "--batch", "5"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["steps"] == 3 and line["warmup"] == 1
    assert line["config"]["global_batch"] == 10 and line["dry_run"] is True and line["scaling"] == "weak"


def test_bench_strong_scaling_mode_splits_one_batch_gloo_dry_run():
    # `--global-batch G`: ONE batch of G images per step for the whole job, rank r takes shard_batch(G, r, world) -- the
    # reference's DataParallel scatter (trains/trainer.py:176; SURVEY 8e: 64 -> 8 per GPU).  Uneven split (9 over 2 ranks: 5 + 4):
    # the padded fixed-size all-gather and the pad-row removal are the real code; the line says "strong".
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--dry-run", "--global-batch", "9"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert line["scaling"] == "strong" and line["n_gpus"] == 2 and line["rccl_ranks"] == 2
    assert line["config"]["global_batch"] == 9 and line["config"]["batch_per_gpu"] == 5       # rank 0's share


def test_flip_helpers_match_the_reference_semantics():
    # models/utils.py:29-51 (flip test): host helpers (torch, device-resident) vs the numpy restatement
    import numpy as np
    import torch
    from h3d_amd import utils
    from oracle import decode as odec
    flip_idx = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]      # COCO left/right joints
    rng = np.random.default_rng(0)
    hm = rng.standard_normal((2, 17, 6, 10)).astype(np.float32)
    hps = rng.standard_normal((2, 34, 6, 10)).astype(np.float32)
    assert np.array_equal(utils.flip_tensor(torch.from_numpy(hm)).numpy(), odec.flip_tensor(hm))
    assert np.array_equal(utils.flip_lr(torch.from_numpy(hm), flip_idx).numpy(), odec.flip_lr(hm, flip_idx))
    assert np.array_equal(utils.flip_lr_off(torch.from_numpy(hps), flip_idx).numpy(), odec.flip_lr_off(hps, flip_idx))
    # overlapping pairs are applied in sequence, as the reference's loop does
    odd = [[0, 1], [1, 2]]
    assert np.array_equal(utils.flip_lr(torch.from_numpy(hm), odd).numpy(), odec.flip_lr(hm, odd))


def test_f16x3_filter_split_is_exact_to_23_bits_and_prescaled_into_the_normal_range():
    """Host half of the f16x3 plans (engine.x3_split / x3_exp; csrc/common.h ET<x3_t>): per 8 consecutive K elements the 8 fp16 high
    terms then the 8 low terms in the 32 bytes of the fp32 values; hi + lo reproduces x to 2^-23 relative once the bank is pre-scaled
    so that its low terms are normal fp16 numbers (an unscaled 0.05 is only good to 2^-20.7)."""
    import numpy as np
    from h3d_amd import engine
    rng = np.random.default_rng(0)
    w = torch.from_numpy((rng.standard_normal((24, 9, 32)) * 0.05).astype(np.float32))
    e = engine.x3_exp(w)
    assert 2.0 ** 13 <= float(w.abs().max()) * 2.0 ** e < 2.0 ** 14
    s = engine.x3_split(w * 2.0 ** e)
    assert s.shape == w.shape and s.dtype == torch.float32
    h = s.contiguous().view(torch.float16).reshape(-1, 4, 2, 8)          # [rows, K/8, (hi | lo), 8]
    hi, lo = h[:, :, 0].float().reshape(w.shape), h[:, :, 1].float().reshape(w.shape)
    assert torch.equal(hi, (w * 2.0 ** e).half().float())
    back = (hi.double() + lo.double()) * 2.0 ** -e
    rel = ((back - w.double()).abs() / w.double().abs().clamp_min(1e-30))
    big = w.abs() > float(w.abs().max()) * 2.0 ** -15                    # filters whose low term is a normal fp16 number
    assert float(rel[big].max()) <= 2.0 ** -23 * 1.01
    # without the pre-scale the same bank is an order of magnitude coarser: the reason h3d_op.wexp exists
    s0 = engine.x3_split(w).contiguous().view(torch.float16).reshape(-1, 4, 2, 8)
    back0 = s0[:, :, 0].double().reshape(w.shape) + s0[:, :, 1].double().reshape(w.shape)
    assert float(((back0 - w.double()).abs() / w.double().abs().clamp_min(1e-30))[big].max()) > 2.0 ** -21
    assert engine.x3_exp(torch.zeros(4, 8)) == 0


def test_build_flags_and_default_library_has_no_superseded_generations():
    L = _lib.lib()
    flags = L.h3d_build_flags()
    assert flags & ~3 == 0
    assert _lib.has_extra() == bool(flags & 1)


def test_plan_faithful_emulation_rounds_where_the_plans_round():
    """oracle/dla.py emulate='bf16_plan' (round 5): small input, CPU only -- it is a bf16-level evaluation of the graph
    (close to the fp32 oracle, not equal), differs from the older conv-input emulation, and with no rounding point selected
    (plan_parts=[]) it is that older emulation's treatment up to the up-sampling tap weights, which the plans keep in fp32."""
    import numpy as np
    from h3d_amd import synth
    from oracle import dla as odla
    heads = {"hm": 1, "wh": 2}
    sd = synth.synth_state_dict(arch.state_dict_shapes(heads, True), seed=0, gain=1.25)
    x = torch.from_numpy(synth.synth_images(1, 64, 64, seed=3))
    with torch.no_grad():
        ref = odla.DLAOracle(sd, heads, use_dcn=True)(x)[0]["hm"]
        old = odla.DLAOracle(sd, heads, use_dcn=True, emulate="bf16")(x)[0]["hm"]
        plan = odla.DLAOracle(sd, heads, use_dcn=True, emulate="bf16_plan")(x)[0]["hm"]
        none = odla.DLAOracle(sd, heads, use_dcn=True, emulate="bf16_plan", plan_parts=[])(x)[0]["hm"]
    scale = float(ref.abs().max())
    for t in (old, plan, none):
        e = float((t - ref).abs().max())
        assert 1e-4 * scale < e < 0.2 * scale, (e, scale)
    assert float((plan - old).abs().max()) > 0
    # plan_parts=[]: conv inputs and raw filters rounded, BatchNorm in fp32 -- the 'bf16' mode's arithmetic except for the depthwise
    # up-sampling weights (fp32 in every plan, rounded by emulate='bf16'): closer to it than either is to fp32
    assert float((none - old).abs().max()) < 0.5 * float((old - ref).abs().max())


# ---- h3d_op.reserved: the flag catalogue of include/h3d.h ------------------------------------------------------------------------
def _flag_catalogue():
    """(groups, defines, macros) of the catalogue section of include/h3d.h: groups = one {name: value} per enum block."""
    text = open(os.path.join(ROOT, "include", "h3d.h")).read()
    text = text[text.index("h3d_op.reserved: the flag catalogue"):text.index("end of the flag catalogue")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    groups = [{n: int(v, 0) for n, v in re.findall(r"(H3D_\w+)\s*=\s*(0x[0-9a-fA-F]+|\d+)", body)} for body in re.findall(r"enum\s*\{(.*?)\}", code, flags=re.S)]
    defines = {n: int(v, 0) for n, v in re.findall(r"^#define (H3D_\w+) (0x[0-9a-fA-F]+|\d+)\s*$", code, flags=re.M)}
    macros = {n: (a.replace(" ", "").split(","), b) for n, a, b in re.findall(r"^#define (H3D_\w+)\(([\w, ]+)\) (.+?)\s*$", code, flags=re.M)}
    return groups, defines, macros


def test_flag_catalogue_is_mirrored_in_lib_and_no_two_flags_of_a_group_collide():
    groups, defines, macros = _flag_catalogue()
    assert len(groups) >= 10 and sum(len(g) for g in groups) >= 40 and len(macros) >= 8, (groups, macros)
    for g in groups + [defines]:
        for name, value in g.items():
            assert getattr(_lib, name[len("H3D_"):]) == value, name
    # the function-like macros: the C body is a Python expression too, over its arguments and the enumerators
    names = {n: v for g in groups for n, v in g.items()}
    for name, (args, body) in macros.items():
        fn = getattr(_lib, name[len("H3D_"):])
        for vals in ((1, 2, 16), (4, 8, 32), (6, 4, 8), (0x12345678, 2, 8)):
            vals = vals[:len(args)]
            assert fn(*vals) == eval(body, dict(names, **dict(zip(args, vals)))), (name, vals)
    # within one group (one op kind and dtype class) and one family, no two flags share a bit (masks name several bits on purpose;
    # H3D_OP_UPADD's two names are values of the whole word, not bits)
    for g in groups:
        for fam in ("H3D_OPF_", "H3D_TUNE_"):
            flags = [(n, v) for n, v in g.items() if n.startswith(fam) and not n.endswith("_MASK") and not n.startswith("H3D_TUNE_UPADD_")]
            for i, (n1, v1) in enumerate(flags):
                for n2, v2 in flags[i + 1:]:
                    assert not v1 & v2, (n1, n2)
    assert _lib.OPF_DCN_STREAM_VARIANT_MASK == (_lib.OPF_DCN_STREAM_WIDE_MARGIN | _lib.OPF_DCN_STREAM_SLOTS512 | _lib.OPF_DCN_STREAM_F16_INPUT
                                                | _lib.TUNE_DCN_STREAM_FORCE_NARROW_WG | _lib.TUNE_DCN_STREAM_FORCE_WIDE_WG)


def _dry_op(kind, dtype, reserved, B, Cin, Cout, H, W, ksize, stride, keep):
    """An h3d_op over fake device pointers: enough for h3d_op_kernel_name's dry run, which launches nothing."""
    fake = 0x10000
    op = _lib.H3dOp()
    op.kind, op.dtype, op.reserved = kind, getattr(_lib, "H3D_" + dtype), reserved
    op.in_, op.w, op.bias, op.out = fake, fake, fake, fake
    up = kind == _lib.OP_UPADD
    op.B, op.H, op.W, op.Cin, op.in_cs, op.Cout, op.out_cs = B, H, W, Cin, Cin, Cout, Cout
    op.Ho, op.Wo = (H * stride, W * stride) if up else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    op.ksize, op.stride, op.relu, op.out_mode, op.wrows = ksize, stride, 1, _lib.OUT_NHWC, -(-Cout // 128) * 128
    if kind == _lib.OP_HEADS:
        d = _lib.H3dHeadsDesc()
        d.nheads = 2
        for i in range(2):
            d.head[i].w2, d.head[i].b2, d.head[i].out, d.head[i].C = fake, fake, fake, 2
        keep.append(d)
        op.in2 = ctypes.addressof(d)
    elif kind not in (_lib.OP_CONV, _lib.OP_CONV_STREAM):
        op.in2, op.in2_cs = fake, Cin if up else 32
    return op


def _dry_op_with(case, over, keep):
    """_dry_op, then the overrides: an h3d_op field by name, "heads": the widths of the heads, "updcn": an h3d_updcn_desc behind in2."""
    op, fake = _dry_op(*case, keep), 0x10000
    for k, v in over.items():
        if k == "heads":
            d = keep[-1]
            d.nheads = len(v)
            for i, c in enumerate(v):
                d.head[i].w2, d.head[i].b2, d.head[i].out, d.head[i].C = fake, fake, fake, c
        elif k == "updcn":
            d = _lib.H3dUpdcnDesc()
            d.skip, d.w_up, d.w_off, d.skip_cs = fake, fake, fake, v
            keep.append(d)
            op.in2 = ctypes.addressof(d)
        else:
            setattr(op, k, v)
    return op


L = _lib
S, F, D, C2, C, U, HD, F16K = L.OP_DCN_FUSED_STREAM, L.OP_DCN_FUSED, L.OP_DCN, L.OP_CONV_STREAM, L.OP_CONV, L.OP_UPADD, L.OP_HEADS, L.OP_DCN_FUSED_F16
# (kind, dtype, reserved, B, Cin, Cout, H, W, ksize, stride, kernel name).  The names are what the library printed for the same words
# written in hex BEFORE the flags had names (recorded from that build, pasted as literals): a word selects the kernel it always did.
DISPATCH = [
    # H3D_OP_DCN_FUSED_STREAM, bf16: 128 -> 64 @24x40 (two workgroups per CU)
    (S, "BF16", 0, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_NO_SLOTS, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 1, 2, true, 0>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 4, 2, true, 256, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 512, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_F16_INPUT, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 256, false, true>"),
    (S, "BF16", L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN | L.OPF_DCN_STREAM_F16_INPUT, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 4, 2, true, 256, true, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512 | L.OPF_DCN_STREAM_F16_INPUT, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 512, true, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN | L.OPF_DCN_STREAM_SLOTS512, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 4, 2, true, 256, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_NO_SLOTS | L.OPF_DCN_STREAM_WIDE_MARGIN, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 1, 2, true, 0>"),
    (S, "BF16", L.OPF_DCN_STREAM_STATS, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 256>"),
    # ... 256 -> 256 @16x16: a small grid, 64-channel workgroups unless forced wide
    (S, "BF16", 0, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 256>"),
    (S, "BF16", L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 4, 2, true, 256>"),
    (S, "BF16", L.TUNE_DCN_STREAM_FORCE_NARROW_WG, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 256>"),
    (S, "BF16", L.TUNE_DCN_STREAM_FORCE_NARROW_WG | L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 4, 2, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 4, 2, true, 256, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN | L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 4, 2, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 512, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512 | L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 4, 2, true, 512>"),
    (S, "BF16", L.OPF_DCN_STREAM_F16_INPUT | L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 4, 2, true, 256, false, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512 | L.OPF_DCN_STREAM_F16_INPUT | L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 4, 2, true, 512, false, true>"),
    # ... 256 -> 256 @32x32 at batch 64: 512 wide workgroups, 128-channel workgroups unless forced narrow
    (S, "BF16", 0, 64, 256, 256, 32, 32, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 4, 2, true, 256>"),
    (S, "BF16", L.TUNE_DCN_STREAM_FORCE_NARROW_WG, 64, 256, 256, 32, 32, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN | L.TUNE_DCN_STREAM_FORCE_NARROW_WG, 64, 256, 256, 32, 32, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 4, 2, true, 256, true>"),
    # ... <= 32 output channels
    (S, "BF16", 0, 1, 64, 32, 20, 20, 3, 1, "dcn3_kernel<unsigned short, 1, 16, 2, 1, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_NO_SLOTS, 1, 64, 32, 20, 20, 3, 1, "dcn3_kernel<unsigned short, 1, 16, 1, 1, true, 0>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN, 1, 64, 32, 20, 20, 3, 1, "dcn3_kernel<unsigned short, 1, 16, 4, 1, true, 256, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512, 1, 64, 32, 20, 20, 3, 1, "dcn3_kernel<unsigned short, 1, 16, 2, 1, true, 512, true>"),
    # ... fp16 plans: F16_INPUT is not read; the dcn5 request is in DISPATCH_DCN5 below
    (S, "F16", 0, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<f16_t, 2, 16, 2, 2, true, 256>"),
    (S, "F16", L.OPF_DCN_STREAM_F16_INPUT, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<f16_t, 2, 16, 2, 2, true, 256>"),
    (S, "F16", L.OPF_DCN_STREAM_WIDE_MARGIN, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<f16_t, 2, 16, 4, 2, true, 256, true>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_F16_KEEP_DCN3, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<f16_t, 2, 16, 2, 2, true, 256>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.OPF_DCN_STREAM_NO_SLOTS, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<f16_t, 2, 16, 1, 2, true, 0>"),
    # H3D_OP_DCN_FUSED_STREAM, f16x3: the margins
    (S, "F16X3", 0, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<x3_t, 2, 16, 2, 1, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN2, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<x3_t, 2, 16, 2, 1, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN3, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<x3_t, 2, 16, 3, 1, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN4, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<x3_t, 2, 16, 4, 1, true, 256>"),
    (S, "F16X3", 0, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<x3_t, 2, 16, 4, 1, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN2, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<x3_t, 2, 16, 2, 1, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN3 | L.TUNE_DCN_STREAM_X3_MARGIN4, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<x3_t, 2, 16, 3, 1, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN2 | L.TUNE_DCN_STREAM_X3_MARGIN4, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<x3_t, 2, 16, 2, 1, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN4, 1, 64, 32, 20, 20, 3, 1, "dcn3_kernel<x3_t, 1, 16, 4, 1, true, 256>"),
    # H3D_OP_DCN_FUSED, f16x3: the margins and the `DCN` module's contract flags
    (F, "F16X3", 0, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<x3_t, 2, 16, 4, 1, false, 0>"),
    (F, "F16X3", L.OPF_DCN_FUSED_RAW_PACK | L.OPF_DCN_FUSED_SCALED_INPUT, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<x3_t, 2, 16, 4, 1, false, 0>"),
    (F, "F16X3", L.TUNE_DCN_FUSED_X3_MARGIN2, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<x3_t, 2, 16, 2, 1, false, 0>"),
    (F, "F16X3", L.TUNE_DCN_FUSED_X3_MARGIN6, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<x3_t, 2, 16, 6, 1, false, 0>"),
    (F, "F16X3", L.TUNE_DCN_FUSED_X3_MARGIN4, 2, 128, 64, 24, 40, 3, 1, "dcn3_kernel<x3_t, 2, 16, 4, 1, false, 0>"),
    (F, "F16X3", 0, 1, 64, 64, 64, 16, 3, 1, "dcn3_kernel<x3_t, 2, 16, 6, 1, false, 0>"),
    (F, "F16X3", L.TUNE_DCN_FUSED_X3_MARGIN4, 1, 64, 64, 64, 16, 3, 1, "dcn3_kernel<x3_t, 2, 16, 4, 1, false, 0>"),
    (F, "F16X3", L.TUNE_DCN_FUSED_X3_MARGIN6 | L.TUNE_DCN_FUSED_X3_MARGIN4, 1, 64, 64, 64, 16, 3, 1, "dcn3_kernel<x3_t, 2, 16, 4, 1, false, 0>"),
    (F, "F16X3", L.TUNE_DCN_FUSED_X3_MARGIN6, 1, 32, 32, 16, 16, 3, 1, "dcn3_kernel<x3_t, 1, 16, 6, 1, false, 0>"),
    # H3D_OP_DCN_FUSED, 2-byte: the workgroup width
    (F, "BF16", 0, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 2, 32, 2, 2, false, 0>"),
    (F, "BF16", L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 256, 256, 16, 16, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 2, 2, false, 0>"),
    (F, "BF16", L.TUNE_DCN_STREAM_FORCE_NARROW_WG, 64, 256, 256, 32, 32, 3, 1, "dcn3_kernel<unsigned short, 2, 32, 2, 2, false, 0>"),
    (F, "BF16", L.TUNE_DCN_STREAM_FORCE_NARROW_WG, 64, 144, 128, 32, 32, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 2, false, 0>"),
    (F, "F16", L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 128, 128, 24, 40, 3, 1, "dcn3_kernel<f16_t, 4, 16, 2, 2, false, 0>"),
    # H3D_OP_DCN: the operator boundary's word
    (D, "F16X3", L.OPF_DCN_MASK_FINAL | L.OPF_DCN_RAW_PACK | L.OPF_DCN_ACT_MAXIMA, 2, 128, 64, 24, 40, 3, 1, "dcn2_kernel<x3_t, 2, 16, 2, 1>"),
    (D, "F16X3", L.OPF_DCN_RAW_PACK, 1, 64, 32, 20, 20, 3, 1, "dcn2_kernel<x3_t, 1, 16, 2, 1>"),
    (D, "F32", L.OPF_DCN_MASK_FINAL, 2, 128, 64, 24, 40, 3, 1, "dcn2_kernel<float, 2, 16, 2, 1>"),
    (D, "BF16", L.OPF_DCN_MASK_FINAL, 2, 128, 64, 24, 40, 3, 1, "dcn2_kernel<unsigned short, 2, 32, 2, 1>"),
    # H3D_OP_CONV_STREAM: tile codes of every variant nibble, the auto code, round 4's rule
    (C2, "BF16", 0, 2, 64, 128, 40, 24, 3, 1, "conv2_kernel<unsigned short, 1, 4, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_AUTO, 2, 64, 128, 40, 24, 3, 1, "conv2_kernel<unsigned short, 1, 4, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(0, 4, 16), 2, 64, 128, 40, 24, 3, 1, "conv2_kernel<unsigned short, 4, 16, 2, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(0, 1, 4), 1, 48, 32, 10, 18, 3, 1, "conv2_kernel<unsigned short, 1, 4, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(2, 4, 8), 1, 64, 128, 40, 24, 3, 1, "conv2_kernel<unsigned short, 4, 8, 2, 1, 2, 2>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(3, 2, 8), 1, 96, 64, 24, 24, 3, 1, "conv2_kernel<unsigned short, 2, 8, 2, 1, 3, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(5, 2, 8), 1, 64, 64, 24, 24, 3, 1, "conv2_kernel<unsigned short, 2, 8, 2, 1, 1, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(6, 4, 8), 1, 128, 128, 24, 40, 3, 1, "conv2_kernel<unsigned short, 4, 8, 2, 1, 2, 1, true>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(6, 2, 8), 2, 64, 64, 24, 40, 3, 1, "conv2_kernel<f16_t, 2, 8, 2, 1, 2, 1, true>"),
    (C2, "BF16", 0, 1, 128, 256, 24, 24, 3, 2, "conv2_kernel<unsigned short, 4, 4, 2, 2, 1, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(2, 4, 4), 1, 128, 256, 24, 24, 3, 2, "conv2_kernel<unsigned short, 4, 4, 2, 2, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(4, 4, 8), 1, 64, 128, 40, 24, 3, 2, "conv2_kernel<unsigned short, 4, 8, 2, 2, 1, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(4, 2, 4), 1, 64, 64, 24, 40, 3, 2, "conv2_kernel<unsigned short, 2, 4, 2, 2, 1, 1>"),
    (C2, "BF16", 0, 16, 128, 256, 4, 4, 3, 1, "conv2_kernel<unsigned short, 1, 4, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_ROUND4_RULE, 16, 128, 256, 4, 4, 3, 1, "conv2_kernel<unsigned short, 4, 4, 2, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_AUTO | L.TUNE_CONV_STREAM_ABLATE(4), 2, 64, 128, 40, 24, 3, 1, "conv2_kernel<unsigned short, 1, 4, 1, 1, 2, 1>"),
    # H3D_OP_CONV 1x1, 2-byte: GEMM kernel (three tiles, forced, refused) and the halo-tile kernel's tile override
    (C, "BF16", 0, 2, 128, 256, 24, 24, 1, 1, "conv_kernel<unsigned short, 1, 1, 4, 64, 8, 4, 2>"),
    (C, "BF16", L.TUNE_CONV_FORCE_GEMM, 2, 128, 64, 24, 24, 1, 1, "gemm1_kernel<unsigned short, 2, 2, 2, 2, 2, 2>"),
    (C, "BF16", 0, 2, 128, 64, 24, 24, 1, 1, "conv_kernel<unsigned short, 1, 1, 2, 64, 8, 4, 2>"),
    (C, "BF16", L.TUNE_CONV_FORCE_GEMM | L.TUNE_CONV_GEMM_TILE(1), 2, 128, 256, 24, 24, 1, 1, "gemm1_kernel<unsigned short, 4, 2, 2, 4, 2, 2>"),
    (C, "BF16", L.TUNE_CONV_FORCE_GEMM | L.TUNE_CONV_GEMM_TILE(2), 2, 128, 256, 24, 24, 1, 1, "gemm1_kernel<unsigned short, 2, 2, 2, 4, 3, 2>"),
    (C, "BF16", L.TUNE_CONV_FORCE_GEMM | L.TUNE_CONV_GEMM_TILE(3), 2, 128, 256, 24, 24, 1, 1, "gemm1_kernel<unsigned short, 2, 2, 2, 2, 2, 2>"),
    (C, "BF16", L.TUNE_CONV_HALO_TILE, 2, 128, 256, 24, 24, 1, 1, "conv_kernel<unsigned short, 1, 1, 4, 64, 8, 4, 2>"),
    (C, "BF16", L.TUNE_CONV_FORCE_GEMM | L.TUNE_CONV_HALO_TILE, 2, 128, 256, 24, 24, 1, 1, "conv_kernel<unsigned short, 1, 1, 4, 64, 8, 4, 2>"),
    (C, "BF16", L.TUNE_CONV_1X1_TILE(4, 16), 2, 128, 256, 24, 24, 1, 1, "conv_kernel<unsigned short, 1, 1, 4, 64, 16, 4, 2>"),
    (C, "BF16", L.TUNE_CONV_1X1_TILE(2, 8), 2, 128, 256, 24, 24, 1, 1, "conv_kernel<unsigned short, 1, 1, 2, 64, 8, 4, 2>"),
    (C, "F16", L.TUNE_CONV_1X1_TILE(2, 16), 2, 128, 64, 24, 24, 1, 1, "conv_kernel<f16_t, 1, 1, 2, 64, 16, 4, 2>"),
    # H3D_OP_CONV, f16x3: 3x3 tiles, the 1x1 chunk / tile overrides
    (C, "F16X3", 0, 1, 64, 128, 32, 32, 3, 1, "conv_kernel<x3_t, 3, 1, 2, 16, 32, 8, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(4, 8, 16), 1, 64, 128, 32, 32, 3, 1, "conv_kernel<x3_t, 3, 1, 4, 16, 16, 8, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(1, 4, 16), 1, 64, 32, 32, 32, 3, 1, "conv_kernel<x3_t, 3, 1, 1, 16, 16, 4, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(2, 4, 8), 1, 64, 64, 32, 32, 3, 2, "conv_kernel<x3_t, 3, 2, 2, 16, 8, 4, 1>"),
    (C, "F16X3", 0, 1, 128, 128, 16, 16, 1, 1, "conv_kernel<x3_t, 1, 1, 4, 64, 8, 4, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_CK16, 1, 128, 128, 16, 16, 1, 1, "conv_kernel<x3_t, 1, 1, 2, 16, 16, 4, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_MT2, 1, 128, 128, 16, 16, 1, 1, "conv_kernel<x3_t, 1, 1, 2, 64, 8, 4, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_CK16 | L.TUNE_CONV_X3_MT2, 1, 128, 128, 16, 16, 1, 1, "conv_kernel<x3_t, 1, 1, 2, 16, 16, 4, 1>"),
    # H3D_OP_UPADD: the tap table's place (f = 2: ksize 4, stride 2)
    (U, "BF16", 0, 1, 256, 256, 8, 8, 4, 2, "upadd_kernel<unsigned short, false, false>"),
    (U, "BF16", L.TUNE_UPADD_TAPS_LDS, 1, 256, 256, 8, 8, 4, 2, "upadd_kernel<unsigned short, false, true>"),
    (U, "BF16", 0, 1, 64, 64, 8, 8, 4, 2, "upadd_kernel<unsigned short, false, true>"),
    (U, "BF16", L.TUNE_UPADD_TAPS_GLOBAL, 1, 64, 64, 8, 8, 4, 2, "upadd_kernel<unsigned short, false, false>"),
    # H3D_OP_HEADS
    (HD, "BF16", 0, 1, 64, 64, 16, 32, 3, 1, "heads_kernel<unsigned short, 16, 1, true>"),
    (HD, "BF16", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, "heads_kernel<unsigned short, 16, 1, false>"),
    (HD, "F32", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, "heads_kernel<float, 8, 1, false>"),
    # Every other kernel instantiation of the op launchers (csrc: conv, conv2, gemm1, stem3, extra, heads, dcn2, dcn3) that neither a row
    # above nor an op of tests/golden/plan_ops.json.gz names, each with the smallest op found for it.  Names recorded from the library
    # BEFORE the launchers took name and kernel from one site (the parent commit's dry run).
    (S, "F16", 0, 1, 16, 16, 4, 4, 3, 1, "dcn3_kernel<f16_t, 1, 16, 1, 1, true, 0>"),
    (S, "F16", 0, 1, 32, 16, 4, 4, 3, 1, "dcn3_kernel<f16_t, 1, 16, 2, 1, true, 256>"),
    (S, "F16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 16, 4, 4, 3, 1, "dcn3_kernel<f16_t, 1, 16, 2, 1, true, 512, true>"),
    (S, "F16", L.OPF_DCN_STREAM_WIDE_MARGIN, 1, 32, 16, 4, 4, 3, 1, "dcn3_kernel<f16_t, 1, 16, 4, 1, true, 256, true>"),
    (S, "F16", 0, 1, 16, 36, 4, 4, 3, 1, "dcn3_kernel<f16_t, 2, 16, 1, 1, true, 0>"),
    (S, "F16", 0, 1, 32, 36, 4, 4, 3, 1, "dcn3_kernel<f16_t, 2, 16, 2, 1, true, 256>"),
    (S, "F16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 36, 4, 4, 3, 1, "dcn3_kernel<f16_t, 2, 16, 2, 1, true, 512, true>"),
    (S, "F16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 64, 4, 4, 3, 1, "dcn3_kernel<f16_t, 2, 16, 2, 2, true, 512, true>"),
    (S, "F16", L.OPF_DCN_STREAM_WIDE_MARGIN, 1, 32, 36, 4, 4, 3, 1, "dcn3_kernel<f16_t, 2, 16, 4, 1, true, 256, true>"),
    (S, "F16", 0, 1, 16, 68, 4, 4, 3, 1, "dcn3_kernel<f16_t, 4, 16, 2, 1, true, 0>"),
    (S, "F16", 0, 1, 32, 260, 128, 128, 3, 1, "dcn3_kernel<f16_t, 4, 16, 4, 1, true, 256>"),
    (S, "F16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 260, 128, 128, 3, 1, "dcn3_kernel<f16_t, 4, 16, 4, 1, true, 512>"),
    (S, "F16", 0, 1, 32, 512, 128, 128, 3, 1, "dcn3_kernel<f16_t, 4, 16, 4, 2, true, 256>"),
    (S, "F16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 512, 128, 128, 3, 1, "dcn3_kernel<f16_t, 4, 16, 4, 2, true, 512>"),
    (S, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 1, 1, true, 0>"),
    (S, "BF16", 0, 1, 32, 36, 4, 4, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 1, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 36, 4, 4, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 1, true, 512, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN, 1, 32, 36, 4, 4, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 4, 1, true, 256, true>"),
    (S, "BF16", 0, 1, 16, 68, 4, 4, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 2, 1, true, 0>"),
    (S, "BF16", 0, 1, 32, 260, 128, 128, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 4, 1, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 260, 128, 128, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 4, 1, true, 512>"),
    (S, "F16X3", 0, 1, 32, 16, 4, 4, 3, 1, "dcn3_kernel<x3_t, 1, 16, 2, 1, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN3, 1, 32, 16, 4, 4, 3, 1, "dcn3_kernel<x3_t, 1, 16, 3, 1, true, 256>"),
    (F, "F16", 0, 1, 16, 16, 4, 4, 3, 1, "dcn3_kernel<f16_t, 1, 16, 2, 1, false, 0>"),
    (F, "F16", 0, 1, 32, 16, 4, 4, 3, 1, "dcn3_kernel<f16_t, 1, 32, 2, 1, false, 0>"),
    (F, "F16", 0, 1, 16, 36, 4, 4, 3, 1, "dcn3_kernel<f16_t, 2, 16, 2, 1, false, 0>"),
    (F, "F16", 0, 1, 16, 64, 4, 4, 3, 1, "dcn3_kernel<f16_t, 2, 16, 2, 2, false, 0>"),
    (F, "F16", 0, 1, 32, 36, 4, 4, 3, 1, "dcn3_kernel<f16_t, 2, 32, 2, 1, false, 0>"),
    (F, "F16", 0, 1, 32, 64, 4, 4, 3, 1, "dcn3_kernel<f16_t, 2, 32, 2, 2, false, 0>"),
    (F, "F16", 0, 1, 16, 260, 128, 128, 3, 1, "dcn3_kernel<f16_t, 4, 16, 2, 1, false, 0>"),
    (F, "F32", 0, 1, 16, 16, 4, 4, 3, 1, "dcn3_kernel<float, 1, 16, 2, 1, false, 0>"),
    (F, "BF16", 0, 1, 16, 16, 4, 4, 3, 1, "dcn3_kernel<unsigned short, 1, 16, 2, 1, false, 0>"),
    (F, "BF16", 0, 1, 32, 16, 4, 4, 3, 1, "dcn3_kernel<unsigned short, 1, 32, 2, 1, false, 0>"),
    (F, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, "dcn3_kernel<unsigned short, 2, 16, 2, 1, false, 0>"),
    (F, "BF16", 0, 1, 32, 36, 4, 4, 3, 1, "dcn3_kernel<unsigned short, 2, 32, 2, 1, false, 0>"),
    (F, "BF16", 0, 1, 16, 260, 128, 128, 3, 1, "dcn3_kernel<unsigned short, 4, 16, 2, 1, false, 0>"),
    (F, "F16X3", L.TUNE_DCN_FUSED_X3_MARGIN2, 1, 16, 16, 4, 4, 3, 1, "dcn3_kernel<x3_t, 1, 16, 2, 1, false, 0>"),
    (F, "F16X3", 0, 1, 16, 16, 4, 4, 3, 1, "dcn3_kernel<x3_t, 1, 16, 4, 1, false, 0>"),
    (D, "F32", 0, 1, 16, 16, 4, 4, 3, 1, "dcn2_kernel<float, 1, 16, 2, 1>"),
    (D, "BF16", 0, 1, 16, 16, 4, 4, 3, 1, "dcn2_kernel<unsigned short, 1, 16, 2, 2>"),
    (D, "BF16", 0, 1, 32, 16, 4, 4, 3, 1, "dcn2_kernel<unsigned short, 1, 32, 2, 2>"),
    (D, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, "dcn2_kernel<unsigned short, 2, 16, 2, 2>"),
    (C2, "F16", 0, 1, 16, 16, 4, 4, 3, 2, "conv2_kernel<f16_t, 1, 4, 1, 2, 2, 1>"),
    (C2, "F16", 0, 64, 16, 16, 24, 40, 3, 1, "conv2_kernel<f16_t, 1, 8, 1, 1, 1, 1>"),
    (C2, "F16", 0, 1, 16, 128, 128, 128, 3, 1, "conv2_kernel<f16_t, 1, 8, 1, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(3, 1, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 1, 8, 1, 1, 3, 1>"),
    (C2, "F16", 0, 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<f16_t, 2, 4, 1, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(4, 2, 4), 1, 16, 36, 4, 4, 3, 2, "conv2_kernel<f16_t, 2, 4, 1, 2, 1, 1>"),
    (C2, "F16", 0, 1, 16, 36, 4, 4, 3, 2, "conv2_kernel<f16_t, 2, 4, 1, 2, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(4, 2, 4), 1, 16, 16, 4, 4, 3, 2, "conv2_kernel<f16_t, 2, 4, 2, 2, 1, 1>"),
    (C2, "F16", 0, 1, 16, 64, 4, 4, 3, 2, "conv2_kernel<f16_t, 2, 4, 2, 2, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(5, 2, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<f16_t, 2, 8, 1, 1, 1, 1>"),
    (C2, "F16", 0, 1, 16, 260, 128, 128, 3, 1, "conv2_kernel<f16_t, 2, 8, 1, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(2, 2, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<f16_t, 2, 8, 1, 1, 2, 2>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(3, 2, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<f16_t, 2, 8, 1, 1, 3, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(5, 2, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 2, 8, 2, 1, 1, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(0, 2, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 2, 8, 2, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(2, 2, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 2, 8, 2, 1, 2, 2>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(3, 2, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 2, 8, 2, 1, 3, 1>"),
    (C2, "F16", 0, 64, 16, 132, 32, 32, 3, 1, "conv2_kernel<f16_t, 4, 16, 1, 1, 2, 1>"),
    (C2, "F16", 0, 2, 16, 512, 128, 128, 3, 1, "conv2_kernel<f16_t, 4, 16, 2, 1, 2, 1, true>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(0, 4, 16), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 16, 2, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(0, 4, 4), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 4, 1, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(3, 4, 4), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 4, 1, 1, 3, 1>"),
    (C2, "F16", 0, 1, 16, 132, 4, 4, 3, 2, "conv2_kernel<f16_t, 4, 4, 1, 2, 1, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(2, 4, 4), 1, 16, 132, 4, 4, 3, 2, "conv2_kernel<f16_t, 4, 4, 1, 2, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(6, 4, 4), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 4, 2, 1, 2, 1, true>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(0, 4, 4), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 4, 2, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(3, 4, 4), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 4, 2, 1, 3, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(2, 4, 4), 1, 16, 128, 4, 4, 3, 2, "conv2_kernel<f16_t, 4, 4, 2, 2, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(5, 4, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 8, 1, 1, 1, 1>"),
    (C2, "F16", 0, 2, 16, 132, 128, 128, 3, 1, "conv2_kernel<f16_t, 4, 8, 1, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(2, 4, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 8, 1, 1, 2, 2>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(4, 4, 8), 1, 16, 36, 4, 4, 3, 2, "conv2_kernel<f16_t, 4, 8, 1, 2, 1, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(5, 4, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 8, 2, 1, 1, 1>"),
    (C2, "F16", 0, 1, 16, 512, 128, 128, 3, 1, "conv2_kernel<f16_t, 4, 8, 2, 1, 2, 1, true>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(0, 4, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 8, 2, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(2, 4, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<f16_t, 4, 8, 2, 1, 2, 2>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(4, 4, 8), 1, 16, 16, 4, 4, 3, 2, "conv2_kernel<f16_t, 4, 8, 2, 2, 1, 1>"),
    (C2, "BF16", 0, 1, 16, 16, 4, 4, 3, 2, "conv2_kernel<unsigned short, 1, 4, 1, 2, 2, 1>"),
    (C2, "BF16", 0, 64, 16, 16, 24, 40, 3, 1, "conv2_kernel<unsigned short, 1, 8, 1, 1, 1, 1>"),
    (C2, "BF16", 0, 1, 16, 128, 128, 128, 3, 1, "conv2_kernel<unsigned short, 1, 8, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(3, 1, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<unsigned short, 1, 8, 1, 1, 3, 1>"),
    (C2, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<unsigned short, 2, 4, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(4, 2, 4), 1, 16, 36, 4, 4, 3, 2, "conv2_kernel<unsigned short, 2, 4, 1, 2, 1, 1>"),
    (C2, "BF16", 0, 1, 16, 36, 4, 4, 3, 2, "conv2_kernel<unsigned short, 2, 4, 1, 2, 2, 1>"),
    (C2, "BF16", 0, 1, 16, 64, 4, 4, 3, 2, "conv2_kernel<unsigned short, 2, 4, 2, 2, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(5, 2, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<unsigned short, 2, 8, 1, 1, 1, 1>"),
    (C2, "BF16", 0, 1, 16, 260, 128, 128, 3, 1, "conv2_kernel<unsigned short, 2, 8, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(2, 2, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<unsigned short, 2, 8, 1, 1, 2, 2>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(3, 2, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<unsigned short, 2, 8, 1, 1, 3, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(0, 2, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<unsigned short, 2, 8, 2, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(2, 2, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<unsigned short, 2, 8, 2, 1, 2, 2>"),
    (C2, "BF16", 0, 64, 16, 132, 32, 32, 3, 1, "conv2_kernel<unsigned short, 4, 16, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(0, 4, 4), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<unsigned short, 4, 4, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(3, 4, 4), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<unsigned short, 4, 4, 1, 1, 3, 1>"),
    (C2, "BF16", 0, 1, 16, 132, 4, 4, 3, 2, "conv2_kernel<unsigned short, 4, 4, 1, 2, 1, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(2, 4, 4), 1, 16, 132, 4, 4, 3, 2, "conv2_kernel<unsigned short, 4, 4, 1, 2, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(6, 4, 4), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<unsigned short, 4, 4, 2, 1, 2, 1, true>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(3, 4, 4), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<unsigned short, 4, 4, 2, 1, 3, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(5, 4, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<unsigned short, 4, 8, 1, 1, 1, 1>"),
    (C2, "BF16", 0, 2, 16, 132, 128, 128, 3, 1, "conv2_kernel<unsigned short, 4, 8, 1, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(2, 4, 8), 1, 16, 36, 4, 4, 3, 1, "conv2_kernel<unsigned short, 4, 8, 1, 1, 2, 2>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(4, 4, 8), 1, 16, 36, 4, 4, 3, 2, "conv2_kernel<unsigned short, 4, 8, 1, 2, 1, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(5, 4, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<unsigned short, 4, 8, 2, 1, 1, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(0, 4, 8), 1, 16, 16, 4, 4, 3, 1, "conv2_kernel<unsigned short, 4, 8, 2, 1, 2, 1>"),
    (C, "F16", 0, 1, 16, 16, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 1, 16, 16, 4, 1>"),
    (C, "F16", 0, 1, 64, 16, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 1, 64, 16, 4, 1>"),
    (C, "F16", 0, 1, 16, 36, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 2, 16, 16, 4, 1>"),
    (C, "F16", L.TUNE_CONV_1X1_TILE(2, 16), 1, 64, 36, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 2, 64, 16, 4, 1>"),
    (C, "F16", 0, 1, 64, 36, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 2, 64, 8, 4, 1>"),
    (C, "F16", 0, 1, 16, 68, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 4, 16, 16, 4, 1>"),
    (C, "F16", 0, 1, 16, 128, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 4, 16, 16, 4, 2>"),
    (C, "F16", L.TUNE_CONV_1X1_TILE(4, 16), 1, 64, 36, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 4, 64, 16, 4, 1>"),
    (C, "F16", L.TUNE_CONV_1X1_TILE(4, 16), 1, 64, 64, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 4, 64, 16, 4, 2>"),
    (C, "F16", 0, 1, 64, 68, 4, 4, 1, 1, "conv_kernel<f16_t, 1, 1, 4, 64, 8, 4, 1>"),
    (C, "F16", 0, 1, 16, 16, 4, 4, 1, 2, "conv_kernel<f16_t, 1, 2, 1, 16, 8, 4, 1>"),
    (C, "F16", 0, 1, 16, 36, 4, 4, 1, 2, "conv_kernel<f16_t, 1, 2, 2, 16, 8, 4, 1>"),
    (C, "F16", 0, 1, 16, 64, 4, 4, 1, 2, "conv_kernel<f16_t, 1, 2, 2, 16, 8, 4, 2>"),
    (C, "F16", 0, 1, 16, 68, 4, 4, 1, 2, "conv_kernel<f16_t, 1, 2, 4, 16, 8, 4, 1>"),
    (C, "F16", 0, 1, 16, 128, 4, 4, 1, 2, "conv_kernel<f16_t, 1, 2, 4, 16, 8, 4, 2>"),
    (C, "F16", 0, 1, 32, 16, 4, 4, 3, 1, "conv_kernel<f16_t, 3, 1, 1, 32, 16, 4, 1>"),
    (C, "F16", 0, 1, 16, 36, 4, 4, 3, 1, "conv_kernel<f16_t, 3, 1, 2, 16, 16, 4, 1>"),
    (C, "F16", 0, 1, 16, 64, 4, 4, 3, 1, "conv_kernel<f16_t, 3, 1, 2, 16, 16, 4, 2>"),
    (C, "F16", 0, 64, 32, 36, 64, 64, 3, 1, "conv_kernel<f16_t, 3, 1, 2, 32, 16, 8, 1>"),
    (C, "F16", 0, 64, 32, 64, 64, 64, 3, 1, "conv_kernel<f16_t, 3, 1, 2, 32, 16, 8, 2>"),
    (C, "F16", 0, 1, 32, 36, 4, 4, 3, 1, "conv_kernel<f16_t, 3, 1, 2, 32, 8, 4, 1>"),
    (C, "F16", 0, 1, 16, 68, 4, 4, 3, 1, "conv_kernel<f16_t, 3, 1, 4, 16, 16, 4, 1>"),
    (C, "F16", 0, 1, 16, 128, 4, 4, 3, 1, "conv_kernel<f16_t, 3, 1, 4, 16, 16, 4, 2>"),
    (C, "F16", 0, 64, 32, 132, 24, 40, 3, 1, "conv_kernel<f16_t, 3, 1, 4, 16, 8, 4, 1>"),
    (C, "F16", 0, 2, 32, 512, 128, 128, 3, 1, "conv_kernel<f16_t, 3, 1, 4, 16, 8, 4, 2>"),
    (C, "F16", 0, 64, 32, 68, 64, 64, 3, 1, "conv_kernel<f16_t, 3, 1, 4, 32, 16, 8, 1>"),
    (C, "F16", 0, 64, 32, 128, 64, 64, 3, 1, "conv_kernel<f16_t, 3, 1, 4, 32, 16, 8, 2>"),
    (C, "F16", 0, 1, 16, 36, 4, 4, 3, 2, "conv_kernel<f16_t, 3, 2, 2, 16, 8, 4, 1>"),
    (C, "F16", 0, 64, 16, 68, 128, 128, 3, 2, "conv_kernel<f16_t, 3, 2, 4, 16, 8, 4, 1>"),
    (C, "F16", 0, 64, 16, 128, 128, 128, 3, 2, "conv_kernel<f16_t, 3, 2, 4, 16, 8, 4, 2>"),
    (C, "F32", 0, 1, 16, 16, 4, 4, 1, 1, "conv_kernel<float, 1, 1, 1, 16, 16, 4, 1>"),
    (C, "F32", 0, 1, 16, 16, 4, 4, 1, 2, "conv_kernel<float, 1, 2, 1, 16, 8, 4, 1>"),
    (C, "BF16", 0, 1, 16, 16, 4, 4, 1, 1, "conv_kernel<unsigned short, 1, 1, 1, 16, 16, 4, 1>"),
    (C, "BF16", 0, 1, 64, 16, 4, 4, 1, 1, "conv_kernel<unsigned short, 1, 1, 1, 64, 16, 4, 1>"),
    (C, "BF16", 0, 1, 16, 36, 4, 4, 1, 1, "conv_kernel<unsigned short, 1, 1, 2, 16, 16, 4, 1>"),
    (C, "BF16", L.TUNE_CONV_1X1_TILE(2, 16), 1, 64, 36, 4, 4, 1, 1, "conv_kernel<unsigned short, 1, 1, 2, 64, 16, 4, 1>"),
    (C, "BF16", 0, 1, 64, 36, 4, 4, 1, 1, "conv_kernel<unsigned short, 1, 1, 2, 64, 8, 4, 1>"),
    (C, "BF16", 0, 1, 16, 68, 4, 4, 1, 1, "conv_kernel<unsigned short, 1, 1, 4, 16, 16, 4, 1>"),
    (C, "BF16", 0, 1, 16, 128, 4, 4, 1, 1, "conv_kernel<unsigned short, 1, 1, 4, 16, 16, 4, 2>"),
    (C, "BF16", L.TUNE_CONV_1X1_TILE(4, 16), 1, 64, 36, 4, 4, 1, 1, "conv_kernel<unsigned short, 1, 1, 4, 64, 16, 4, 1>"),
    (C, "BF16", 0, 1, 64, 68, 4, 4, 1, 1, "conv_kernel<unsigned short, 1, 1, 4, 64, 8, 4, 1>"),
    (C, "BF16", 0, 1, 16, 16, 4, 4, 1, 2, "conv_kernel<unsigned short, 1, 2, 1, 16, 8, 4, 1>"),
    (C, "BF16", 0, 1, 16, 36, 4, 4, 1, 2, "conv_kernel<unsigned short, 1, 2, 2, 16, 8, 4, 1>"),
    (C, "BF16", 0, 1, 16, 64, 4, 4, 1, 2, "conv_kernel<unsigned short, 1, 2, 2, 16, 8, 4, 2>"),
    (C, "BF16", 0, 1, 16, 68, 4, 4, 1, 2, "conv_kernel<unsigned short, 1, 2, 4, 16, 8, 4, 1>"),
    (C, "BF16", 0, 1, 32, 16, 4, 4, 3, 1, "conv_kernel<unsigned short, 3, 1, 1, 32, 16, 4, 1>"),
    (C, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, "conv_kernel<unsigned short, 3, 1, 2, 16, 16, 4, 1>"),
    (C, "BF16", 0, 1, 16, 64, 4, 4, 3, 1, "conv_kernel<unsigned short, 3, 1, 2, 16, 16, 4, 2>"),
    (C, "BF16", 0, 64, 32, 36, 64, 64, 3, 1, "conv_kernel<unsigned short, 3, 1, 2, 32, 16, 8, 1>"),
    (C, "BF16", 0, 64, 32, 64, 64, 64, 3, 1, "conv_kernel<unsigned short, 3, 1, 2, 32, 16, 8, 2>"),
    (C, "BF16", 0, 1, 32, 36, 4, 4, 3, 1, "conv_kernel<unsigned short, 3, 1, 2, 32, 8, 4, 1>"),
    (C, "BF16", 0, 1, 16, 68, 4, 4, 3, 1, "conv_kernel<unsigned short, 3, 1, 4, 16, 16, 4, 1>"),
    (C, "BF16", 0, 1, 16, 128, 4, 4, 3, 1, "conv_kernel<unsigned short, 3, 1, 4, 16, 16, 4, 2>"),
    (C, "BF16", 0, 64, 32, 132, 24, 40, 3, 1, "conv_kernel<unsigned short, 3, 1, 4, 16, 8, 4, 1>"),
    (C, "BF16", 0, 2, 32, 512, 128, 128, 3, 1, "conv_kernel<unsigned short, 3, 1, 4, 16, 8, 4, 2>"),
    (C, "BF16", 0, 64, 32, 68, 64, 64, 3, 1, "conv_kernel<unsigned short, 3, 1, 4, 32, 16, 8, 1>"),
    (C, "BF16", 0, 64, 32, 128, 64, 64, 3, 1, "conv_kernel<unsigned short, 3, 1, 4, 32, 16, 8, 2>"),
    (C, "BF16", 0, 1, 16, 36, 4, 4, 3, 2, "conv_kernel<unsigned short, 3, 2, 2, 16, 8, 4, 1>"),
    (C, "BF16", 0, 64, 16, 68, 128, 128, 3, 2, "conv_kernel<unsigned short, 3, 2, 4, 16, 8, 4, 1>"),
    (C, "BF16", 0, 64, 16, 128, 128, 128, 3, 2, "conv_kernel<unsigned short, 3, 2, 4, 16, 8, 4, 2>"),
    (C, "F16X3", 0, 1, 16, 16, 4, 4, 1, 1, "conv_kernel<x3_t, 1, 1, 1, 16, 16, 4, 1>"),
    (C, "F16X3", 0, 1, 16, 16, 4, 4, 1, 2, "conv_kernel<x3_t, 1, 2, 1, 16, 8, 4, 1>"),
    (C, "F16X3", 0, 1, 16, 36, 4, 4, 1, 2, "conv_kernel<x3_t, 1, 2, 2, 16, 8, 4, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(2, 4, 16), 1, 16, 16, 4, 4, 3, 1, "conv_kernel<x3_t, 3, 1, 2, 16, 16, 4, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(2, 4, 8), 1, 16, 16, 4, 4, 3, 1, "conv_kernel<x3_t, 3, 1, 2, 16, 8, 4, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(4, 8, 32), 1, 16, 16, 4, 4, 3, 1, "conv_kernel<x3_t, 3, 1, 4, 16, 32, 8, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(4, 4, 8), 1, 16, 16, 4, 4, 3, 1, "conv_kernel<x3_t, 3, 1, 4, 16, 8, 4, 1>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(1, 8, 16), 1, 16, 16, 4, 4, 3, 2, "conv_kernel<x3_t, 3, 2, 1, 16, 16, 8, 1>"),
    (C, "F16", 0, 1, 128, 128, 128, 128, 1, 1, "gemm1_kernel<f16_t, 2, 2, 2, 2, 2, 2>"),
    (C, "F16", L.TUNE_CONV_FORCE_GEMM | L.TUNE_CONV_GEMM_TILE(2), 1, 128, 16, 4, 4, 1, 1, "gemm1_kernel<f16_t, 2, 2, 2, 4, 3, 2>"),
    (C, "F16", 0, 2, 128, 512, 128, 128, 1, 1, "gemm1_kernel<f16_t, 4, 2, 2, 4, 2, 2>"),
    (L.OP_COPY, "F16", 0, 1, 64, 64, 8, 8, 1, 1, "copy_kernel<f16_t>"),
    (L.OP_COPY, "F32", 0, 1, 64, 64, 8, 8, 1, 1, "copy_kernel<float>"),
    (L.OP_COPY, "BF16", 0, 1, 64, 64, 8, 8, 1, 1, "copy_kernel<unsigned short>"),
    (L.OP_STEM, "F16", 0, 1, 3, 64, 16, 16, 7, 2, "stem_s2_kernel<f16_t>"),
    (L.OP_IM2COL, "F16", 0, 1, 3, 160, 16, 16, 7, 2, "im2col_kernel<f16_t>"),
    (L.OP_MAXPOOL3, "F16", 0, 1, 64, 64, 16, 16, 3, 2, "maxpool3_kernel<f16_t>"),
]
# ... and those that need an op _dry_op does not build: (..., stride, overrides, kernel name) with the overrides of _dry_op_with: "out_mode"
# (anything but NHWC takes the general epilogue, EPI = 0; H3D_OUT_NHWC_F16 is upadd's fp16 output), "heads", "in2_cs", "Ho" / "Wo"
DISPATCH_WITH = [
    (S, "F16", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 1, 16, 1, 0, true, 0>"),
    (S, "F16", 0, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 1, 16, 2, 0, true, 256>"),
    (S, "F16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 1, 16, 2, 0, true, 512, true>"),
    (S, "F16", L.OPF_DCN_STREAM_WIDE_MARGIN, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 1, 16, 4, 0, true, 256, true>"),
    (S, "F16", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 2, 16, 1, 0, true, 0>"),
    (S, "F16", 0, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 2, 16, 2, 0, true, 256>"),
    (S, "F16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 2, 16, 2, 0, true, 512, true>"),
    (S, "F16", L.OPF_DCN_STREAM_WIDE_MARGIN, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 2, 16, 4, 0, true, 256, true>"),
    (S, "F16", 0, 1, 16, 68, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 4, 16, 2, 0, true, 0>"),
    (S, "F16", 0, 1, 32, 260, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 4, 16, 4, 0, true, 256>"),
    (S, "F16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 260, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 4, 16, 4, 0, true, 512>"),
    (S, "BF16", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 1, 16, 1, 0, true, 0>"),
    (S, "BF16", 0, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 1, 16, 2, 0, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 1, 16, 2, 0, true, 512, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 1, 16, 4, 0, true, 256, true>"),
    (S, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 2, 16, 1, 0, true, 0>"),
    (S, "BF16", 0, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 2, 16, 2, 0, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 2, 16, 2, 0, true, 512, true>"),
    (S, "BF16", L.OPF_DCN_STREAM_WIDE_MARGIN, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 2, 16, 4, 0, true, 256, true>"),
    (S, "BF16", 0, 1, 16, 68, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 4, 16, 2, 0, true, 0>"),
    (S, "BF16", 0, 1, 32, 260, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 4, 16, 4, 0, true, 256>"),
    (S, "BF16", L.OPF_DCN_STREAM_SLOTS512, 1, 32, 260, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 4, 16, 4, 0, true, 512>"),
    (S, "F16X3", 0, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 1, 16, 2, 0, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN3, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 1, 16, 3, 0, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN4, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 1, 16, 4, 0, true, 256>"),
    (S, "F16X3", 0, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 2, 16, 2, 0, true, 256>"),
    (S, "F16X3", L.TUNE_DCN_STREAM_X3_MARGIN3, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 2, 16, 3, 0, true, 256>"),
    (S, "F16X3", 0, 1, 128, 128, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 2, 16, 4, 0, true, 256>"),
    (F, "F16", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 1, 16, 2, 0, false, 0>"),
    (F, "F16", 0, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 1, 32, 2, 0, false, 0>"),
    (F, "F16", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 2, 16, 2, 0, false, 0>"),
    (F, "F16", 0, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 2, 32, 2, 0, false, 0>"),
    (F, "F16", 0, 1, 16, 260, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<f16_t, 4, 16, 2, 0, false, 0>"),
    (F, "F32", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<float, 1, 16, 2, 0, false, 0>"),
    (F, "F32", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<float, 2, 16, 2, 0, false, 0>"),
    (F, "BF16", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 1, 16, 2, 0, false, 0>"),
    (F, "BF16", 0, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 1, 32, 2, 0, false, 0>"),
    (F, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 2, 16, 2, 0, false, 0>"),
    (F, "BF16", 0, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 2, 32, 2, 0, false, 0>"),
    (F, "BF16", 0, 1, 16, 260, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<unsigned short, 4, 16, 2, 0, false, 0>"),
    (F, "F16X3", L.TUNE_DCN_FUSED_X3_MARGIN2, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 1, 16, 2, 0, false, 0>"),
    (F, "F16X3", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 1, 16, 4, 0, false, 0>"),
    (F, "F16X3", 0, 1, 16, 16, 64, 64, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 1, 16, 6, 0, false, 0>"),
    (F, "F16X3", L.TUNE_DCN_FUSED_X3_MARGIN2, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 2, 16, 2, 0, false, 0>"),
    (F, "F16X3", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 2, 16, 4, 0, false, 0>"),
    (F, "F16X3", 0, 1, 16, 36, 64, 64, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn3_kernel<x3_t, 2, 16, 6, 0, false, 0>"),
    (C2, "F16", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 1, 4, 0, 1, 2, 1>"),
    (C2, "F16", 0, 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 1, 4, 0, 2, 2, 1>"),
    (C2, "F16", 0, 64, 16, 16, 24, 40, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 1, 8, 0, 1, 1, 1>"),
    (C2, "F16", 0, 1, 16, 128, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 1, 8, 0, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(3, 1, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 1, 8, 0, 1, 3, 1>"),
    (C2, "F16", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 2, 4, 0, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(4, 2, 4), 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 2, 4, 0, 2, 1, 1>"),
    (C2, "F16", 0, 1, 16, 36, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 2, 4, 0, 2, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(5, 2, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 2, 8, 0, 1, 1, 1>"),
    (C2, "F16", 0, 1, 16, 256, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 2, 8, 0, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(2, 2, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 2, 8, 0, 1, 2, 2>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(3, 2, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 2, 8, 0, 1, 3, 1>"),
    (C2, "F16", 0, 2, 16, 512, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 4, 16, 0, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(0, 4, 4), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 4, 4, 0, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(3, 4, 4), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 4, 4, 0, 1, 3, 1>"),
    (C2, "F16", 0, 1, 16, 128, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 4, 4, 0, 2, 1, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(2, 4, 4), 1, 16, 128, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 4, 4, 0, 2, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(5, 4, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 4, 8, 0, 1, 1, 1>"),
    (C2, "F16", 0, 1, 16, 512, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 4, 8, 0, 1, 2, 1>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(2, 4, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 4, 8, 0, 1, 2, 2>"),
    (C2, "F16", L.TUNE_CONV_STREAM_TILE(4, 4, 8), 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<f16_t, 4, 8, 0, 2, 1, 1>"),
    (C2, "BF16", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 1, 4, 0, 1, 2, 1>"),
    (C2, "BF16", 0, 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 1, 4, 0, 2, 2, 1>"),
    (C2, "BF16", 0, 64, 16, 16, 24, 40, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 1, 8, 0, 1, 1, 1>"),
    (C2, "BF16", 0, 1, 16, 128, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 1, 8, 0, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(3, 1, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 1, 8, 0, 1, 3, 1>"),
    (C2, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 2, 4, 0, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(4, 2, 4), 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 2, 4, 0, 2, 1, 1>"),
    (C2, "BF16", 0, 1, 16, 36, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 2, 4, 0, 2, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(5, 2, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 2, 8, 0, 1, 1, 1>"),
    (C2, "BF16", 0, 1, 16, 256, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 2, 8, 0, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(2, 2, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 2, 8, 0, 1, 2, 2>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(3, 2, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 2, 8, 0, 1, 3, 1>"),
    (C2, "BF16", 0, 2, 16, 512, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 4, 16, 0, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(0, 4, 4), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 4, 4, 0, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(3, 4, 4), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 4, 4, 0, 1, 3, 1>"),
    (C2, "BF16", 0, 1, 16, 128, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 4, 4, 0, 2, 1, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(2, 4, 4), 1, 16, 128, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 4, 4, 0, 2, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(5, 4, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 4, 8, 0, 1, 1, 1>"),
    (C2, "BF16", 0, 1, 16, 512, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 4, 8, 0, 1, 2, 1>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(2, 4, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 4, 8, 0, 1, 2, 2>"),
    (C2, "BF16", L.TUNE_CONV_STREAM_TILE(4, 4, 8), 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv2_kernel<unsigned short, 4, 8, 0, 2, 1, 1>"),
    (C, "F16", 0, 1, 16, 16, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 1, 1, 1, 16, 16, 4, 0>"),
    (C, "F16", 0, 1, 16, 36, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 1, 1, 2, 16, 16, 4, 0>"),
    (C, "F16", L.TUNE_CONV_1X1_TILE(2, 16), 1, 64, 36, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 1, 1, 2, 64, 16, 4, 0>"),
    (C, "F16", 0, 1, 16, 68, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 1, 1, 4, 16, 16, 4, 0>"),
    (C, "F16", L.TUNE_CONV_1X1_TILE(4, 16), 1, 64, 36, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 1, 1, 4, 64, 16, 4, 0>"),
    (C, "F16", 0, 1, 16, 16, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 1, 2, 1, 16, 8, 4, 0>"),
    (C, "F16", 0, 1, 16, 36, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 1, 2, 2, 16, 8, 4, 0>"),
    (C, "F16", 0, 1, 16, 68, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 1, 2, 4, 16, 8, 4, 0>"),
    (C, "F16", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 1, 1, 16, 16, 4, 0>"),
    (C, "F16", 0, 1, 32, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 1, 1, 32, 16, 4, 0>"),
    (C, "F16", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 1, 2, 16, 16, 4, 0>"),
    (C, "F16", 0, 64, 32, 36, 64, 64, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 1, 2, 32, 16, 8, 0>"),
    (C, "F16", 0, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 1, 2, 32, 8, 4, 0>"),
    (C, "F16", 0, 1, 16, 68, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 1, 4, 16, 16, 4, 0>"),
    (C, "F16", 0, 2, 32, 512, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 1, 4, 16, 8, 4, 0>"),
    (C, "F16", 0, 64, 32, 68, 64, 64, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 1, 4, 32, 16, 8, 0>"),
    (C, "F16", 0, 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 2, 1, 16, 8, 4, 0>"),
    (C, "F16", 0, 1, 16, 36, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 2, 2, 16, 8, 4, 0>"),
    (C, "F16", 0, 64, 16, 68, 128, 128, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<f16_t, 3, 2, 4, 16, 8, 4, 0>"),
    (C, "F32", 0, 1, 16, 16, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<float, 1, 2, 1, 16, 8, 4, 0>"),
    (C, "F32", 0, 1, 16, 36, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<float, 1, 2, 2, 16, 8, 4, 0>"),
    (C, "F32", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<float, 3, 1, 2, 16, 16, 4, 0>"),
    (C, "F32", 0, 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<float, 3, 2, 1, 16, 8, 4, 0>"),
    (C, "F32", 0, 1, 16, 36, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<float, 3, 2, 2, 16, 8, 4, 0>"),
    (C, "BF16", 0, 1, 16, 16, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 1, 1, 1, 16, 16, 4, 0>"),
    (C, "BF16", 0, 1, 16, 36, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 1, 1, 2, 16, 16, 4, 0>"),
    (C, "BF16", L.TUNE_CONV_1X1_TILE(2, 16), 1, 64, 36, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 1, 1, 2, 64, 16, 4, 0>"),
    (C, "BF16", 0, 1, 16, 68, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 1, 1, 4, 16, 16, 4, 0>"),
    (C, "BF16", L.TUNE_CONV_1X1_TILE(4, 16), 1, 64, 36, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 1, 1, 4, 64, 16, 4, 0>"),
    (C, "BF16", 0, 1, 16, 16, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 1, 2, 1, 16, 8, 4, 0>"),
    (C, "BF16", 0, 1, 16, 36, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 1, 2, 2, 16, 8, 4, 0>"),
    (C, "BF16", 0, 1, 16, 68, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 1, 2, 4, 16, 8, 4, 0>"),
    (C, "BF16", 0, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 1, 1, 16, 16, 4, 0>"),
    (C, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 1, 2, 16, 16, 4, 0>"),
    (C, "BF16", 0, 64, 32, 36, 64, 64, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 1, 2, 32, 16, 8, 0>"),
    (C, "BF16", 0, 1, 32, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 1, 2, 32, 8, 4, 0>"),
    (C, "BF16", 0, 1, 16, 68, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 1, 4, 16, 16, 4, 0>"),
    (C, "BF16", 0, 2, 32, 512, 128, 128, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 1, 4, 16, 8, 4, 0>"),
    (C, "BF16", 0, 64, 32, 68, 64, 64, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 1, 4, 32, 16, 8, 0>"),
    (C, "BF16", 0, 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 2, 1, 16, 8, 4, 0>"),
    (C, "BF16", 0, 1, 16, 36, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 2, 2, 16, 8, 4, 0>"),
    (C, "BF16", 0, 64, 16, 68, 128, 128, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<unsigned short, 3, 2, 4, 16, 8, 4, 0>"),
    (C, "F16X3", 0, 1, 16, 36, 4, 4, 1, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 1, 1, 2, 16, 16, 4, 0>"),
    (C, "F16X3", 0, 1, 16, 16, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 1, 2, 1, 16, 8, 4, 0>"),
    (C, "F16X3", 0, 1, 16, 36, 4, 4, 1, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 1, 2, 2, 16, 8, 4, 0>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(1, 4, 16), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 1, 1, 16, 16, 4, 0>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(2, 4, 16), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 1, 2, 16, 16, 4, 0>"),
    (C, "F16X3", 0, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 1, 2, 16, 16, 8, 0>"),
    (C, "F16X3", 0, 1, 16, 68, 32, 32, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 1, 2, 16, 32, 8, 0>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(2, 4, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 1, 2, 16, 8, 4, 0>"),
    (C, "F16X3", 0, 1, 16, 68, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 1, 4, 16, 16, 8, 0>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(4, 8, 32), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 1, 4, 16, 32, 8, 0>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(4, 4, 8), 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 1, 4, 16, 8, 4, 0>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(1, 8, 16), 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 2, 1, 16, 16, 8, 0>"),
    (C, "F16X3", 0, 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 2, 1, 16, 8, 4, 0>"),
    (C, "F16X3", 0, 1, 16, 36, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 2, 2, 16, 16, 8, 0>"),
    (C, "F16X3", L.TUNE_CONV_X3_TILE(2, 4, 8), 1, 16, 16, 4, 4, 3, 2, {"out_mode": L.OUT_NCHW_F32}, "conv_kernel<x3_t, 3, 2, 2, 16, 8, 4, 0>"),
    (HD, "F16", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (2, 2)}, "heads_kernel<f16_t, 16, 1, false>"),
    (HD, "F16", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (40, 40)}, "heads_kernel<f16_t, 16, 2, false>"),
    (HD, "F16", 0, 1, 64, 64, 16, 32, 3, 1, {"heads": (2, 40)}, "heads_kernel<f16_t, 16, 2, true, true>"),
    (HD, "F16", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (70, 70)}, "heads_kernel<f16_t, 16, 3, false>"),
    (HD, "F16", 0, 1, 64, 64, 16, 32, 3, 1, {"heads": (2, 70)}, "heads_kernel<f16_t, 16, 3, true, true>"),
    (HD, "F32", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (40, 40)}, "heads_kernel<float, 8, 2, false>"),
    (HD, "F32", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (70, 70)}, "heads_kernel<float, 8, 3, false>"),
    (HD, "BF16", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (40, 40)}, "heads_kernel<unsigned short, 16, 2, false>"),
    (HD, "BF16", 0, 1, 64, 64, 16, 32, 3, 1, {"heads": (2, 40)}, "heads_kernel<unsigned short, 16, 2, true, true>"),
    (HD, "BF16", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (70, 70)}, "heads_kernel<unsigned short, 16, 3, false>"),
    (HD, "F16X3", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (2, 2)}, "heads_kernel<x3_t, 8, 1, false>"),
    (HD, "F16X3", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (40, 40)}, "heads_kernel<x3_t, 8, 2, false>"),
    (HD, "F16X3", L.TUNE_HEADS_SEPARATE_BIAS, 1, 64, 64, 16, 32, 3, 1, {"heads": (70, 70)}, "heads_kernel<x3_t, 8, 3, false>"),
    # the fused residual branch of the fp16 stem (in2 = its 64-channel output); depth2space's [B,2H,2W,C] output
    (L.OP_DEPTH2SPACE, "F16", 0, 1, 64, 16, 8, 8, 1, 1, {"Ho": 16, "Wo": 16}, "depth2space_kernel<f16_t>"),
    (L.OP_STEM3, "F16", 0, 1, 3, 32, 16, 16, 3, 2, {"in2_cs": 64}, "stem3_kernel<f16_t, true>"),
]
DISPATCH_EXTRA_WITH = [
    # "updcn": H3D_OP_UPDCN_F16's descriptor behind in2 (the value is its skip stride); Ho / Wo = f * the input's
    (F16K, "BF16", L.TUNE_DCN_F16_ONE_WG_PER_CU, 1, 64, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn4_kernel<1, 0, 0, 0>"),
    (F16K, "BF16", 0, 1, 64, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn4_kernel<1, 0, 1, 0>"),
    (L.OP_UPDCN_F16, "BF16", 0, 1, 64, 16, 4, 4, 3, 2, {"updcn": 64, "Ho": 8, "Wo": 8, "out_mode": L.OUT_NCHW_F32}, "dcn4_kernel<1, 0, 1, 1>"),
    (L.OP_UPDCN_F16, "BF16", 0, 1, 64, 16, 4, 4, 3, 2, {"updcn": 64, "Ho": 8, "Wo": 8}, "dcn4_kernel<1, 1, 1, 1>"),
    (F16K, "BF16", L.TUNE_DCN_F16_ONE_WG_PER_CU, 1, 64, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn4_kernel<2, 0, 0, 0>"),
    (F16K, "BF16", 0, 1, 64, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn4_kernel<2, 0, 1, 0>"),
    (L.OP_UPDCN_F16, "BF16", 0, 1, 64, 36, 4, 4, 3, 2, {"updcn": 64, "Ho": 8, "Wo": 8, "out_mode": L.OUT_NCHW_F32}, "dcn4_kernel<2, 0, 1, 1>"),
    (L.OP_UPDCN_F16, "BF16", 0, 1, 64, 36, 4, 4, 3, 2, {"updcn": 64, "Ho": 8, "Wo": 8}, "dcn4_kernel<2, 1, 1, 1>"),
    (L.OP_UPDCN_F16, "BF16", 0, 1, 64, 64, 4, 4, 3, 2, {"updcn": 64, "Ho": 8, "Wo": 8}, "dcn4_kernel<2, 2, 1, 1>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5, 1, 16, 16, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn5_kernel<1, 2, 0, 256>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5, 1, 16, 36, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn5_kernel<2, 2, 0, 256>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 16, 68, 4, 4, 3, 1, {"out_mode": L.OUT_NCHW_F32}, "dcn5_kernel<4, 4, 0, 256>"),
]
DISPATCH_EXTRA = [
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5, 2, 128, 64, 24, 40, 3, 1, "dcn5_kernel<2, 2, 2, 256>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5, 1, 64, 32, 20, 20, 3, 1, "dcn5_kernel<1, 2, 1, 256>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 256, 256, 16, 16, 3, 1, "dcn5_kernel<4, 4, 2, 256>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5, 1, 256, 256, 16, 16, 3, 1, "dcn5_kernel<2, 2, 2, 256>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_DCN5_XP(2), 2, 128, 64, 24, 40, 3, 1, "dcn5_kernel<2, 2, 2, 256, 2>"),
    (F16K, "BF16", 0, 1, 64, 64, 24, 40, 3, 1, "dcn4_kernel<2, 2, 1, 0>"),
    (F16K, "BF16", L.TUNE_DCN_F16_ONE_WG_PER_CU, 1, 64, 64, 24, 40, 3, 1, "dcn4_kernel<2, 2, 0, 0>"),
    # every other instantiation of csrc/dcn1.hip, dcn4.hip and dcn5.hip an op reaches, names from the parent commit's `make EXTRA=1` library
    (F16K, "BF16", L.TUNE_DCN_F16_ONE_WG_PER_CU, 1, 64, 16, 4, 4, 3, 1, "dcn4_kernel<1, 1, 0, 0>"),
    (F16K, "BF16", 0, 1, 64, 16, 4, 4, 3, 1, "dcn4_kernel<1, 1, 1, 0>"),
    (F16K, "BF16", L.TUNE_DCN_F16_ONE_WG_PER_CU, 1, 64, 36, 4, 4, 3, 1, "dcn4_kernel<2, 1, 0, 0>"),
    (F16K, "BF16", 0, 1, 64, 36, 4, 4, 3, 1, "dcn4_kernel<2, 1, 1, 0>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5, 1, 16, 36, 4, 4, 3, 1, "dcn5_kernel<2, 2, 1, 256>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_DCN5_XP(12), 1, 16, 64, 4, 4, 3, 1, "dcn5_kernel<2, 2, 2, 256, 12>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_DCN5_XP(14), 1, 16, 64, 4, 4, 3, 1, "dcn5_kernel<2, 2, 2, 256, 14>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_DCN5_XP(17), 1, 16, 64, 4, 4, 3, 1, "dcn5_kernel<2, 2, 2, 256, 17>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_DCN5_XP(1), 1, 16, 64, 4, 4, 3, 1, "dcn5_kernel<2, 2, 2, 256, 1>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_DCN5_XP(3), 1, 16, 64, 4, 4, 3, 1, "dcn5_kernel<2, 2, 2, 256, 3>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_DCN5_XP(4), 1, 16, 64, 4, 4, 3, 1, "dcn5_kernel<2, 2, 2, 256, 4>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_DCN5_XP(8), 1, 16, 64, 4, 4, 3, 1, "dcn5_kernel<2, 2, 2, 256, 8>"),
    (S, "F16", L.TUNE_DCN_STREAM_F16_DCN5 | L.TUNE_DCN_STREAM_FORCE_WIDE_WG, 1, 16, 68, 4, 4, 3, 1, "dcn5_kernel<4, 4, 1, 256>"),
    (L.OP_DCN_V1, "F32", 0, 1, 16, 16, 4, 4, 3, 1, "dcn_kernel<float, 1, 16>"),
    (L.OP_DCN_V1, "F32", 0, 1, 16, 36, 4, 4, 3, 1, "dcn_kernel<float, 2, 16>"),
    (L.OP_DCN_V1, "BF16", 0, 1, 16, 16, 4, 4, 3, 1, "dcn_kernel<unsigned short, 1, 16>"),
    (L.OP_DCN_V1, "BF16", 0, 1, 32, 16, 4, 4, 3, 1, "dcn_kernel<unsigned short, 1, 32>"),
    (L.OP_DCN_V1, "BF16", 0, 1, 16, 36, 4, 4, 3, 1, "dcn_kernel<unsigned short, 2, 16>"),
    (L.OP_DCN_V1, "BF16", 0, 1, 32, 36, 4, 4, 3, 1, "dcn_kernel<unsigned short, 2, 32>"),
    (L.OP_DCN_V1, "BF16", 0, 1, 16, 68, 4, 4, 3, 1, "dcn_kernel<unsigned short, 4, 16>"),
]


def test_flag_words_select_the_kernels_they_always_did():
    lib, keep, buf = _lib.lib(), [], ctypes.create_string_buffer(200)
    assert len(DISPATCH) >= 40
    # the superseded generations: their names in a `make EXTRA=1` library, H3D_ERR_UNSUPPORTED (-4) in the default one
    extra = DISPATCH_EXTRA if _lib.has_extra() else [c[:-1] + (-4,) for c in DISPATCH_EXTRA]
    for case in DISPATCH + extra:
        rc = lib.h3d_op_kernel_name(ctypes.byref(_dry_op(*case[:-1], keep)), buf, 200)
        assert (buf.value.decode() if rc == 0 else rc) == case[-1], (case, rc, lib.h3d_last_error())
    extra_with = DISPATCH_EXTRA_WITH if _lib.has_extra() else [c[:-1] + (-4,) for c in DISPATCH_EXTRA_WITH]
    for case in DISPATCH_WITH + extra_with:
        op = _dry_op_with(case[:-2], case[-2], keep)
        rc = lib.h3d_op_kernel_name(ctypes.byref(op), buf, 200)
        assert (buf.value.decode() if rc == 0 else rc) == case[-1], (case, rc, lib.h3d_last_error())
