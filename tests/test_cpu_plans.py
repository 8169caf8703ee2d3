"""The launch plans, pinned: every configuration of tools/dump_plans.py is lowered again on the CPU and must be the recorded op array
(tests/golden/plan_ops.json.gz) -- the same integer fields, the same kernels, the same bytes of packed weights behind every pointer and
the same aliasing between buffers.  The fixture is the output of that tool; regenerate it only for a deliberate change of a plan."""
import gzip
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location("dump_plans", os.path.join(ROOT, "tools", "dump_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dump_plans = _load_tool()
NAMES = [name for name, _ in dump_plans.configurations()]


@pytest.fixture(scope="module")
def pinned(golden_dir):
    with gzip.open(os.path.join(golden_dir, "plan_ops.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


@pytest.fixture(scope="module")
def builder():
    return dump_plans.Builder()


def _rebuild(builder, name):
    return json.loads(json.dumps(dump_plans.record([name], builder)[name]))       # (tuples -> lists, as the fixture holds them)


def _first_difference(got, want, where=""):
    """Human-readable place of the first difference between two records."""
    if isinstance(want, dict) and isinstance(got, dict) and "plans" in want and "plans" in got:
        for i, (g, w) in enumerate(zip(got["plans"], want["plans"])):
            if g != w:
                return _first_difference(g, w, "sub-plan %d: " % i)
    if isinstance(want, dict) and isinstance(got, dict) and "ops" in want and "ops" in got:
        for i, (g, w) in enumerate(zip(got["ops"], want["ops"])):
            if g != w:
                fields = sorted(k for k in set(g) | set(w) if g.get(k) != w.get(k))
                return "%sop %d differs in %s\n  now:    %s\n  pinned: %s" % (where, i, fields, json.dumps(g, sort_keys=True),
                                                                            json.dumps(w, sort_keys=True))
        if len(got["ops"]) != len(want["ops"]):
            return "%s%d ops now, %d pinned" % (where, len(got["ops"]), len(want["ops"]))
    if isinstance(want, dict) and isinstance(got, dict):
        for k in sorted(set(got) | set(want)):
            if got.get(k) != want.get(k):
                return "%s%r differs\n  now:    %s\n  pinned: %s" % (where, k, json.dumps(got.get(k), sort_keys=True)[:2000],
                                                                   json.dumps(want.get(k), sort_keys=True)[:2000])
    return "%srecords differ\n  now:    %s\n  pinned: %s" % (where, json.dumps(got, sort_keys=True)[:2000], json.dumps(want, sort_keys=True)[:2000])


def test_fixture_holds_exactly_the_listed_configurations(pinned):
    assert sorted(pinned) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_plan_is_the_pinned_op_array(name, pinned, builder):
    got, want = _rebuild(builder, name), pinned[name]
    assert got == want, "%s: %s" % (name, _first_difference(got, want))


def test_a_second_build_in_the_same_process_gives_the_same_record(pinned):
    """Fresh packers, other addresses: the record does not depend on where the allocator put anything."""
    for name in ("dla34/bf16/default", "dla34/f16x3/fuse_heads=0"):
        assert _rebuild(dump_plans.Builder(), name) == _rebuild(dump_plans.Builder(), name) == pinned[name]


def test_pinned_configurations_cover_the_lowering_branches(pinned):
    """The properties the configurations were chosen for, read off the fixture itself."""
    kinds = {n: [op["kind"] for op in r["ops"]] for n, r in pinned.items() if "ops" in r}
    from h3d_amd import _lib
    assert pinned["dla34/f16/fuse_offsets=0"] == {"raises": ["RuntimeError", "fp16 plans run the fused DeformConv kernel only (fuse_offsets=False "
                                                                                "is a bf16 / f32 debugging path)"]}
    assert pinned["dla34/bf16/W=98"]["raises"][0] == "RuntimeError" and "multiples of 32" in pinned["dla34/bf16/W=98"]["raises"][1]
    assert all("raises" not in r for n, r in pinned.items() if n not in ("dla34/f16/fuse_offsets=0", "dla34/bf16/W=98")), \
        [n for n, r in pinned.items() if "raises" in r]
    assert kinds["dla34/bf16/default"][0] == _lib.OP_STEM3 and kinds["dla34/bf16/fuse_stem=0,stream_convs=0"][0] == _lib.OP_STEM
    assert _lib.OP_HEADS in kinds["dla34/bf16/default"] and _lib.OP_HEADS not in kinds["dla34/bf16/fuse_heads=0"]
    assert kinds["dla34/bf16/mixed_heads=1"].count(_lib.OP_HEADS) == 1
    assert _lib.OP_DCN in kinds["dla34/bf16/fuse_offsets=0"] and _lib.OP_DCN_FUSED in kinds["dla34/f32/default"]
    assert _lib.OP_UPDCN_F16 in kinds["dla34/bf16/stream_dcn=1"]
    if not _lib.has_extra():        # (the superseded generation: the default library answers H3D_ERR_UNSUPPORTED, and the op is still pinned)
        assert -4 in [op["kernel"] for op in pinned["dla34/bf16/stream_dcn=1"]["ops"]]
    assert _lib.OP_IM2COL in kinds["resdcn101/f32"] and _lib.OP_IM2COL in kinds["hourglass/f32"] and _lib.OP_DEPTH2SPACE in kinds["resdcn101/bf16"]
    assert pinned["dla34/bf16/lower_heads=0"]["outputs"] == [] and pinned["dla34/bf16/default"]["outputs"] == list(dump_plans.HEADS)
    assert len(pinned["hourglass/bf16"]["all_outputs"]) == 2
    variants = {op["reserved"] & (_lib.OPF_DCN_STREAM_WIDE_MARGIN | _lib.OPF_DCN_STREAM_SLOTS512)
                for op in pinned["dla34/bf16/dcn_variant"]["ops"] if op["kind"] == _lib.OP_DCN_FUSED_STREAM}
    assert variants == {0, _lib.OPF_DCN_STREAM_WIDE_MARGIN, _lib.OPF_DCN_STREAM_SLOTS512}
    # retargeted sub-plans: sub-plan i writes its heads at batch offset i * 8 of the SAME full tensors
    for name in ("dla34/bf16/split16", "dla34/bf16/split16,fuse_heads=0"):
        outs = []
        for sub in pinned[name]["plans"]:
            ptrs = [h["out"] for op in sub["ops"] if op["kind"] == _lib.OP_HEADS for h in op["in2"]["head"]]
            ptrs += [op["out"] for op in sub["ops"] if op["kind"] == _lib.OP_CONV and op["out_mode"] == _lib.OUT_NCHW_F32]
            assert len(ptrs) == len(dump_plans.HEADS)
            outs.append(ptrs)
        for a, b in zip(*outs):
            assert a[0] == b[0] == "a" and a[3] == b[3] and a[2] == 0 and b[2] == a[3] // 2
