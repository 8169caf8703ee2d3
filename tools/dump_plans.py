"""Pin the launch plans: lower a fixed list of configurations ON THE CPU (the lowering is pure host code) and record every op.

    python tools/dump_plans.py tests/golden/plan_ops.json.gz        # (re)write the fixture
    python tools/dump_plans.py --list                               # the configuration names

tests/test_cpu_plans.py rebuilds every configuration with `record()` and compares it with the fixture, so a change of the host
code (packing, lowering) that alters an op field, a byte of a packed filter bank, an aliasing relation between buffers or the kernel
an op dispatches is caught without a GPU.  Per op: every integer field of `h3d_op`, the kernel name of `h3d_op_kernel_name`'s dry run
(or its error code), and every pointer as [class, ordinal, byte offset, tensor bytes(, sha256[:16])]: class "a" = a tensor of
plan.keep / images / outputs / all_outputs, "w" = a tensor of `pw.t` (with the hash of its bytes); ordinals count distinct tensors
by first appearance in op order, so the ALLOCATION order is free while slices, offsets and aliasing are not.  The descriptors behind
H3D_OP_HEADS / H3D_OP_UPDCN_F16 are resolved the same way.  A non-null pointer that resolves to nothing is an error.

Only surface that must stay is used: PackedWeights(...), .t, .from_tensors, Plan(pw, B, H, W, **flags), plan.ops / op_array / keep /
images / outputs / all_outputs / dcn_layers / retarget_outputs, _lib.H3dOp / H3dHeadsDesc / H3dUpdcnDesc, h3d_op_kernel_name."""
import bisect
import ctypes
import gzip
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import h3d_amd  # noqa: E402,F401
from h3d_amd import _lib, arch, arch_hg, arch_res, synth  # noqa: E402
from h3d_amd.engine import PackedWeights, Plan  # noqa: E402

CPU = torch.device("cpu")
HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2, "pose": 72, "shape": 10}      # multi_pose + SMPL
CTDET = {"hm": 80, "wh": 2, "reg": 2}
PTR_FIELDS = ("in_", "in2", "w", "bias", "out")
INT_FIELDS = tuple(n for n, _ in _lib.H3dOp._fields_ if n not in PTR_FIELDS)


def _tensors(x):
    """Every torch tensor reachable from x (tuples, lists, dicts)."""
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            yield from _tensors(v)
    elif isinstance(x, (tuple, list)):
        for v in x:
            yield from _tensors(v)


def _sha16(t):
    st = t.untyped_storage()
    raw = torch.empty(0, dtype=torch.uint8).set_(st)
    return hashlib.sha256(memoryview(raw.numpy())).hexdigest()[:16]


class Unresolved(Exception):
    """An error of this tool, never a pinned result."""


class Resolver:
    """Device pointer -> [class, ordinal, offset, bytes(, hash)] over the storages of a plan's buffers and of the packed weights."""

    def __init__(self, plan, pw, hashes, extra=()):
        spans = {}
        for cls, src in (("w", pw.t), ("a", [plan.keep, plan.images, plan.outputs, plan.all_outputs, list(extra)])):
            for t in _tensors(src):
                st = t.untyped_storage()
                if st.nbytes():
                    spans.setdefault(st.data_ptr(), (st.nbytes(), cls, t))
        self.starts = sorted(spans)
        self.spans, self.hashes, self.ordinal = spans, hashes, {}

    def __call__(self, p):
        if not p:
            return None
        i = bisect.bisect_right(self.starts, p) - 1
        start = self.starts[i] if i >= 0 else None
        if start is None or p >= start + self.spans[start][0]:
            raise Unresolved("pointer 0x%x resolves to no tensor of the plan or of the packed weights" % p)
        n, cls, t = self.spans[start]
        o = self.ordinal.setdefault(start, sum(1 for s in self.ordinal if self.spans[s][1] == cls))
        r = [cls, o, p - start, n]
        if cls == "w":
            if (start, n) not in self.hashes:
                self.hashes[(start, n)] = _sha16(t)
            r.append(self.hashes[(start, n)])
        return r


def kernel_name(op):
    buf = ctypes.create_string_buffer(256)
    rc = _lib.lib().h3d_op_kernel_name(ctypes.byref(op), buf, 256)
    return buf.value.decode() if rc == 0 else int(rc)


def plan_record(plan, pw, hashes, extra=()):
    res = Resolver(plan, pw, hashes, extra)
    ops = []
    assert len(plan.op_array) == len(plan.ops)
    for i in range(len(plan.ops)):
        op = plan.op_array[i]                                # (what h3d_run_ops gets; plan.ops must say the same, see `stale`)
        r = {k: int(getattr(op, k)) for k in INT_FIELDS}
        r["kernel"] = kernel_name(op)
        for k in PTR_FIELDS:
            if k != "in2":
                r[k] = res(getattr(op, k))
        if op.kind == _lib.OP_HEADS:
            d = ctypes.cast(op.in2, ctypes.POINTER(_lib.H3dHeadsDesc)).contents
            r["in2"] = {"nheads": int(d.nheads), "wexp": int(d.wexp),
                        "head": [{"C": int(h.C), "wexp2": int(h.wexp2), "w2": res(h.w2), "b2": res(h.b2), "out": res(h.out)}
                                 for h in d.head[:d.nheads]]}
        elif op.kind == _lib.OP_UPDCN_F16:
            d = ctypes.cast(op.in2, ctypes.POINTER(_lib.H3dUpdcnDesc)).contents
            r["in2"] = {"skip": res(d.skip), "w_up": res(d.w_up), "w_off": res(d.w_off), "skip_cs": int(d.skip_cs),
                        "reserved": int(d.reserved)}
        else:
            r["in2"] = res(op.in2)
        ops.append(r)
    size = ctypes.sizeof(_lib.H3dOp)
    stale = [i for i in range(len(plan.ops))                 # plan.ops entries that differ from the launched array (retargeted outputs)
             if ctypes.string_at(ctypes.addressof(plan.ops[i]), size) != ctypes.string_at(ctypes.addressof(plan.op_array[i]), size)]
    return {"ops": ops, "stale": stale, "dcn_layers": [[p, int(i)] for p, i in plan.dcn_layers], "outputs": list(plan.outputs),
            "all_outputs": None if plan.all_outputs is None else [list(o) for o in plan.all_outputs]}


class Builder:
    """Synthetic weights and packers shared between the configurations of one backbone / dtype, as an engine shares them between plans."""

    def __init__(self):
        self.sd, self.pw, self.hashes = {}, {}, {}

    def packer(self, arch_name, dtype):
        if arch_name not in self.sd:
            shapes = (arch_hg.state_dict_shapes(HEADS) if arch_name == "hourglass" else
                      arch_res.state_dict_shapes(CTDET, 64) if arch_name == "resdcn101" else arch.state_dict_shapes(HEADS, True))
            self.sd[arch_name] = synth.synth_state_dict(shapes, seed=0, gain=1.25)
        if (arch_name, dtype) not in self.pw:
            heads, hc = (CTDET, 64) if arch_name == "resdcn101" else (HEADS, 256)
            self.pw[arch_name, dtype] = PackedWeights(self.sd[arch_name], heads, True, dtype, CPU, hc, arch_name)
        pw = self.pw[arch_name, dtype]
        return pw, self.hashes.setdefault((arch_name, dtype), {})

    def plan(self, arch_name, dtype, B, H, W, dcn_variant=None, **flags):
        pw, hashes = self.packer(arch_name, dtype)
        pw.dcn_variant = dict(dcn_variant or {})
        try:
            return plan_record(Plan(pw, B, H, W, **flags), pw, hashes)
        finally:
            pw.dcn_variant = {}

    def split(self, dtype, B, H, W, n, **flags):
        """What DLAEngine._forward_split builds: n sub-plans whose head outputs are slices of full-batch tensors."""
        pw, hashes = self.packer("dla34", dtype)
        sub = B // n
        plans = [Plan(pw, sub, H, W, **flags) for _ in range(n)]
        full = {h: torch.empty((B,) + tuple(o.shape[1:]), dtype=o.dtype, device=o.device) for h, o in plans[0].outputs.items()}
        for i, p in enumerate(plans):
            p.retarget_outputs({h: full[h][i * sub:(i + 1) * sub] for h in full})
        return {"plans": [plan_record(p, pw, hashes, extra=full.values()) for p in plans]}

    def bare(self, dtype):
        """PackedWeights.from_tensors on one 64 -> 64 DeformConv layer: the hashes of what each routine returns."""
        sd = synth.synth_state_dict({"p.conv.weight": (64, 64, 3, 3), "p.conv.bias": (64,), "p.conv.conv_offset_mask.weight": (27, 64, 3, 3),
                                     "p.conv.conv_offset_mask.bias": (27,), "p.actf.0.weight": (64,), "p.actf.0.bias": (64,),
                                     "p.actf.0.running_mean": (64,), "p.actf.0.running_var": (64,)}, seed=0, gain=1.25)
        pw = PackedWeights.from_tensors(sd, dtype, CPU)
        om = ("p.conv.conv_offset_mask.weight", "p.conv.conv_offset_mask.bias")
        calls = (("conv", lambda: pw.conv("p.conv.weight", "p.conv.bias", "p.actf.0")),
                 ("conv_half", lambda: pw.conv("p.conv.weight", "p.conv.bias", "p.actf.0", as_half=True)),
                 ("conv_pad", lambda: pw.conv(om[0], om[1], pad_cout_to=32)),
                 ("offset_conv", lambda: pw.offset_conv(om[0], om[1], 128)),
                 ("dcn_stream", lambda: pw.dcn_stream("p")), ("dcn_stream_ck32", lambda: pw.dcn_stream("p", 32)),
                 ("dcn_stream_x3", lambda: pw.dcn_stream_x3("p")), ("conv_stream", lambda: pw.conv_stream("p.conv.weight", "p.conv.bias", "p.actf.0")))
        out = {}
        for name, f in calls:
            out[name] = guarded(lambda: [[str(v.dtype), list(v.shape), _sha16(v.contiguous().clone())] if torch.is_tensor(v) else v
                                         for v in f()])
        out["wexp"] = sorted(pw.wexp.values())
        out["keys"] = [repr(k) for k in pw.t]
        return out


def guarded(f):
    """f(), or the exception it raises as a record (a configuration that raises is pinned as such)."""
    try:
        return f()
    except Unresolved:
        raise
    except Exception as e:
        return {"raises": [type(e).__name__, str(e)]}


def configurations():
    """[(name, callable(builder) -> record)] in a fixed order."""
    c = []

    def add(name, f):
        c.append((name, lambda b: guarded(lambda: f(b))))

    def dla(name, dtype, B=2, H=64, W=96, **kw):
        add(name, lambda b: b.plan("dla34", dtype, B, H, W, **kw))

    for dt in ("bf16", "f16", "f16x3", "f32"):
        dla("dla34/%s/default" % dt, dt)
        dla("dla34/%s/fuse_heads=0" % dt, dt, fuse_heads=False)
        dla("dla34/%s/fuse_offsets=0" % dt, dt, fuse_offsets=False)      # f16: raises
        dla("dla34/%s/dcn_patches=0" % dt, dt, dcn_patches=False)
        dla("dla34/%s/fuse_stem=0,stream_convs=0" % dt, dt, fuse_stem=False, stream_convs=False)
    for k, v in (("stream_dcn3", False), ("node_f16", False), ("mixed_heads", 1), ("wide_heads_m2", 3), ("fuse_stem_proj", True),
                 ("dcn_wide_margin", 1), ("dcn_slots512", 1), ("stream_dcn", True), ("conv1x1_th16_min_cin", 64), ("lower_heads", False),
                 ("stream_s2", False), ("share_pool", False)):
        dla("dla34/bf16/%s=%d" % (k, v), "bf16", **{k: v})
    dla("dla34/bf16/stream_dcn3=0,dense_dcn3_min_tiles=0", "bf16", stream_dcn3=False, dense_dcn3_min_tiles=0)
    dla("dla34/bf16/dcn_variant", "bf16", dcn_variant={"dla_up.ida_0.proj_1": _lib.OPF_DCN_STREAM_WIDE_MARGIN,
                                                       "ida_up.node_2": _lib.OPF_DCN_STREAM_SLOTS512})
    dla("dla34/bf16/W=98", "bf16", W=98)
    dla("dla34/bf16/B=3,96x160", "bf16", B=3, H=96, W=160)
    dla("dla34/bf16/B=64,512x512", "bf16", B=64, H=512, W=512)
    add("dla34/bf16/split16", lambda b: b.split("bf16", 16, 64, 96, 2))
    add("dla34/bf16/split16,fuse_heads=0", lambda b: b.split("bf16", 16, 64, 96, 2, fuse_heads=False))
    for dt in ("bf16", "f32"):
        add("resdcn101/%s" % dt, lambda b, dt=dt: b.plan("resdcn101", dt, 1, 64, 64))
        add("hourglass/%s" % dt, lambda b, dt=dt: b.plan("hourglass", dt, 1, 128, 128))
    add("resdcn101/bf16/stem_s2_direct=0", lambda b: b.plan("resdcn101", "bf16", 1, 64, 64, stem_s2_direct=False))
    for dt in ("bf16", "f16", "f16x3", "f32"):
        add("from_tensors/%s" % dt, lambda b, dt=dt: b.bare(dt))
    return c


def record(names=None, builder=None):
    """{name: record} of the configurations (all, or those in `names`)."""
    builder = builder or Builder()
    return {name: f(builder) for name, f in configurations() if names is None or name in names}


def main(argv):
    if argv[:1] == ["--list"]:
        print("\n".join(name for name, _ in configurations()))
        return 0
    if len(argv) != 1:
        print(__doc__)
        return 2
    rec = record()
    again = record(names=[n for n, _ in configurations()][:15])
    for n, r in again.items():
        assert r == rec[n], "building %s twice gave two different records" % n
    data = json.dumps(rec, sort_keys=True, separators=(",", ":")).encode()
    with open(argv[0], "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))
    print("%s: %d configurations, %d ops, %d bytes of JSON, %d on disk" % (
        argv[0], len(rec), sum(len(p["ops"]) for r in rec.values() for p in r.get("plans", [r]) if "ops" in p), len(data),
        os.path.getsize(argv[0])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
