// Plan interpreter + error plumbing of libh3d_hip.so.
#include "common.h"
#include <stdlib.h>

static thread_local char g_err[512] = "";

void h3d_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static thread_local char g_kname[160] = "";
static thread_local bool g_dry = false;

bool h3d_note_kernel(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kname, sizeof(g_kname), fmt, ap);
    va_end(ap);
    return g_dry;
}

#ifdef H3D_ABLATE
unsigned long long *h3d_stamp_buffer()
{
    static unsigned long long *buf = [] { void *p = nullptr; (void)hipMalloc(&p, sizeof(unsigned long long) * 65536 * H3D_NSTAMP); return (unsigned long long *)p; }();
    return buf;
}
// profiling builds only (not declared in include/h3d.h): copy the phase stamps of the last launch to the host
extern "C" int h3d_debug_stamps(unsigned long long *dst, int n)
{
    return hipMemcpy(dst, h3d_stamp_buffer(), sizeof(unsigned long long) * n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

int h3d_xcd_mode()
{
    static const int mode = [] { const char *e = getenv("H3D_XCD"); return e ? atoi(e) : 1; }();   // on unless H3D_XCD=0
    return mode;
}

extern "C" const char *h3d_last_error(void) { return g_err; }
extern "C" int h3d_abi_version(void) { return H3D_ABI_VERSION; }
extern "C" int h3d_build_flags(void)
{
    int f = 0;
#ifdef H3D_EXTRA
    f |= H3D_BUILD_EXTRA;
#endif
#ifdef H3D_ABLATE
    f |= H3D_BUILD_ABLATE;
#endif
    return f;
}

int h3d_launch_conv(const h3d_op &op, hipStream_t st);
int h3d_launch_stem(const h3d_op &op, hipStream_t st);
int h3d_launch_elementwise(const h3d_op &op, hipStream_t st);
int h3d_launch_dcn(const h3d_op &op, hipStream_t st);
int h3d_launch_heads(const h3d_op &op, hipStream_t st);
int h3d_launch_dcn2(const h3d_op &op, hipStream_t st);
int h3d_launch_dcn3(const h3d_op &op, hipStream_t st);
int h3d_launch_dcn3_fold(const h3d_op &op, const h3d_op &up, hipStream_t st, bool *folded);
int h3d_launch_conv_stream(const h3d_op &op, hipStream_t st);
bool h3d_conv_stream_entry_takes(const h3d_op &pool, const h3d_op &proj, const h3d_op &conv);
int h3d_launch_conv_stream_entry(const h3d_op &pool, const h3d_op &proj, const h3d_op &conv, hipStream_t st);
int h3d_launch_dcn4(const h3d_op &op, hipStream_t st);
int h3d_launch_updcn(const h3d_op &op, hipStream_t st);
int h3d_launch_stem3(const h3d_op &op, hipStream_t st);
int h3d_launch_extra(const h3d_op &op, hipStream_t st);

static int run_one(const h3d_op &op, int i, hipStream_t st, const h3d_op *up = nullptr, bool *folded = nullptr);
static int fail_at(int rc, const h3d_op &op, int i);

// ops[i], or ops[i] and the *folded ops behind it as one launch.  One op more: a fused DeformConv stream op directly followed by an H3D_OP_UPADD that carries
// H3D_OPF_UPADD_FOLDED and whose skip (`in2`) is the DeformConv's `out`, where the DeformConv launcher has a folding tile for the pair
// (csrc/dcn3.hip h3d_launch_dcn3_fold).  Two ops more: the entry of a Tree, [H3D_OP_MAXPOOL, 1x1 H3D_OP_CONV, stride-2 H3D_OP_CONV_STREAM] that all
// carry H3D_OPF_TREE_ENTRY, where csrc/conv2.hip has the tile for the triple (h3d_conv_stream_entry_takes: the structure and the shapes).
// Everywhere else the flags are ignored: the result never depends on the plan's claim being used.
static int run_at(const h3d_op *ops, int i, int n, hipStream_t st, int *folded)
{
    *folded = 0;
    if (i + 1 < n && ops[i].kind == H3D_OP_DCN_FUSED_STREAM && ops[i + 1].kind == H3D_OP_UPADD && (ops[i + 1].reserved & H3D_OPF_UPADD_FOLDED) &&
        ops[i].out && ops[i + 1].in2 == ops[i].out) {
        bool pair = false;
        const int rc = run_one(ops[i], i, st, &ops[i + 1], &pair);
        *folded = pair;
        return rc;
    }
    if (i + 2 < n && ops[i].kind == H3D_OP_MAXPOOL && (ops[i].reserved & H3D_OPF_TREE_ENTRY) &&
        h3d_conv_stream_entry_takes(ops[i], ops[i + 1], ops[i + 2])) {
        *folded = 2;
        return fail_at(h3d_launch_conv_stream_entry(ops[i], ops[i + 1], ops[i + 2], st), ops[i], i);
    }
    return run_one(ops[i], i, st);
}

extern "C" int h3d_op_kernel_name(const h3d_op *op, char *buf, int buflen)
{
    if (!op || !buf || buflen <= 0) H3D_FAIL(H3D_ERR_ARG, "op_kernel_name: null argument");
    g_dry = true;
    g_kname[0] = 0;
    const int rc = run_one(*op, 0, nullptr);
    g_dry = false;
    snprintf(buf, buflen, "%s", g_kname);
    return rc;
}

extern "C" int h3d_run_ops_timed(const h3d_op *ops, int n, void *stream, float *ms)
{
    if (!ops || n <= 0 || !ms) H3D_FAIL(H3D_ERR_ARG, "run_ops_timed: null argument");
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t *ev = (hipEvent_t *)malloc(sizeof(hipEvent_t) * (n + 1));
    if (!ev) H3D_FAIL(H3D_ERR_ARG, "run_ops_timed: out of host memory");
    for (int i = 0; i <= n; ++i) (void)hipEventCreate(&ev[i]);
    int rc = H3D_OK;
    (void)hipEventRecord(ev[0], st);
    for (int i = 0; i < n; ++i) ms[i] = 0.f;
    for (int i = 0; i < n && rc == H3D_OK; ++i) {
        int folded = 0;
        rc = run_at(ops, i, n, st, &folded);
        (void)hipEventRecord(ev[i + 1], st);
        for (; folded > 0; --folded) {           // the launch's time stands under its first op; the ops folded into it report 0 ms
            ++i;
            ms[i] = -1.f;
            (void)hipEventRecord(ev[i + 1], st);
        }
    }
    if (rc == H3D_OK) {
        (void)hipEventSynchronize(ev[n]);
        for (int i = 0; i < n; ++i) {
            if (ms[i] < 0.f) ms[i] = 0.f;
            else (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
        }
    }
    for (int i = 0; i <= n; ++i) (void)hipEventDestroy(ev[i]);
    free(ev);
    return rc;
}

extern "C" int h3d_run_ops(const h3d_op *ops, int n, void *stream)
{
    if (!ops || n < 0) H3D_FAIL(H3D_ERR_ARG, "run_ops: null plan");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < n; ++i) {
        int folded = 0;
        const int rc = run_at(ops, i, n, st, &folded);
        if (rc != H3D_OK) return rc;
        i += folded;
    }
    return H3D_OK;
}

static int run_one(const h3d_op &op, int i, hipStream_t st, const h3d_op *up, bool *folded)
{
    int rc;
    if (op.B <= 0 || op.H <= 0 || op.W <= 0 || op.Ho <= 0 || op.Wo <= 0 || op.Cin <= 0 || op.Cout <= 0) {
        h3d_set_error("op %d (kind %d): non-positive dimension", i, op.kind);
        return H3D_ERR_SHAPE;
    }
    switch (op.kind) {
    case H3D_OP_STEM: rc = h3d_launch_stem(op, st); break;
    case H3D_OP_STEM3: rc = h3d_launch_stem3(op, st); break;
    case H3D_OP_CONV: rc = h3d_launch_conv(op, st); break;
    case H3D_OP_CONV_STREAM: rc = h3d_launch_conv_stream(op, st); break;
    case H3D_OP_DCN: rc = h3d_launch_dcn2(op, st); break;
#ifdef H3D_EXTRA
    case H3D_OP_DCN_V1: rc = h3d_launch_dcn(op, st); break;
    case H3D_OP_DCN_FUSED_F16: rc = h3d_launch_dcn4(op, st); break;
    case H3D_OP_UPDCN_F16: rc = h3d_launch_updcn(op, st); break;
#else
    case H3D_OP_DCN_V1:
    case H3D_OP_DCN_FUSED_F16:
    case H3D_OP_UPDCN_F16:
        h3d_set_error("op %d (kind %d): a superseded kernel generation, built only by `make EXTRA=1` (csrc/Makefile)", i, op.kind);
        return H3D_ERR_UNSUPPORTED;
#endif
    case H3D_OP_DCN_FUSED:
    case H3D_OP_DCN_FUSED_STREAM: rc = up ? h3d_launch_dcn3_fold(op, *up, st, folded) : h3d_launch_dcn3(op, st); break;
    case H3D_OP_HEADS: rc = h3d_launch_heads(op, st); break;
    case H3D_OP_MAXPOOL:
    case H3D_OP_UPADD:
    case H3D_OP_COPY: rc = h3d_launch_elementwise(op, st); break;
    case H3D_OP_IM2COL:
    case H3D_OP_MAXPOOL3:
    case H3D_OP_DEPTH2SPACE: rc = h3d_launch_extra(op, st); break;
    default: h3d_set_error("op %d: unknown kind %d", i, op.kind); return H3D_ERR_ARG;
    }
    return fail_at(rc, op, i);
}

static int fail_at(int rc, const h3d_op &op, int i)
{
    if (rc != H3D_OK) {
        char tmp[400];
        snprintf(tmp, sizeof(tmp), "%s", h3d_last_error());
        h3d_set_error("op %d (kind %d): %s", i, op.kind, tmp);
    }
    return rc;
}
