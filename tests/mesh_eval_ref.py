"""include/h3d.h section 8b restated with plain loops over Python floats (IEEE binary64, one rounding per operation): one pair at a time,
one thread at a time, one matrix element at a time.  mesh_eval.evaluate_numpy (vectorised) must equal this bit for bit
(tests/test_oracle_mesh_eval.py); the kernels are held to evaluate_numpy (tests/test_gpu_mesh_eval.py)."""
import math

THREADS, WAVE, MAX_SWEEPS, TOL = 256, 64, 30, 2.0 ** -50


def block_sum(n, valid, f):
    """SUM: f(i) over the valid i of range(n) in the order of the 256 threads, the wave tree and the four waves."""
    part = []
    for t in range(THREADS):
        acc = 0.0
        for i in range(t, n, THREADS):
            if valid[i]:
                acc = acc + f(i)
        part.append(acc)
    waves = []
    for w in range(THREADS // WAVE):
        v = part[WAVE * w:WAVE * (w + 1)]
        off = WAVE // 2
        while off >= 1:
            for lane in range(off):
                v[lane] = v[lane] + v[lane + off]
            off //= 2
        waves.append(v[0])
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def length(d):
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def col(X, j):
    return [X[0][j], X[1][j], X[2][j]]


def dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def similarity(M, var):
    """M[r][c], var -> (s, R[r][c])."""
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if var == 0.0:
        return 1.0, eye
    A = [row[:] for row in M]
    V = [row[:] for row in eye]
    for _ in range(MAX_SWEEPS):
        skipped = 0
        for p, q in ((0, 1), (0, 2), (1, 2)):
            a, b, g = dot(col(A, p), col(A, p)), dot(col(A, q), col(A, q)), dot(col(A, p), col(A, q))
            if abs(g) <= TOL * max(a, b):
                skipped += 1
                continue
            h = b - a
            g2 = 2.0 * g
            if abs(g2) <= abs(h):
                r = g2 / h
                t = r / (1.0 + math.sqrt(1.0 + r * r))
            else:
                z = h / g2
                u = 1.0 / (abs(z) + math.sqrt(1.0 + z * z))
                t = -u if z < 0.0 else u
            cs = 1.0 / math.sqrt(1.0 + t * t)
            sn = cs * t
            for X in (A, V):
                for row in range(3):
                    old_p, old_q = X[row][p], X[row][q]
                    X[row][p] = cs * old_p - sn * old_q
                    X[row][q] = sn * old_p + cs * old_q
        if skipped == 3:
            break
    nn = [dot(col(A, j), col(A, j)) for j in range(3)]
    order, dv = [0, 1, 2], 1.0
    for first, later in ((0, 1), (1, 2), (0, 1)):
        if nn[order[later]] > nn[order[first]]:
            order[first], order[later] = order[later], order[first]
            dv = -dv
    c = [col(A, j) for j in order]
    v = [col(V, j) for j in order]
    S = [math.sqrt(nn[j]) for j in order]
    if S[0] == 0.0:
        return 0.0, eye
    U0 = [c[0][r] / S[0] for r in range(3)]
    U1 = None
    if S[1] > 0.0:
        u = [c[1][r] / S[1] for r in range(3)]
        hh = dot(u, U0)
        w = [u[r] - hh * U0[r] for r in range(3)]
        nw = length(w)
        if nw >= 0.5:
            U1 = [w[r] / nw for r in range(3)]
    if U1 is None:
        k = 0
        for r in (1, 2):
            if abs(U0[r]) < abs(U0[k]):
                k = r
        w = [(1.0 if r == k else 0.0) - U0[k] * U0[r] for r in range(3)]
        nw = length(w)
        U1 = [w[r] / nw for r in range(3)]
    U2 = [U0[1] * U1[2] - U0[2] * U1[1], U0[2] * U1[0] - U0[0] * U1[2], U0[0] * U1[1] - U0[1] * U1[0]]
    R = [[(U0[r] * v[0][cc] + U1[r] * v[1][cc]) + dv * (U2[r] * v[2][cc]) for cc in range(3)] for r in range(3)]
    d = -dv if dot(c[2], U2) < 0.0 else dv
    return ((S[0] + S[1]) + d * S[2]) / var, R


def pair_errors(p, g, valid=None, root_p=None, root_g=None, root=(1, 2)):
    """One valid pair: p, g = n points (any sequence of 3 float32 values each), valid = n flags or None, root sources or None
    -> (plain, aligned, count, [s, R row-major (9), t (3)])."""
    n = len(p)
    p = [[float(v) for v in pt] for pt in p]
    g = [[float(v) for v in pt] for pt in g]
    valid = [True] * n if valid is None else [bool(v) for v in valid]
    count = sum(valid)
    if count == 0:
        return 0.0, 0.0, 0, [0.0] * 13
    op = og = [0.0, 0.0, 0.0]
    if root_p is not None:
        a, b = root
        op = [(float(root_p[a][c]) + float(root_p[b][c])) * 0.5 for c in range(3)]
        og = [(float(root_g[a][c]) + float(root_g[b][c])) * 0.5 for c in range(3)]
    dn = float(count)
    plain = block_sum(n, valid, lambda i: length([(p[i][c] - op[c]) - (g[i][c] - og[c]) for c in range(3)])) / dn
    mp = [block_sum(n, valid, lambda i, c=c: p[i][c]) / dn for c in range(3)]
    mg = [block_sum(n, valid, lambda i, c=c: g[i][c]) / dn for c in range(3)]
    x = [[p[i][c] - mp[c] for c in range(3)] for i in range(n)]
    y = [[g[i][c] - mg[c] for c in range(3)] for i in range(n)]
    M = [[block_sum(n, valid, lambda i, r=r, c=c: y[i][r] * x[i][c]) for c in range(3)] for r in range(3)]
    var = block_sum(n, valid, lambda i: (x[i][0] * x[i][0] + x[i][1] * x[i][1]) + x[i][2] * x[i][2])
    s, R = similarity(M, var)
    t = [mg[r] - s * ((R[r][0] * mp[0] + R[r][1] * mp[1]) + R[r][2] * mp[2]) for r in range(3)]

    def aligned_distance(i):
        q = [s * ((R[r][0] * p[i][0] + R[r][1] * p[i][1]) + R[r][2] * p[i][2]) + t[r] for r in range(3)]
        return length([q[r] - g[i][r] for r in range(3)])
    aligned = block_sum(n, valid, aligned_distance) / dn
    return plain, aligned, count, [s] + [R[r][c] for r in range(3) for c in range(3)] + t


def metric_means(err, count):
    """err = P pairs of (plain, aligned), count = P integers -> ([mean plain, mean aligned], pairs with count > 0)."""
    lanes = [[0.0, 0.0] for _ in range(WAVE)]
    pairs = 0
    for lane in range(WAVE):
        for i in range(lane, len(count), WAVE):
            if count[i] > 0:
                lanes[lane][0] = lanes[lane][0] + err[i][0]
                lanes[lane][1] = lanes[lane][1] + err[i][1]
                pairs += 1
    off = WAVE // 2
    while off >= 1:
        for lane in range(off):
            lanes[lane][0] = lanes[lane][0] + lanes[lane + off][0]
            lanes[lane][1] = lanes[lane][1] + lanes[lane + off][1]
        off //= 2
    if pairs == 0:
        return [0.0, 0.0], 0
    return [lanes[0][0] / float(pairs), lanes[0][1] / float(pairs)], pairs
