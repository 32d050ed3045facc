"""Cases, 80-bit references and error bounds for the IW / entropy / CSR / gradient ops.

TEST INFRASTRUCTURE ONLY (host code; torch is imported lazily and nothing here needs a GPU).

The kernels of csrc/entropy.hip and csrc/csr.hip are tested op by op: every case goes through an
`ops`-shaped module (tests/cpu_ops.py on the CPU, mepol_amd.ops on the GPU) and every output is
compared with a reference computed here in np.longdouble (x87 80-bit, 64-bit mantissa) from
the formulas of oracle/mepol_oracle.py (importance_weights, entropy, kl, entropy_grad_logp).

How the bounds are made.  u0 = 2^-53 is the unit roundoff of f64.  An output that is a sum of n
terms x_i formed in ANY order (sequential, pairwise, lane-strided, tree) has an error of at most
(n - 1) u0 sum|x_i| to first order (Higham, Accuracy and Stability of Numerical Algorithms,
section 4.2: every term passes through at most n - 1 roundings).  Every bound below is of that
shape: m u0 A with A the sum of the absolute values of the terms on the output's path and m
the number of roundings on it, plus the propagated bounds of the inputs.  They are computed
from the reference and the shapes alone, never from what an implementation returned.  Two
constants are stated rather than derived:

  LIBM   4 ulp (8 u0 relative) for one call of exp / log / pow.  glibc documents <= 1 ulp for
         the three in f64 and the GPU vendors' math libraries publish 1 to 2 ulp for them; 4
         covers either side with margin and is still ~1e-15, far below a dropped 1/N term.
  SLACK  1.01 on every bound: the second-order terms of the first-order analysis (all the
         relative errors here are below 1e-10, so their squares are far inside 1%) and the
         reference's own error (80-bit sums of up to 4e4 terms: < 4e4 * 2^-64, a thousandth
         of the f64 bound of the same sum).

Non-finite reference entries (D = 0 with eps = 0 gives r = inf, g = nan, H = -inf) must be
reproduced exactly (nan for nan, the same infinity); finite entries still meet their bound.
"""
import functools
import math
import types

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the x87 80-bit type on this platform"

U0 = LD(2) ** -53
LIBM = 8 * U0
SLACK = LD("1.01")

RAGGED_LENS = [0, 1, 63, 64, 65, 127, 128, 129, 200, 37, 4, 5]
RAGGED_T = 208
LANES = 64             # iw_scan / reverse_scan: one wave per trajectory, chunk = ceil(len / 64)
GAMMA_STRIDE = 32768   # particles per grid-stride pass of gamma_kernel (2048 blocks x 16)

# name -> largest observed error / bound over every check() so far (see __main__ below)
RATIOS = {}


def ld(x):
    return np.asarray(x, dtype=LD)


# =============================================================================================
# The checkers
# =============================================================================================
def check(name, got, ref, bound):
    """|got - ref| <= bound where ref is finite; the same nan / inf where it is not."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = ld(ref).reshape(-1)
    bound = np.broadcast_to(ld(bound).reshape(-1) if np.ndim(bound) else ld(bound), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{name}: nan positions differ"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf].astype(np.float64)), f"{name}: infinities differ"
    if not fin.any():
        return 0.0
    err = np.abs(ld(got[fin]) - ref[fin])
    b = bound[fin]
    assert np.all(np.isfinite(b)) and np.all(b >= 0), f"{name}: bound not finite"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, err / b, np.where(err == 0, 0, np.inf))
    worst = float(np.max(ratio))
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst if math.isfinite(worst) else 1e300)
    i = int(np.argmax(ratio))
    assert worst <= 1.0, (f"{name}: error / bound = {worst:.3g} at {i} "
                          f"(got {got[fin][i]!r}, ref {float(ref[fin][i])!r}, "
                          f"err {float(err[i]):.3g}, bound {float(b[i]):.3g})")
    return worst


def check_equal_int(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.array_equal(got, ref), f"{name}: integer lists differ"


def bits_equal(a, b):
    """Bit-for-bit equality of two tensors (nan == nan when the payload is the same)."""
    import torch

    if a is None or b is None:
        return a is None and b is None
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return a.shape == b.shape and bool(torch.equal(a, b))


# =============================================================================================
# References with their bounds.  Every function returns a SimpleNamespace of longdouble arrays:
# value `x` with its bound `bx`.  `d*` arguments are bounds on the error of an input that is
# itself a computed quantity (the chained tests); they default to exact inputs.
# =============================================================================================
def iw_ref(logp_t, logp_b, offsets):
    """oracle.importance_weights: u = exp(cumsum(logp_t - logp_b)) per trajectory, w = u / sum u.

    c_t = sum_{s<=t} D_s, D_s = fl(lt_s - lb_s).  A 64-lane chunked scan (chunk = ceil(L / 64))
    forms c_t from the terms s < b + chunk (b = t's chunk start; the lane's whole chunk enters
    through the wave scan and is taken out again), so its path holds the terms s <= t + chunk:
      1 rounding for D_s, at most (l + 1) chunk - 1 <= b + chunk - 1 adds for the scan total,
      1 for `incl - s`, at most t - b + 1 adds to reach t: m = t + chunk + 2 roundings, each
      on a partial sum of magnitude <= A_t = sum_{s <= min(L-1, t+chunk)} |D_s|.
    A sequential cumsum is the special case chunk = 0.  u = exp(c): relative error
    |c^ - c| + LIBM.  traj_sum = sum_t u_t (L - 1 adds of positive terms), U = sum_n traj_sum
    (nt - 1 adds), w = u / U (1 rounding)."""
    off = np.asarray(offsets, dtype=np.int64)
    nt, N = logp_t.shape[0], int(off[-1])
    u, bu = np.zeros(N, LD), np.zeros(N, LD)
    ts, bts = np.zeros(nt, LD), np.zeros(nt, LD)
    for n in range(nt):
        p, L = int(off[n]), int(off[n + 1] - off[n])
        if L == 0:
            continue  # traj_sum = 0 exactly, no particles
        d = ld(logp_t[n, :L]) - ld(logp_b[n, :L])
        x = np.exp(np.cumsum(d))
        a = np.cumsum(np.abs(d))
        chunk = -(-L // LANES)
        t = np.arange(L)
        bc = (t + chunk + 2) * U0 * a[np.minimum(L - 1, t + chunk)]
        bx = x * (bc + LIBM) * SLACK
        u[p:p + L], bu[p:p + L] = x, bx
        ts[n] = np.sum(x)
        bts[n] = (np.sum(bx) + (L - 1) * U0 * ts[n]) * SLACK
    U = np.sum(ts)
    bU = (np.sum(bts) + (nt - 1) * U0 * U) * SLACK
    w = u / U
    bw = w * (bu / u + bU / U + U0) * SLACK
    return types.SimpleNamespace(u=u, bu=bu, ts=ts, bts=bts, U=U, bU=bU, w=w, bw=bw)


def normalize_ref(u, U):
    """w = u / U from f64 u and U: one correctly rounded division, |err| <= u0 |w|."""
    w = ld(u) / ld(U)
    return types.SimpleNamespace(w=w, bw=U0 * np.abs(w) * SLACK)


def gathered_ref(xu_all, world, n, nt, du=None, dts=None):
    """w[r n + i] = xu[r, i] / U, U = sum of the world * nt sums xu[r, n + t] (positive terms,
    world nt - 1 adds in any order), then one division."""
    x = ld(xu_all).reshape(world, n + nt)
    u, ts = x[:, :n].reshape(-1), x[:, n:].reshape(-1)
    du = np.zeros_like(u) if du is None else ld(du).reshape(-1)
    dts = np.zeros_like(ts) if dts is None else ld(dts).reshape(-1)
    U = np.sum(ts)
    bU = (np.sum(dts) + (world * nt - 1) * U0 * np.sum(np.abs(ts))) * SLACK
    w = u / U
    bw = (np.abs(w) * (bU / U + U0) + du / U) * SLACK
    return types.SimpleNamespace(w=w, bw=bw, U=U, bU=bU)


def entropy_ref(w, idxT, D, k, ns, G, B, eps, n_w=None, dw=None):
    """oracle.entropy / kl / the g of entropy_grad_logp for n query rows.

    W_i = sum_{c<k} w[I[i,c]]  (k - 1 adds of positive terms + the inputs' dw)
    V_i = D[i,k]^ns pi^(ns/2) / G: two pow calls, one product, one division in some order:
          relative 2 LIBM + 2 u0 (pi is the f64 constant on both sides, as in the oracle).
    r = W / (V + eps): one add, one division.       lr = log(r + eps): one add, LIBM |lr|.
    term = (W / k) lr: a division and a product.    kl_term = log(k / (n_w W) + eps): a
    product, a division, an add, then LIBM |kl_term|.
    g = -(1/k)(lr + r / (r + eps)): q = r / (r + eps) carries r's relative error twice (r^ and
    fl(r^ + eps) are taken as independent: looser than the truth, never tighter) and 3
    roundings; the sum, 1/k and the product are 3 more, relative to |g| (|lr + q| = k |g|).
    The sums over the n rows: n - 1 adds in any order.  H = -sum + B: one rounding.
    KL = (1/n_w) sum: the reciprocal and the product."""
    w = ld(w)
    n, kk = D.shape[0], LD(k)
    n_w = w.shape[0] if n_w is None else n_w
    dw = np.zeros_like(w) if dw is None else ld(dw)
    I = np.asarray(idxT)[:k].T.astype(np.int64).reshape(n, k)
    assert I.min(initial=0) >= 0 and I.max(initial=0) < w.shape[0]
    W = np.sum(w[I], axis=1)
    bW = (np.sum(dw[I], axis=1) + (k - 1) * U0 * W) * SLACK
    relW = bW / W
    C = ld(np.pi) ** (ld(ns) / 2) / ld(G)
    V = ld(D[:, k]) ** ld(ns) * C
    eps = ld(eps)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = W / (V + eps)
        relr = relW + (2 * LIBM + 2 * U0) + U0 + U0
        lr = np.log(r + eps)
        blr = (relr + U0) + LIBM * np.abs(lr)
        th = (W / kk) * lr
        bth = (np.abs(th) * (relW + 2 * U0) + (W / kk) * blr) * SLACK
        tk = np.log(kk / (n_w * W) + eps)
        btk = ((relW + 3 * U0) + LIBM * np.abs(tk)) * SLACK
        q = r / (r + eps)
        bq = np.abs(q) * (2 * relr + 3 * U0)
        g = -(1 / kk) * (lr + q)
        bg = ((blr + bq) / kk + 4 * U0 * np.abs(g)) * SLACK
        Sth, Stk = np.sum(th), np.sum(tk)
        bSth = (np.sum(bth) + (n - 1) * U0 * np.sum(np.abs(th))) * SLACK
        bStk = (np.sum(btk) + (n - 1) * U0 * np.sum(np.abs(tk))) * SLACK
        H = -Sth + ld(B)
        bH = (bSth + U0 * np.abs(H)) * SLACK
        KL = Stk / n_w
        bKL = (bStk / n_w + 2 * U0 * np.abs(KL)) * SLACK
    out4 = np.array([H, KL, Sth, Stk], dtype=LD)
    bout4 = np.array([bH, bKL, bSth, bStk], dtype=LD)
    return types.SimpleNamespace(W=W, bW=bW, g=g, bg=bg, out4=out4, bout4=bout4)


def gamma_ref(g, w_own, csr_off, csr_rows, dg=None, dw=None):
    """gamma_j = sum_{i in list(j)} g_i (len_j - 1 adds in any order, A = sum |g_i|, + the
    inputs' dg); S = sum_j gamma_j w_j: a product per term, n_own - 1 adds in any order (block
    partials, then their sum, is one such order)."""
    g, w = ld(g), ld(w_own)
    off = np.asarray(csr_off, dtype=np.int64)
    n_own = w.shape[0]
    rows = np.asarray(csr_rows, dtype=np.int64)[:int(off[-1])]
    assert rows.min(initial=0) >= 0 and rows.max(initial=0) < g.shape[0]
    dg = np.zeros_like(g) if dg is None else ld(dg)
    dw = np.zeros_like(w) if dw is None else ld(dw)
    lens = np.diff(off)
    seg = np.repeat(np.arange(n_own), lens)
    gamma, A, Dg = np.zeros(n_own, LD), np.zeros(n_own, LD), np.zeros(n_own, LD)
    np.add.at(gamma, seg, g[rows])
    np.add.at(A, seg, np.abs(g[rows]))
    np.add.at(Dg, seg, dg[rows])
    bgamma = (Dg + np.maximum(lens - 1, 0) * U0 * A) * SLACK
    p = gamma * w
    S = np.sum(p)
    bS = (np.sum(bgamma * np.abs(w) + np.abs(gamma) * dw + U0 * np.abs(p))
          + (n_own - 1) * U0 * np.sum(np.abs(p))) * SLACK
    return types.SimpleNamespace(gamma=gamma, bgamma=bgamma, S=S, bS=bS)


def partials_sum_ref(partials):
    """S as the reverse scan forms it from block partials: nparts - 1 adds in any order."""
    p = ld(partials)
    return np.sum(p), max(p.shape[0] - 1, 0) * U0 * np.sum(np.abs(p)) * SLACK


def reverse_ref(gamma, w, S, offsets, T_stride, grad_H, dgamma=None, dw=None, dS=0):
    """grad[n, s] = gH sum_{t>=s} (gamma_t - S) w_t, zeros from s = len_n on.

    c_t = (gamma_t - S) w_t: a subtraction and a product, plus the inputs' bounds.  The suffix
    sum mirrors iw_ref's prefix sum: a 64-lane chunked scan reaches s through the terms
    t >= s - chunk with m = (L - s) + chunk + 2 roundings, A_s = sum_{t >= max(0, s-chunk)}
    (|gamma_t| + |S|) w_t (>= sum |c_t|).  The product with gH is one more rounding."""
    gamma, w, S, gH = ld(gamma), ld(w), ld(S), ld(grad_H)
    dgamma = np.zeros_like(gamma) if dgamma is None else ld(dgamma)
    dw = np.zeros_like(w) if dw is None else ld(dw)
    off = np.asarray(offsets, dtype=np.int64)
    nt = off.shape[0] - 1
    out, bout = np.zeros((nt, T_stride), LD), np.zeros((nt, T_stride), LD)
    for n in range(nt):
        p, L = int(off[n]), int(off[n + 1] - off[n])
        if L == 0:
            continue
        gs, ws = gamma[p:p + L], w[p:p + L]
        c = (gs - S) * ws
        dc = ((dgamma[p:p + L] + ld(dS) + U0 * np.abs(gs - S)) * np.abs(ws)
              + np.abs(gs - S) * dw[p:p + L] + U0 * np.abs(c))
        a = (np.abs(gs) + np.abs(S)) * np.abs(ws)
        suf = lambda x: np.cumsum(x[::-1])[::-1]  # noqa: E731
        R, sufA, sufD = suf(c), suf(a), suf(dc)
        chunk = -(-L // LANES)
        s = np.arange(L)
        j = np.maximum(0, s - chunk)
        b = sufD[j] + ((L - s) + chunk + 2) * U0 * sufA[j]
        out[n, :L] = gH * R
        bout[n, :L] = (np.abs(gH) * b + U0 * np.abs(out[n, :L])) * SLACK
    return types.SimpleNamespace(grad=out, bgrad=bout)


def emit_ref(x_all, world, stride, off, B, n_global, sums_cur):
    """vals = (B - sums_cur[0], (sum_r x[r, off+1]) / n_global), sums_cur' = rank-order sums of
    x[r, off], x[r, off+1]: world - 1 adds each; one subtraction; one division."""
    x = ld(x_all).reshape(world, stride)
    s0, s1 = np.sum(x[:, off]), np.sum(x[:, off + 1])
    b0 = (world - 1) * U0 * np.sum(np.abs(x[:, off])) * SLACK
    b1 = (world - 1) * U0 * np.sum(np.abs(x[:, off + 1])) * SLACK
    v0 = ld(B) - ld(sums_cur)[0]
    v1 = s1 / n_global
    return types.SimpleNamespace(vals=np.array([v0, v1], LD),
                                 bvals=np.array([U0 * np.abs(v0) * SLACK,
                                                 (b1 / n_global + U0 * np.abs(v1)) * SLACK], LD),
                                 sums=np.array([s0, s1], LD), bsums=np.array([b0, b1], LD))


# =============================================================================================
# Case generators (seeded; plain numpy arrays; every index in range, every offset monotone)
# =============================================================================================
def offsets_of(lengths):
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.int64))
    return off


def iw_case(name, lengths, T_stride, seed, drift=None):
    """logp_t / logp_b [nt, T_stride] with Delta of order 0.05; the padded tail of every row holds
    +-50 (an implementation that reads past a length produces weights off by e^+-50).
    drift: {trajectory: d} adds d to every Delta of that trajectory."""
    rng = np.random.default_rng(seed)
    nt = len(lengths)
    assert max(lengths) <= T_stride and sum(lengths) > 0
    lb = -3.0 + rng.standard_normal((nt, T_stride))
    lt = lb + 0.05 * rng.standard_normal((nt, T_stride))
    for n, d in (drift or {}).items():
        lt[n] += d
    for n, L in enumerate(lengths):
        lt[n, L:] = lb[n, L:] + np.where(np.arange(T_stride - L) % 2 == 0, 50.0, -50.0)
    off = offsets_of(lengths)
    return types.SimpleNamespace(name=name, logp_t=lt, logp_b=lb, offsets=off, N=int(off[-1]),
                                 lengths=list(lengths), T=T_stride, nt=nt)


@functools.lru_cache(maxsize=None)
def iw_cases():
    out = [iw_case("ragged", RAGGED_LENS, RAGGED_T, 1),
           # |sum Delta| ~ 30 inside trajectories 8 (len 200) and 7 (len 129): u spans e^+-30
           iw_case("ragged_drift", RAGGED_LENS, RAGGED_T, 2, drift={8: 0.15, 7: -0.2325}),
           iw_case("nt1", [7], 9, 3)]
    for nt in (3, 4, 5):
        for where, z in (("first", 0), ("mid", nt // 2), ("last", nt - 1)):
            rng = np.random.default_rng(100 + 10 * nt + z)
            lens = [int(x) for x in rng.integers(1, 71, nt)]
            lens[z] = 0
            out.append(iw_case(f"nt{nt}_zero_{where}", lens, 72, 10 * nt + z))
    out.append(iw_case("nt4_zero_ends", [0, 66, 3, 0], 72, 50))
    for nt in (2047, 2048, 2049, 4100):
        rng = np.random.default_rng(nt)
        out.append(iw_case(f"nt{nt}", [int(x) for x in rng.integers(1, 6, nt)], 5, nt + 1))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def iw_reference(name):
    c = iw_cases()[name]
    return iw_ref(c.logp_t, c.logp_b, c.offsets)


def _positive_weights(rng, n):
    w = np.exp(1.5 * rng.standard_normal(n))
    return w / w.sum()


def entropy_case(name, n, k, kp1, ns, eps, seed, n_w=None, zero_rows=(), w=None):
    """idxT [kp1, n] int32 with ids in [0, n_w), D [n, kp1] > 0 (zero_rows: D[i, k] = 0), w [n_w]
    positive.  With n_w > n every row also names ids >= n (another rank's particles)."""
    rng = np.random.default_rng(seed)
    n_w = n if n_w is None else n_w
    idxT = rng.integers(0, n_w, (kp1, n)).astype(np.int32)
    if n_w > n:
        idxT[0] = rng.integers(n, n_w, n)
    D = np.sort(rng.uniform(0.05, 2.0, (n, kp1)), axis=1)
    for i in zero_rows:
        D[i, :k + 1] = 0.0
    w = _positive_weights(rng, n_w) if w is None else np.asarray(w, dtype=np.float64)
    assert w.shape == (n_w,) and np.all(w > 0)
    return types.SimpleNamespace(name=name, n=n, n_w=n_w, k=k, kp1=kp1, ns=ns, eps=eps,
                                 G=math.gamma(ns / 2 + 1), B=0.1234 + 0.01 * k, idxT=idxT, D=D,
                                 w=w)


@functools.lru_cache(maxsize=None)
def entropy_cases():
    out = []
    ks, nss, epss = (1, 7, 8, 9, 30), (2, 7, 29), (0.0, 1e-15)
    i = 0
    for k in ks:
        for n in (1, 255, 256, 257, 1000):
            kp1 = k + 1 if i % 2 == 0 else k + 3
            out.append(entropy_case(f"k{k}_n{n}", n, k, kp1, nss[i % 3], epss[(i // 3) % 2],
                                    200 + i))
            i += 1
    for ns in nss:  # every ns with both eps, so no pairing is left to the cycling above
        for eps in epss:
            out.append(entropy_case(f"ns{ns}_eps{eps:g}", 257, 8, 9, ns, eps, 300 + i))
            i += 1
    out.append(entropy_case("global_ids", 257, 9, 10, 7, 1e-15, 400, n_w=771))
    out.append(entropy_case("global_ids_k30", 255, 30, 31, 2, 0.0, 401, n_w=2040))
    zr = (0, 3, 100, 255, 256)
    out.append(entropy_case("zeroD_eps0", 257, 7, 8, 2, 0.0, 402, zero_rows=zr))
    out.append(entropy_case("zeroD_eps", 257, 7, 8, 2, 1e-15, 403, zero_rows=zr))
    out.append(entropy_case("zeroD_eps_ns29", 257, 8, 11, 29, 1e-15, 404, zero_rows=zr))
    for nm in ("ragged", "ragged_drift"):
        w = np.asarray(iw_reference(nm).w, dtype=np.float64)
        out.append(entropy_case(f"w_{nm}", w.shape[0], 4, 5, 2, 1e-15, 405, w=w))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def entropy_reference(name):
    c = entropy_cases()[name]
    return entropy_ref(c.w, c.idxT, c.D, c.k, c.ns, c.G, c.B, c.eps, n_w=c.n_w)


HUB_LENS = (64, 64 * 2 + 1, 64 + 15, 64 * 3 + 16, 64 + 17, 64 * 3 + 63, 257)


def table_case(name, nq, k, n_ids, seed, hub_len=0, empties=()):
    """idxT [k, nq] int32, ids in [0, n_ids): random ids that avoid `empties` (ids that own
    nothing) and the hub id, which sits in column 0 of rows [0, hub_len) and nowhere else, so
    its list has exactly hub_len entries."""
    rng = np.random.default_rng(seed)
    hub = n_ids // 3
    banned = set(empties) | ({hub} if hub_len else set())
    allowed = np.array([j for j in range(n_ids) if j not in banned] or [hub], dtype=np.int32)
    idxT = allowed[rng.integers(0, allowed.shape[0], (k, nq))].astype(np.int32)
    assert hub_len <= nq
    idxT[0, :hub_len] = hub
    hub_len = int((idxT == hub).sum()) if hub_len else 0  # (a one-id table is all hub)
    return types.SimpleNamespace(name=name, nq=nq, k=k, n_ids=n_ids, idxT=idxT, hub=hub,
                                 hub_len=hub_len, empties=tuple(empties))


def _empties(n, last=True):
    """Ids that own nothing: id 0, the last id, a run of 40 in the middle."""
    if n < 8:
        return ()
    mid = n // 2
    return (0,) + ((n - 1,) if last else ()) + tuple(range(mid, min(mid + 40, n - 1)))


GAMMA_N = (1, 15, 16, 17, 4095, 32768, 32769, 40002)


@functools.lru_cache(maxsize=None)
def table_cases():
    out = []
    for i, L in enumerate(HUB_LENS):
        k = (1, 2, 30)[i % 3]
        out.append(table_case(f"hub{L}_k{k}", 257, k, 257, 500 + i, hub_len=L,
                              empties=_empties(257)))
    out.append(table_case("hub255_k2", 257, 2, 257, 520, hub_len=255, empties=_empties(257)))
    out.append(table_case("hub208_k30", 257, 30, 257, 521, hub_len=208, empties=_empties(257)))
    for k in (1, 2, 30):
        out.append(table_case(f"nq1_k{k}", 1, k, 5, 530 + k))
    for n in GAMMA_N:  # k = 2 keeps the large tables small
        # 32769: the one particle of gamma_kernel's second grid-stride pass must own something
        out.append(table_case(f"n{n}_k2", n, 2, n, 540 + n, hub_len=min(n, 64 * 5 + 17),
                              empties=_empties(n, last=n != GAMMA_STRIDE + 1)))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def csr_reference(name, world=1, rank=0):
    """(off, rows[:off[-1]], col_offset, n_own) of rank's contiguous id slice by cpu_ops."""
    import cpu_ops
    import torch

    c = table_cases()[name]
    lo, hi = slice_bounds(c.n_ids, world, rank)
    off, rows = cpu_ops.csr_build(torch.as_tensor(c.idxT), c.k, hi - lo, col_offset=lo,
                                  row_offset=0, nq=c.nq)
    off = off.numpy()
    return off, rows.numpy()[:int(off[-1])], lo, hi - lo


def slice_bounds(n, world, rank):
    """Uneven contiguous split of n ids over world ranks."""
    cuts = [min(n, (n * r) // world + r % 2) for r in range(world)] + [n]
    return cuts[rank], cuts[rank + 1]


def gamma_case(table_name, seed):
    """g over the table's nq rows (standard normal), positive w over its n_ids owned ids."""
    c = table_cases()[table_name]
    assert c.n_ids == c.nq
    rng = np.random.default_rng(seed)
    off, rows, _, _ = csr_reference(table_name)
    return types.SimpleNamespace(name=table_name, g=rng.standard_normal(c.nq),
                                 w=_positive_weights(rng, c.n_ids), off=off, rows=rows,
                                 n_own=c.n_ids)


@functools.lru_cache(maxsize=None)
def gamma_cases():
    names = [f"n{n}_k2" for n in GAMMA_N] + [f"hub{L}_k{(1, 2, 30)[i % 3]}"
                                             for i, L in enumerate(HUB_LENS)]
    names += ["hub255_k2", "hub208_k30"]
    return {nm: gamma_case(nm, 600 + i) for i, nm in enumerate(names)}


@functools.lru_cache(maxsize=None)
def gamma_reference(name):
    c = gamma_cases()[name]
    return gamma_ref(c.g, c.w, c.off, c.rows)


def reverse_case(name, lengths, T_stride, seed, nparts):
    """gamma / w over sum(lengths) particles and `nparts` block partials (nparts = 0: S_ext)."""
    rng = np.random.default_rng(seed)
    N = int(sum(lengths))
    return types.SimpleNamespace(name=name, offsets=offsets_of(lengths), nt=len(lengths),
                                 T=T_stride, lengths=list(lengths),
                                 gamma=3.0 * rng.standard_normal(N), w=_positive_weights(rng, N),
                                 partials=rng.standard_normal(max(nparts, 1)) / max(nparts, 1),
                                 nparts=nparts, S_ext=float(rng.standard_normal()) * 0.1)


@functools.lru_cache(maxsize=None)
def reverse_cases():
    out = [reverse_case(f"ragged_parts{p}", RAGGED_LENS, RAGGED_T, 700 + p, p)
           for p in (1, 52, 2047, 2048, 2049)]
    out.append(reverse_case("ragged_ext", RAGGED_LENS, RAGGED_T, 710, 0))
    out.append(reverse_case("nt5_zero_last", [3, 70, 0, 1, 0], 72, 711, 3))
    out.append(reverse_case("nt1_full", [72], 72, 712, 0))
    return {c.name: c for c in out}


def ragged_lengths_for_ranks(seed, groups=6, per_group=4, particles=500, T=256):
    """groups x per_group trajectory lengths in [0, T], every group summing to `particles`, so
    2- and 3-way contiguous trajectory slices hold equal particle counts (the gathered
    normalisation's layout needs one n per rank); a zero length in every second group."""
    rng = np.random.default_rng(seed)
    lens = []
    for gi in range(groups):
        while True:
            cut = np.sort(rng.integers(0, particles + 1, per_group - 1))
            ls = np.diff(np.concatenate([[0], cut, [particles]]))
            if ls.max() <= T and ls.min() >= 1:
                break
        ls = [int(x) for x in ls]
        if gi % 2 == 1:  # fold one trajectory into a neighbour: a zero length
            j = int(np.argmin(ls))
            i = int(np.argmin([x if t != j else 10 ** 9 for t, x in enumerate(ls)]))
            if ls[i] + ls[j] <= T:
                ls[i] += ls[j]
                ls[j] = 0
        lens += ls
    return lens


@functools.lru_cache(maxsize=None)
def chain_case(name="even3000"):
    """A ragged batch with its k-NN-like table for the whole chain IW -> entropy -> CSR -> gamma
    -> reverse scan.  even3000: 3000 particles that split evenly over 2 and 3 ranks (the
    rank-sliced round trip and its one-rank reference); ragged_drift: the ragged length set
    with u over e^+-30, so the reverse scan is fed by the gamma of real weights (one rank)."""
    if name == "ragged_drift":
        iw, ent = iw_cases()["ragged_drift"], entropy_cases()["w_ragged_drift"]
        return types.SimpleNamespace(iw=iw, ent=ent, k=ent.k)
    assert name == "even3000"
    lens = ragged_lengths_for_ranks(800)
    iw = iw_case("chain", lens, 256, 801)
    k = 4
    ent = entropy_case("chain", iw.N, k, k + 1, 2, 1e-15, 802)
    ent.idxT[0] = np.arange(iw.N)  # a k-NN table names the row itself first
    return types.SimpleNamespace(iw=iw, ent=ent, k=k)


@functools.lru_cache(maxsize=None)
def chain_reference(grad_H=-1.0, name="even3000"):
    """The one-rank chain in 80-bit with every stage's bound carried into the next."""
    import cpu_ops
    import torch

    c = chain_case(name)
    iw = iw_ref(c.iw.logp_t, c.iw.logp_b, c.iw.offsets)
    e = c.ent
    en = entropy_ref(iw.w, e.idxT, e.D, e.k, e.ns, e.G, e.B, e.eps, dw=iw.bw)
    off, rows = cpu_ops.csr_build(torch.as_tensor(e.idxT), e.k, c.iw.N)
    ga = gamma_ref(en.g, iw.w, off.numpy(), rows.numpy(), dg=en.bg, dw=iw.bw)
    rv = reverse_ref(ga.gamma, iw.w, ga.S, c.iw.offsets, c.iw.T, grad_H, dgamma=ga.bgamma,
                     dw=iw.bw, dS=ga.bS)
    return types.SimpleNamespace(iw=iw, ent=en, gamma=ga, rev=rv)


# =============================================================================================
# Runners: one case through an `ops`-shaped module, every output checked.  `dev` is the torch
# device of the tensors handed to it ("cpu" for tests/cpu_ops.py).
# =============================================================================================
def _t(x, dev, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(dev)


def _n(x):
    return x.detach().cpu().numpy()


def run_iw(ops, dev, c, ref=None):
    """iw_forward with both `normalize` settings and iw_normalize; returns the tensors."""
    ref = ref if ref is not None else iw_reference(c.name)
    lt, lb, off = _t(c.logp_t, dev), _t(c.logp_b, dev), _t(c.offsets, dev)
    u, ts, w, U = ops.iw_forward(lt, lb, off, c.N)
    check("u", _n(u), ref.u, ref.bu)
    check("traj_sum", _n(ts), ref.ts, ref.bts)
    check("U", _n(U), ref.U, ref.bU)
    check("w", _n(w), ref.w, ref.bw)
    u2, ts2, w2, U2 = ops.iw_forward(lt, lb, off, c.N, normalize=False)
    assert w2 is None and U2 is None
    check("u", _n(u2), ref.u, ref.bu)
    check("traj_sum", _n(ts2), ref.ts, ref.bts)
    # iw_normalize by an external total (a value the kernel did not form itself)
    Ux = _t(np.float64(float(ref.U) * 1.37), dev)
    w3 = ops.iw_normalize(u2, Ux)
    nr = normalize_ref(_n(u2), _n(Ux))
    check("w_normalize", _n(w3), nr.w, nr.bw)
    return dict(u=u, ts=ts, w=w, U=U, u2=u2, ts2=ts2, w3=w3)


def run_entropy(ops, dev, c, ref=None):
    ref = ref if ref is not None else entropy_reference(c.name)
    out4, W, g = ops.entropy_forward(_t(c.w, dev), _t(c.idxT, dev), _t(c.D, dev), c.k, c.ns, c.G,
                                     c.B, c.eps, n_w=c.n_w)
    check("W", _n(W), ref.W, ref.bW)
    check("g", _n(g), ref.g, ref.bg)
    for i, nm in enumerate(("H", "KL", "sum_term", "sum_klterm")):
        check(nm, _n(out4)[i], ref.out4[i], ref.bout4[i])
    return dict(out4=out4, W=W, g=g)


def run_entropy_emit(ops, dev, c1, c2):
    """The emit form twice into one [g | out4] block, as the sharded replay holds it: vals[0]
    is what out4[0] held on entry, bit for bit; vals[1] is the new KL."""
    import torch

    assert c1.n == c2.n
    n = c1.n
    xg = torch.zeros(n + 4, dtype=torch.float64, device=dev)
    xg[n] = 7.25
    vals = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    held = 7.25
    outs = []
    for c in (c1, c2):
        ref = entropy_reference(c.name)
        out4, W, g = ops.entropy_forward(_t(c.w, dev), _t(c.idxT, dev), _t(c.D, dev), c.k, c.ns,
                                         c.G, c.B, c.eps, n_w=c.n_w, g_out=xg[:n], out4=xg[n:],
                                         vals=vals)
        assert out4.data_ptr() == xg[n:].data_ptr() and g.data_ptr() == xg.data_ptr()
        v = _n(vals)
        assert v[0] == held, ("emit: vals[0] is not the H held on entry", v[0], held)
        check("emit_KL", v[1], ref.out4[1], ref.bout4[1])
        check("g", _n(xg[:n]), ref.g, ref.bg)
        for i, nm in enumerate(("H", "KL", "sum_term", "sum_klterm")):
            check(nm, _n(xg[n:])[i], ref.out4[i], ref.bout4[i])
        held = float(_n(xg[n:])[0])
        outs.append((vals.clone(), xg.clone()))
    return outs


def run_csr(ops, dev, c, world=1):
    """csr_build of every rank's id slice against cpu_ops.csr_build; with world > 1 the ranks'
    lists concatenate to the one-rank lists, and a row offset shifts the row ids only."""
    idxT = _t(c.idxT, dev)
    offs, rows_all, outs = [], [], []
    for r in range(world):
        lo, hi = slice_bounds(c.n_ids, world, r)
        if hi - lo == 0:
            continue
        ro, rr, _, _ = csr_reference(c.name, world, r)
        off, rows = ops.csr_build(idxT, c.k, hi - lo, col_offset=lo, row_offset=0, nq=c.nq)
        off_h = _n(off)
        assert off_h.dtype == np.int32
        check_equal_int("csr_off", off_h, ro)
        check_equal_int("csr_rows", _n(rows)[:int(off_h[-1])], rr)
        outs.append((off, rows))
        if world > 1:
            off2, rows2 = ops.csr_build(idxT, c.k, hi - lo, col_offset=lo, row_offset=1000,
                                        nq=c.nq)
            check_equal_int("csr_off", _n(off2), ro)
            check_equal_int("csr_rows", _n(rows2)[:int(off_h[-1])], rr + 1000)
        offs.append(off_h)
        rows_all.append(_n(rows)[:int(off_h[-1])])
    if world > 1:
        one_off, one_rows, _, _ = csr_reference(c.name)
        cat = [np.zeros(1, np.int64)]
        for o in offs:
            cat.append(o[1:].astype(np.int64) + cat[-1][-1])
        check_equal_int("csr_off", np.concatenate(cat), one_off.astype(np.int64))
        check_equal_int("csr_rows", np.concatenate(rows_all), one_rows)
    return outs


def run_gamma(ops, dev, c, nparts_fn=None):
    import torch

    ref = gamma_reference(c.name)
    rows = c.rows if c.rows.shape[0] else np.zeros(1, np.int32)
    gamma, partials, nparts = ops.entropy_gamma(_t(c.g, dev), _t(c.w, dev), _t(c.off, dev),
                                                _t(rows, dev))
    if nparts_fn is not None:
        assert nparts == nparts_fn(c.n_own)
        assert nparts == min((c.n_own * 16 + 255) // 256, 2048)
    check("gamma", _n(gamma), ref.gamma, ref.bgamma)
    # the partials' exact sum (fsum: one rounding, u0 |S|, allowed for below) against S
    Sp = math.fsum(_n(partials)[:nparts].tolist())
    check("S", Sp, ref.S, ref.bS + U0 * np.abs(ref.S))
    assert isinstance(partials, torch.Tensor)
    return dict(gamma=gamma, partials=partials, nparts=nparts)


def run_reverse(ops, dev, c, grad_H, rev_fn=None):
    """entropy_reverse_scan with S from partials (nparts > 0) or S_ext.  rev_fn: the caller's
    own launch (the GPU test pre-fills the output with nan)."""
    fn = rev_fn if rev_fn is not None else ops.entropy_reverse_scan
    gH = _t(np.float64(grad_H), dev)
    if c.nparts > 0:
        S, dS = partials_sum_ref(c.partials[:c.nparts])
        grad = fn(_t(c.gamma, dev), _t(c.w, dev), _t(c.partials, dev), c.nparts,
                  _t(c.offsets, dev), c.nt, c.T, gH)
    else:
        S, dS = ld(c.S_ext), 0
        grad = fn(_t(c.gamma, dev), _t(c.w, dev), _t(c.partials, dev), 0, _t(c.offsets, dev),
                  c.nt, c.T, gH, S_ext=_t(np.float64(c.S_ext), dev))
    ref = reverse_ref(c.gamma, c.w, S, c.offsets, c.T, grad_H, dS=dS)
    assert tuple(grad.shape) == (c.nt, c.T)
    check("grad_logp", _n(grad), ref.grad, ref.bgrad)
    return grad


GATHER_SHAPES = [(world, n, nt) for world in (1, 2, 3, 8) for n in (255, 257) for nt in (3, 200)]


@functools.lru_cache(maxsize=None)
def gather_case(world, n, nt):
    rng = np.random.default_rng(900 + 100 * world + n + nt)
    xu = np.exp(2.0 * rng.standard_normal((world, n + nt)))
    xg1 = rng.standard_normal((world, n + 4))
    xg2 = rng.standard_normal((world, n + 4))
    return types.SimpleNamespace(world=world, n=n, nt=nt, xu=xu, xg=(xg1, xg2), B=0.77)


def run_gathered(ops, dev, c):
    import torch

    w_out = torch.full((c.world * c.n,), float("nan"), dtype=torch.float64, device=dev)
    w = ops.iw_normalize_gathered(_t(c.xu.reshape(-1), dev), c.world, c.n, c.nt, w_out)
    ref = gathered_ref(c.xu, c.world, c.n, c.nt)
    check("w_gathered", _n(w), ref.w, ref.bw)
    return w


def run_emit(ops, dev, c):
    """Two successive sharded_emit calls: the second's vals[0] is B - the first's H-sum."""
    import torch

    n, stride, off = c.n, c.n + 4, c.n + 2
    sums = torch.tensor([0.5, -0.25], dtype=torch.float64, device=dev)
    vals = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    out = []
    for xg in c.xg:
        held = _n(sums).copy()
        ops.sharded_emit(_t(xg.reshape(-1), dev), c.world, stride, off, c.B, c.world * n, sums,
                         vals)
        ref = emit_ref(xg, c.world, stride, off, c.B, c.world * n, held)
        check("emit_vals", _n(vals), ref.vals, ref.bvals)
        check("emit_sums", _n(sums), ref.sums, ref.bsums)
        out.append((vals.clone(), sums.clone()))
    return out


def run_chain(ops, dev, world, grad_H=-1.0, name="even3000"):
    """The rank-sliced round trip of parallel.py on one device, collectives by hand: per rank
    iw_forward(normalize=False) -> [all-gather] -> iw_normalize_gathered -> entropy_forward(n_w =
    N) -> [all-gather of g] -> csr_build(col_offset) -> entropy_gamma -> [sum of S] ->
    reverse_scan(S_ext); the reassembled H, KL and grad_logp against the one-rank reference."""
    import torch

    c, ref = chain_case(name), chain_reference(grad_H, name)
    iw, e = c.iw, c.ent
    N, nt = iw.N, iw.nt
    per = nt // world
    n = N // world
    ranks = []
    for r in range(world):
        tr = slice(r * per, (r + 1) * per)
        off = iw.offsets[r * per:(r + 1) * per + 1] - iw.offsets[r * per]
        assert int(off[-1]) == n and int(iw.offsets[r * per]) == r * n
        ranks.append(types.SimpleNamespace(tr=tr, off=_t(off, dev), R0=r * n))
    xu_all = torch.empty(world * (n + per), dtype=torch.float64, device=dev)
    for r, rk in enumerate(ranks):
        u, ts, w_none, _ = ops.iw_forward(_t(iw.logp_t[rk.tr], dev), _t(iw.logp_b[rk.tr], dev),
                                          rk.off, n, normalize=False)
        assert w_none is None
        xu_all[r * (n + per):r * (n + per) + n] = u
        xu_all[r * (n + per) + n:(r + 1) * (n + per)] = ts
    H_sum, KL_sum, g_all = [], [], []
    for r, rk in enumerate(ranks):
        w_glob = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
        ops.iw_normalize_gathered(xu_all, world, n, per, w_glob)  # every rank forms its own
        rk.w_glob = w_glob
        q = slice(rk.R0, rk.R0 + n)
        out4, W, g = ops.entropy_forward(w_glob, _t(e.idxT[:, q], dev), _t(e.D[q], dev), e.k, e.ns,
                                         e.G, e.B, e.eps, n_w=N)
        check("W", _n(W), ref.ent.W[q], ref.ent.bW[q])
        o = _n(out4)
        H_sum.append(float(o[2]))
        KL_sum.append(float(o[3]))
        g_all.append(g)
    assert all(bits_equal(ranks[0].w_glob, rk.w_glob) for rk in ranks)
    check("w", _n(ranks[0].w_glob), ref.iw.w, ref.iw.bw)
    g_all = torch.cat(g_all)
    check("g", _n(g_all), ref.ent.g, ref.ent.bg)
    # rank-order sums of the raw sums: world - 1 more adds of the same terms (any-order bound)
    check("H", -sum(H_sum) + e.B, ref.ent.out4[0], ref.ent.bout4[0])
    check("KL", sum(KL_sum) / N, ref.ent.out4[1], ref.ent.bout4[1])
    idx_all = _t(e.idxT[:e.k], dev)
    S_parts = []
    for rk in ranks:
        off, rows = ops.csr_build(idx_all, e.k, n, col_offset=rk.R0, row_offset=0, nq=N)
        w_local = rk.w_glob[rk.R0:rk.R0 + n].contiguous()
        rk.gamma, partials, nparts = ops.entropy_gamma(g_all, w_local, off, rows)
        rk.w_local = w_local
        S_parts.append(partials[:nparts].sum().reshape(1))
        check("gamma", _n(rk.gamma), ref.gamma.gamma[rk.R0:rk.R0 + n],
              ref.gamma.bgamma[rk.R0:rk.R0 + n])
    S = torch.cat(S_parts).sum().reshape(())
    check("S", _n(S), ref.gamma.S, ref.gamma.bS)
    gH = _t(np.float64(grad_H), dev)
    grads = []
    for rk in ranks:
        grads.append(ops.entropy_reverse_scan(rk.gamma, rk.w_local, S.reshape(1), 0, rk.off, per,
                                              iw.T, gH, S_ext=S))
    grad = torch.cat(grads)
    check("grad_logp", _n(grad), ref.rev.grad, ref.rev.bgrad)
    return grad


# =============================================================================================
# Every case through one backend, and the table of the largest error / bound per output:
#   python tests/entropy_cases.py cpu|gpu [out.json]
# =============================================================================================
CSR_SHARDED = [("hub129_k2", 2), ("hub129_k2", 3), ("hub208_k30", 2), ("hub208_k30", 3),
               ("nq1_k30", 2), ("n4095_k2", 3), ("n40002_k2", 2)]
GRAD_HS = (1.0, -1.0, 0.37)


def run_all(ops, dev, rev_fn=None, nparts_fn=None):
    for c in iw_cases().values():
        run_iw(ops, dev, c)
    ec = entropy_cases()
    for c in ec.values():
        run_entropy(ops, dev, c)
    run_entropy_emit(ops, dev, ec["ns7_eps1e-15"], ec["ns2_eps0"])
    for c in table_cases().values():
        run_csr(ops, dev, c)
    for name, world in CSR_SHARDED:
        run_csr(ops, dev, table_cases()[name], world)
    for c in gamma_cases().values():
        run_gamma(ops, dev, c, nparts_fn)
    for c in reverse_cases().values():
        for gH in GRAD_HS:
            run_reverse(ops, dev, c, gH, rev_fn)
    for s in GATHER_SHAPES:
        run_gathered(ops, dev, gather_case(*s))
        run_emit(ops, dev, gather_case(*s))
    for world in (1, 2, 3):
        run_chain(ops, dev, world)
    run_chain(ops, dev, 1, 0.37, "ragged_drift")


def gpu_reverse_scan_nan_filled(gamma, w, partials, nparts, offsets, nt, T_stride, grad_H,
                                S_ext=None):
    """ops.entropy_reverse_scan into a buffer pre-filled with nan: an unwritten tail shows."""
    import torch

    from mepol_amd import ops
    from mepol_amd._lib import call, ptr

    grad = torch.full((nt, T_stride), float("nan"), dtype=torch.float64, device=w.device)
    call("mepol_entropy_reverse_scan", ptr(gamma), ptr(w), ptr(partials), nparts, ptr(S_ext),
         ptr(offsets), nt, T_stride, ptr(grad_H), ptr(grad), ops._stream())
    return grad


if __name__ == "__main__":
    import json
    import os
    import sys
    import time

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t0 = time.time()
    if sys.argv[1] == "gpu":
        import torch

        from mepol_amd import ops as gpu_ops

        run_all(gpu_ops, torch.device("cuda"), gpu_reverse_scan_nan_filled,
                gpu_ops.entropy_gamma_nparts)
    else:
        import cpu_ops as host_ops

        run_all(host_ops, "cpu")
    for key in sorted(RATIOS):
        print(f"{key:14s} {RATIOS[key]:.4f}")
    print(f"# {sys.argv[1]}: all cases within bounds, {time.time() - t0:.1f} s")
    overall = dict(RATIOS)
    # the same figure at the largest shape of each family alone (the overall maxima above sit in
    # the smallest cases, where one or two roundings meet a bound of one or two)
    backend = (gpu_ops, torch.device("cuda")) if sys.argv[1] == "gpu" else (host_ops, "cpu")
    rev = gpu_reverse_scan_nan_filled if sys.argv[1] == "gpu" else None
    headline = {
        "iw ragged_drift": lambda: run_iw(*backend, iw_cases()["ragged_drift"]),
        "iw nt4100": lambda: run_iw(*backend, iw_cases()["nt4100"]),
        "entropy k30_n1000": lambda: run_entropy(*backend, entropy_cases()["k30_n1000"]),
        "entropy w_ragged_drift": lambda: run_entropy(*backend,
                                                      entropy_cases()["w_ragged_drift"]),
        "gamma n40002_k2": lambda: run_gamma(*backend, gamma_cases()["n40002_k2"]),
        "reverse ragged_parts2048": lambda: run_reverse(
            *backend, reverse_cases()["ragged_parts2048"], 0.37, rev),
        "chain world 3": lambda: run_chain(*backend, 3),
    }
    large = {}
    for title, fn in headline.items():
        RATIOS.clear()
        fn()
        large[title] = dict(RATIOS)
        print(f"{title:26s} " + "  ".join(f"{k} {v:.2g}" for k, v in sorted(RATIOS.items())))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w", encoding="utf-8") as f:
            json.dump({"overall": overall, "largest_shapes": large}, f, indent=1, sort_keys=True)
