"""Named k-NN cases at the edges of the f16 screen's error bound, and a host model of the screen.

The k-NN (csrc/knn.hip, knn_select.hpp, knn_exact.hip) ranks candidates by an f16 MFMA screen and
certifies every query with E = e_terms 2^-24 (C^2 + 2 C |q|), C the largest candidate norm; only
uncertified queries take the exhaustive f64 scan.  A bound that is too small for some input
returns wrong neighbours that nothing downstream can notice, so the cases here sit where E is
weakest, and every one is compared bit for bit with oracle.mepol_oracle.knn_exact:

  scale     one point set times 2^e, largest norm 1e-36 .. 1e18 (squared norms that underflow
            f32, f32-subnormal coordinates, and a normal cloud with 200 rows at 1e-30);
  qc_ratio  queries != candidates with max |q| / max |c| = 2^+-10, 2^+-20, 2^+-40 (large
            queries: norms from the candidates' size up to the largest, which sets sigma for
            all), and one huge query among copies of candidates;
  offset    X = offset + noise (C large, neighbour spacing tiny: almost nothing certifies), and
            a constant column of 2^15 beside N(0, 2^-10) columns;
  lattice   the 4096 points of {0..3}^6: distinct points, exactly tied distances, tie groups
            across the k+1 cut;
  plans     one (n, d, k+1) per reachable (KS16, nh, LIST16) of make_plan and split hints that
            reach every refine_kernel<64, MAXP>, as a query shard of 203 rows, n = 1 (mod 32).

plan_model() restates make_plan, off_domain() the screen's domain (knn_common.hpp), and
screen_model() the screen's arithmetic in numpy: the f32 norms and sigma, A = [-2 sigma c,
|sigma c|^2] and B = [sigma q, 1] split into f16 hi / lo, the products the plan forms, the
1 / sigma^2 the values are reported with, and E.  It reads no kernel output.  Simplifications: the
products are summed in f64 and rounded to f32 once (the kernels' f32 accumulation error, which E
pays for separately, is left out), and the partial lists are one global approximate top-64.
`parent=True` models the arithmetic before the domain was introduced (the norm of a row whose
squared norm underflows is sqrtf of that, and nothing is routed away from the screen).

Data is built from default_rng(seed) only; scaling is by powers of two of points on a 2^-10
grid, so that every `scale` case is its base set times 2^e exactly, subnormal coordinates
included.  `python tests/knn_cases.py` prints the table of model ratios.
"""
import functools
import math
import os
import sys
from dataclasses import dataclass, field

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import mepol_oracle as O  # noqa: E402

F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


# ---------------------------------------------------------------------------------------------
# make_plan and the screen's domain, restated
# ---------------------------------------------------------------------------------------------
LIST_CHOICES = (8, 16, 20, 22, 24, 32, 40)  # kListChoices
SCREEN_MAX_D, SCREEN_MAX_KP1, MAX_SPLIT = 63, 60, 16


def plan_model(nc, nq, d, kp1, split=0):
    """make_plan (csrc/knn.hip) for a screened shape, MEPOL_KNN_NH unset."""
    assert d <= SCREEN_MAX_D and kp1 <= SCREEN_MAX_KP1 and kp1 <= nc
    KS16 = (d + 1 + 15) // 16
    keep = (kp1 + 1) // 2 + 2
    LIST16 = next((v for v in LIST_CHOICES if v >= keep + 4), 40)
    band = 3.0 / 2048.0 * (nc / kp1) ** (2.0 / d)
    nh = 2 if band > 0.03 else 1
    fits2 = (KS16 <= 3 and LIST16 <= (32 if KS16 == 3 else 40)) or (KS16 == 4 and LIST16 <= 32)
    if not fits2:
        nh = 1
    e_terms = (8192 + 64 + 2 * (2 * 16 * KS16 + 16 + d)) if nh == 1 else 2 * (3 * 16 * KS16 + 16 + d)
    if nh == 1 and KS16 <= 3:
        e_terms += 8192 + 64
    nct, nqt = (nc + 31) // 32, (nq + 31) // 32
    if split <= 0:
        split = min(MAX_SPLIT, max(1, (1600 + nqt // 2) // max(nqt, 1)))
        split = max(split, 2)
        split = min(split, max(2, 256 // (2 * LIST16)))
        while split > 1 and nct // split < 16:
            split -= 1
    split = max(1, min(split, MAX_SPLIT))
    M = 2 * split * LIST16
    maxp = (M + 63) // 64
    inst = next(v for v in (2, 4, 8, 16, 32) if maxp <= v)  # launch_refine
    return dict(KS16=KS16, nh=nh, LIST16=LIST16, split=split, e_terms=e_terms, keep=keep, M=M,
                MAXP=inst, query_lo=nh == 2 or KS16 >= 4)


def _bits(x):
    return int(np.float32(x).view(np.uint32))


SCREEN_MIN_BITS, SCREEN_MAX_BITS, SCREEN_QC_BITS = 0x23800000, 0x5E800000, 5 << 23


def off_domain(cmax, qmax):
    """off_screen_domain (csrc/knn_common.hpp) on the two reported maxima (f32)."""
    c, q = _bits(cmax), _bits(qmax)
    m = max(c, q)
    return m != 0 and (m < SCREEN_MIN_BITS or m >= SCREEN_MAX_BITS or q > c + SCREEN_QC_BITS)


# ---------------------------------------------------------------------------------------------
# the screen's arithmetic
# ---------------------------------------------------------------------------------------------
def _fma_sumsq32(Y):
    """s2 = fmaf(v, v, s2) over the columns in order, f32 (v * v is exact in f64; the one f64
    rounding of the sum before the f32 rounding is far below the f32 one)."""
    s2 = np.zeros(Y.shape[0], np.float32)
    Y64 = Y.astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        for f in range(Y.shape[1]):
            s2 = (Y64[:, f] * Y64[:, f] + s2.astype(np.float64)).astype(np.float32)
    return s2


def reported_max_norm(X, parent=False):
    """norms_kernel: (max norm as f32, rows whose squared norm overflows)."""
    X = np.asarray(X, np.float32)
    s2 = _fma_sumsq32(X)
    over = ~np.isfinite(s2)
    with np.errstate(invalid="ignore"):
        nrm = np.sqrt(s2).astype(np.float32)
    if not parent:
        mag = np.abs(X).max(axis=1).astype(np.float32)
        tiny = (mag != 0) & (s2 < np.float32(F32_MIN_NORMAL))
        up = (mag.view(np.uint32) + np.uint32(3 << 23)).view(np.float32)
        nrm = np.where(tiny, up, nrm)
    nrm = np.where(over, np.float32(0), nrm)
    return np.float32(nrm.max()), int(over.sum())


def knn_scale(cmax, qmax):
    """knn_scale (csrc/knn_common.hpp): sigma = 2^e, the clamp to +-100 included."""
    m = np.float32(max(cmax, qmax))
    if not (m > 0) or not (m < np.float32(3e38)):
        return np.float32(1)
    with np.errstate(over="ignore"):
        _, e = np.frexp(np.float32(127.9) / m)
    e = max(-100, min(100, int(e) - 1))
    return np.float32(math.ldexp(1.0, e))


def _split16(V):
    with np.errstate(over="ignore", under="ignore"):
        hi = V.astype(np.float16)
        lo = (V - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def screen_model(X, Q, plan, kp1, parent=False, nsel=64):
    """The screen on candidates X and queries Q under `plan` (plan_model).  Returns a dict:
    ratio  max |approx - exact| / E over every (query, candidate), in the screen's quantity
           |c|^2 - 2 q.c (the exact one taken as d^2 - |q|^2 in f64);
    wrong  queries that refine's test certifies although the exact top-(k+1) of the approximate
           top-64 is not the true one;
    certified, routed (the input is outside the screen's domain: every query takes the
    exhaustive stage), sigma, C."""
    X = np.ascontiguousarray(X, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    nc, d = X.shape
    cmax, cover = reported_max_norm(X, parent)
    qmax, qover = reported_max_norm(Q, parent)
    routed = bool(cover or qover) or (not parent and off_domain(cmax, qmax))
    sg = knn_scale(cmax, qmax)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        inv_s2 = np.float32(1) / (sg * sg)  # f32: sigma^2 overflows beyond 2^63
        Y = (sg * X).astype(np.float32)
        cn = _fma_sumsq32(Y)
        A = np.concatenate([(np.float32(-2) * sg * X).astype(np.float32), cn[:, None]], axis=1)
        B = np.concatenate([(sg * Q).astype(np.float32), np.ones((len(Q), 1), np.float32)], axis=1)
        ahi, alo = _split16(A)
        bhi, blo = _split16(B)
        acc = bhi @ ahi.T
        if plan["query_lo"]:
            acc += blo @ ahi.T
        if plan["nh"] == 2:
            acc += bhi @ alo.T
        approx = (acc.astype(np.float32) * inv_s2).astype(np.float64)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    d2 = np.zeros((len(Q), nc))
    for f in range(d):
        t = Q64[:, f:f + 1] - X64[None, :, f]
        d2 += t * t
    qn2 = (Q64 * Q64).sum(axis=1)
    C = float(cmax)
    E = plan["e_terms"] * 2.0 ** -24 * (C * C + 2.0 * C * np.sqrt(qn2)) + 1e-300
    with np.errstate(invalid="ignore"):
        err = np.abs(approx - (d2 - qn2[:, None]))
    err = np.where(np.isnan(err), np.inf, err)
    ratio = float((err / E[:, None]).max())
    # refine's certification on one global approximate top-nsel
    idx = np.arange(nc)
    wrong = certified = 0
    for r in range(len(Q)):
        order = np.lexsort((idx, approx[r]))
        sel = order[:nsel]
        bnd = approx[r, order[nsel]] if nc > nsel else np.inf
        ex = np.lexsort((sel, d2[r, sel]))[:kp1]
        got = sel[ex]
        ek = d2[r, got[-1]]
        ok = (not bnd < np.inf) or ek < (bnd + qn2[r]) - E[r]
        if ok:
            certified += 1
            true = np.lexsort((idx, d2[r]))[:kp1]
            wrong += int(not np.array_equal(true, got))
    return dict(ratio=ratio, wrong=wrong, certified=certified, routed=routed, sigma=float(sg), C=C,
                qmax=float(qmax))


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
@dataclass
class Case:
    family: str
    name: str
    X: np.ndarray
    kp1: int
    Q: np.ndarray = None          # None: self-query
    split: int = 0
    base: str = None              # scale: the unscaled case this one is 2^exp times
    exp: int = 0
    in_contract: bool = True      # self-query or qmax <= cmax, norms in the normal f32 range
    parent_fails: bool = False    # adversarial by construction: parent model ratio > 1
    claim: dict = field(default_factory=dict)  # plans: the plan this case stands for

    @property
    def queries(self):
        return self.X if self.Q is None else self.Q


def _grid(rng, n, d):
    """N(0, 1) on a 2^-10 grid: times 2^e it stays exact in f32 down to subnormal coordinates."""
    return (np.round(rng.standard_normal((n, d)) * 1024.0) / 1024.0).astype(np.float32)


def _pow2(X, e):
    Y = np.ldexp(X.astype(np.float64), e)
    Y32 = Y.astype(np.float32)
    assert np.array_equal(Y32.astype(np.float64), Y), "the scaling is not exact in f32"
    return Y32


def _max_norm(X):
    return float(np.sqrt((X.astype(np.float64) ** 2).sum(axis=1)).max())


SCALE_BASES = {"a": (3000, 7, 5, 101), "b": (4097, 29, 31, 102)}  # n, d, k+1, seed
SCALE_TARGETS = ["1e-36", "1e-30", "1e-24", "3e-23", "1e-22", "1e-19", "1e-10", "1", "1e10", "1e18"]
SCALE_NAMES = [f"{b}_{t}" for b in SCALE_BASES for t in SCALE_TARGETS] + ["a_subnormal", "a_mixed"]


@functools.lru_cache(maxsize=None)
def _scale_base(b):
    n, d, kp1, seed = SCALE_BASES[b]
    return _grid(np.random.default_rng(seed), n, d), kp1


@functools.lru_cache(maxsize=None)
def scale_case(name):
    b, t = name.split("_")
    X0, kp1 = _scale_base(b)
    if t == "mixed":
        # a normal-scale cloud plus 200 rows at 1e-30: C is normal, the in-contract control
        X = X0.copy()
        X[1000:1200] = _pow2(X0[1000:1200], -100)
        return Case("scale", name, X, kp1)
    if t == "subnormal":
        e = round(math.log2(1e-40 / float(np.abs(X0).max())))  # coordinates ~1e-40 and below
    else:
        e = round(math.log2(float(t) / _max_norm(X0)))
    X = _pow2(X0, e)
    tiny = _max_norm(X) ** 2 < F32_MIN_NORMAL
    return Case("scale", name, X, kp1, base=f"{b}_base", exp=e, in_contract=not tiny,
                parent_fails=t == "subnormal" or (t != "1" and float(t) <= 1e-24))


@functools.lru_cache(maxsize=None)
def scale_base_case(b):
    X0, kp1 = _scale_base(b)
    return Case("scale", f"{b}_base", X0, kp1)


QC_SHAPES = {"d3": (20000, 3, 51, 201), "d7": (20000, 7, 51, 202), "d29": (4000, 29, 31, 203)}
QC_LOG2 = [10, 20, 40, -10, -20, -40]
QC_NQ = 67
QC_NAMES = [f"{s}_q{'p' if r > 0 else 'm'}{abs(r)}" for s in QC_SHAPES for r in QC_LOG2] + [
    f"{s}_one_huge" for s in QC_SHAPES]


@functools.lru_cache(maxsize=None)
def qc_case(name):
    s, rest = name.split("_", 1)
    n, d, kp1, seed = QC_SHAPES[s]
    rng = np.random.default_rng(seed)
    G0 = _grid(rng, n, d)
    Q0 = _grid(rng, QC_NQ, d)
    if rest == "one_huge":
        X = _pow2(G0, -20)
        Q = X[rng.choice(n, QC_NQ, replace=False)].copy()
        Q[QC_NQ // 2] = _pow2(Q0[:1], 20)[0]  # max |q| / max |c| ~ 2^40, for every query's sigma
        return Case("qc_ratio", name, X, kp1, Q=Q, in_contract=False, parent_fails=True)
    r = int(rest[2:]) * (1 if rest[1] == "p" else -1)
    if r < 0:
        # small queries: one N(0, 1) cloud 2^-|r| the size of the candidates' (in contract)
        e = math.ceil(-r + math.log2(_max_norm(Q0) / _max_norm(G0)))
        X, Q = _pow2(G0, -20 + e), _pow2(Q0, -20)
    else:
        # large queries: row i of an N(0, 1) cloud times 2^(r i / (nq - 1)), so the query norms
        # run from the candidates' size to 2^r times it.  The largest query sets sigma for all of
        # them; it meets the f16 floor in the operand -2 sigma c, the candidate-sized ones in
        # their own operand sigma q and in the norm column |sigma c|^2, which f16 rounds to a
        # multiple of 2^-24 or to 0 while their E ~ C^2 gives it no room.
        steps = np.round(r * np.arange(QC_NQ) / (QC_NQ - 1)).astype(int)
        Qr = np.stack([_pow2(Q0[i:i + 1], int(steps[i]))[0] for i in range(QC_NQ)])
        e = math.ceil(r - math.log2(_max_norm(Qr) / _max_norm(G0)))
        X, Q = _pow2(G0, -20), _pow2(Qr, -20 + e)
    ratio = _max_norm(Q) / _max_norm(X)
    assert 2.0 ** abs(r) <= (ratio if r > 0 else 1 / ratio) < 2.0 ** (abs(r) + 1)
    return Case("qc_ratio", name, X, kp1, Q=Q, in_contract=r < 0, parent_fails=r >= 20)


OFFSET_NAMES = [f"d{d}_r{r}" for d in (2, 29) for r in (10, 18)] + ["const_col"]


@functools.lru_cache(maxsize=None)
def offset_case(name):
    if name == "const_col":
        rng = np.random.default_rng(303)
        X = _pow2(_grid(rng, 3000, 8), -10)
        X[:, 0] = 2.0 ** 15  # f16-subnormal operands next to large ones
        return Case("offset", name, X, 5)
    d, r = int(name.split("_")[0][1:]), int(name.split("_")[1][1:])
    rng = np.random.default_rng(300 + d + r)
    X = (np.float32(2.0 ** r) + rng.standard_normal((3000, d))).astype(np.float32)
    return Case("offset", name, X, 5 if d == 2 else 31)


LATTICE_NAMES = [f"k{k}" for k in (7, 8, 13, 14)]


@functools.lru_cache(maxsize=None)
def _lattice():
    pts = np.stack(np.meshgrid(*[np.arange(4)] * 6, indexing="ij"), axis=-1).reshape(-1, 6)
    return pts[np.random.default_rng(404).permutation(len(pts))].astype(np.float32)


@functools.lru_cache(maxsize=None)
def lattice_case(name):
    # a point has 6 (corner) to 12 (interior) lattice neighbours at distance 1, then up to 60 at
    # sqrt 2: with the point itself, k+1 = 7 / 13 end exactly on a group there and cut one
    # elsewhere, 8 / 14 take one more
    return Case("lattice", name, _lattice(), int(name[1:]))


PLAN_NS = (4097, 19969)  # both = 1 (mod 32); the larger reaches nh = 2
PLAN_NQ = 203            # a query shard: a multiple of neither 4 nor 32
REFINE_MAXP = (2, 4, 8, 16, 32)


def sweep_triples(plan_fn):
    """{(KS16, nh, LIST16): first (n, d, k+1) in sweep order} over d = 1..63, k+1 = 1..60."""
    seen = {}
    for n in PLAN_NS:
        for d in range(1, SCREEN_MAX_D + 1):
            for kp1 in range(1, SCREEN_MAX_KP1 + 1):
                p = plan_fn(n, PLAN_NQ, d, kp1)
                seen.setdefault((p["KS16"], p["nh"], p["LIST16"]), (n, d, kp1))
    return seen


@functools.lru_cache(maxsize=None)
def plan_specs():
    """{name: (n, d, k+1, split hint, claimed plan)}: one per triple of the sweep, then one per
    refine_kernel<64, MAXP> by split hints on the shapes with the shortest and longest lists."""
    specs = {}
    for (ks, nh, lst), (n, d, kp1) in sorted(sweep_triples(plan_model).items()):
        specs[f"ks{ks}_nh{nh}_l{lst}"] = (n, d, kp1, 0, plan_model(n, PLAN_NQ, d, kp1))
    want = set(REFINE_MAXP)
    for n, d, kp1 in ((4097, 29, 31), (4097, 12, 60)):
        for split in range(1, MAX_SPLIT + 1):
            p = plan_model(n, PLAN_NQ, d, kp1, split)
            if p["MAXP"] in want:
                want.discard(p["MAXP"])
                specs[f"maxp{p['MAXP']}_d{d}_s{split}"] = (n, d, kp1, split, p)
    assert not want, f"no split hint reaches refine_kernel<64, {sorted(want)}>"
    return specs


PLAN_NAMES = list(plan_specs())


@functools.lru_cache(maxsize=None)
def plan_case(name):
    n, d, kp1, split, claim = plan_specs()[name]
    rng = np.random.default_rng(500 + 64 * d + kp1 + n % 7)
    X = rng.standard_normal((n, d)).astype(np.float32)
    rows = np.sort(rng.choice(n, PLAN_NQ, replace=False))
    return Case("plans", name, X, kp1, Q=X[rows].copy(), split=split, claim=claim)


FAMILIES = {"scale": (SCALE_NAMES, scale_case), "qc_ratio": (QC_NAMES, qc_case),
            "offset": (OFFSET_NAMES, offset_case), "lattice": (LATTICE_NAMES, lattice_case),
            "plans": (PLAN_NAMES, plan_case)}


def case_ids():
    return [(fam, name) for fam, (names, _) in FAMILIES.items() for name in names]


def get_case(family, name):
    return FAMILIES[family][1](name)


# ---------------------------------------------------------------------------------------------
# the oracle, once per case (and once per base set for the exact power-of-two scalings)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_direct(family, name):
    c = scale_base_case(name[0]) if name.endswith("_base") else get_case(family, name)
    D, I = O.knn_exact(c.X, c.kp1, Q=c.Q)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


def oracle(family, name, direct=False):
    """(D, I) of oracle.mepol_oracle.knn_exact.  A `scale` case that is its base set times 2^e
    exactly has the base's I and the base's D times 2^e, exactly (every f64 operation of the
    oracle scales with it: no f64 underflow at these sizes); direct=True runs the oracle on the
    case itself (tests/test_knn_cases_host.py compares the two)."""
    c = get_case(family, name)
    if c.base is None or direct:
        return _oracle_direct(family, name)
    D0, I0 = _oracle_direct("scale", c.base)
    D = np.ldexp(D0, c.exp)
    assert np.all((D == 0) | (np.abs(D) >= np.finfo(np.float64).tiny))
    return D, I0


def routed(c):
    """The case is outside the screen's domain: every query takes the exhaustive stage."""
    cmax, cover = reported_max_norm(c.X)
    qmax, qover = reported_max_norm(c.queries)
    return bool(cover or qover) or off_domain(cmax, qmax)


MODEL_NQ = 128  # self-query cases: the model takes the first 128 rows as queries


@functools.lru_cache(maxsize=None)
def model(family, name, parent=False):
    c = get_case(family, name)
    Q = c.X[:MODEL_NQ] if c.Q is None else c.Q
    plan = plan_model(len(c.X), len(c.queries), c.X.shape[1], c.kp1, c.split)
    return screen_model(c.X, Q, plan, c.kp1, parent=parent)


def ratio_table():
    lines = [f"{'family':9s} {'case':22s} {'nh':>2s} {'sigma':>9s} {'C':>9s} {'qmax':>9s} "
             f"{'parent ratio':>12s} {'wrong':>5s} {'ratio':>10s} {'wrong':>5s} routed"]
    for fam, name in case_ids():
        c = get_case(fam, name)
        plan = plan_model(len(c.X), len(c.queries), c.X.shape[1], c.kp1, c.split)
        p, m = model(fam, name, True), model(fam, name, False)
        lines.append(f"{fam:9s} {name:22s} {plan['nh']:2d} {m['sigma']:9.2e} {m['C']:9.2e} "
                     f"{m['qmax']:9.2e} {p['ratio']:12.3e} {p['wrong']:5d} {m['ratio']:10.3e} "
                     f"{m['wrong']:5d} {'yes' if m['routed'] else 'no'}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(ratio_table())
