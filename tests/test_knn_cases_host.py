"""The k-NN cases of tests/knn_cases.py on the host: the data, the oracle, the plan and the model.

No GPU.  This file shows that
  * every case builds deterministically, is finite, is answered by the oracle, and is the exact
    power-of-two multiple of its base set where it claims to be;
  * plan_model restates make_plan: it agrees with mepol_knn_plan_info (host only) over the whole
    sweep d = 1..63, k+1 = 1..60 at both sizes, the `plans` cases visit every (KS16, nh, LIST16)
    the library's sweep finds and every refine_kernel<64, MAXP>, and each has k+1 <= n;
  * in the host model of the screen (knn_cases.screen_model) every in-contract case (self-query
    or max |q| <= max |c|, norms in the normal f32 range) stays within the bound E and is not
    routed away from the screen, before and after the screen's domain was introduced;
  * the adversarial cases break the model of the arithmetic before the domain existed, and with
    the domain every case is within E or routed to the exhaustive stage.
tests/test_gpu_knn_ops.py runs the same cases through the HIP kernels.
"""
import numpy as np
import pytest

import knn_cases as K

ALL = K.case_ids()


@pytest.mark.parametrize("family,name", ALL)
def test_case_builds_and_oracle_answers(family, name):
    c = K.get_case(family, name)
    n, d = c.X.shape
    assert c.X.dtype == np.float32 and np.isfinite(c.X).all()
    assert n <= 20000 and 1 <= c.kp1 <= n
    if c.Q is not None:
        assert c.Q.dtype == np.float32 and np.isfinite(c.Q).all()
        assert len(c.Q) <= 256 and c.Q.shape[1] == d
    again = K.FAMILIES[family][1].__wrapped__(name)
    assert np.array_equal(again.X, c.X) and (c.Q is None or np.array_equal(again.Q, c.Q))
    D, I = K.oracle(family, name)
    assert D.shape == I.shape == (len(c.queries), c.kp1)
    assert np.isfinite(D).all() and (D[:, 1:] >= D[:, :-1]).all()
    assert ((I >= 0) & (I < n)).all()


@pytest.mark.parametrize("name", [n for n in K.SCALE_NAMES if n[0] == "a" and n != "a_mixed"]
                         + ["b_1e-36", "b_1e18"])
def test_scaled_oracle_is_the_base_oracle_scaled(name):
    """The shared reference of a `scale` case (the base set's I, its D times 2^e) is what the
    oracle gives on the case itself, bit for bit."""
    c = K.get_case("scale", name)
    X0 = K.scale_base_case(name[0]).X
    assert np.array_equal(c.X.astype(np.float64), np.ldexp(X0.astype(np.float64), c.exp))
    D, I = K.oracle("scale", name)
    Dd, Id = K.oracle("scale", name, direct=True)
    assert np.array_equal(D, Dd) and np.array_equal(I, Id)


def test_scale_cases_reach_the_edges():
    tiny = np.float32(K.F32_MIN_NORMAL)
    # squared norms in the f32 subnormal range: a few units of 2^-149 at 1e-22, about one at
    # 3e-23 (each partial sum then rounds to 0 or to 2^-149)
    s2 = K._fma_sumsq32(K.get_case("scale", "a_1e-22").X)
    assert 0 < s2.max() < tiny
    last = 2.0 ** -149
    assert 0.5 * last < K._max_norm(K.get_case("scale", "a_3e-23").X) ** 2 < 2 * last
    assert K._fma_sumsq32(K.get_case("scale", "a_3e-23").X).max() <= last
    assert K._fma_sumsq32(K.get_case("scale", "a_1e-24").X).max() == 0
    sub = K.get_case("scale", "a_subnormal").X
    assert 0 < np.abs(sub).max() < tiny
    mixed = K.get_case("scale", "a_mixed").X
    n2 = (mixed.astype(np.float64) ** 2).sum(axis=1)
    assert (n2 < 1e-55).sum() == 200 and n2.max() > 1


def test_lattice_ties_straddle_the_cut():
    X = K.get_case("lattice", "k7").X
    assert len(np.unique(X, axis=0)) == 4096
    for name in K.LATTICE_NAMES:
        D, _ = K.oracle("lattice", name)
        kp1 = D.shape[1]
        Dn, _ = K.O.knn_exact(X, kp1 + 1, Q=X[:512])
        tied = Dn[:, kp1] == Dn[:, kp1 - 1]  # the first excluded point ties with the last kept
        assert tied.any() and (D[:, 0] == 0).all()


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def knn_plan(monkeypatch_module):
    from mepol_amd import ops

    return ops.knn_plan


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    mp.delenv("MEPOL_KNN_NH", raising=False)
    yield mp
    mp.undo()


KEYS = ("KS16", "nh", "LIST16", "split")


def test_plan_model_is_make_plan(knn_plan):
    for n in K.PLAN_NS + (3000, 20000):
        for nq in (K.PLAN_NQ, n):
            for d in range(1, K.SCREEN_MAX_D + 1):
                for kp1 in range(1, K.SCREEN_MAX_KP1 + 1):
                    got, want = knn_plan(n, nq, d, kp1), K.plan_model(n, nq, d, kp1)
                    assert all(got[k] == want[k] for k in KEYS), (n, nq, d, kp1, got, want)
                    assert got["mfma_products"] == 1 + want["query_lo"] + (want["nh"] == 2)


def test_plan_cases_visit_every_reachable_plan(knn_plan):
    found = K.sweep_triples(knn_plan)
    assert {t[1] for t in found} == {1, 2}, "the sweep no longer reaches both candidate forms"
    visited, maxp = set(), set()
    for name in K.PLAN_NAMES:
        n, d, kp1, split, claim = K.plan_specs()[name]
        assert kp1 <= n and n % 32 == 1 and K.PLAN_NQ % 4 and K.PLAN_NQ % 32
        got = knn_plan(n, K.PLAN_NQ, d, kp1, split)
        assert all(got[k] == claim[k] for k in KEYS), (name, got, claim)
        visited.add((got["KS16"], got["nh"], got["LIST16"]))
        maxp.add(claim["MAXP"])
        assert claim["M"] == 2 * got["split"] * got["LIST16"]
    assert visited == set(found), sorted(set(found) - visited)
    assert maxp == set(K.REFINE_MAXP)  # rank merge (<= 4) and argmin rounds (> 4)


# ---------------------------------------------------------------------------------------------
# the model of the screen
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name", [fn for fn in ALL if K.get_case(*fn).in_contract])
def test_in_contract_cases_stay_within_the_bound(family, name):
    for parent in (True, False):
        m = K.model(family, name, parent)
        assert m["ratio"] <= 1 and m["wrong"] == 0 and not m["routed"], (parent, m)
    # the domain changes nothing here: the same sigma, C and ratio
    assert K.model(family, name, True) == K.model(family, name, False)


@pytest.mark.parametrize("family,name", [fn for fn in ALL if K.get_case(*fn).parent_fails])
def test_adversarial_cases_break_the_bound_without_the_domain(family, name):
    """The `scale` cases at or below 1e-24 (and the subnormal coordinates) and the `qc_ratio`
    cases at or above 2^20 exceed E in the model of the arithmetic before the domain existed.

    The `qc_ratio` query norms run from the candidates' size up to 2^r times it.  A query set of
    one size, 2^20 times the candidates', stays within E under candidate-hi plans (model ratios
    0.65 to 0.8: the 2 x 8192 units for the relative f16 rounding absorb the floor of the
    operand -2 sigma c up to about 2^21); what breaks those plans at 2^20 is the norm column
    |sigma c|^2, which f16 rounds to 0, against the candidate-sized queries whose E ~ C^2."""
    m = K.model(family, name, parent=True)
    assert m["ratio"] > 1 and not m["routed"], m


@pytest.mark.parametrize("family,name", ALL)
def test_every_case_is_within_the_bound_or_routed(family, name):
    m = K.model(family, name)
    assert m["routed"] == K.routed(K.get_case(family, name))
    assert m["routed"] or (m["ratio"] <= 1 and m["wrong"] == 0), m


def test_domain_edges():
    f = np.float32
    assert not K.off_domain(f(0), f(0))                              # all-zero input stays
    assert K.off_domain(f(2.0 ** -57), f(2.0 ** -57)) and not K.off_domain(f(2.0 ** -56), f(0))
    assert K.off_domain(f(2.0 ** 62), f(1)) and not K.off_domain(np.nextafter(f(2.0 ** 62), f(0)), f(1))
    assert not K.off_domain(f(1), f(32)) and K.off_domain(f(1), np.nextafter(f(32), f(64)))
    assert not K.off_domain(f(1), f(2.0 ** -40))                     # small queries are in
    assert K.off_domain(f(0), f(1))
    # a row whose squared norm underflows is reported as at least |x| (at most 8 |x| for normal
    # coordinates), never as zero
    for scale in (2.0 ** -70, 2.0 ** -100, 2.0 ** -140):
        x = (np.arange(1, 64, dtype=np.float64) * scale).astype(np.float32)[None, :]
        true = float(np.sqrt((x.astype(np.float64) ** 2).sum()))
        got, _ = K.reported_max_norm(x)
        assert true <= float(got) and (float(got) <= 8 * true or x.max() < K.F32_MIN_NORMAL)
        assert K.off_domain(got, got)
