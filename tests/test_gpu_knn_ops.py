"""The k-NN kernels case by case where the f16 screen's error bound is weakest.

Every case of tests/knn_cases.py goes through mepol_amd.ops.knn (csrc/knn.hip, knn_select.hpp,
knn_exact.hip) in the synchronous and the deferred-check form: D and I bit-equal to the CPU
oracle's exhaustive f64 scan, the transposed int32 table equal to I, a second run the same bits,
0 <= n_fallback <= nq.  There are no tolerances.  Per family:
  scale     I is the unscaled set's I and D its D times 2^e, bit for bit (the scaling is exact);
  plans     ops.knn_plan reports the (KS16, nh, LIST16, split) the case stands for, the library's
            own sweep finds no plan without a case, and MEPOL_KNN_SEED 0 / 1 / 2 give the same
            bits on the smallest case of each candidate form;
  qc_ratio, offset   correctness only: how many queries take the exhaustive stage is not asserted.
A case outside the screen's domain (knn_cases.routed) reports every query as answered by the
exhaustive stage; an in-domain `scale` or `plans` case does not.
The host model of the same cases is in tests/test_knn_cases_host.py; what the kernels of the
commit before the screen's domain gave on these cases is in profiles/r16/knn_ops/README.md.
"""
import warnings

import numpy as np
import pytest
import torch

import knn_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from mepol_amd import ops as gpu_ops

    return gpu_ops


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    monkeypatch.delenv("MEPOL_KNN_NH", raising=False)
    monkeypatch.delenv("MEPOL_KNN_SEED", raising=False)


def _run(ops, cuda, c, defer=False):
    X = torch.as_tensor(c.X, device=cuda)
    Q = None if c.Q is None else torch.as_tensor(c.Q, device=cuda)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no case here has an overflowing squared norm
        out = ops.knn(X, c.kp1, query=Q, split=c.split, return_fallback=True, defer_check=defer)
        if defer:
            out[4].raise_if_invalid()
    torch.cuda.synchronize()
    D, I, I32T, nfb = out[:4]
    return D.cpu().numpy(), I.cpu().numpy(), I32T.cpu().numpy(), int(nfb.item())


def _wrong_rows(D, I, Do, Io):
    return int(((D.view(np.int64) != Do.view(np.int64)) | (I != Io)).any(axis=1).sum())


def check_case(ops, cuda, c, Do, Io):
    """The assertions every case makes; returns n_fallback of the synchronous run."""
    nq = len(c.queries)
    first = None
    for defer in (False, True, False):
        D, I, I32T, nfb = _run(ops, cuda, c, defer)
        print(f"{c.family}/{c.name} defer={defer}: wrong rows {_wrong_rows(D, I, Do, Io)} of {nq}, "
              f"n_fallback {nfb}")
        assert D.shape == Do.shape and np.array_equal(D.view(np.int64), Do.view(np.int64))
        assert np.array_equal(I, Io)
        assert np.array_equal(I32T.T, I)
        assert 0 <= nfb <= nq
        first = nfb if first is None else first
    return first


@pytest.mark.parametrize("family,name", K.case_ids())
def test_case(cuda, ops, family, name):
    c = K.get_case(family, name)
    if family == "plans":
        got = ops.knn_plan(len(c.X), len(c.Q), c.X.shape[1], c.kp1, c.split)
        assert got["mode"] == "screened"
        assert all(got[k] == c.claim[k] for k in ("KS16", "nh", "LIST16", "split")), (got, c.claim)
    Do, Io = K.oracle(family, name)
    nfb = check_case(ops, cuda, c, Do, Io)
    # the screen runs exactly where its domain says (knn_cases.off_domain); how many queries it
    # then certifies is not asserted
    if K.routed(c):
        assert nfb == len(c.queries)
    elif family in ("scale", "plans"):
        assert nfb < len(c.queries)


@pytest.mark.parametrize("base", list(K.SCALE_BASES))
def test_scale_is_the_unscaled_run_scaled(cuda, ops, base):
    """The kernels' own unscaled result, times 2^e: the same I, and D bit for bit wherever the
    product is a normal f64 (everywhere, at these sizes)."""
    D0, I0, _, _ = _run(ops, cuda, K.scale_base_case(base))
    for name in K.SCALE_NAMES:
        c = K.get_case("scale", name)
        if name[0] != base or c.base is None:
            continue
        D, I, _, _ = _run(ops, cuda, c)
        want = np.ldexp(D0, c.exp)
        normal = (want == 0) | (np.abs(want) >= np.finfo(np.float64).tiny)
        assert normal.all()
        assert np.array_equal(I, I0), name
        assert np.array_equal(D.view(np.int64), want.view(np.int64)), name


def test_plan_sweep_has_no_untested_plan(ops):
    found = K.sweep_triples(ops.knn_plan)
    visited = {(c["KS16"], c["nh"], c["LIST16"]) for *_, c in K.plan_specs().values()}
    assert visited == set(found), sorted(set(found) - visited)
    assert {c["MAXP"] for *_, c in K.plan_specs().values()} == set(K.REFINE_MAXP)


def _smallest_plan_case(nh):
    names = [n for n in K.PLAN_NAMES if K.plan_specs()[n][4]["nh"] == nh]
    return min(names, key=lambda n: (K.plan_specs()[n][0] * K.plan_specs()[n][1], K.plan_specs()[n][2]))


@pytest.mark.parametrize("nh", [1, 2])
@pytest.mark.parametrize("seed", ["0", "1", "2"])
def test_plans_seed_invariance(cuda, ops, monkeypatch, nh, seed):
    name = _smallest_plan_case(nh)
    c = K.get_case("plans", name)
    Do, Io = K.oracle("plans", name)
    monkeypatch.setenv("MEPOL_KNN_SEED", seed)
    D, I, I32T, nfb = _run(ops, cuda, c)
    assert np.array_equal(D.view(np.int64), Do.view(np.int64)) and np.array_equal(I, Io)
    assert np.array_equal(I32T.T, I) and 0 <= nfb <= len(c.Q)
