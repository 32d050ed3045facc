"""The register-fed form of dh1_layer1_backward (dh1_direct_kernel) on the GPU.

Every case of tests/dh1_direct_cases.py first asserts, through mepol_dh1_layer1_plan_info, the
kernel it runs, then runs the mask= and w2= forms twice each: equal bits on both calls and
between the forms, every output within the m u0 A bound of the np.longdouble reference, and the
bits of the f64-h1 form, which runs the LDS kernel as before this kernel existed.  The small
shapes name the register-fed kernel (form="direct"); F = 32 is NH = 3, where it does not exist,
and runs the LDS kernel; the case with 265 tiles leaves the choice to the library and must get
the register-fed kernel; every small shape left to the library gets the LDS kernel, run again
with its bits compared.
"""
import pytest

import dh1_direct_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from mepol_amd import ops as gpu_ops

    return gpu_ops


def _plan(ops, form):
    return lambda n, K, M, F, w2: ops.dh1_layer1_plan(n, K, M, F, mask=True, w2=w2, form=form)


@pytest.mark.parametrize("name", list(D.cases()))
def test_case(cuda, ops, name):
    from mepol_amd._lib import MepolError

    c = D.cases()[name]
    if name == "auto_many_tiles":
        assert D.direct_auto(c.n, c.K, c.M, c.F)
        D.run(ops, cuda, c, plan=_plan(ops, "auto"), form="auto", want="direct",
              lds_reference=True)
    elif D.direct_fits(c.K, c.M, c.F):
        got = D.run(ops, cuda, c, plan=_plan(ops, "direct"), form="direct", want="direct",
                    lds_reference=True)
        assert not D.direct_auto(c.n, c.K, c.M, c.F)
        auto = D.run(ops, cuda, c, plan=_plan(ops, "auto"), form="auto", want="lds")
        for f in ("mask", "w2"):
            assert D.bits_equal(got[f][0], auto[f][0]) and D.bits_equal(got[f][1], auto[f][1])
    else:  # the one case built not to use it
        assert name == "F32"
        with pytest.raises(MepolError):
            ops.dh1_layer1_plan(c.n, c.K, c.M, c.F, mask=True, w2=True, form="direct")
        D.run(ops, cuda, c, plan=_plan(ops, "auto"), form="auto", want="lds", lds_reference=True)


def test_odd_hidden0_keeps_the_lds_kernel(cuda, ops):
    """hidden0 = 81: the mask= form exists (w2= needs an even hidden0), runs the LDS kernel and
    gives the f64-h1 form's bits; asking for the register-fed kernel is refused."""
    import torch
    from mepol_amd._lib import MepolError

    c = D.case("M81", 65, 18, 81, 5, 15999)
    assert ops.dh1_layer1_plan(c.n, c.K, c.M, c.F, mask=True)["form"] == "lds"
    dz2, W2t, h1, x = [D._t(v, cuda) for v in (c.dz2, c.W2t, c.h1, c.x)]
    mask = D._t(D.G._pack_mask(c.h1 > 0), cuda)
    dW, db = ops.dh1_layer1_backward(dz2, W2t, h1, x)
    dWm, dbm = ops.dh1_layer1_backward(dz2, W2t, h1, x, mask=mask)
    assert torch.equal(dW, dWm) and torch.equal(db, dbm)
    ref = D.G.dh1_ref(c.dz2, c.W2t, D.G._gt0(D.G.ld(c.h1)), c.x)
    D.check("dh1d_dW1_odd", D._n(dWm), ref.dW, ref.bdW)
    D.check("dh1d_db1_odd", D._n(dbm), ref.db, ref.bdb)
    out = torch.full((c.M, c.F), -7.25, dtype=torch.float64, device=cuda)
    with pytest.raises(MepolError):
        ops.dh1_layer1_backward(dz2, W2t, h1, x, mask=mask, dW_out=out, form="direct")
    assert bool((out == -7.25).all()), "a refused call wrote its output"
