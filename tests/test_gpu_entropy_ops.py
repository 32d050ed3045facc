"""The IW / entropy / CSR / gradient kernels op by op against 80-bit references, ragged included.

Every case of tests/entropy_cases.py goes through mepol_amd.ops (csrc/entropy.hip, csrc/csr.hip)
with the same checkers that tests/test_entropy_cases_host.py applies to the CPU stand-ins: each
output within m u0 A of the np.longdouble reference (the derivations are in entropy_cases.py),
integer lists equal to cpu_ops.csr_build.  The shapes are the smallest that reach each branch:
the 64-lane chunking of the scans, the last partial block of four trajectories, zero lengths,
block_reduce_array's 8-way path (>= 2047 values), gamma_kernel's grid-stride loop (> 32768
owned particles; 40002 leaves a wave whose lane groups differ in trip count), hub segments of
64 m + r entries, empty segments, and the sharded arguments of parallel.py.
"""
import types

import numpy as np
import pytest
import torch

import entropy_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from mepol_amd import ops as gpu_ops

    return gpu_ops


# ---------------------------------------------------------------------------------------------
# op by op
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.iw_cases()))
def test_iw_scan_and_normalise(cuda, ops, name):
    c = E.iw_cases()[name]
    a = E.run_iw(ops, cuda, c)
    b = E.run_iw(ops, cuda, c)
    # the scan does not depend on `normalize`, and nothing depends on the run
    assert E.bits_equal(a["u"], a["u2"]) and E.bits_equal(a["ts"], a["ts2"])
    for key in a:
        assert E.bits_equal(a[key], b[key]), key


@pytest.mark.parametrize("name", list(E.entropy_cases()))
def test_entropy_forward(cuda, ops, name):
    c = E.entropy_cases()[name]
    a = E.run_entropy(ops, cuda, c)
    b = E.run_entropy(ops, cuda, c)
    for key in a:
        assert E.bits_equal(a[key], b[key]), key


def test_entropy_forward_emit_twice(cuda, ops):
    c = E.entropy_cases()
    a = E.run_entropy_emit(ops, cuda, c["ns7_eps1e-15"], c["ns2_eps0"])
    b = E.run_entropy_emit(ops, cuda, c["ns7_eps1e-15"], c["ns2_eps0"])
    for (va, xa), (vb, xb) in zip(a, b):
        assert E.bits_equal(va, vb) and E.bits_equal(xa, xb)


@pytest.mark.parametrize("name", list(E.table_cases()))
def test_csr_build(cuda, ops, name):
    c = E.table_cases()[name]
    (off_a, rows_a), = E.run_csr(ops, cuda, c)
    (off_b, rows_b), = E.run_csr(ops, cuda, c)
    ne = int(off_a[-1])
    assert E.bits_equal(off_a, off_b) and E.bits_equal(rows_a[:ne], rows_b[:ne])


@pytest.mark.parametrize("name,world", E.CSR_SHARDED)
def test_csr_build_rank_slices(cuda, ops, name, world):
    E.run_csr(ops, cuda, E.table_cases()[name], world)


@pytest.mark.parametrize("name", list(E.gamma_cases()))
def test_gamma(cuda, ops, name):
    c = E.gamma_cases()[name]
    a = E.run_gamma(ops, cuda, c, ops.entropy_gamma_nparts)
    b = E.run_gamma(ops, cuda, c, ops.entropy_gamma_nparts)
    n = a["nparts"]
    assert E.bits_equal(a["gamma"], b["gamma"])
    assert E.bits_equal(a["partials"][:n], b["partials"][:n])


def test_gamma_on_the_device_csr(cuda, ops):
    """entropy_gamma over csr_build's own output (the product's pairing), and its 2048
    partials through the reverse scan: S = sum(partials) on the 8-way path."""
    t = E.table_cases()["n40002_k2"]
    c = E.gamma_cases()["n40002_k2"]
    ref = E.gamma_reference("n40002_k2")
    off, rows = ops.csr_build(E._t(t.idxT, cuda), t.k, t.n_ids)
    gamma, partials, nparts = ops.entropy_gamma(E._t(c.g, cuda), E._t(c.w, cuda), off, rows)
    assert nparts == 2048
    E.check("gamma", E._n(gamma), ref.gamma, ref.bgamma)
    lens = [int(x) for x in np.random.default_rng(40002).integers(0, 401, 199)]
    while sum(lens) > 40002 - 1:
        lens[int(np.argmax(lens))] //= 2
    lens.append(40002 - sum(lens))
    T = max(lens) + 3
    offsets = E.offsets_of(lens)
    gH = E._t(np.float64(-1.0), cuda)
    grad = E.gpu_reverse_scan_nan_filled(gamma, E._t(c.w, cuda), partials, nparts,
                                         E._t(offsets, cuda), len(lens), T, gH)
    rv = E.reverse_ref(ref.gamma, c.w, ref.S, offsets, T, -1.0, dgamma=ref.bgamma, dS=ref.bS)
    E.check("grad_logp", E._n(grad), rv.grad, rv.bgrad)


@pytest.mark.parametrize("gH", E.GRAD_HS)
@pytest.mark.parametrize("name", list(E.reverse_cases()))
def test_reverse_scan(cuda, ops, name, gH):
    c = E.reverse_cases()[name]
    a = E.run_reverse(ops, cuda, c, gH, E.gpu_reverse_scan_nan_filled)
    b = E.run_reverse(ops, cuda, c, gH, E.gpu_reverse_scan_nan_filled)
    assert E.bits_equal(a, b)
    # ops.entropy_reverse_scan itself (an uninitialised buffer): the same bits
    assert E.bits_equal(a, E.run_reverse(ops, cuda, c, gH))


@pytest.mark.parametrize("world,n,nt", E.GATHER_SHAPES)
def test_gathered_normalise_and_sharded_emit(cuda, ops, world, n, nt):
    c = E.gather_case(world, n, nt)
    assert E.bits_equal(E.run_gathered(ops, cuda, c), E.run_gathered(ops, cuda, c))
    a, b = E.run_emit(ops, cuda, c), E.run_emit(ops, cuda, c)
    for (va, sa), (vb, sb) in zip(a, b):
        assert E.bits_equal(va, vb) and E.bits_equal(sa, sb)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_sliced_round_trip(cuda, ops, world):
    assert E.bits_equal(E.run_chain(ops, cuda, world), E.run_chain(ops, cuda, world))


def test_ragged_chain_feeds_the_reverse_scan(cuda, ops):
    """The ragged length set end to end on one rank: the reverse scan over the gamma of
    weights that span e^+-30."""
    E.run_chain(ops, cuda, 1, 0.37, "ragged_drift")


def test_bad_arguments_are_refused_on_the_host(cuda, ops):
    """The four entry points that validate on the host return MEPOL_ERR_BAD_ARG (no launch)."""
    from mepol_amd._lib import MepolInputError, call, ptr

    x = torch.ones(16, dtype=torch.float64, device=cuda)
    i32 = torch.zeros(16, dtype=torch.int32, device=cuda)
    off = torch.zeros(2, dtype=torch.int64, device=cuda)
    st = ops._stream()
    with pytest.raises(MepolInputError):
        call("mepol_iw_forward", ptr(x), ptr(x), 0, 4, ptr(off), 0, ptr(x), ptr(x), None, None, st)
    with pytest.raises(MepolInputError):  # kp1 <= k
        call("mepol_entropy_forward", ptr(x), ptr(i32), ptr(x), 2, 2, 3, 3, 2.0, 1.0, 0.0, 0.0,
             ptr(x), ptr(x), ptr(x), ptr(x), st)
    with pytest.raises(MepolInputError):  # world = 0
        call("mepol_iw_normalize_gathered", ptr(x), 0, 4, 2, ptr(x), st)
    with pytest.raises(MepolInputError):  # off + 1 >= stride
        call("mepol_sharded_emit", ptr(x), 2, 8, 7, 0.0, 8, ptr(x), ptr(x), st)
    torch.cuda.synchronize()
    assert bool((x == 1).all())


# ---------------------------------------------------------------------------------------------
# ragged lengths through the drop-in functions (the eager path: the graph loop declines them)
# ---------------------------------------------------------------------------------------------
RTOL, GRAD_RTOL = 1e-9, 1e-8  # tests/test_gpu_entropy.py's


def _close(got, ref, rtol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.all(np.isfinite(ref)) and got.shape == ref.shape
    scale = max(np.abs(ref).max(), 1e-300)
    assert np.abs(got - ref).max() <= rtol * scale, (np.abs(got - ref).max(), scale)


@pytest.fixture(scope="module")
def ragged_batch(cuda):
    """6 trajectories of T = 120 with lengths [120, 1, 64, 97, 0, 120]: d = 2 states, the next
    states of the real particles only, their k-NN from ops.knn, a [32, 32] policy pair, and the
    oracle's f64 CPU values over the same tensors."""
    from mepol_amd import ops as gpu_ops
    from mepol_amd.policy import GaussianPolicy
    from oracle import mepol_oracle as O

    lens, T, nf, a, k = [120, 1, 64, 97, 0, 120], 120, 2, 2, 4
    nt = len(lens)
    rng = np.random.default_rng(1200)
    states = rng.standard_normal((nt, T + 1, nf)).astype(np.float32)
    actions = (0.5 * rng.standard_normal((nt, T, a))).astype(np.float32)
    nxt = np.concatenate([states[n, 1:L + 1] for n, L in enumerate(lens)], axis=0)
    torch.manual_seed(1200)
    beh = GaussianPolicy([32, 32], nf, a)
    tgt = GaussianPolicy([32, 32], nf, a)
    tgt.load_state_dict(beh.state_dict())
    with torch.no_grad():
        for p in tgt.parameters():
            p.add_(0.02 * torch.randn_like(p))
    sd_b = {n: v.detach().clone() for n, v in beh.state_dict().items()}
    sd_t = {n: v.detach().clone() for n, v in tgt.state_dict().items()}
    D, I, _ = gpu_ops.knn(torch.as_tensor(nxt, device=cuda), k + 1)
    G, B, eps = float(np.pi), 0.25, 1e-15  # ns = 2: Gamma(2) pi = pi; B any constant
    st = torch.as_tensor(states, dtype=torch.float64)
    ac = torch.as_tensor(actions, dtype=torch.float64)
    rtl = torch.as_tensor(lens, dtype=torch.int64).reshape(nt, 1)

    def cpu_policy(sd):
        p = O.TorchPolicy([32, 32], nf, a)
        p.load_state_dict(sd)
        return p

    rb, rt = cpu_policy(sd_b), cpu_policy(sd_t)
    Dc, Ic = D.cpu(), I.cpu()
    args = (rb, rt, st, ac, nt, lens)
    with torch.no_grad():
        w = O.torch_iw(*args)
        kl, kerr = O.torch_kl(*args, Ic, k, eps)
    H = O.torch_entropy(*args, Dc, Ic, k, G, B, nf, eps)
    H.backward()
    gradH = {n: p.grad.clone() for n, p in rt.named_parameters()}
    opt = torch.optim.Adam(rt.parameters(), lr=1e-3)
    loss, nerr = O.torch_policy_update(opt, *args, Dc, Ic, k, G, B, nf, eps)
    ref = types.SimpleNamespace(
        w=w.numpy(), kl=float(kl), kerr=kerr, H=float(H.detach()), gradH=gradH,
        loss=float(loss.detach()),
        nerr=nerr, step_grad={n: p.grad.clone() for n, p in rt.named_parameters()},
        stepped={n: p.detach().clone() for n, p in rt.named_parameters()})
    return types.SimpleNamespace(lens=lens, T=T, nt=nt, k=k, G=G, B=B, eps=eps, ns=nf,
                                 beh=beh.to(cuda), tgt=tgt.to(cuda), st=st.to(cuda),
                                 ac=ac.to(cuda), rtl=rtl.to(cuda), D=D, I=I, ref=ref)


def test_ragged_batch_through_the_drop_in_functions(cuda, ragged_batch):
    from mepol_amd.algorithms import device_loop
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.algorithms import particles as P

    b, ref = ragged_batch, ragged_batch.ref
    assert not ref.kerr and not ref.nerr
    common = (b.beh, b.tgt, b.st, b.ac, b.nt, b.rtl)
    with torch.no_grad():
        w = M.compute_importance_weights(*common)
    assert w.shape == (sum(b.lens),)
    _close(w.cpu().numpy(), ref.w, RTOL)
    kl, kerr = M.compute_kl(*common, b.D, b.I, b.k, b.eps)
    assert not kerr
    _close(kl.item(), ref.kl, RTOL)
    b.tgt.zero_grad()
    H = M.compute_entropy(*common, b.D, b.I, b.k, b.G, b.B, b.ns, b.eps)
    _close(H.item(), ref.H, RTOL)
    H.backward()
    for n, p in b.tgt.named_parameters():
        _close(p.grad.cpu().numpy(), ref.gradH[n].numpy(), GRAD_RTOL)
    opt = torch.optim.Adam(b.tgt.parameters(), lr=1e-3)
    batch = P.lookup(b.st, b.ac, b.rtl, b.D, b.I)
    assert batch.dense is False and batch.N == sum(b.lens)
    assert device_loop.supported(batch, b.beh, b.tgt, opt) is False
    loss, nerr = M.policy_update(opt, *common, b.D, b.I, b.k, b.G, b.B, b.ns, b.eps)
    assert not nerr
    _close(loss.item(), ref.loss, RTOL)
    for n, p in b.tgt.named_parameters():
        _close(p.grad.cpu().numpy(), ref.step_grad[n].numpy(), GRAD_RTOL)
        _close(p.detach().cpu().numpy(), ref.stepped[n].numpy(), GRAD_RTOL)
