"""TRPO policy step on the HIP kernels: the four Fisher-vector-product entry points against the
torch expression of their formulas, PolicyFisher.hvp / conj_gradient / trpo_step against the
reference's method (tests/trpo_reference.py, torch f64 on the CPU), and the dispatch."""
import functools

import pytest
import torch
import torch.nn as nn

import trpo_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-10  # per tensor: max |dev - ref| <= TOL * max |ref| (the project's forward tolerance)
ROWS = [500, 517, 2049]  # the floor; not a multiple of 16 or 64; several row blocks and a tail


@pytest.fixture(autouse=True)
def _floor_500(monkeypatch):
    """The kernel-path tests run at the smallest batch the kernels serve, whatever
    FVP_MIN_ROWS a measurement settled on (test_default_floor checks the default itself)."""
    monkeypatch.setenv("MEPOL_FVP_MIN_ROWS", "500")


def _gen(seed):
    return dict(dtype=torch.float64, device="cuda",
                generator=torch.Generator(device="cuda").manual_seed(seed))


def _close(name, got, want):
    err = (got - want).abs().max().item()
    bound = TOL * max(want.abs().max().item(), 1e-300)
    print(f"{name}: max err {err:.3e} (bound {bound:.3e})")
    assert got.shape == want.shape and err <= bound, name


# ---- per-kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("f,o", [(2, 300), (5, 18), (29, 400)])
def test_layer_tangent(cuda, n, f, o):
    from mepol_amd import ops

    kw = _gen(n + f)
    x, W, b = torch.randn(n, f, **kw), torch.randn(o, f, **kw), torch.randn(o, **kw)
    dW, db = torch.randn(o, f, **kw), torch.randn(o, **kw)
    h = ops.layer_forward(x, W, b)
    out = torch.full((n, o), float("nan"), dtype=torch.float64, device="cuda")
    t = ops.layer_tangent(x, dW, db, h, out=out)
    assert t is out
    _close("layer_tangent", t, (x @ dW.t() + db) * (h > 0))


@pytest.mark.parametrize("variant", [0, 2], ids=["tile128", "tile64"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("k,m", [(300, 300), (400, 300), (34, 18)])
def test_hidden_tangent(cuda, n, k, m, variant):
    from mepol_amd import ops

    kw = _gen(n + k + variant)
    t_in, h_in = torch.randn(n, k, **kw), torch.relu(torch.randn(n, k, **kw))
    W, dW = torch.randn(m, k, **kw) / k ** 0.5, torch.randn(m, k, **kw) / k ** 0.5
    b, db = torch.randn(m, **kw), torch.randn(m, **kw)
    z = h_in @ W.t()  # pre-bias
    lin = t_in @ W.t() + h_in @ dW.t() + db
    # last layer: the mask from the pre-bias z and the bias
    got = ops.hidden_tangent(t_in, h_in, W, dW, db, z, b, variant=variant)
    _close("hidden_tangent z + b", got, lin * (z + b > 0))
    # inner layer: the mask from the ReLU output, null bias; into a caller's buffer
    h_out = torch.relu(z + b)
    out = torch.full((n, m), float("nan"), dtype=torch.float64, device="cuda")
    got = ops.hidden_tangent(t_in, h_in, W, dW, db, h_out, None, out=out, variant=variant)
    assert got is out
    _close("hidden_tangent h", got, lin * (h_out > 0))
    assert torch.equal(got, ops.hidden_tangent(t_in, h_in, W, dW, db, h_out, variant=variant))


@pytest.mark.parametrize("variant", [1, 3, 5, 6, 7, 8, 9, 10])
def test_hidden_tangent_tuning_tilings(cuda, variant):
    """mepol_gemm_nt's other tilings give the same product (ragged rows, k-tiles and columns)."""
    from mepol_amd import ops

    n, k, m = 517, 134, 178
    kw = _gen(variant)
    t_in, h_in = torch.randn(n, k, **kw), torch.relu(torch.randn(n, k, **kw))
    W, dW = torch.randn(m, k, **kw) / k ** 0.5, torch.randn(m, k, **kw) / k ** 0.5
    b, db = torch.randn(m, **kw), torch.randn(m, **kw)
    z = h_in @ W.t()
    got = ops.hidden_tangent(t_in, h_in, W, dW, db, z, b, variant=variant)
    _close(f"hidden_tangent variant {variant}", got,
           (t_in @ W.t() + h_in @ dW.t() + db) * (z + b > 0))


MEAN_SHAPES = [(500, 300, 2), (517, 300, 3), (2049, 300, 8), (517, 18, 2), (500, 18, 3),
               (517, 34, 8), (517, 300, 1), (517, 300, 20), (517, 512, 32)]


@pytest.mark.parametrize("n,h,a", MEAN_SHAPES)
def test_mean_tangent(cuda, n, h, a):
    from mepol_amd import ops

    kw = _gen(n + h + a)
    t, z, bz = torch.randn(n, h, **kw), torch.randn(n, h, **kw), torch.randn(h, **kw)
    Wm, dWm = torch.randn(a, h, **kw), torch.randn(a, h, **kw)
    dbm, scale = torch.randn(a, **kw), torch.rand(a, **kw) + 0.5
    c = ops.mean_tangent(t, z, Wm, dWm, dbm, scale, bz=bz)
    _close("mean_tangent", c, scale * (t @ Wm.t() + torch.relu(z + bz) @ dWm.t() + dbm))
    c0 = ops.mean_tangent(t, z, Wm, dWm, dbm, scale)  # null bias
    _close("mean_tangent, no bias", c0, scale * (t @ Wm.t() + torch.relu(z) @ dWm.t() + dbm))


@pytest.mark.parametrize("n,h,a", MEAN_SHAPES)
def test_mean_backward(cuda, n, h, a):
    from mepol_amd import ops

    kw = _gen(n + h + a + 1)
    c, z, bz = torch.randn(n, a, **kw), torch.randn(n, h, **kw), torch.randn(h, **kw)
    Wm = torch.randn(a, h, **kw)
    dz, dWm, dbm, dbz = ops.mean_backward(c, z, Wm, bz=bz)
    ref_dz = (c @ Wm) * (z + bz > 0)
    _close("dz", dz, ref_dz)
    _close("dWm", dWm, c.t() @ torch.relu(z + bz))
    _close("dbm", dbm, c.sum(0))
    _close("dbz", dbz, ref_dz.sum(0))
    # the same bits on a second call, with a caller-owned workspace and buffers
    ws = ops.mean_backward_workspace(n, h, a, c.device)
    outs = tuple(torch.full_like(t, float("nan")) for t in (dWm, dbm, dbz))
    dz2, *rest = ops.mean_backward(c, z, Wm, bz=bz, ws=ws, dz_out=torch.full_like(z, float("nan")),
                                   outs=outs)
    for p, q in zip((dz, dWm, dbm, dbz), (dz2, *rest)):
        assert torch.equal(p, q)
    # null dz; null bz and dbz
    none_dz, dWm3, dbm3, dbz3 = ops.mean_backward(c, z, Wm, bz=bz, need_dz=False)
    assert none_dz is None and torch.equal(dWm3, dWm) and torch.equal(dbz3, dbz)
    dz4, dWm4, dbm4, dbz4 = ops.mean_backward(c, z, Wm)
    assert dbz4 is None and torch.equal(dbm4, dbm)
    _close("dz, no bias", dz4, (c @ Wm) * (z > 0))
    _close("dWm, no bias", dWm4, c.t() @ torch.relu(z))


def test_bad_arguments_are_rejected_before_any_launch(cuda):
    from mepol_amd import _lib, ops

    kw = _gen(0)
    n, k, m = 64, 34, 18
    t_in, h_in = torch.randn(n, k, **kw), torch.randn(n, k, **kw)
    W, dW, db = torch.randn(m, k, **kw), torch.randn(m, k, **kw), torch.randn(m, **kw)
    mask = torch.randn(n, m, **kw)
    with pytest.raises(_lib.MepolInputError):  # unknown tiling
        ops.hidden_tangent(t_in, h_in, W, dW, db, mask, variant=4)
    flat = torch.randn(m * k + 1, **kw)
    with pytest.raises(_lib.MepolInputError):  # dW 8 bytes off a 16-byte boundary
        ops.hidden_tangent(t_in, h_in, W, flat[1:].view(m, k), db, mask)
    with pytest.raises(_lib.MepolError):  # hidden > 512: MEPOL_ERR_UNSUPPORTED
        ops.mean_tangent(torch.randn(8, 514, **kw), torch.randn(8, 514, **kw),
                         torch.randn(2, 514, **kw), torch.randn(2, 514, **kw),
                         torch.randn(2, **kw), torch.randn(2, **kw))
    c, z, Wm = torch.randn(n, 2, **kw), torch.randn(n, m, **kw), torch.randn(2, m, **kw)
    ws = ops.mean_backward_workspace(n, m, 2, c.device)
    with pytest.raises(_lib.MepolError, match="workspace"):
        ops.mean_backward(c, z, Wm, ws=ws[:-1])
    # n = 0: success, nothing launched or written
    import ctypes

    from mepol_amd._lib import ptr

    out = torch.full((n, m), 7.0, dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call("mepol_hidden_tangent", ptr(t_in), ptr(h_in), 0, k, ptr(W), ptr(dW), ptr(db), m,
              ptr(mask), None, ptr(out), 0, st)
    _lib.call("mepol_layer_tangent", ptr(t_in), 0, k, ptr(dW), ptr(db), m, ptr(mask), ptr(out), st)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_mask_edge_relu_prime_of_zero_is_zero(cuda):
    """A pre-activation of exactly 0 is masked (torch's relu'(0) = 0): an all-zero state row with
    zero biases gives t = 0 in every layer and delta mu = V_bm for that row, and a mask_src +
    mask_bias that cancels to exactly 0.0 in chosen positions is masked there."""
    from mepol_amd import ops

    kw = _gen(5)
    n, f, h0, h1, a = 517, 2, 34, 18, 3
    x = torch.randn(n, f, **kw)
    x[7] = 0.0
    W1, W2, Wm = torch.randn(h0, f, **kw), torch.randn(h1, h0, **kw), torch.randn(a, h1, **kw)
    b1 = torch.zeros(h0, dtype=torch.float64, device="cuda")
    b2 = torch.zeros(h1, dtype=torch.float64, device="cuda")
    V1, Vb1 = torch.randn(h0, f, **kw), torch.randn(h0, **kw)
    V2, Vb2 = torch.randn(h1, h0, **kw), torch.randn(h1, **kw)
    Vm, Vbm = torch.randn(a, h1, **kw), torch.randn(a, **kw)
    hid1 = ops.layer_forward(x, W1, b1)
    z2 = ops.gemm_nt(hid1, W2, variant=2)
    assert bool((hid1[7] == 0).all()) and bool((z2[7] == 0).all())
    t1 = ops.layer_tangent(x, V1, Vb1, hid1)
    t2 = ops.hidden_tangent(t1, hid1, W2, V2, Vb2, z2, b2, variant=2)
    assert bool((t1[7] == 0).all()) and bool((t2[7] == 0).all())
    scale = torch.ones(a, dtype=torch.float64, device="cuda")
    c = ops.mean_tangent(t2, z2, Wm, Vm, Vbm, scale, bz=b2)
    assert torch.equal(c[7], Vbm)
    _close("t2", t2, (t1 @ W2.t() + hid1 @ V2.t() + Vb2) * (z2 + b2 > 0))
    # z + b == 0.0 exactly where b = -z: masked there, and only there
    zz, bb = torch.randn(n, h1, **kw), torch.randn(h1, **kw)
    rows = torch.arange(0, n, 5, device="cuda")
    cols = rows % h1
    zz[rows, cols] = -bb[cols]
    got = ops.hidden_tangent(t1, hid1, W2, V2, Vb2, zz, bb, variant=0)
    lin = t1 @ W2.t() + hid1 @ V2.t() + Vb2
    assert bool((got[rows, cols] == 0).all())
    _close("cancelled mask", got, lin * (zz + bb > 0))
    dz, _, _, _ = ops.mean_backward(c, zz, Wm, bz=bb)
    assert bool((dz[rows, cols] == 0).all())


# ---- PolicyFisher ----------------------------------------------------------------------------
POLICIES = {"300x300": (2, [300, 300], 2), "400x300": (29, [400, 300], 8),
            "34x18": (5, [34, 18], 3), "64x48x32": (2, [64, 48, 32], 2)}
N = 517


@functools.lru_cache(maxsize=None)
def _case(name, activation=nn.ReLU):
    """(reference policy, states, actions, advantages) on the CPU, built once per policy."""
    nf, hidden, a = POLICIES.get(name) or EXTRA[name]
    act = torch.tanh if activation is nn.Tanh else torch.relu
    ref = R.RefPolicy.random(nf, hidden, a, seed=11, act=act)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(N, nf, generator=g, dtype=torch.float64)
    noise = torch.randn(N, a, generator=g, dtype=torch.float64)
    actions = (ref.mean(x) + noise * torch.exp(ref.log_std)).detach()
    adv = noise[:, 0] - 0.5 * noise[:, -1] + 0.25 * noise[:, 0] * noise[:, -1]
    return ref, x, actions, adv


EXTRA = {"tanh": (2, [64, 48], 2), "64x47": (2, [64, 47], 2), "64x48": (2, [64, 48], 2)}


@functools.lru_cache(maxsize=None)
def _ref_hvp(name, activation=nn.ReLU):
    ref, x, _, _ = _case(name, activation)
    v = torch.randn(ref.flat().numel(), generator=torch.Generator().manual_seed(13),
                    dtype=torch.float64)
    return v, R.make_hvp(ref, x, 0.1)(v).detach()


def _gpu_policy(name, activation=nn.ReLU):
    from mepol_amd.policy import GaussianPolicy

    nf, hidden, a = POLICIES.get(name) or EXTRA[name]
    ref = _case(name, activation)[0]
    p = GaussianPolicy(hidden, nf, a, activation=activation)
    ref.load_into(p)
    return p.to("cuda")


def _count_calls(monkeypatch, ops, name):
    calls = []
    real = getattr(ops, name)

    def counted(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.mark.parametrize("name", list(POLICIES))
def test_hvp_matches_reference(cuda, monkeypatch, name):
    from mepol_amd.algorithms import trpo

    ref, x, _, _ = _case(name)
    v, want = _ref_hvp(name)
    policy = _gpu_policy(name)
    xs = x.cuda()
    fisher = trpo.PolicyFisher(policy, xs, 0.1)
    assert fisher.kernels
    got = fisher.hvp(v.cuda())
    err = R.per_tensor_rel(ref.params(), got.cpu(), want)
    print(f"hvp {name}: kernels vs reference {err:.2e}")
    assert err <= TOL
    assert torch.equal(got, fisher.hvp(v.cuda()))  # the same bits
    monkeypatch.setenv("MEPOL_FVP_MIN_ROWS", str(N + 1))
    forced = trpo.PolicyFisher(policy, xs, 0.1)
    assert not forced.kernels
    err_fb = R.per_tensor_rel(ref.params(), got.cpu(), forced.hvp(v.cuda()).cpu())
    print(f"hvp {name}: kernels vs forced fallback {err_fb:.2e}")
    assert err_fb <= TOL


@pytest.mark.parametrize("name,activation,rows", [("tanh", nn.Tanh, N), ("64x47", nn.ReLU, N),
                                                  ("64x48", nn.ReLU, 499)])
def test_dispatch_fallback(cuda, monkeypatch, name, activation, rows):
    from mepol_amd import ops
    from mepol_amd.algorithms import trpo

    ref, x, _, _ = _case(name, activation)
    x = x[:rows]
    v = _ref_hvp(name, activation)[0]
    want = R.make_hvp(ref, x, 0.1)(v).detach()
    calls = _count_calls(monkeypatch, ops, "hidden_tangent")
    fisher = trpo.PolicyFisher(_gpu_policy(name, activation), x.cuda(), 0.1)
    got = fisher.hvp(v.cuda())
    assert not fisher.kernels and not calls
    assert R.per_tensor_rel(ref.params(), got.cpu(), want) <= TOL


def test_dispatch_kernels_at_the_floor(cuda, monkeypatch):
    from mepol_amd import ops
    from mepol_amd.algorithms import trpo

    ref, x, _, _ = _case("64x48")
    x = x[:500]
    v = _ref_hvp("64x48")[0]
    want = R.make_hvp(ref, x, 0.1)(v).detach()
    calls = _count_calls(monkeypatch, ops, "hidden_tangent")
    fisher = trpo.PolicyFisher(_gpu_policy("64x48"), x.cuda(), 0.1)
    got = fisher.hvp(v.cuda())
    assert fisher.kernels and len(calls) == 1
    assert R.per_tensor_rel(ref.params(), got.cpu(), want) <= TOL


def test_default_floor(cuda, monkeypatch):
    """Without the override the floor is FVP_MIN_ROWS: one row under it takes the fallback."""
    from mepol_amd.algorithms import trpo

    monkeypatch.delenv("MEPOL_FVP_MIN_ROWS")
    floor = trpo.FVP_MIN_ROWS
    assert trpo.fvp_min_rows() == floor
    policy = _gpu_policy("64x48")
    x = torch.randn(floor, 2, **_gen(1))
    assert trpo.fvp_kernels_ok(policy, x) and not trpo.fvp_kernels_ok(policy, x[:floor - 1])


# ---- conjugate gradient and the whole step ----------------------------------------------------
def _gain_grad(ref, x, actions, adv):
    old = ref.log_p(x, actions).detach()
    gain = torch.mean(torch.exp(ref.log_p(x, actions) - old) * adv)
    return torch.cat([t.reshape(-1) for t in torch.autograd.grad(gain, ref.params())])


@functools.lru_cache(maxsize=None)
def _ref_cg(name):
    """(g, the reference's x, its noise floor): the floor is the reference against itself with
    the batch rows permuted, relative to max |x| (at least one f64 ulp)."""
    ref, x, actions, adv = _case(name)
    g = _gain_grad(ref, x, actions, adv)
    xr = R.conj_gradient(R.make_hvp(ref, x, 0.1), g, 10).detach()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(14))
    xp = R.conj_gradient(R.make_hvp(ref, x[perm], 0.1), g, 10).detach()
    floor = max((xr - xp).abs().max().item() / xr.abs().max().item(), 2.0 ** -52)
    return g, xr, floor


@pytest.mark.parametrize("name", list(POLICIES))
def test_cg_direction_within_100_noise_floors(cuda, name):
    from mepol_amd.algorithms import trpo

    g, xr, floor = _ref_cg(name)
    fisher = trpo.PolicyFisher(_gpu_policy(name), _case(name)[1].cuda(), 0.1)
    assert fisher.kernels
    xd = trpo.conj_gradient(fisher.hvp, g.cuda(), 10).cpu()
    err = (xd - xr).abs().max().item() / xr.abs().max().item()
    print(f"cg {name}: device vs reference {err:.2e}, reference noise floor {floor:.2e}")
    assert err <= 100 * floor


STEP_SEED = 5  # chosen on the CPU reference: trial 0 is rejected on the KL, trial 1 accepted


def _step_case(seed=STEP_SEED, n=N, nf=2, hidden=(64, 48), a=2):
    ref = R.RefPolicy.random(nf, list(hidden), a, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(n, nf, generator=g, dtype=torch.float64)
    noise = torch.randn(n, a, generator=g, dtype=torch.float64)
    actions = (ref.mean(x) + noise * torch.exp(ref.log_std)).detach()
    adv = noise[:, 0] - 0.5 * noise[:, 1] + 0.25 * noise[:, 0] * noise[:, 1]
    return ref, x, actions, adv


def test_trpo_step_end_to_end(cuda):
    from mepol_amd.algorithms import trpo
    from mepol_amd.policy import GaussianPolicy

    thresh = 0.01
    ref, x, actions, adv = _step_case()
    policy = GaussianPolicy([64, 48], 2, 2)
    ref.load_into(policy)
    policy = policy.to("cuda")
    theta0 = ref.flat()
    mu0, ls0 = ref.mean(x).detach(), ref.log_std.detach().clone()
    ok_ref, it_ref, trials, _ = R.trpo_step(ref, x, actions, adv, thresh)
    # a condition on the inputs: every trial is decided with margin, and one is rejected
    assert ok_ref and it_ref >= 1
    scale = adv.abs().mean().item()
    for imp, k in trials:
        assert abs(imp) >= 1e-6 * scale and abs(k - thresh) >= 1e-6 * thresh
    # the reference's own noise floor: the same step with the batch rows permuted
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(15))
    ref_p = R.RefPolicy.random(2, [64, 48], 2, seed=STEP_SEED)
    ok_p, it_p, _, _ = R.trpo_step(ref_p, x[perm], actions[perm], adv[perm], thresh)
    assert (ok_p, it_p) == (ok_ref, it_ref)
    floor = max((ref.flat() - ref_p.flat()).abs().max().item(), 2.0 ** -52)

    ok, it = trpo.trpo_step(policy, x.cuda(), actions.cuda(), adv.cuda(), thresh)
    assert (ok, it) == (ok_ref, it_ref)
    theta = torch.cat([p.detach().reshape(-1) for p in policy.parameters()]).cpu()
    err = (theta - ref.flat()).abs().max().item()
    print(f"trpo_step: accepted at {it}, parameters vs reference {err:.2e}, floor {floor:.2e}")
    assert err <= 100 * floor and not torch.equal(theta, theta0)
    final = R.RefPolicy.random(2, [64, 48], 2, seed=STEP_SEED)
    final.assign(theta)
    assert R.kl(mu0, ls0, final.mean(x), final.log_std).item() < thresh


def test_trpo_step_exhausts_backtracking(cuda):
    """A threshold so small that the proposed steps do not change a single parameter bit: no
    trial improves the gain, all 10 are rejected and the parameters come back bit-identical."""
    from mepol_amd.algorithms import trpo
    from mepol_amd.policy import GaussianPolicy

    thresh = 1e-290
    ref, x, actions, adv = _step_case()
    theta0 = ref.flat()
    # a condition on the inputs, on the reference alone: the largest trial step rounds away
    ok_ref, it_ref, _, xdir = R.trpo_step(ref, x, actions, adv, thresh)
    assert (ok_ref, it_ref) == (False, 9)
    hx = R.make_hvp(ref, x, 0.1)(xdir)
    step = (1 / torch.sqrt(torch.dot(xdir, hx) / (2 * thresh))).item()
    assert torch.equal(theta0 + step * xdir.detach(), theta0)
    policy = GaussianPolicy([64, 48], 2, 2)
    ref.load_into(policy)
    policy = policy.to("cuda")
    ok, it = trpo.trpo_step(policy, x.cuda(), actions.cuda(), adv.cuda(), thresh)
    assert (ok, it) == (False, 9)
    theta = torch.cat([p.detach().reshape(-1) for p in policy.parameters()]).cpu()
    assert torch.equal(theta, theta0)
