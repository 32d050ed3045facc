"""The launch lists of the policy's kernel paths outside the graph body: which mepol_amd.ops
kernels get_log_p and its backward, PolicyFisher's construction, one Fisher-vector product and
policy_mean call, and in which order.  tests/test_gpu_loop_launch_order.py holds the graph
body's lists.

The calls are recorded on the attributes of the mepol_amd.ops module itself, so a list does not
depend on which module makes the call.  The lists are written out here, not derived from the
code under test: a change that needs one of them edited has moved a launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RECORDED = ("policy_forward", "layer_forward", "gemm_nt", "head_forward",
            "head_backward", "weight_grad", "hidden_backward", "layer_backward",
            "layer_tangent", "hidden_tangent", "mean_tangent", "mean_backward")
N, NF, A = 512, 3, 2  # just over policy.FUSED_MIN_ROWS and trpo.FVP_MIN_ROWS
DEEP, TWO = [64, 48, 32, 16], [64, 48]


def _forward(L):
    return ["layer_forward"] + (L - 1) * ["gemm_nt"] + ["head_forward"]


def _serial_backward(L):
    return (L - 1) * ["weight_grad", "hidden_backward"] + ["layer_backward"]


def _hvp(L):
    return (["layer_tangent"] + (L - 1) * ["hidden_tangent"] + ["mean_tangent", "mean_backward"]
            + _serial_backward(L))


@pytest.fixture
def calls(cuda, monkeypatch):
    from mepol_amd import ops

    for name in ("MEPOL_FUSED_MIN_ROWS", "MEPOL_FVP_MIN_ROWS"):
        monkeypatch.delenv(name, raising=False)
    made = []

    def recorded(name, real):
        def wrapper(*args, **kw):
            made.append(name)
            return real(*args, **kw)
        return wrapper

    for name in RECORDED:
        monkeypatch.setattr(ops, name, recorded(name, getattr(ops, name)))
    return made


def _case(hidden):
    from mepol_amd.policy import GaussianPolicy

    dev = torch.device("cuda")
    torch.manual_seed(11)
    policy = GaussianPolicy(hidden, NF, A).to(dev)
    g = torch.Generator(device=dev).manual_seed(12)
    kw = dict(dtype=torch.float64, device=dev, generator=g)
    states = torch.randn(N, NF, **kw)
    actions = torch.randn(N, A, **kw)
    v = torch.randn(sum(p.numel() for p in policy.parameters()), **kw)
    return policy, states, actions, v


def _take(calls):
    torch.cuda.synchronize()
    out = list(calls)
    print(out)
    del calls[:]
    return out


@pytest.mark.parametrize("hidden,forward,backward", [
    (DEEP, _forward(4), ["head_backward"] + _serial_backward(4)),
    # the two torch.mm (z2's dh1, and dW2 below 16,384 rows) are not ops calls
    (TWO, ["policy_forward"], ["head_backward", "layer_backward"]),
], ids=["deep4", "two-layer"])
def test_get_log_p_launch_list(calls, hidden, forward, backward):
    policy, states, actions, _ = _case(hidden)
    logp = policy.get_log_p(states, actions)
    assert _take(calls) == forward
    logp.sum().backward()
    assert _take(calls) == backward
    assert all(p.grad is not None for p in policy.parameters())


@pytest.mark.parametrize("hidden", [DEEP, TWO], ids=["deep4", "two-layer"])
def test_fisher_launch_list(calls, hidden):
    from mepol_amd.algorithms import trpo

    L = len(hidden)
    policy, states, _, v = _case(hidden)
    fisher = trpo.PolicyFisher(policy, states, 0.1)
    assert fisher.kernels
    assert _take(calls) == _forward(L)
    first = fisher.hvp(v)
    assert _take(calls) == _hvp(L)
    # the same bits for the same vector (PolicyFisher's promise; its scratch is shared by every
    # product, and `first` must not alias it)
    kept = first.clone()
    second = fisher.hvp(v)
    assert _take(calls) == _hvp(L)
    assert torch.equal(first, kept) and torch.equal(first, second)


def test_policy_mean_launch_list(calls):
    from mepol_amd.algorithms import trpo

    policy, states, actions, _ = _case(DEEP)
    assert trpo.fvp_kernels_ok(policy, states)
    mu = trpo.policy_mean(policy, states, actions)
    assert _take(calls) == _forward(4)
    assert mu.shape == (N, A)
