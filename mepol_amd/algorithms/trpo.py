"""TRPO's natural-gradient policy step for GaussianPolicy (src/algorithms/trpo.py:14-84, 345-424).

The reference takes every Hessian-vector product of KL(theta_0 || theta) by a double backward
through policy(states).  All cg_iters + 1 products of a step are taken at the same theta_0 over
the same states, and at theta_0 the Hessian has a closed form ("TRPO policy step"):

    network parameters   H v = (1/n) sum_i J_i^T diag(1 / (u + 1e-7)) J_i v,  u = exp(2 log_std),
                         J_i = d mu_i / d theta_net
    log_std              (H v)_a = 2 u_a^2 (u_a - 1e-7) / (u_a + 1e-7)^3 v_a   (a diagonal block)

so PolicyFisher runs ONE forward, keeps its activations, and every product is a tangent pass
(ops.layer_tangent, ops.hidden_tangent, ops.mean_tangent) and a backward pass (ops.mean_backward,
ops.weight_grad, ops.hidden_backward, ops.layer_backward) on the library's HIP kernels.  Shapes
the kernels do not take (one hidden layer, odd widths, other activations, batches under
FVP_MIN_ROWS, CPU tensors) use the reference's own method, a double backward over a plain
F.linear restatement of mu (it must not go through policy._Linear, whose weight gradient is a
kernel call without an autograd graph behind it).

conj_gradient, assign_flat_params and backtracking keep the reference's names, argument order
and control flow; trpo_step is its policy update (old log-probabilities, gain and gradient,
conjugate gradient, Lagrange multiplier, backtracking line search).  Sampling, the critic and
the goal_rl command line are not part of this module.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import kernel_path, ops
from .. import policy as _policy
from ..kernel_path import linear_layers

KL_VAR_EPS = 1e-7  # the epsilon on the variance in the reference's KL (trpo.py:384)

# Rows from which PolicyFisher takes the HIP kernels; MEPOL_FVP_MIN_ROWS overrides it, read per
# call.  The smallest batch of tools/trpo_step_bench.py's sweep from which the kernel path beat
# the double backward for both policies ("TRPO policy step").
FVP_MIN_ROWS = _policy.FUSED_MIN_ROWS

FVP_MIN_LAYERS, FVP_MAX_LAYERS = 2, kernel_path.MULTILAYER_MAX
FVP_MAX_WIDTH = kernel_path.HEAD_MAX_WIDTH  # of EVERY hidden layer, not only the head's input
FVP_MAX_FEATURES = kernel_path.MAX_FEATURES
FVP_MAX_ACTIONS = kernel_path.HEAD_MAX_ACTIONS


def fvp_min_rows():
    v = os.environ.get("MEPOL_FVP_MIN_ROWS")
    return int(v) if v else FVP_MIN_ROWS


def fvp_kernels_ok(policy, states):
    """True when PolicyFisher (and the constraint's mean) take the HIP kernels: an f64 ReLU policy
    on the GPU with 2 to 6 hidden layers of even width <= 512, at most 64 features and 32
    actions, and a batch of at least fvp_min_rows() rows."""
    layers = linear_layers(policy)
    return (states.is_cuda and states.dim() == 2 and states.dtype == torch.float64
            and policy.log_std.is_cuda and policy.log_std.dtype == torch.float64
            and policy.activation is nn.ReLU
            and FVP_MIN_LAYERS <= len(layers) <= FVP_MAX_LAYERS
            and all(m.out_features % 2 == 0 and m.out_features <= FVP_MAX_WIDTH for m in layers)
            and policy.num_features <= FVP_MAX_FEATURES
            and policy.action_dim <= FVP_MAX_ACTIONS
            and states.shape[0] >= fvp_min_rows())


def plain_mean(policy, states):
    """mu(states) restated with F.linear and the policy's activation modules: twice
    differentiable in every parameter at any batch size."""
    h = states
    for layer in policy.net:
        h = F.linear(h, layer.weight, layer.bias) if isinstance(layer, nn.Linear) else layer(h)
    return F.linear(h, policy.mean.weight, policy.mean.bias)


def gaussian_kl(mu0, log_std0, mu1, log_std1):
    """KL(0 || 1) of the reference (trpo.py:381-386), the epsilon on the new variance."""
    var0 = torch.exp(log_std0) ** 2
    var1 = torch.exp(log_std1) ** 2
    return (0.5 * ((var0 + (mu1 - mu0) ** 2) / (var1 + KL_VAR_EPS) - 1)
            + log_std1 - log_std0).sum(dim=1).mean()


def policy_mean(policy, states, actions=None):
    """mu(states) without a graph: the forward kernels (kernel_path.hidden_forward,
    ops.head_forward) where fvp_kernels_ok, the policy's own mean_action otherwise."""
    with torch.no_grad():
        if not fvp_kernels_ok(policy, states):
            return policy.mean_action(states)
        layers = linear_layers(policy)
        x = states.contiguous()
        Ws = [m.weight.detach().contiguous() for m in layers]
        bs = [m.bias.detach().contiguous() for m in layers]
        _, zL = kernel_path.hidden_forward(x, Ws, bs)
        if actions is None:
            actions = torch.zeros((x.shape[0], policy.action_dim), dtype=torch.float64,
                                  device=x.device)
        mu, _ = ops.head_forward(zL, policy.mean.weight.detach().contiguous(),
                                 policy.mean.bias.detach().contiguous(),
                                 policy.log_std.detach().contiguous(), actions.contiguous(),
                                 bz=bs[-1])
        return mu


class PolicyFisher:
    """Hessian-vector products of KL(theta_0 || theta) at theta = theta_0, the policy's
    parameters when this object is built, over `states`, plus cg_damping * v.

    hvp(v_flat) -> flat, both laid out as torch.cat([p.reshape(-1) for p in
    policy.parameters()]).  On the kernel path (fvp_kernels_ok) the forward activations, a copy
    of theta_0 and all scratch are made once here; hvp only enqueues kernels (no host
    synchronisation, no allocation besides the result) and gives the same bits for the same v.
    Otherwise hvp is the reference's double backward at the policy's CURRENT parameters, which
    the caller leaves at theta_0 while it takes products."""

    def __init__(self, policy, states, cg_damping):
        self.policy = policy
        self.damping = float(cg_damping)
        self.params = list(policy.parameters())
        self.numel = sum(p.numel() for p in self.params)
        self.kernels = fvp_kernels_ok(policy, states)
        self.log_std0 = policy.log_std.detach().clone()
        if self.kernels:
            self._init_kernels(states)
        else:
            self.states = states.detach()
            with torch.no_grad():
                self.mu0 = plain_mean(policy, self.states)

    # ---- kernel path ----------------------------------------------------------------------
    def _init_kernels(self, states):
        policy = self.policy
        dev = states.device
        x = states.detach().contiguous()
        n = x.shape[0]
        layers = linear_layers(policy)
        L = len(layers)
        self.x, self.n, self.L = x, n, L
        self.Ws = [m.weight.detach().clone().contiguous() for m in layers]
        self.bs = [m.bias.detach().clone().contiguous() for m in layers]
        self.Wm = policy.mean.weight.detach().clone().contiguous()
        self.bm = policy.mean.bias.detach().clone().contiguous()
        widths = [W.shape[0] for W in self.Ws]
        a = self.Wm.shape[0]
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.no_grad():
            self.hs, self.zL = kernel_path.hidden_forward(x, self.Ws, self.bs)
            self.mu0, _ = ops.head_forward(self.zL, self.Wm, self.bm, self.log_std0,
                                           torch.zeros((n, a), **f64), bz=self.bs[-1])
            u = torch.exp(2.0 * self.log_std0)
            self.scale = 1.0 / ((u + KL_VAR_EPS) * n)
            self.ls_coef = 2.0 * u * u * (u - KL_VAR_EPS) / (u + KL_VAR_EPS) ** 3
        self.variants = [ops.gemm_nt_variant(n, w) for w in widths]

        # v and the result in a padded layout whose segments start on 16-byte boundaries (the
        # matrix-core kernels' operand contract); one gather in, one gather out per product
        role = {id(policy.log_std): ("ls", 0), id(policy.mean.weight): ("Wm", 0),
                id(policy.mean.bias): ("bm", 0)}
        for l, m in enumerate(layers):
            role[id(m.weight)] = ("W", l)
            role[id(m.bias)] = ("b", l)
        gather, scatter, segs, pos, flat = [], [], {}, 0, 0
        for p in self.params:
            k = p.numel()
            segs[role[id(p)]] = (pos, k, tuple(p.shape))
            gather.append(torch.arange(flat, flat + k))
            scatter.append(torch.arange(pos, pos + k))
            if k % 2:
                gather.append(torch.zeros(1, dtype=torch.int64))
            pos += k + k % 2
            flat += k
        self._gather = torch.cat(gather).to(dev)
        self._scatter = torch.cat(scatter).to(dev)
        self._vpad = torch.zeros(pos, **f64)
        self._opad = torch.zeros(pos, **f64)

        def views(buf):
            return {key: buf[o:o + k].view(shape) for key, (o, k, shape) in segs.items()}

        self._vin, self._vout = views(self._vpad), views(self._opad)
        # t_l and dz_l share a buffer per layer: t_l is dead once c is formed
        self._act = [torch.empty((n, w), **f64) for w in widths]
        self._c = torch.empty((n, a), **f64)
        self._db_unused = torch.empty(widths[0], **f64)
        self._ws_mean = ops.mean_backward_workspace(n, widths[-1], a, dev)
        self._ws_wg = [None] + [ops.weight_grad_workspace(n, widths[l], widths[l - 1], dev)
                                for l in range(1, L)]
        self._ws_hb = [None] + [ops.hidden_backward_workspace(n, widths[l - 1], dev)
                                for l in range(1, L)]
        self._ws_layer = ops.layer_workspace(n, x.shape[1], widths[0], dev)
        # kernel_path.hidden_backward's outputs: dW_l and db_l into the result, dz_l over t_l
        self._backward_out = dict(
            dW_out=[self._vout["W", l] for l in range(L)],
            db_out=[self._vout["b", l] for l in range(L - 1)], dz_out=self._act,
            ws_wgrad=self._ws_wg, ws_hidden=self._ws_hb, ws_layer=self._ws_layer,
            layer_db_out=self._db_unused)

    def _hvp_kernels(self, v):
        L, vin, out = self.L, self._vin, self._vout
        torch.index_select(v, 0, self._gather, out=self._vpad)
        # tangent pass: t_l = mask_l * (t_{l-1} W_l^T + h_{l-1} V_W_l^T + V_b_l), t_0 = 0
        t = ops.layer_tangent(self.x, vin["W", 0], vin["b", 0], self.hs[0], out=self._act[0])
        for l in range(1, L):
            last = l == L - 1
            t = ops.hidden_tangent(t, self.hs[l - 1], self.Ws[l], vin["W", l], vin["b", l],
                                   self.zL if last else self.hs[l],
                                   self.bs[l] if last else None, out=self._act[l],
                                   variant=self.variants[l])
        c = ops.mean_tangent(t, self.zL, self.Wm, vin["Wm", 0], vin["bm", 0], self.scale,
                             bz=self.bs[-1], out=self._c)
        # backward pass J^T c
        dz, _, _, _ = ops.mean_backward(c, self.zL, self.Wm, bz=self.bs[-1], ws=self._ws_mean,
                                        dz_out=self._act[L - 1],
                                        outs=(out["Wm", 0], out["bm", 0], out["b", L - 1]))
        kernel_path.hidden_backward(dz, self.x, self.Ws, self.hs, **self._backward_out)
        torch.mul(self.ls_coef, vin["ls", 0], out=out["ls", 0])
        res = torch.index_select(self._opad, 0, self._scatter)
        return res.add_(v, alpha=self.damping)

    # ---- the reference's method -----------------------------------------------------------
    def _hvp_autograd(self, v):
        policy = self.policy
        with torch.enable_grad():
            kl = gaussian_kl(self.mu0, self.log_std0, plain_mean(policy, self.states),
                             policy.log_std)
            grads = torch.autograd.grad(kl, self.params, create_graph=True)
            flat = torch.cat([g.reshape(-1) for g in grads])
            grads2 = torch.autograd.grad(torch.sum(flat * v), self.params, allow_unused=True)
        res = torch.cat([(torch.zeros_like(p) if g is None else g).reshape(-1)
                         for g, p in zip(grads2, self.params)])
        return res + self.damping * v

    def hvp(self, v_flat):
        v = v_flat.detach()
        if v.dim() != 1 or v.numel() != self.numel:
            raise ValueError(f"hvp: a flat vector of {self.numel} entries is needed")
        if not self.kernels:
            return self._hvp_autograd(v)
        if not v.is_cuda or v.dtype != torch.float64:
            raise ValueError("hvp: the kernel path takes an f64 vector on the policy's device")
        with torch.no_grad():
            return self._hvp_kernels(v.contiguous())


def assign_flat_params(model, flat_params):
    """Writes the flat parameter vector (the layout of torch.cat over model.parameters()) into
    the model's parameters, in place: their storage, and so its alignment, stays."""
    params = list(model.parameters())
    if flat_params.dim() != 1 or flat_params.numel() != sum(p.numel() for p in params):
        raise ValueError("assign_flat_params: the vector does not match the model's parameters")
    offset = 0
    with torch.no_grad():
        for p in params:
            k = p.numel()
            p.data.copy_(flat_params[offset:offset + k].view(p.shape))
            offset += k


def backtracking(model, compute_objective, compute_constraint, constrain_thresh, search_dir,
                 step, max_iters=10, just_check_constraint=False):
    """Backtracking line search from the model's parameters along step * search_dir, the step
    halved per trial: accepts the first trial whose objective improved (unless
    just_check_constraint) and whose constraint is finite and under constrain_thresh.  Returns
    (True, new_params, i) or, after max_iters rejections, (False, old_params, max_iters - 1) with
    the parameters restored.  The two scalars of a trial are read on the host."""
    old_objective = float(compute_objective())
    old_params = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    thresh = float(constrain_thresh)
    for i in range(max_iters):
        new_params = old_params + (0.5 ** i) * step * search_dir
        assign_flat_params(model, new_params)
        new_objective = float(compute_objective())
        new_constraint = float(compute_constraint())
        improved = math.isfinite(new_objective) and new_objective - old_objective > 0
        if ((just_check_constraint or improved) and math.isfinite(new_constraint)
                and new_constraint < thresh):
            return True, new_params, i
    assign_flat_params(model, old_params)
    return False, old_params, max_iters - 1


def conj_gradient(Ax, b, iters):
    """`iters` conjugate-gradient iterations for A x = b from x = 0; Ax(p) returns A p.  alpha,
    beta and the dot products stay 0-dim device tensors: nothing is read on the host."""
    x = torch.zeros_like(b)
    r = b.clone()
    p = b.clone()
    rr = torch.dot(r, r)
    for i in range(iters):
        Ap = Ax(p)
        alpha = rr / torch.dot(p, Ap)
        x = x + alpha * p
        if i + 1 == iters:
            break
        r = r - alpha * Ap
        rr_new = torch.dot(r, r)
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x


def trpo_step(policy, states, actions, advantages, kl_thresh, cg_iters=10, cg_damping=0.1,
              max_backtracks=10):
    """One TRPO policy update (trpo.py:345-424): maximise mean(exp(logp - logp_old) A) inside
    KL(old || new) < kl_thresh.  Returns (success, backtrack_iters); on failure the parameters
    are the ones before the call.  The gain, its gradient and the line search's evaluations go
    through GaussianPolicy.get_log_p (the fused kernels at its batch sizes), the constraint's
    mean through policy_mean, the Fisher-vector products through PolicyFisher."""
    params = list(policy.parameters())
    with torch.no_grad():
        old_log_prob = policy.get_log_p(states, actions)

    def compute_gain():
        return torch.mean(torch.exp(policy.get_log_p(states, actions) - old_log_prob) * advantages)

    fisher = PolicyFisher(policy, states, cg_damping)
    mu0, log_std0 = fisher.mu0, fisher.log_std0

    def compute_kl():
        with torch.no_grad():
            return gaussian_kl(mu0, log_std0, policy_mean(policy, states, actions),
                               policy.log_std.detach())

    def objective():
        with torch.no_grad():
            return compute_gain()

    g = torch.cat([t.reshape(-1) for t in torch.autograd.grad(compute_gain(), params)])
    x = conj_gradient(fisher.hvp, g, cg_iters)
    # 1 / lagrange is the largest step along x inside the quadratic model of the constraint
    lagrange = torch.sqrt(torch.dot(x, fisher.hvp(x)) / (2 * kl_thresh))
    success, _, backtrack_iters = backtracking(policy, objective, compute_kl, kl_thresh, x,
                                               1 / lagrange, max_iters=max_backtracks)
    return success, backtrack_iters
