"""TRPO for GaussianPolicy: drop-in for src/algorithms/trpo.py of the reference.

  collect_sample_batch(env, policy, batch_size, traj_len, num_workers)           :86-172
  process_traj(gamma, lambd, vfuncs, states, actions, rewards, boot_value)       :175-201
  trpo(env_maker, env_name, num_epochs, batch_size, traj_len, ...)               :204-493
  conj_gradient, assign_flat_params, backtracking                                :14-84
  trpo_step: the policy update inside trpo()                                     :345-424
  process_batch: the per-trajectory loop and concatenation inside trpo()         :281-331

Policy step.  The reference takes every Hessian-vector product of KL(theta_0 || theta) by a double
backward through policy(states).  All cg_iters + 1 products of a step are taken at the same
theta_0 over the same states, and at theta_0 the Hessian has a closed form ("TRPO
policy step"):

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

Sampling and batch processing ("TRPO sampling and batch processing").  The reference
steps one env at a time through policy.predict.  For a GridWorld or MountainCar goal env and a
ReLU policy with two to six hidden layers (kernel_path.goal_sampler) collect_sample_batch rolls
whole rounds of trajectories out in one launch each (ops.rollout_goal for two layers,
ops.rollout_deep_goal for three to six: termination and the sparse reward inside the kernel; for
a threshold goal, on GridWorld or MountainCar, ops.rollout_goal_threshold and
ops.rollout_deep_goal_threshold), applies the reference's step budget on the device
(ops.traj_budget) and reads two or three words per round.  Any other reward of the reached state
alone (envs.BatchReward: BoxGoal, AnyGoal, a user's own; kernel_path.cut_sampler) takes the same
rounds on the un-terminated one-launch rollouts (ops.rollout_mlp, ops.rollout_deep), one batched
reward call per round and ops.traj_cut, which cuts every trajectory at its first done;
process_batch computes targets, GAE advantages and the packed batch with ops.gae and
ops.standardize.  Every other env, policy or device takes the reference's sequential loop, and
CPU tensors a numpy restatement of the same arithmetic.

Critic fit ("Critic fit").  The critic is a torch module; the Adam branch of its fit
(all critic_iters passes over the DataLoader's mini-batches) runs as one launch of one resident
workgroup (ops.critic_fit) where kernel_path.critic_fit_ok accepts the critic and its optimizer,
over the same mini-batches and with the optimizer's state left as the loop would leave it.
L-BFGS, CPU critics and other shapes take the reference's loop under autograd.

conj_gradient, assign_flat_params and backtracking keep the reference's names, argument order
and control flow.
"""
import math
import os
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import kernel_path, ops
from .. import policy as _policy
from ..envs.wrappers import ThresholdGoal, unwrap
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


# ---------------------------------------------------------------------------------------------
# Sampling (trpo.py:86-172)
# ---------------------------------------------------------------------------------------------
# What the last collect_sample_batch call did: "path" is "kernel" (a goal-mode rollout), "cut" (an
# un-terminated rollout cut by a BatchReward) or "host", "rounds" the rollout launches of the two
# kernel routes; "kernel_batches" / "cut_batches" / "host_batches" count calls since import.
SAMPLER_STATS = {"path": None, "rounds": 0, "kernel_batches": 0, "host_batches": 0,
                 "cut_batches": 0}

ROUND_MAX_TRAJ = 65536  # mepol_traj_budget's limit
_ROUND_CAPACITY = {}


BALL, THRESHOLD = "ball", "threshold"  # the goal kinds of the rollout kernels
CUT = "cut"                            # no goal in the kernel: the un-terminated rollouts
MOUNTAINCAR, GRIDWORLD = kernel_path.MOUNTAINCAR, kernel_path.GRIDWORLD  # their env_id
MAZE = kernel_path.MAZE


def _round_capacity(h0, h1, a_dim, device, env_id=GRIDWORLD, kind=BALL):
    """Trajectories per round that cost no more time than one: the most for which the plan of
    the instance that runs (ops.rollout_goal_plan for GridWorld's ball goal,
    ops.rollout_goal_threshold_plan for a threshold goal on env_id, ops.rollout_mlp_plan for the
    cut route's un-terminated rollout: each kernel's own occupancy) still reports the
    multi-workgroup form, found once per shape, env, kind (so route) and MEPOL_ROLLOUT_MW setting
    by bisection, or, where there is no such form, one workgroup per CU."""
    key = (h0, h1, a_dim, device, os.environ.get("MEPOL_ROLLOUT_MW"), env_id, kind)
    if key not in _ROUND_CAPACITY:
        def multi(n):
            plan = (ops.rollout_goal_plan(n, h0, h1, a_dim, env_id=env_id) if kind == BALL
                    else ops.rollout_mlp_plan(n, h0, h1, a_dim, env_id=env_id) if kind == CUT
                    else ops.rollout_goal_threshold_plan(env_id, n, h0, h1, a_dim))
            return plan["workgroups_per_traj"] > 1

        lo, hi = 0, 1 << 16  # multi(n) holds up to some n < hi (no device holds 65,536 parts)
        while lo + 1 < hi:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if multi(mid) else (lo, mid)
        _ROUND_CAPACITY[key] = lo or torch.cuda.get_device_properties(device).multi_processor_count
    return _ROUND_CAPACITY[key]


def _round_capacity_deep(widths, a_dim, device, env_id=GRIDWORLD, kind=BALL):
    """_round_capacity for a policy with 3 to 6 hidden layers: the trajectories (one workgroup
    each) the device holds at once (ops.rollout_deep_goal_plan, ops.rollout_deep_goal_threshold_plan
    for a threshold goal on env_id, or ops.rollout_deep_plan for the cut route's un-terminated
    rollout), found once per shape, env, kind (so route) and MEPOL_ROLLOUT_KL setting (the
    resident rows set the kernel's LDS, so its occupancy)."""
    key = (tuple(widths), a_dim, device, os.environ.get("MEPOL_ROLLOUT_KL"), env_id, kind)
    if key not in _ROUND_CAPACITY:
        plan = (ops.rollout_deep_goal_plan(widths, a_dim, env_id=env_id) if kind == BALL
                else ops.rollout_deep_plan(env_id, widths, a_dim) if kind == CUT
                else ops.rollout_deep_goal_threshold_plan(env_id, widths, a_dim))
        _ROUND_CAPACITY[key] = max(plan["resident_workgroups"], 1)
    return _ROUND_CAPACITY[key]


def _draw_round(base, R, T, a_dim, device, generator):
    """Initial states [R, 2] in the env's own dtype (GridWorld f32, MountainCar f64) and action
    noise f64 [T, R, a] of one round, in this order."""
    init = base.reset_batch_torch(R, device, generator)
    noise = torch.randn((T, R, a_dim), dtype=torch.float64, device=device, generator=generator)
    return init, noise


def _goal_round(goal, layers, head, env_id, maze=None):
    """(fill, cap kind) of the in-kernel goal route: fill(init, noise, states, actions, rewards)
    runs one round on the GOAL instance of env x goal kind (kernel_path.goal_sampler admits no
    other pair) and returns (lens, dones, err, rerun), the last two None for the deep rollouts,
    which have no error word and so no re-run.  maze: the box maze's struct for env_id 2."""
    deep = len(layers) > 2
    kind = THRESHOLD if isinstance(goal, ThresholdGoal) else BALL
    test = (goal.goal, goal.radius) if kind == BALL else (goal.index, goal.threshold)

    def fill(init, noise, states, actions, rewards):
        R = init.shape[0]
        lens = torch.empty(R, dtype=torch.int32, device=init.device)
        dones = torch.empty(R, dtype=torch.int32, device=init.device)
        roll = (*head, init, noise, *test, states, actions, rewards, lens, dones)
        if deep:
            if kind == BALL:
                ops.rollout_deep_goal(layers, *roll, env_id=env_id, maze=maze)
            else:
                ops.rollout_deep_goal_threshold(env_id, layers, *roll, maze=maze)
            return lens, dones, None, None
        (W1, b1), (W2, b2) = layers
        if kind == BALL:
            err, rerun = ops.rollout_goal(W1, b1, W2, b2, *roll, env_id=env_id,
                                          defer_check=True, maze=maze)
        else:
            err, rerun = ops.rollout_goal_threshold(env_id, W1, b1, W2, b2, *roll,
                                                    defer_check=True, maze=maze)
        return lens, dones, err, rerun

    return fill, kind


def _cut_round(goal, layers, head, env_id, maze=None):
    """(fill, cap kind) of the "roll out, then cut" route (kernel_path.cut_sampler): fill rolls
    the round out UN-terminated in one launch (ops.rollout_mlp, which handles its own error word,
    or ops.rollout_deep), evaluates the BatchReward once over the env's own state after every
    step (MountainCar's f64 `visited`; GridWorld's and the maze's f32 records widened, which is
    exact) and cuts
    every trajectory at its first done (ops.traj_cut): the outputs of a goal-mode rollout."""
    deep = len(layers) > 2
    who = type(goal).__name__

    def fill(init, noise, states, actions, rewards):
        R, T = init.shape[0], noise.shape[0]
        visited = (torch.empty((R, T, 2), dtype=torch.float64, device=init.device)
                   if env_id == MOUNTAINCAR else None)
        if deep:
            ops.rollout_deep(env_id, layers, *head, init, noise, states, actions, visited=visited,
                             maze=maze)
        else:
            ops.rollout_mlp(env_id, *layers[0], *layers[1], *head, init, noise, states, actions,
                            visited=visited, maze=maze)
        env_states = visited if visited is not None else states[:, 1:].to(torch.float64)
        out = goal.batch(env_states)
        if not (isinstance(out, tuple) and len(out) == 2 and all(torch.is_tensor(x) for x in out)):
            raise ValueError(f"{who}.batch must return (reward, done), two tensors")
        reward, done = out
        if tuple(reward.shape) != (R, T) or tuple(done.shape) != (R, T):
            raise ValueError(f"{who}.batch must return reward and done of shape [n, T] = "
                             f"{(R, T)}; got {tuple(reward.shape)} and {tuple(done.shape)}")
        if done.dtype != torch.bool or not reward.is_floating_point():
            raise ValueError(f"{who}.batch must return a float reward and a bool done; got "
                             f"{reward.dtype} and {done.dtype}")
        if reward.device != init.device or done.device != init.device:
            raise ValueError(f"{who}.batch must keep its results on the states' device")
        rewards.copy_(reward)  # rounds to f32
        lens, dones = ops.traj_cut(done.contiguous(), rewards, states, actions)
        return lens, dones, None, None

    return fill, CUT


def _collect_kernel(env, policy, goal, layers, batch_size, T, generator, draw, round_traj,
                    cut_env=None):
    """The round loop of both kernel routes: goal_sampler's (cut_env None; termination inside the
    rollout kernel) and cut_sampler's (cut_env = its env_id).  Only `fill`, the part that leaves
    (states, actions, rewards, lens, dones) of a round, differs."""
    dev = policy.device
    base = unwrap(env)
    a_dim = policy.action_dim
    env_id = kernel_path.kernel_env(base) if cut_env is None else cut_env
    widths = [W.shape[0] for W, _ in layers]
    head = (policy.mean.weight.detach(), policy.mean.bias.detach(), policy.log_std.detach())
    maze = kernel_path.maze_of(base, env_id)
    maze = ops.maze_struct(maze) if maze is not None else None
    fill, kind = (_goal_round if cut_env is None else _cut_round)(goal, layers, head, env_id, maze)
    # the occupancy of the instance that runs
    cap = (_round_capacity_deep(widths, a_dim, dev, env_id, kind) if len(layers) > 2
           else _round_capacity(*widths, a_dim, dev, env_id, kind))
    steps_idx = torch.arange(T + 1, device=dev)
    remaining, rounds, parts = int(batch_size), 0, []
    while remaining > 0:
        R = int(round_traj) if round_traj else max(-(-remaining // T), cap)
        R = min(R, ROUND_MAX_TRAJ)
        init, noise = (draw(R, T, a_dim, dev) if draw is not None
                       else _draw_round(base, R, T, a_dim, dev, generator))
        states = torch.empty((R, T + 1, 2), dtype=torch.float32, device=dev)
        actions = torch.empty((R, T, a_dim), dtype=torch.float32, device=dev)
        rewards = torch.empty((R, T), dtype=torch.float32, device=dev)
        if env_id != MOUNTAINCAR:
            init = init.to(torch.float32)
        lens, dones, err, rerun = fill(init, noise, states, actions, rewards)
        kept_len, kept_done, _, meta = ops.traj_budget(lens, dones, remaining)
        if err is None:
            # the round's one host synchronisation: {trajectories used, steps kept}
            m, kept = meta.tolist()
        else:
            # the round's one host synchronisation: {trajectories used, steps kept, error word}
            m, kept, bad = torch.cat([meta, err.to(torch.int64)]).tolist()
            if bad:
                rerun()
                kept_len, kept_done, _, meta = ops.traj_budget(lens, dones, remaining)
                m, kept = meta.tolist()
        rounds += 1
        # a budget-cut last trajectory keeps the state it reached and nothing behind it, as the
        # reference's arrays do; that takes the reward of a goal it reached behind the cut, too
        last = kept_len[m - 1]
        states[m - 1].masked_fill_((steps_idx > last)[:, None], 0)
        actions[m - 1].masked_fill_((steps_idx[:T] >= last)[:, None], 0)
        rewards[m - 1].masked_fill_(steps_idx[:T] >= last, 0)
        parts.append((states[:m], actions[:m], rewards[:m], kept_len[:m], kept_done[:m]))
        remaining -= kept
    path = "kernel" if cut_env is None else "cut"
    SAMPLER_STATS.update(path=path, rounds=rounds)
    SAMPLER_STATS[path + "_batches"] += 1
    st, ac, rw, ln, dn = (torch.cat(x) if len(parts) > 1 else x[0] for x in zip(*parts))
    return st, ac, rw, ln.reshape(-1, 1), dn.reshape(-1, 1).bool()


def _collect_host(env, policy, batch_size, traj_len):
    """The reference's one-worker loop (trpo.py:87-157): one env, one policy.predict per step."""
    steps = 0
    nf = env.num_features
    a_dim = env.action_space.shape[0]
    total = []
    while steps < batch_size:
        states = np.zeros((1, traj_len + 1, nf), dtype=np.float32)
        actions = np.zeros((1, traj_len, a_dim), dtype=np.float32)
        rewards = np.zeros((1, traj_len), dtype=np.float32)
        s = env.reset()
        done, t = False, -1
        for t in range(traj_len):
            states[0, t] = s
            a = policy.predict(s).numpy()
            actions[0, t] = a
            ns, r, done, _ = env.step(a)
            rewards[0, t] = r
            s = ns
            steps += 1
            if done is True or steps == batch_size:
                break
        states[0, t + 1] = s
        total.append((states, actions, rewards, np.array([[t + 1]], dtype=np.int32),
                      np.array([[done]], dtype=bool)))
    SAMPLER_STATS.update(path="host", rounds=0)
    SAMPLER_STATS["host_batches"] += 1
    dev = getattr(policy, "device", torch.device("cpu"))
    return tuple(torch.as_tensor(np.vstack(x), device=dev) for x in zip(*total))


def collect_sample_batch(env, policy, batch_size, traj_len, num_workers=1, generator=None,
                         draw=None, round_traj=None):
    """Trajectories of at most traj_len steps until exactly batch_size steps are collected, the
    last one cut (trpo.py:86-172).  Returns tensors on the policy's device: states f32
    [m, T+1, nf], actions f32 [m, T, a], rewards f32 [m, T], real_traj_lens int32 [m, 1], dones
    bool [m, 1]; rows behind a trajectory's end are zero.

    Where kernel_path.goal_sampler takes (env, policy), rounds of R trajectories are rolled out
    in one launch each and cut to the remaining budget on the device; taking the first m of a
    parallel round in index order has the distribution of the reference's sequential sampling
    (DESIGN.md).  R = round_traj, or the larger of ceil(remaining / traj_len) and the most
    trajectories the multi-workgroup rollout holds (_round_capacity; for 3 to 6 hidden layers
    the workgroups the device holds at once, _round_capacity_deep).  `generator` seeds the
    draws; `draw(R, T, a, device) -> (init [R, 2] in the env's dtype, GridWorld f32 / MountainCar
    f64, noise f64 [T, R, a])` replaces them (tests).  num_workers is ignored there.

    Where kernel_path.cut_sampler takes them instead (any BatchReward: a reward of the reached
    state alone), the same rounds run un-terminated and are cut at each trajectory's first done
    (_cut_round); the draws, the budget and the results' layout are the goal route's, and a round
    always costs traj_len steps.  Everything else runs the reference's sequential loop with one
    worker."""
    if not hasattr(env.action_space, "shape") or hasattr(env.action_space, "n"):
        raise NotImplementedError("collect_sample_batch: continuous action spaces only")
    if batch_size > 0:
        spec = kernel_path.goal_sampler(env, policy)
        cut = kernel_path.cut_sampler(env, policy) if spec is None else None
        if spec is not None or cut is not None:
            goal, layers, cut_env = (*spec, None) if spec is not None else cut
            with torch.no_grad():
                return _collect_kernel(env, policy, goal, layers, batch_size, int(traj_len),
                                       generator, draw, round_traj, cut_env=cut_env)
    return _collect_host(env, policy, int(batch_size), int(traj_len))


# ---------------------------------------------------------------------------------------------
# Targets and advantages (trpo.py:175-201, 281-331)
# ---------------------------------------------------------------------------------------------
def _np64(x):
    """x (tensor, array or scalar) as an f64 numpy array; f32 values widen exactly."""
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def process_traj(gamma, lambd, vfuncs, states, actions, rewards, boot_value):
    """Discounted targets and GAE advantages of one trajectory (trpo.py:175-201), on the host.
    The reference's operator order in f64; unlike the reference the results stay f64 (it rounds
    every step's value to f32)."""
    n = np.shape(states)[0]
    v, r = _np64(vfuncs).reshape(-1), _np64(rewards).reshape(-1)
    boot = _np64(boot_value).reshape(-1)[0]
    gamma, lambd = np.float64(gamma), np.float64(lambd)
    targets = np.zeros(n, dtype=np.float64)
    curr_target = boot
    for i in reversed(range(n)):
        targets[i] = r[i] + gamma * curr_target
        curr_target = targets[i]
    advantages = np.zeros(n, dtype=np.float64)
    curr_advantage = np.float64(0)
    for i in reversed(range(n)):
        v_next = boot if i == n - 1 else v[i + 1]
        advantages[i] = (r[i] + gamma * v_next - v[i]) + gamma * lambd * curr_advantage
        curr_advantage = advantages[i]
    return targets, advantages


def process_batch(states, actions, rewards, real_traj_lens, dones, values, gamma, lambd):
    """The epoch's update batch from a sampled one (trpo.py:281-341): per trajectory the first
    real_traj_len steps, targets and GAE advantages bootstrapped from values[i, len] unless done,
    concatenated, the advantages standardised.  values f64 [m, T+1]: the critic at every recorded
    state.  Returns f64 (epoch_states [N, nf], epoch_actions [N, a], epoch_targets [N, 1],
    epoch_advantages [N]) on the inputs' device.  CUDA inputs take ops.gae + ops.standardize, CPU
    inputs a numpy restatement of the same arithmetic."""
    m, T = rewards.shape
    lens = real_traj_lens.reshape(-1)
    if states.is_cuda:
        lens = lens.to(torch.int32)
        offsets = torch.zeros(m + 1, dtype=torch.int64, device=states.device)
        torch.cumsum(lens, 0, out=offsets[1:])
        targets, adv, st, ac = ops.gae(rewards, values.detach().to(torch.float64), lens,
                                       dones.reshape(-1).to(torch.int32), offsets,
                                       int(offsets[-1]), gamma, lambd, states, actions)
        return st, ac, targets.unsqueeze(1), ops.standardize(adv)
    S, A, R = states.numpy(), actions.numpy(), rewards.numpy()
    V, L, D = values.detach().numpy().astype(np.float64), lens.numpy(), dones.reshape(-1).numpy()
    out = []
    for i in range(m):
        n = int(L[i])
        boot = np.float64(0) if D[i] else V[i, n]
        t, a = process_traj(gamma, lambd, V[i, :n], S[i, :n], A[i, :n], R[i, :n], boot)
        out.append((S[i, :n].astype(np.float64), A[i, :n].astype(np.float64), t, a))
    st, ac, targets, adv = (np.concatenate(x) for x in zip(*out))
    adv = (adv - adv.mean()) / adv.std()
    return (torch.from_numpy(st), torch.from_numpy(ac), torch.from_numpy(targets).unsqueeze(1),
            torch.from_numpy(adv))


# ---------------------------------------------------------------------------------------------
# Driver (trpo.py:204-493)
# ---------------------------------------------------------------------------------------------
CRITIC_FIT_STATS = {"path": None, "kernel_calls": 0, "steps": 0}


def critic_fit_index(n, critic_iters, critic_batch_size):
    """Row indices of the mini-batches DataLoader(TensorDataset(...), batch_size, shuffle=True,
    drop_last=True) yields over critic_iters passes, [critic_iters * (n // batch) * batch] int32
    on the host, with the same draws from torch's global CPU generator: per pass the iterator's
    base seed, then the RandomSampler's own seed and permutation."""
    keep = (n // critic_batch_size) * critic_batch_size
    sampler = torch.utils.data.RandomSampler(range(n))
    passes = []
    for _ in range(critic_iters):
        torch.empty((), dtype=torch.int64).random_()  # the DataLoader iterator's base seed
        passes.append(torch.tensor(list(sampler), dtype=torch.int32)[:keep])
    return torch.cat(passes)


def _fit_critic_kernel(params, vfunc_optimizer, epoch_states, epoch_targets, critic_iters,
                       critic_batch_size):
    """All critic_iters passes of the Adam fit in one launch (ops.critic_fit), leaving
    vfunc_optimizer's state as its own steps would: moments in place, step advanced."""
    index = critic_fit_index(epoch_states.shape[0], critic_iters, critic_batch_size)
    n_steps = index.numel() // critic_batch_size
    state = vfunc_optimizer.state
    for p in params:  # a fresh optimizer: the entries Adam itself creates at its first step
        if len(state[p]) == 0:
            state[p]["step"] = torch.tensor(0.0, dtype=_scalar_dtype())
            state[p]["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state[p]["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    g = vfunc_optimizer.param_groups[0]
    first = int(float(state[params[0]]["step"])) + 1
    tensors = ([p.data for p in params] + [state[p]["exp_avg"] for p in params]
               + [state[p]["exp_avg_sq"] for p in params])
    with torch.no_grad():
        loss = ops.critic_fit(epoch_states, epoch_targets.reshape(-1),
                              index.to(epoch_states.device), critic_batch_size, tensors[:6],
                              tensors[6:12], tensors[12:], g["lr"], betas=g["betas"],
                              eps=g["eps"], first_step=first)
        _spread_non_finite(tensors, loss)
    for p in params:
        state[p]["step"] += n_steps
        p.grad = None
    CRITIC_FIT_STATS["kernel_calls"] += 1
    CRITIC_FIT_STATS["steps"] += n_steps


def _spread_non_finite(tensors, loss):
    """Make a fit that met a non-finite value show it as the host loop does.  The kernel's ReLU
    is a select, so a NaN state coordinate leaves every loss finite and only one column of W1
    (and of its moments) NaN, where autograd's loop returns every tensor NaN (mepol_amd.h,
    mepol_critic_fit).  All on the device, no synchronisation: each tensor is multiplied in
    place by 1.0 when every parameter, moment and loss is finite (the same bits) and by NaN when
    one is not, so the next epoch's values are NaN as they would have been."""
    flat = torch.cat([t.reshape(-1) for t in tensors] + [loss.reshape(-1)])
    one = torch.ones((), dtype=flat.dtype, device=flat.device)
    torch._foreach_mul_(tensors, torch.where(torch.isfinite(flat).all(), one, one * float("nan")))


def _scalar_dtype():
    try:
        from torch.optim.optimizer import _get_scalar_dtype

        return _get_scalar_dtype()
    except ImportError:
        return torch.float32


def _fit_critic(vfunc, vfunc_optimizer, optimizer, epoch_states, epoch_targets, critic_reg,
                critic_iters, critic_batch_size):
    """The reference's critic update (trpo.py:426-457).  Its Adam branch runs as one launch
    (ops.critic_fit) over the mini-batches the DataLoader would have drawn when
    kernel_path.critic_fit_ok accepts the critic and its optimizer; else, and for L-BFGS, the
    reference's loop.  CRITIC_FIT_STATS['path'] names the path taken."""
    params = None
    if optimizer != 'lbfgs' and critic_iters >= 1:
        # targets [N, 1], as process_batch returns them: against the critic's [B, 1] output a
        # 1-D target broadcasts to [B, B] in the loop below, which is another loss
        tgt = epoch_targets
        if (tgt.dim() == 2 and tgt.shape[1] == 1 and tgt.is_cuda and tgt.dtype == torch.float64
                and tgt.is_contiguous() and epoch_states.dim() == 2
                and epoch_states.is_contiguous() and tgt.shape[0] == epoch_states.shape[0]):
            params = kernel_path.critic_fit_ok(vfunc, vfunc_optimizer, epoch_states,
                                               critic_batch_size)
    if params is not None:
        CRITIC_FIT_STATS["path"] = "kernel"
        _fit_critic_kernel(params, vfunc_optimizer, epoch_states, epoch_targets, critic_iters,
                           critic_batch_size)
        return
    CRITIC_FIT_STATS["path"] = "host"
    if optimizer == 'lbfgs':
        def compute_vfunc_loss():
            vfunc_optimizer.zero_grad()
            state_values = vfunc(epoch_states)
            params = torch.cat([torch.reshape(w, (-1,)) for w in vfunc.parameters()], dim=0)
            l2 = torch.sum(params ** 2, dim=0)
            loss = torch.mean((state_values - epoch_targets) ** 2) + critic_reg * l2
            loss.backward()
            return loss
        vfunc_optimizer.step(compute_vfunc_loss)
        return
    dataset = torch.utils.data.TensorDataset(epoch_states, epoch_targets)
    dloader = torch.utils.data.DataLoader(dataset, batch_size=critic_batch_size, shuffle=True,
                                          drop_last=True)
    for _ in range(critic_iters):
        vfunc_optimizer.zero_grad()
        for mb_states, mb_targets in dloader:
            vfunc_optimizer.zero_grad()
            loss = torch.mean((vfunc(mb_states) - mb_targets) ** 2)
            loss.backward()
            vfunc_optimizer.step()


def trpo(env_maker, env_name, num_epochs, batch_size, traj_len, gamma=0.995, lambd=0.98,
         vfunc=None, policy=None, optimizer='lbfgs', critic_lr=1e-2, critic_reg=1e-3,
         critic_iters=1, critic_batch_size=64, cg_iters=10, cg_damping=0.1, kl_thresh=0.01,
         num_workers=1, out_path=None, seed=None):
    """The reference's TRPO loop (trpo.py:204-493) on the policy's device in f64, with its
    outputs: <env_name>.csv (Epoch,NumSamples,ExecutionTime,AverageReturn,BacktrackSuccess,
    BacktrackIters), log_file.txt and policy_weights under out_path.  Per epoch: sample
    (collect_sample_batch), one batched critic call over the padded states, process_batch,
    trpo_step, the critic fit.  The critic is moved to the policy's device and f64."""
    from .mepol import _save_policy, _summary_writer

    env = env_maker()
    if not hasattr(env.action_space, "shape") or hasattr(env.action_space, "n"):
        raise NotImplementedError("trpo: continuous action spaces only")
    if seed is None:
        seed = np.random.randint(2 ** 16)
    env.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)

    device = policy.device
    vfunc.to(device=device, dtype=torch.float64)
    if optimizer == 'adam':
        vfunc_optimizer = torch.optim.Adam(vfunc.parameters(), lr=critic_lr)
    elif optimizer == 'lbfgs':
        vfunc_optimizer = torch.optim.LBFGS(vfunc.parameters(), lr=critic_lr, max_iter=25)
    else:
        raise NotImplementedError()

    writer = _summary_writer(out_path)
    log_file = open(os.path.join(out_path, 'log_file.txt'), 'a', encoding="utf-8")
    csv_file_1 = open(os.path.join(out_path, f"{env_name}.csv"), 'w')
    csv_file_1.write(",".join(['Epoch', 'NumSamples', 'ExecutionTime', 'AverageReturn',
                               'BacktrackSuccess', 'BacktrackIters']))
    csv_file_1.write("\n")
    csv_file_1.flush()

    num_samples = 0
    for epoch in range(num_epochs):
        t0 = time.time()
        states, actions, rewards, real_traj_lens, dones = collect_sample_batch(
            env, policy, batch_size, traj_len, num_workers)
        num_traj, _, nf = states.shape
        with torch.no_grad():
            values = vfunc(states.to(torch.float64).reshape(-1, nf)).reshape(num_traj, -1)
        epoch_states, epoch_actions, epoch_targets, epoch_advantages = process_batch(
            states, actions, rewards, real_traj_lens, dones, values, gamma, lambd)
        # rewards behind a trajectory's end are zero
        total_reward = float(rewards.sum(dtype=torch.float64))

        success, backtrack_iters = trpo_step(policy, epoch_states, epoch_actions,
                                             epoch_advantages, kl_thresh, cg_iters=cg_iters,
                                             cg_damping=cg_damping)
        _fit_critic(vfunc, vfunc_optimizer, optimizer, epoch_states, epoch_targets, critic_reg,
                    critic_iters, critic_batch_size)

        num_samples += epoch_states.shape[0]
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        execution_time = time.time() - t0
        average_return = total_reward / num_traj

        writer.add_scalar("Num samples", num_samples, global_step=epoch)
        writer.add_scalar("Execution time (s)", execution_time, global_step=epoch)
        writer.add_scalar("AverageReturn", average_return, global_step=epoch)
        writer.add_scalar("BacktrackSuccess", success, global_step=epoch)
        writer.add_scalar("BacktrackIters", backtrack_iters, global_step=epoch)
        table = [["Epoch", epoch], ["Num samples", num_samples],
                 ["Execution time (s)", f"{execution_time:.3f}"],
                 ["AverageReturn", f"{average_return:.3f}"], ["BacktrackSuccess", success],
                 ["BacktrackIters", backtrack_iters]]
        try:
            from tabulate import tabulate

            fancy_grid = tabulate(table, headers="firstrow", tablefmt="fancy_grid",
                                  numalign='right')
        except ImportError:
            fancy_grid = "\n".join(f"{a}: {b}" for a, b in table)
        print(fancy_grid)
        log_file.write(fancy_grid)
        log_file.flush()
        csv_file_1.write(f"{epoch},{num_samples},{execution_time},{average_return},{success},"
                         f"{backtrack_iters}\n")
        csv_file_1.flush()
        _save_policy(policy, os.path.join(out_path, 'policy_weights'))
    log_file.close()
    csv_file_1.close()
