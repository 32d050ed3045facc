"""What the Gaussian policy's HIP kernel path takes, and its layer chain, each written once for
get_log_p (policy.py), the graph loop (algorithms/device_loop.py), TRPO's Fisher products
(algorithms/trpo.py) and the one-launch rollouts (algorithms/mepol.py).  The gates stay with
those consumers and add what only they know (row floors, dtypes, the optimizer); the gates of
TRPO's samplers (goal_sampler, cut_sampler) are here because they join an env with a policy, and
kernel_env, which says whether an env is the one the kernels step."""
import os

import torch
import torch.nn as nn

from . import ops

# Shape limits of the kernels; ops.py keeps the fused two-layer kernels' own (policy_forward_ok).
MAX_FEATURES = 64                      # input layer: csrc/mlp.hip, csrc/policy_fwd.hip
HEAD_MAX_WIDTH = 512                   # last hidden width of the fused head, csrc/head.hip
HEAD_MAX_ACTIONS = 32
MULTILAYER_MIN, MULTILAYER_MAX = 3, 6  # hidden layers of the deep chain (2 L + 3 <= 16 tensors)
ROLLOUT_MAX_WIDTH = 512                # one-launch rollouts: csrc/envs.hip, csrc/rollout_deep.hip
ROLLOUT_MAX_ACTIONS = 8
ROLLOUT_FEATURES = 2
GRIDWORLD_DEFAULTS = (6, 0.2, 2.5)     # (dim, max_delta, wall_width) the kernels' GridWorld has
# the kernels' MountainCar (csrc/env_step.hpp)
MOUNTAINCAR_FIELDS = ("min_position", "max_position", "max_speed", "goal_position", "power")
MOUNTAINCAR_DEFAULTS = (-1.2, 0.6, 0.07, 0.45, 0.0015)

TWO_LAYER, MULTILAYER = "two-layer", "multilayer"


def linear_layers(policy):
    """The policy's hidden Linear layers, in order (policy.net without its activations)."""
    return [m for m in policy.net if isinstance(m, nn.Linear)]


def network_kind(widths, num_features):
    """The chain that runs hidden layers of these widths: TWO_LAYER (_TwoLayerLogp,
    DeviceIteration), MULTILAYER (3 to 6 layers, all even: 16-B aligned weight rows for the
    matrix-core kernels; hidden_forward / hidden_backward), or None (only the head's kernels)."""
    if num_features > MAX_FEATURES:
        return None
    if len(widths) == 2:
        return TWO_LAYER
    if MULTILAYER_MIN <= len(widths) <= MULTILAYER_MAX and all(w % 2 == 0 for w in widths):
        return MULTILAYER
    return None


def _at(seq, i):
    return None if seq is None else seq[i]


def hidden_forward(x, Ws, bs, hs_out=None, z_out=None):
    """([h_1 .. h_{L-1}], z_L) of L >= 2 hidden layers: h_1 = relu(x W_1^T + b_1) (csrc/mlp.hip),
    h_l = relu(h_{l-1} W_l^T + b_l) and z_L = h_{L-1} W_L^T WITHOUT its bias, as the head kernels
    take it (f64 MFMA GEMM, csrc/gemm.hip, in the tiling ops.gemm_nt_variant gives).  hs_out
    (L - 1 tensors) / z_out: optional buffers for the results (the graph loop's static ones)."""
    n, L = x.shape[0], len(Ws)
    hs = [ops.layer_forward(x, Ws[0], bs[0], out=_at(hs_out, 0))]
    for l in range(1, L - 1):
        hs.append(ops.gemm_nt(hs[-1], Ws[l], bias=bs[l], relu=True, out=_at(hs_out, l),
                              variant=ops.gemm_nt_variant(n, Ws[l].shape[0])))
    zL = ops.gemm_nt(hs[-1], Ws[L - 1], out=z_out,
                     variant=ops.gemm_nt_variant(n, Ws[L - 1].shape[0]))
    return hs, zL


def hidden_backward(dz, x, Ws, hs, dW_out=None, db_out=None, dz_out=None, ws_wgrad=None,
                    ws_hidden=None, ws_layer=None, layer_db_out=None):
    """([dW_1 .. dW_L], [db_1 .. db_{L-1}]) from dz = dL/dz_L, on one stream.  0-based below:
    Ws[l] = W_{l+1} (Ws[0] is not read), hs[l] = h_{l+1}.  For l = L-1 .. 1 the split-K
    dW = dz^T h_{l-1} (csrc/wgrad.hip), then (dz, db) of the layer below (ops.hidden_backward,
    csrc/gemm.hip); then layer 1's dW from dz_1 (its ReLU mask is idempotent on the masked dz_1).
    Optional, indexed by l: dW_out, db_out and dz_out (the layer's own), ws_wgrad and ws_hidden
    (entry 0 unused); ws_layer and layer_db_out are layer 1's scratch and its repeated db_1."""
    L = len(hs) + 1
    dW, db = [None] * L, [None] * (L - 1)
    for l in range(L - 1, 0, -1):
        dW[l] = ops.weight_grad(dz, hs[l - 1], out=_at(dW_out, l), ws=_at(ws_wgrad, l))
        dz, db[l - 1] = ops.hidden_backward(dz, Ws[l], hs[l - 1], ws=_at(ws_hidden, l),
                                            dz_out_buf=_at(dz_out, l - 1),
                                            db_out=_at(db_out, l - 1))
    dW[0], _ = ops.layer_backward(dz, hs[0], x, ws=ws_layer, dW_out=_at(dW_out, 0),
                                  db_out=layer_db_out)
    return dW, db


MOUNTAINCAR, GRIDWORLD, MAZE = 0, 1, 2  # the kernels' env_id
ENV_ACTIONS = (1, 2, 2)                 # action count of each


def kernel_env(base):
    """The kernels' env_id for `base`, MOUNTAINCAR (0) or GRIDWORLD (1), when it is exactly a
    MountainCarContinuous or a GridWorldContinuous (no subclass) with the constants the HIP env
    steps are compiled with (csrc/env_step.hpp), MAZE (2) when it is exactly a BoxMazeContinuous
    (no subclass: its layout is the kernels' argument, see maze_of), else None: every route that
    steps an env inside a kernel asks this first."""
    from .envs.gridworld import GridWorldContinuous
    from .envs.maze import BoxMazeContinuous
    from .envs.mountain_car import MountainCarContinuous

    if type(base) is GridWorldContinuous:
        # the kernel's GridWorld is the default one: its size, step and walls are constants there
        if (base.dim, base.max_delta, base.wall_width) == GRIDWORLD_DEFAULTS:
            return GRIDWORLD
    elif type(base) is MountainCarContinuous:
        # and so are MountainCar's
        if tuple(getattr(base, k) for k in MOUNTAINCAR_FIELDS) == MOUNTAINCAR_DEFAULTS:
            return MOUNTAINCAR
    elif type(base) is BoxMazeContinuous:
        return MAZE
    return None


def maze_of(base, env_id):
    """The `maze=` argument of the ops rollout wrappers: `base` itself for MAZE, else None."""
    return base if env_id == MAZE else None


def goal_sampler(env, policy):
    """(goal, layers) when TRPO's sampler (algorithms/trpo.py collect_sample_batch) takes a
    one-launch goal rollout, else None: an f64 policy on the GPU that
    algorithms.mepol._rollout_layers accepts (a 2 -> [h_1 .. h_L] -> a ReLU MLP, widths <= 512),
    and a CustomRewardEnv directly over
      GridWorldContinuous (the default one, two actions) or a BoxMazeContinuous (any layout)
                          whose reward is a GridGoal (its f32 goal and radius are the kernel's
                          arguments) or a ThresholdGoal, or
      MountainCarContinuous (exactly that type with the kernel's constants, one action) whose
                          reward is a ThresholdGoal (its index, 0 or 1, and threshold are the
                          kernel's arguments).
    goal is that reward object; its type and the env's name the kernel's goal kind and env.
    len(layers) names the kernel: the tuple ((W1, b1), (W2, b2)) for ops.rollout_goal /
    ops.rollout_goal_threshold, a list [(W1, b1), ..., (W_L, b_L)] of 3 to 6 layers for
    ops.rollout_deep_goal / ops.rollout_deep_goal_threshold.  The deep gate has no
    ROLLOUT_DEEP_MAX_WORDS cap: that is where the deep kernel stops beating MEPOL's replayed
    per-step graph, and the sampler's only alternative is the host loop.
    MEPOL_TRPO_SAMPLER=host turns the kernel path off."""
    from .envs.wrappers import CustomRewardEnv, GridGoal, ThresholdGoal

    if os.environ.get("MEPOL_TRPO_SAMPLER", "kernel") == "host":
        return None
    if type(env) is not CustomRewardEnv:
        return None
    goal = env.get_reward
    if isinstance(goal, ThresholdGoal):
        if goal.index not in (0, 1) or goal.threshold != goal.threshold:
            return None
    elif not isinstance(goal, GridGoal):
        return None
    env_id = kernel_env(env.env)
    if env_id is None or (env_id == MOUNTAINCAR and not isinstance(goal, ThresholdGoal)):
        return None
    layers = _sampler_layers(env, policy, env_id)
    return None if layers is None else (goal, layers)


def _sampler_layers(env, policy, env_id):
    """The policy's layers as the one-launch rollouts take them (a tuple of two for
    ops.rollout_mlp and the two-layer goal kernels, a list of 3 to 6 for the deep ones) when it is
    an f64 policy on the GPU with the env's action count, else None: the policy half of
    goal_sampler and cut_sampler."""
    from .algorithms.mepol import _rollout_layers, _rollout_mlp_layers

    a_dim = ENV_ACTIONS[env_id]
    log_std = getattr(policy, "log_std", None)
    if (log_std is None or not log_std.is_cuda or log_std.dtype != torch.float64
            or getattr(policy, "action_dim", None) != a_dim
            or policy.mean.weight.dtype != torch.float64):
        return None
    return (_rollout_mlp_layers(policy, env.num_features, a_dim)
            or _rollout_layers(policy, env.num_features, a_dim, deep=True, word_cap=False))


def cut_sampler(env, policy):
    """(reward, layers, env_id) when TRPO's sampler takes the "roll out, then cut" route, else
    None: a CustomRewardEnv directly over an env kernel_env accepts, whose reward is a
    BatchReward (envs/wrappers.py: a function of the reached state alone, defined for batches),
    and a policy as goal_sampler takes it.  A round is then an UN-terminated one-launch rollout
    (ops.rollout_mlp / ops.rollout_deep), one reward.batch call over its recorded states and
    ops.traj_cut.  It serves every goal the in-kernel kinds do not cover; GridGoal and
    ThresholdGoal are no BatchReward and keep goal_sampler's route, which is tried first.
    MEPOL_TRPO_SAMPLER=host turns this route off too."""
    from .envs.wrappers import BatchReward, CustomRewardEnv

    if os.environ.get("MEPOL_TRPO_SAMPLER", "kernel") == "host":
        return None
    if type(env) is not CustomRewardEnv or not isinstance(env.get_reward, BatchReward):
        return None
    env_id = kernel_env(env.env)
    if env_id is None:
        return None
    layers = _sampler_layers(env, policy, env_id)
    return None if layers is None else (env.get_reward, layers, env_id)


def critic_fit_refusal(vfunc, vfunc_optimizer, states, critic_batch_size):
    """(reason, params) of TRPO's critic-fit gate: reason is None and params the critic's six
    tensors [W1, b1, W2, b2, W3, b3] when the one-launch kernel (ops.critic_fit) takes the fit,
    else reason says in a few words why not and params is None.  The checks run from the
    switch and the network's form to the optimizer and, last, the device."""
    if os.environ.get("MEPOL_CRITIC_FIT", "kernel") == "host":
        return "MEPOL_CRITIC_FIT=host", None
    kinds = (nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear)
    if type(vfunc) is not nn.Sequential or len(vfunc) != len(kinds):
        return "not Linear/ReLU/Linear/ReLU/Linear: layer count", None
    if any(type(m) is not k for m, k in zip(vfunc, kinds)):
        return "not Linear/ReLU/Linear/ReLU/Linear: layer types", None
    l1, l2, l3 = vfunc[0], vfunc[2], vfunc[4]
    if any(l.bias is None for l in (l1, l2, l3)) or l3.out_features != 1:
        return "a layer without bias, or an output wider than 1", None
    nf, h0, h1 = l1.in_features, l1.out_features, l2.out_features
    batch = int(critic_batch_size)
    if not (1 <= nf <= ops.CRITIC_FIT_MAX_FEATURES and 1 <= h0 <= ops.CRITIC_FIT_MAX_WIDTH
            and 1 <= h1 <= ops.CRITIC_FIT_MAX_WIDTH and 1 <= batch <= ops.CRITIC_FIT_MAX_BATCH):
        return "shape outside the kernel's limits", None
    if states.dim() != 2 or states.shape[1] != nf or states.shape[0] < batch:
        return "states do not fit the critic, or hold less than one mini-batch", None
    params = [l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias]
    if states.dtype != torch.float64 or any(p.dtype != torch.float64 for p in params):
        return "dtype is not float64", None
    if type(vfunc_optimizer) is not torch.optim.Adam:
        return "optimizer is not torch.optim.Adam", None
    if len(vfunc_optimizer.param_groups) != 1:
        return "more than one parameter group", None
    g = vfunc_optimizer.param_groups[0]
    if len(g["params"]) != 6 or any(a is not b for a, b in zip(g["params"], params)):
        return "the optimizer does not hold exactly the critic's tensors", None
    if (tuple(g["betas"]) != (0.9, 0.999) or g["eps"] != 1e-8
            or not isinstance(g["lr"], (int, float))):
        return "betas, eps or lr are not Adam's plain defaults", None
    if g["weight_decay"] != 0 or g.get("decoupled_weight_decay", False):
        return "weight decay", None
    if g["amsgrad"]:
        return "amsgrad", None
    if g["maximize"] or g.get("capturable", False):
        return "maximize or capturable", None
    # the optimizer's state: none yet, or Adam's own for all six tensors at one step number
    st = [vfunc_optimizer.state.get(p, {}) for p in params]
    if any(len(s) for s in st):
        if (any(set(s) != {"step", "exp_avg", "exp_avg_sq"} for s in st)
                or len({float(s["step"]) for s in st}) != 1):
            return "optimizer state is not Adam's at one step number", None
        for s, p in zip(st, params):
            for t in (s["exp_avg"], s["exp_avg_sq"]):
                if (t.dtype != p.dtype or t.device != p.device or t.shape != p.shape
                        or not t.is_contiguous()):
                    return "optimizer moments do not match the parameters", None
    if (not states.is_cuda or any(p.device != states.device for p in params)
            or not all(p.is_contiguous() for p in params)):
        return "not on the GPU (or not contiguous)", None
    return None, params


def critic_fit_ok(vfunc, vfunc_optimizer, states, critic_batch_size):
    """The critic's six tensors [W1, b1, W2, b2, W3, b3] when TRPO's critic fit
    (algorithms/trpo.py _fit_critic) takes the one-launch kernel (ops.critic_fit), else None: an
    nn.Sequential of exactly Linear / ReLU / Linear / ReLU / Linear(., 1) within the kernel's
    limits, f64 on the GPU like the states; a torch.optim.Adam with one parameter group holding
    exactly those tensors, default betas and eps, no weight decay, amsgrad and maximize off, not
    capturable.  MEPOL_CRITIC_FIT=host turns the kernel path off.  critic_fit_refusal gives the
    reason."""
    return critic_fit_refusal(vfunc, vfunc_optimizer, states, critic_batch_size)[1]
