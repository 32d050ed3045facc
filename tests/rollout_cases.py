"""Cases for the rollout kernels (csrc/envs.hip: rollout_step_kernel, rollout_mlp_kernel,
rollout_mlp_mw_kernel with its goal instances; csrc/rollout_deep.hip), shared by
test_rollout_cases_host.py (CPU: the cases are what they claim) and test_gpu_rollout_ops.py (the
kernels against the oracle's k-ordered rollout).  Tiny on purpose: n = 3 trajectories of T = 12
steps unless a family says otherwise.

Also a small model of the kernels' loop bounds (mw_model, kl_model), so that the host test can
prove which code paths a shape reaches, and the MountainCar margin calculation: a row or a
trajectory step whose pre-clamp value lies within 1e-9 of a threshold could take another branch
after a last-ulp difference in cos(), and is not allowed in a case."""
import functools
import math

import numpy as np
import torch

from oracle import mepol_oracle as O

N, T = 3, 12
ENVS = ("mountaincar", "gridworld")
K_CHUNKS = 4          # both kernel forms (ops.rollout_mlp_plan reports it; the GPU test asserts it)
MW_MAX_H0 = 306       # the multi-workgroup form's LDS limit (envs.hip: kRollMwMaxH0)
MAX_H = 512           # kRollMaxH
MARGIN = 1e-9

SHAPES = [(1, 1), (2, 130), (3, 64), (4, 65), (5, 65), (9, 7), (28, 64), (29, 1), (32, 128),
          (36, 64), (60, 65), (68, 192), (96, 512), (64, 512), (306, 64), (307, 64), (512, 1),
          (512, 512)]


# ---- the kernels' loop bounds ----------------------------------------------------------------
def mw_model(h0, h1, a_dim=2):
    """rollout_mlp_mw_kernel's bounds for a [h0, h1] policy: L rows per wave, the four waves'
    lengths, np parts, nw waves of the one-workgroup form, the last part's columns, the K loop's
    path per wave ("lt8": tail only, "one": the primed batch alone, "pipe": the prefetch loop runs)
    with its tail rows, and whether the host accepts the form."""
    L = -(-h0 // 4)
    lens = [min(min(w * L, h0) + L, h0) - min(w * L, h0) for w in range(4)]
    np_ = -(-h1 // 64)
    nw = -(-max(h0, h1) // 64)

    def path(n):
        return ("lt8" if n < 8 else "one" if n < 16 else "pipe", n % 8)

    return dict(L=L, lens=lens, np=np_, nw=nw, last_cols=h1 - 64 * (np_ - 1),
                paths=[path(n) for n in lens], words=np_ * a_dim,
                accepted=h0 <= MW_MAX_H0 and np_ * a_dim <= 64)


def kl_effective(h0, h1, kl):
    """The W2^T rows rollout_mlp_kernel keeps in LDS under MEPOL_ROLLOUT_KL = kl (150 KB cap)."""
    threads = -(-max(h0, h1) // 64) * 64
    cap = (150 * 1024) // (threads * 8)
    return max(0, min(cap, kl, h0))


def kl_model(h0, h1, kl):
    """Per chunk of rollout_mlp_kernel's layer-2 sum: (rows from LDS, full batches of 8 streamed
    rows, streamed tail rows)."""
    KL = kl_effective(h0, h1, kl)
    L = -(-h0 // K_CHUNKS)
    out = []
    for r in range(K_CHUNKS):
        ka = min(r * L, h0)
        kb = min(ka + L, h0)
        lds = max(0, min(kb, KL) - ka)
        rest = (kb - ka) - lds
        out.append((lds, rest // 8, rest % 8))
    return out


# ---- MountainCar margins ---------------------------------------------------------------------
def mc_margins(S, A):
    """For MountainCar steps from states S [m, 2] (f64) with actions A [m]: the smallest distance
    of a pre-clamp value from a threshold it is compared with, per row, and which clamps fire
    (dict of bool [m]).  NaN actions are skipped (margin inf)."""
    p, v, a = S[:, 0].astype(np.float64), S[:, 1].astype(np.float64), np.asarray(A, np.float64)
    with np.errstate(invalid="ignore"):
        force = np.minimum(np.maximum(a, -1.0), 1.0)
        v1 = v + (force * 0.0015 - 0.0025 * np.cos(3 * p))
        vc = np.minimum(np.maximum(v1, -0.07), 0.07)
        p1 = p + vc
        pc = np.minimum(np.maximum(p1, -1.2), 0.6)
        at_min = pc == -1.2
        d = np.minimum.reduce([np.abs(v1 - 0.07), np.abs(v1 + 0.07), np.abs(p1 - 0.6),
                               np.abs(p1 + 1.2), np.abs(pc - 0.45),
                               np.where(at_min & (vc != 0.0), np.abs(vc), np.inf)])
        # a start exactly at a clamp value that is carried through unchanged is not a comparison
        # that cos() can disturb: p1 == threshold only when v is exactly 0 there
        fired = dict(vmax=v1 > 0.07, vmin=v1 < -0.07, pmax=p1 > 0.6, pmin=p1 < -1.2,
                     reset=at_min & (vc < 0), goal=pc > 0.45)
    d = np.where(np.isnan(a), np.inf, d)
    return d, fired


# ---- policies and cases ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def policy(hidden, a_dim, log_std, seed=11):
    """A CPU GaussianPolicy with the mean layer scaled as test_gpu_goal_rl._scaled_policy scales
    it (the untouched random policy parks GridWorld against the outer wall)."""
    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(seed)
    pol = GaussianPolicy(list(hidden), 2, a_dim, log_std)
    with torch.no_grad():
        pol.mean.weight.mul_(0.02)
        pol.mean.bias.fill_(0.05)
    return pol


def state_dict(pol):
    return {k: v.detach().cpu().numpy() for k, v in pol.state_dict().items()}


def _init(env, n, rng):
    """Starts spread over the state space (opposite quadrants / both slopes), so that a layer-1
    unit that is dead on one trajectory fires on another."""
    if env == "mountaincar":
        base = np.array([[-0.9, 0.02], [0.3, -0.03], [-0.5, 0.0]])
        return (base[:n] + rng.uniform(-0.02, 0.02, (n, 2)) * [1.0, 0.1]).astype(np.float64)
    base = np.array([[-5.0, -4.5], [4.6, 4.9], [4.3, -4.8]])
    return (base[:n] + rng.uniform(-0.2, 0.2, (n, 2))).astype(np.float32)


def make_case(name, env, hidden, a_dim=None, n=N, steps=T, seed=0, init=None, noise=None, **extra):
    if a_dim is None:
        a_dim = 1 if env == "mountaincar" else 2
    rng = np.random.default_rng(1000 + seed)
    init = _init(env, n, rng) if init is None else init
    noise = rng.standard_normal((steps, n, a_dim)) if noise is None else noise
    case = dict(name=name, env=env, hidden=tuple(hidden), a_dim=a_dim, n=n, T=steps,
                log_std=-0.5 if env == "mountaincar" else -1.5, init=init, noise=noise, **extra)
    init.setflags(write=False)
    noise.setflags(write=False)
    return case


_POLICIES = {}


def case_policy(case):
    """The case's policy: policy() with the biases of hidden units that are dead at every start
    state (below 0.01) raised until they fire at one (about half the units of a random policy
    never fire on MountainCar's small states, and a row or column that only ever meets a zero is
    not tested).
    Units that fire somewhere keep their bias, so ReLU still clamps on the other trajectories."""
    key = (case["hidden"], case["a_dim"], case["log_std"], case["init"].tobytes())
    if key not in _POLICIES:
        import copy

        pol = copy.deepcopy(policy(case["hidden"], case["a_dim"], case["log_std"]))
        h = torch.as_tensor(case["init"].astype(np.float64))
        with torch.no_grad():
            for lin in pol.net:
                if not isinstance(lin, torch.nn.Linear):
                    continue
                top = (h @ lin.weight.t() + lin.bias).max(dim=0).values
                dead = top < 0.01
                lin.bias[dead] += lin.bias[dead].abs() - top[dead] + 0.01
                h = torch.relu(h @ lin.weight.t() + lin.bias)
        _POLICIES[key] = pol
    return _POLICIES[key]


def hidden_activity(case):
    """Per hidden layer, max over the start states of each unit's activation (numpy order)."""
    sd = state_dict(case_policy(case))
    h, out, i = case["init"].astype(np.float64), [], 0
    while f"net.{i}.weight" in sd:
        h = np.maximum(h @ sd[f"net.{i}.weight"].T + sd[f"net.{i}.bias"], 0.0)
        out.append(h.max(axis=0))
        i += 2
    return out


def oracle(case, std=None, noise=None):
    """(S f32 [n, T+1, 2], A f32 [n, T, a]) of O.rollout_kordered with the kernels' k_chunks; std
    defaults to numpy's exp(log_std) (the GPU tests pass the device's)."""
    sd = state_dict(case_policy(case))
    std = np.exp(sd["log_std"]) if std is None else std
    return O.rollout_kordered(case["env"], sd, std, case["init"],
                              case["noise"] if noise is None else noise, case["T"], K_CHUNKS)


def shapes_cases():
    return [make_case(f"shapes-{env[:2]}-{h0}x{h1}", env, (h0, h1), seed=i)
            for env in ENVS for i, (h0, h1) in enumerate(SHAPES)]


KL_H1 = 65


def kl_settings(h0):
    L = -(-h0 // K_CHUNKS)
    # the issue's set, and 2: the only setting here that leaves a chunk exactly one streamed batch
    return sorted({0, 1, 2, L - 1, L, L + 1, h0 - 1, h0})


def kl_cases():
    return [make_case(f"kl-{h0}-{kl}", "gridworld", (h0, KL_H1), seed=40 + h0, kl=kl)
            for h0 in (37, 300) for kl in kl_settings(h0)]


def adim_cases():
    return [make_case(f"adim-{h0}x{h1}-a{a}-T{steps}", "mountaincar", (h0, h1), a_dim=a,
                      steps=steps, seed=60 + a)
            for (h0, h1) in ((5, 65), (64, 512)) for a in (1, 3, 8) for steps in (T, 1)]


def short_cases():
    return [make_case(f"short-{env[:2]}-T{steps}-n{n}", env, (36, 64), n=n, steps=steps,
                      seed=80 + 2 * steps + n)
            for env in ENVS for steps in (1, 2) for n in (1, 3)]


# ---- env_edges: starts from the boundary fixtures' rows --------------------------------------
def _golden(name):
    from conftest import load_golden

    return load_golden(name)


def _row(z, label):
    (i,) = np.flatnonzero(z["name"] == label)
    return z["S"][i]


BIG = 50.0  # noise that saturates the action clip whatever the policy's mean is


def env_edges_cases(hidden=(36, 64)):
    """Two MountainCar and one GridWorld case whose trajectories meet every clamp / the walls
    within T steps; `hidden` is the policy (the deep rollout runs them with three layers)."""
    mc, gw = _golden("env_mc_edges"), _golden("env_gw_edges")
    rng = np.random.default_rng(7)
    out = []
    # a: into the left wall and its reset; over the goal; velocity clamp from below +0.07
    init = np.stack([_row(mc, "pmin/past"), np.array([0.40, 0.07]), np.array([-0.5, 0.0699])])
    noise = rng.standard_normal((T, N, 1))
    noise[:, 0, 0] = -BIG
    noise[:, 1, 0] = BIG
    noise[:, 2, 0] = BIG
    out.append(make_case("env_edges-mc-a", "mountaincar", hidden, init=init, noise=noise))
    # b: velocity clamp from above -0.07 then the left wall; past the right end; off the left wall
    init = np.stack([np.array([-0.5, -0.0699]), _row(mc, "pmax/past"),
                     _row(mc, "pmin/start_v_pos")])
    noise = rng.standard_normal((T, N, 1))
    noise[:, 0, 0] = -BIG
    noise[:, 1, 0] = BIG
    out.append(make_case("env_edges-mc-b", "mountaincar", hidden, init=init, noise=noise))
    # GridWorld: one moved step from a wall side and from x = 6, bumping and retreating in turn;
    # and down through the west door
    init = np.stack([_row(gw, "wall0/side_x0"), _row(gw, "bound/on_x+"),
                     _row(gw, "door/W/enter")]).astype(np.float32)
    noise = rng.standard_normal((T, N, 2))
    noise[:, 0, 0] = BIG * (-1.0) ** np.arange(T)
    noise[:, 1, 0] = BIG * (-1.0) ** np.arange(T)
    noise[:, 2, 1] = -BIG
    out.append(make_case("env_edges-gw", "gridworld", hidden, init=init, noise=noise))
    return out


def f64_rollout(case):
    """MountainCar in f64 with the numpy MLP (its summation order differs from the kernels' by
    ~1e-16 in the action: nothing against MARGIN): states [T+1, n, 2] and actions [T, n]."""
    sd = state_dict(case_policy(case))
    std = np.exp(sd["log_std"])
    s = case["init"].astype(np.float64)
    S, A = [s], []
    for t in range(case["T"]):
        a = O.mlp_mean(sd, s) + case["noise"][t] * std
        s = O.mountaincar_step(s, a)
        S.append(s)
        A.append(a[:, 0])
    return np.stack(S), np.stack(A)


# ---- nan_action ------------------------------------------------------------------------------
NAN_STEP, NAN_TRAJ = 4, 1


def nan_cases():
    out = []
    for env in ENVS:
        c = make_case(f"nan_action-{env[:2]}", env, (36, 64), seed=90)
        noise = c["noise"].copy()
        noise[NAN_STEP, NAN_TRAJ, 0] = np.nan  # numpy's default NaN: 0x7ff8000000000000
        noise.setflags(write=False)
        c["noise_nan"] = noise
        # the coordinates the reference's step turns NaN for a NaN first action component
        c["nan_coords"] = (0, 1) if env == "mountaincar" else (0,)
        out.append(c)
    return out


# ---- goal ------------------------------------------------------------------------------------
GOAL_T = 6
GOAL_OFF = np.array([0.03125, -0.0625], dtype=np.float32)


def goal_distance(s, goal):
    """sqrt(dx^2 + dy^2) in f32, every operation rounded on its own (envs.hip: goal_hit)."""
    d = np.asarray(s, np.float32) - np.asarray(goal, np.float32)
    q = np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])
    return np.sqrt(np.float32(q))


def goal_cases():
    return [make_case(f"goal-{h0}x{h1}", "gridworld", (h0, h1), seed=95) for h0, h1 in
            ((5, 65), (64, 48))]


def goal_settings(S):
    """[(label, goal f32 [2], radius, trajectory 0 ends at GOAL_T?)] for an oracle rollout S."""
    at = S[0, GOAL_T]
    goal = (at + GOAL_OFF).astype(np.float32)
    d = float(goal_distance(at, goal))
    assert d > 0 and math.isfinite(d)
    return [("radius=d", goal, d, True), ("radius<d", goal, float(np.nextafter(d, 0.0)), False),
            ("radius=0", at.copy(), 0.0, True)]
