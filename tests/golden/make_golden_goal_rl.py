"""Generate tests/golden/goal_rl_*.npz by running the REFERENCE's TRPO batch code.

Test infrastructure only, beside make_golden.py and with the same shims (ref_stubs.install):

    python tests/golden/make_golden_goal_rl.py

It no-ops when the reference is absent.  Only inputs and the outputs the reference produced are
written.

  goal_rl_process_traj.npz   process_traj (src/algorithms/trpo.py:175-201) on numpy inputs:
                             several lengths, terminated (boot 0) and bootstrapped.
  goal_rl_budget.npz         collect_sample_batch (:86-157, one worker) on a scripted env with
                             fixed episode lengths and a policy whose predict returns zeros: the
                             real_traj_lens, dones and step count it returns.

Two shims are local to this file: the stub gym.spaces has no Discrete (trpo.py:106 names it),
and trpo.py:116 uses np.bool, which numpy removed.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

GAMMA, LAMBD = 0.995, 0.98
NEVER = 10 ** 6  # an episode that does not terminate inside any traj_len used here

# (episode lengths in the order the env plays them, traj_len, batch_size)
BUDGET_CASES = {
    "cut_midway": ([5, 7, NEVER, 3], 20, 25),        # third trajectory cut after 13 steps
    "cut_on_termination": ([4, 6, 9], 20, 10),       # budget reached as episode 2 terminates
    "exact_at_traj_len": ([NEVER, NEVER, 2], 5, 10),  # budget reached as trajectory 2 times out
    "below_first": ([9, 4], 20, 3),                  # first trajectory cut
    "many": ([3, NEVER, 1, 1, 8, NEVER, 2, 5, NEVER, 4], 12, 50),
}


def _save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"wrote {name}: {os.path.getsize(path) / 1e3:.1f} kB")


def gen_process_traj(T):
    rng = np.random.default_rng(20)
    out = {"gamma": np.array(GAMMA), "lambd": np.array(LAMBD)}
    for c, (n, done) in enumerate([(1, True), (1, False), (5, True), (5, False), (37, False),
                                   (130, True), (130, False)]):
        rewards = np.zeros(n, dtype=np.float32)
        if done:
            rewards[-1] = 1  # the sparse goal reward
        else:
            rewards[:] = rng.standard_normal(n).astype(np.float32)  # a dense one
        vfuncs = rng.standard_normal(n)
        boot = 0 if done else float(rng.standard_normal())
        states = np.zeros((n, 2), dtype=np.float32)
        actions = np.zeros((n, 2), dtype=np.float32)
        targets, advantages = T.process_traj(GAMMA, LAMBD, vfuncs, states, actions, rewards, boot)
        assert targets.dtype == np.float32 and advantages.dtype == np.float32
        out.update({f"c{c}_rewards": rewards, f"c{c}_vfuncs": vfuncs,
                    f"c{c}_boot": np.array(float(boot)), f"c{c}_done": np.array(done),
                    f"c{c}_targets": targets, f"c{c}_advantages": advantages})
    out["num_cases"] = np.array(c + 1)
    _save("goal_rl_process_traj.npz", **out)


class _ScriptedEnv:
    """Episodes of the given lengths, one after another; done (a Python bool, as the
    reference's `done is True` needs) on an episode's last step."""

    def __init__(self, ep_lens, Box):
        self.ep_lens = list(ep_lens)
        self.episode = -1
        self.num_features = 2
        self.action_space = Box(-np.ones(2, dtype=np.float32), np.ones(2, dtype=np.float32))

    def reset(self):
        self.episode += 1
        self.t = 0
        return np.zeros(2, dtype=np.float32)

    def step(self, a):
        self.t += 1
        done = self.t >= self.ep_lens[self.episode]
        return np.full(2, self.t, dtype=np.float32), (1 if done else 0), done, {}


class _ZeroPolicy:
    def predict(self, s):
        import torch

        return torch.zeros(2)


def gen_budget(T, Box):
    out = {}
    for name, (ep_lens, traj_len, batch_size) in BUDGET_CASES.items():
        env = _ScriptedEnv(ep_lens, Box)
        states, actions, rewards, lens, dones = T.collect_sample_batch(env, _ZeroPolicy(),
                                                                       batch_size, traj_len)
        assert states.shape[0] == lens.shape[0] == dones.shape[0]
        out.update({f"{name}_ep_lens": np.array(ep_lens, dtype=np.int64),
                    f"{name}_traj_len": np.array(traj_len), f"{name}_batch_size": np.array(batch_size),
                    f"{name}_real_traj_lens": lens.astype(np.int32),
                    f"{name}_dones": dones.astype(np.bool_),
                    f"{name}_steps": np.array(int(lens.sum())),
                    f"{name}_reward_sum": np.array(float(rewards.sum()))})
    out["names"] = np.array(list(BUDGET_CASES))
    _save("goal_rl_budget.npz", **out)


def main():
    sys.path.insert(0, HERE)
    import ref_stubs
    from make_golden import REF  # where the reference lives

    if not os.path.isdir(REF):
        print("reference not present; nothing to do")
        return
    ref_stubs.install(REF)
    spaces = sys.modules["gym.spaces"]
    if not hasattr(spaces, "Discrete"):
        spaces.Discrete = type("Discrete", (), {})
    if not hasattr(np, "bool"):
        np.bool = np.bool_

    import src.algorithms.trpo as T

    gen_process_traj(T)
    gen_budget(T, spaces.Box)


if __name__ == "__main__":
    main()
