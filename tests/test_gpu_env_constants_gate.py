"""collect_particles_device takes the HIP-stepped routes only for the envs the kernels are compiled
for (kernel_path.kernel_env): a GridWorld of another size is stepped on the host with its own
constants, the default one still rolls out in one launch with the bits a direct kernel call gives
for the same draws."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _policy(seed=5):
    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(seed)
    return GaussianPolicy([36, 64], 2, 2, -1.5).cuda()


def test_gridworld_of_another_size_is_stepped_with_its_own_constants(cuda):
    """dim = 8: every start lies outside the kernels' 6 x 6 grid, where no step would ever be
    accepted and the states would stay constant."""
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.envs import ErgodicEnv, GridWorldContinuous

    base = GridWorldContinuous(dim=8)
    env = ErgodicEnv(base)
    env.seed(3)
    states, actions, lens, nxt = M.collect_particles_device(env, _policy(), 2, 5, None)
    assert states.shape == (2, 6, 2) and actions.shape == (2, 5, 2) and nxt.shape == (10, 2)
    assert states.dtype == torch.float32 and lens.reshape(-1).tolist() == [5, 5]
    S = states.cpu().numpy().astype(np.float64)
    assert (S[:, 0] >= -8).all() and (S[:, 0] <= -6).all()         # the env's own start box
    assert (np.abs(S[:, -1] - S[:, 0]).max(axis=-1) > 0).all()      # they leave their starts
    assert (np.abs(S) < 8).all()                                    # and stay inside the grid
    step = np.abs(np.diff(S, axis=1))
    assert step.max() <= base.max_delta + float(np.spacing(np.float32(8)))
    assert np.array_equal(nxt.cpu().numpy(), states[:, 1:].reshape(-1, 2).cpu().numpy())
    with pytest.raises(NotImplementedError):                        # as for any host-stepped env
        M.collect_particles_device(env, _policy(), 2, 5, None, shard=(0, 2))


@pytest.mark.parametrize("env_name", ["gridworld", "mountaincar"])
def test_default_envs_still_take_the_one_launch_kernel(cuda, env_name):
    from mepol_amd import ops
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.envs import ErgodicEnv, GridWorldContinuous, MountainCarContinuous
    from mepol_amd.policy import GaussianPolicy

    env_id, a = (1, 2) if env_name == "gridworld" else (0, 1)
    base = GridWorldContinuous() if env_id else MountainCarContinuous()
    torch.manual_seed(5)
    pol = GaussianPolicy([36, 64], 2, a, -1.5 if env_id else -0.5).cuda()
    n, T = 3, 7
    gen = torch.Generator(device="cuda").manual_seed(11)
    states, actions, _, _ = M.collect_particles_device(ErgodicEnv(base), pol, n, T, None,
                                                       generator=gen)
    # the kernel route's draws, in its order, and the kernel itself
    gen = torch.Generator(device="cuda").manual_seed(11)
    init = base.reset_batch_torch(n, pol.device, gen)
    noise = torch.randn((T, n, a), dtype=torch.float64, device="cuda", generator=gen)
    S = torch.zeros((n, T + 1, 2), dtype=torch.float32, device="cuda")
    A = torch.zeros((n, T, a), dtype=torch.float32, device="cuda")
    (l1, l2) = [m for m in pol.net if isinstance(m, torch.nn.Linear)]
    ops.rollout_mlp(env_id, l1.weight.detach(), l1.bias.detach(), l2.weight.detach(),
                    l2.bias.detach(), pol.mean.weight.detach(), pol.mean.bias.detach(),
                    pol.log_std.detach(), init, noise, S, A)
    assert torch.equal(states, S) and torch.equal(actions, A)
    assert bool((S[:, 1:] != S[:, :-1]).any())
