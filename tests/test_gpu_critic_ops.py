"""TRPO's critic-fit kernel (ops.critic_fit, csrc/critic_fit.hip) shape by shape.

Every op-level case of tests/critic_cases.py goes through mepol_amd.ops with the runners that
tests/test_critic_cases_host.py applies to the CPU stand-ins: one step at every shape where the
launch arithmetic changes, each output within its derived m u0 A bound of the np.longdouble
reference, under three sets of Adam scalars and from zero moments; small integers with planted
zero pre-activations bit for bit; every tensor of a call carved out of one 0xff-filled buffer with
guard words; loss_out = NULL; split launches against one launch, bit for bit; the prefetch
boundaries of 1 to 4 steps; non-finite data in rows that are and are not read; chains of 8 and
40 steps within 100 x the spread between two references.  The host file asserts what the case
list covers and that each planted mistake fails here.  The largest error / bound per output is
printed by the last test (recorded in profiles/r20/critic_ops/README.md).
"""
import ctypes

import numpy as np
import pytest
import torch

import critic_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from mepol_amd import ops as gpu_ops

    for k in [k for k in C.RATIOS if k.startswith("critic_fit.")]:
        del C.RATIOS[k]   # what the host file recorded in this process: the last test prints the GPU's
    C.CHAIN_DEVIATIONS.clear()
    return gpu_ops


@pytest.mark.parametrize("group", list(C.SHAPE_GROUPS))
def test_one_step_within_the_derived_bounds(cuda, ops, group):
    for shape in C.SHAPE_GROUPS[group]:
        for variant in C.VARIANTS:
            C.run_one_step(ops, cuda, shape, variant)


def test_planted_zero_pre_activations_bit_for_bit(cuda, ops):
    C.run_exact(ops, cuda)


@pytest.mark.parametrize("shape,variant", C.CANARY_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_nothing_is_written_next_to_a_tensor(cuda, ops, shape, variant):
    got = C.run_canary(ops, cuda, C.one_step_case(shape, variant))
    C.check_step("canary", got, C.one_step_reference(shape, variant))


def test_nothing_is_written_next_to_a_tensor_over_five_steps(cuda, ops):
    C.run_canary(ops, cuda, C.steps_case("split_ragged"))


@pytest.mark.parametrize("name", ("split_ragged", "exact"))
def test_null_loss_out_changes_no_other_bit(cuda, ops, name):
    """loss_out = NULL through the C entry point (ops.critic_fit always passes a buffer)."""
    from mepol_amd._lib import call, ptr

    c = C.steps_case(name) if name != "exact" else C.exact_case()
    want = C.launch(ops, cuda, c)
    lr, betas, eps = C.scalars(c)
    dev = lambda a: torch.from_numpy(np.array(a, copy=True)).to(cuda)
    states, targets, index = dev(c["states"]), dev(c["targets"]), dev(c["index"])
    p, m, v = ([dev(a) for a in c[k]] for k in ("params", "m", "v"))
    n_steps = c["index"].size // c["B"]
    scal = ops.adam_step_scalars(lr, betas, c["first_step"], n_steps).to(cuda)
    arr = ctypes.c_void_p * 6
    call("mepol_critic_fit", ptr(states), ptr(targets), c["N"], ptr(index), n_steps, c["B"],
         c["nf"], c["h0"], c["h1"], arr(*[t.data_ptr() for t in p]),
         arr(*[t.data_ptr() for t in m]), arr(*[t.data_ptr() for t in v]), ptr(scal),
         float(betas[0]), float(betas[1]), float(eps), None, ops._stream())
    torch.cuda.synchronize()
    got = {"params": [t.cpu().numpy() for t in p], "m": [t.cpu().numpy() for t in m],
           "v": [t.cpu().numpy() for t in v], "loss": want["loss"]}
    assert C.same_bits(got, want)


@pytest.mark.parametrize("name", C.SPLIT_NAMES)
def test_two_launches_equal_one(cuda, ops, name):
    C.run_split(ops, cuda, name)


@pytest.mark.parametrize("name", C.SPLIT_NAMES)
def test_every_step_fits_its_own_batch(cuda, ops, name):
    C.run_prefetch(ops, cuda, name)


def test_non_finite_state_rows_that_no_index_reads_change_nothing(cuda, ops):
    assert C.same_bits(C.launch(ops, cuda, C.steps_case("unread_clean")),
                       C.launch(ops, cuda, C.steps_case("unread_nonfinite")))


@pytest.mark.parametrize("name", list(C.NONFINITE))
def test_non_finite_row_that_is_read(cuda, ops, name):
    C.run_nonfinite(ops, cuda, name)


@pytest.mark.parametrize("name", C.CHAIN_NAMES)
def test_chain_within_100x_the_references_spread(cuda, ops, name):
    """The 8-step chains run with eps = 0: a padded element's Adam update is then 0 / 0, which
    must not reach the next step (it did: profiles/r20/critic_ops/README.md)."""
    C.run_chain(ops, cuda, name)


def test_driver_surfaces_a_nan_state_as_the_host_loop_does(cuda, monkeypatch):
    """ops.critic_fit on a NaN state coordinate returns finite losses and one NaN column
    (nan_state above); _fit_critic's kernel path must leave what the host loop leaves: every
    parameter and moment NaN, so the next epoch's values show it."""
    from mepol_amd.algorithms import trpo as TR
    from mepol_amd.experiments.goal_rl import create_critic

    for path in ("kernel", "host"):
        monkeypatch.setenv("MEPOL_CRITIC_FIT", path)
        torch.manual_seed(31)
        vfunc = create_critic(2).to(device=cuda, dtype=torch.float64)
        opt = torch.optim.Adam(vfunc.parameters(), lr=1e-2)
        g = torch.Generator().manual_seed(32)
        states = torch.rand(128, 2, generator=g, dtype=torch.float64).cuda()
        targets = torch.randn(128, 1, generator=g, dtype=torch.float64).cuda()
        states[17, 1] = float("nan")
        torch.manual_seed(79)
        TR._fit_critic(vfunc, opt, "adam", states, targets, 1e-3, 1, 64)  # both batches: 128 rows
        assert TR.CRITIC_FIT_STATS["path"] == path
        for p in vfunc.parameters():
            assert torch.isnan(p).all(), path
            assert torch.isnan(opt.state[p]["exp_avg"]).all(), path
            assert torch.isnan(opt.state[p]["exp_avg_sq"]).all(), path
        with torch.no_grad():
            assert torch.isnan(vfunc(torch.rand(4, 2, dtype=torch.float64, device=cuda))).all()


def test_print_the_largest_error_over_bound_per_output(cuda):
    ratios = {k: v for k, v in C.RATIOS.items() if k.startswith("critic_fit.")}
    for k in sorted(ratios):
        print(f"GPU: {k:40s} {ratios[k]:.3f}")
    for name, (d, rel, atol, rtol) in C.CHAIN_DEVIATIONS.items():
        print(f"GPU: {name}: deviation {d:.3e} (allowed {atol:.3e}), loss {rel:.3e} ({rtol:.3e})")
    assert all(v <= 1.0 for v in ratios.values())
