"""mepol_traj_cut on the GPU against the numpy restatement (traj_cut_cases.cut_reference), bit for
bit on every case of the table: uint32 views, so NaN payloads and signed zeros count, and the
inputs hold 0xffffffff behind every end, so only zeros the kernel wrote pass."""
import numpy as np
import pytest
import torch

import traj_cut_cases as TC

pytestmark = pytest.mark.gpu


def _run(ops, c, done=None):
    d = torch.tensor(c.done if done is None else done, device="cuda")
    R, S, A = (torch.tensor(x, device="cuda") for x in (c.R, c.S, c.A))
    lens, dones = ops.traj_cut(d, R, S, A)
    return R, S, A, lens, dones


def _assert_equal(got, want, name):
    for key, g, w in zip(("rewards", "states", "actions", "len", "done"), got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, key)
        assert np.array_equal(TC.bits(g), TC.bits(w)), (name, key, int((TC.bits(g) != TC.bits(w)).sum()))


@pytest.mark.parametrize("key", TC.case_keys(), ids=TC.case_ids())
def test_traj_cut_matches_the_restatement(cuda, key):
    from mepol_amd import ops

    c = TC.case(*key)
    want = TC.cut_reference(c.done, c.R, c.S, c.A)
    assert np.array_equal(want[3], c.lens) and np.array_equal(want[4], c.dones)
    got = _run(ops, c)
    _assert_equal(got, want, c.name)
    # a second call on its own output changes nothing
    R, S, A, lens, dones = got
    lens2, dones2 = ops.traj_cut(torch.tensor(c.done, device="cuda"), R, S, A)
    _assert_equal((R, S, A, lens2, dones2), want, c.name + " (second call)")


def test_traj_cut_takes_a_bool_mask_and_checks_its_arguments(cuda):
    from mepol_amd import ops

    c = TC.case(3, 65, 2)
    want = TC.cut_reference(c.done, c.R, c.S, c.A)
    _assert_equal(_run(ops, c, done=c.done != 0), want, "bool")
    d = torch.tensor(c.done, device="cuda")
    R, S, A = (torch.tensor(x, device="cuda") for x in (c.R, c.S, c.A))
    with pytest.raises(ValueError, match="ROCm device"):
        ops.traj_cut(d.cpu(), R, S, A)
    with pytest.raises(ValueError, match="shapes"):
        ops.traj_cut(d[:, :-1].contiguous(), R, S, A)
    with pytest.raises(ValueError, match="shapes"):
        ops.traj_cut(d, R, S[:, :-1].contiguous(), A)
    with pytest.raises(ValueError, match="bool or uint8"):
        ops.traj_cut(d.to(torch.int32), R, S, A)
    with pytest.raises(ValueError, match="bool or uint8"):
        ops.traj_cut(d, R.double(), S, A)
    with pytest.raises(ValueError, match="contiguous"):
        ops.traj_cut(d, R, S, A.transpose(0, 1).contiguous().transpose(0, 1))
    with pytest.raises(ValueError, match="contiguous"):
        ops.traj_cut(d.t().contiguous().t(), R, S, A)
    # nothing above wrote anything
    for t, src in ((R, c.R), (S, c.S), (A, c.A)):
        assert np.array_equal(TC.bits(t.cpu().numpy()), TC.bits(src))
    lens, dones = ops.traj_cut(d[:0], R[:0], S[:0], A[:0])  # n = 0: no launch
    assert lens.shape == (0,) and dones.shape == (0,)


def test_rollout_deep_plan_reports_the_plain_instances_occupancy(cuda):
    from mepol_amd import ops

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for env_id, a in ((0, 1), (1, 2)):
        for widths in ((64, 48, 64), (300, 300, 300)):
            wg = ops.rollout_deep_plan(env_id, widths, a)["resident_workgroups"]
            # an instance that can be launched holds at least one workgroup per compute unit
            assert wg >= cus and wg % cus == 0
