"""Host-side decisions of the small-batch path (batches under 16384 rows on the HIP kernels):
the row tile mepol_policy_forward_plan_info reports, the admission floor of
GaussianPolicy._fused_head_ok and the gemm_nt variant of the deep policy's layers.  No GPU:
the plan call is host only."""
import ctypes

import pytest
import torch


def _plan(n, nf=2, h0=300, h1=300):
    from mepol_amd import _lib

    tile = ctypes.c_int(-1)
    rc = _lib.load().mepol_policy_forward_plan_info(n, nf, h0, h1, ctypes.byref(tile))
    return rc, tile.value


@pytest.mark.parametrize("n", [16384, 16385, 200000])
def test_plan_keeps_the_64_row_tile_from_16384_rows(n):
    assert _plan(n) == (0, 64)
    assert _plan(n, 29, 400, 300) == (0, 64)


def test_plan_takes_a_shorter_tile_below():
    rc, tile = _plan(8000)
    assert rc == 0 and tile in (32, 16)
    assert _plan(1) == (0, 16)
    # the shortest tile whose grid fits one workgroup per CU (256), the 64-row kernel beyond
    assert _plan(4096) == (0, 16) and _plan(4097) == (0, 32)
    assert _plan(8000) == (0, 32)
    assert _plan(8192) == (0, 32) and _plan(8193) == (0, 64)
    assert _plan(16383) == (0, 64)


def test_plan_wrapper_and_odd_hidden0():
    from mepol_amd import ops

    assert ops.policy_forward_plan(8000, 2, 300, 300) == {"row_tile": _plan(8000)[1]}
    assert ops.policy_forward_plan(1000, 2, 37, 45) == {"row_tile": 64}  # the one-kernel form


def test_plan_rejects_bad_arguments():
    from mepol_amd import _lib

    lib = _lib.load()
    tile = ctypes.c_int()
    assert _plan(8000, 2, 300, 321)[0] == 1001   # hidden1 > 320
    assert _plan(8000, 65, 300, 300)[0] == 1001  # in_features > 64
    assert lib.mepol_policy_forward_plan_info(8000, 2, 300, 300, None) == 1001
    assert lib.mepol_policy_forward_plan_info(0, 2, 300, 300, ctypes.byref(tile)) == 1001
    with pytest.raises(_lib.MepolInputError):
        _lib.call("mepol_policy_forward_plan_info", 8000, 2, 300, 321, ctypes.byref(tile))
    assert lib.mepol_abi_version() == 4


def test_floors(monkeypatch):
    from mepol_amd import policy as P

    monkeypatch.delenv("MEPOL_FUSED_MIN_ROWS", raising=False)
    assert P.SPLITK_MIN_ROWS == 16384
    assert 0 < P.FUSED_MIN_ROWS <= 8000
    assert P.fused_min_rows() == P.FUSED_MIN_ROWS
    monkeypatch.setenv("MEPOL_FUSED_MIN_ROWS", "12345")  # read at call time
    assert P.fused_min_rows() == 12345
    assert P.FUSED_MIN_ROWS <= 8000 and P.SPLITK_MIN_ROWS == 16384


@pytest.mark.parametrize("n", [1, 8000, 16384, 200000])
def test_fused_head_is_off_for_cpu_tensors(monkeypatch, n):
    from mepol_amd.policy import GaussianPolicy

    monkeypatch.setenv("MEPOL_FUSED_MIN_ROWS", "1")
    pol = GaussianPolicy([8, 8], 2, 1)
    s, a = torch.zeros(n, 2, dtype=torch.float64), torch.zeros(n, 1, dtype=torch.float64)
    assert not pol._fused_head_ok(s, a)
    assert not pol._fused_head_ok(s, a, 1)


def test_gemm_nt_variant_rule():
    from mepol_amd import ops

    for n in (16384, 16385, 20000, 200000):
        for m in (32, 160, 300, 512):
            assert ops.gemm_nt_variant(n, m) == 0
    assert ops.gemm_nt_variant(8000, 300) == 2   # 63 x 2 = 126 tiles of 128 x 160: under 256
    assert ops.gemm_nt_variant(2000, 32) == 2
    assert ops.gemm_nt_variant(16383, 300) == 0  # 128 x 2 = 256 tiles
    assert ops.gemm_nt_variant(16383, 160) == 2  # 128 x 1
