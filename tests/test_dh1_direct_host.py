"""Host side of the register-fed dh1_layer1_backward: the plan and workspace queries, and the
cases of tests/dh1_direct_cases.py through numpy stand-ins.  No GPU: the queries are host only and
a launcher refuses a short workspace before it launches anything.

The kernel-ordered stand-in sums as dh1_direct_kernel does: k in MFMA steps {s, 4 + s, 8 + s,
12 + s} of each k-tile of 16, the row block's eight 32-row parts in row order, the records through
sum_records<16>.  It and the plain-f64 stand-in of tests/cpu_ops.py meet every bound, so the
bounds the GPU test applies are not tighter than correct f64 arithmetic in this order.
"""
import ctypes
import re
import types

import numpy as np
import pytest

import cpu_ops
import dh1_direct_cases as D

SHAPES = sorted({(c.n, c.K, c.M, c.F) for c in D.cases().values()})


def _mm_steps(a, b):
    """a [n, K] b^T [m, K] in f64, four k per step in the kernel's step order."""
    acc = np.zeros((a.shape[0], b.shape[0]))
    K = a.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, K, 16):
            for s in range(4):
                idx = [k for k in (k0 + s, k0 + 4 + s, k0 + 8 + s, k0 + 12 + s) if k < K]
                if idx:
                    acc = acc + a[:, idx] @ b[:, idx].T
    return acc


def _sum_records(recs):
    total = 0.0
    for g in range(16):
        waves = []
        for w in range(4):
            s = 0.0
            for b in range(g + 16 * w, len(recs), 64):
                s = s + recs[b]
            waves.append(s)
        total = total + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    return total


def k_dh1(dz2, W2t, h1, x, ws=None, dW_out=None, db_out=None, mask=None, w2=None):
    Wt = np.ascontiguousarray(w2.numpy().T) if w2 is not None else W2t.numpy()
    on = cpu_ops._unpack_mask(mask, Wt.shape[0]) if mask is not None else cpu_ops._gt0(h1.numpy())
    dz2, x = dz2.numpy(), x.numpy()
    n = dz2.shape[0]
    x1 = np.concatenate([x, np.ones((n, 1))], axis=1)
    recs = []
    for lo in range(0, n, 256):
        rec = 0.0
        for a in range(lo, min(n, lo + 256), 32):  # 4 waves x 2 halves of 32 rows, in row order
            b = min(n, a + 32)
            dz1 = cpu_ops._sel(on[a:b], _mm_steps(dz2[a:b], Wt))
            part = np.zeros((Wt.shape[0], x1.shape[1]))
            with np.errstate(invalid="ignore", over="ignore"):
                for r0 in range(a, b, 4):  # one MFMA step per 4 rows
                    part = part + dz1[r0 - a:r0 - a + 4].T @ x1[r0:r0 + 4]
            rec = rec + part
        recs.append(rec)
    tot = _sum_records(recs)
    return cpu_ops._into(dW_out, tot[:, :-1]), cpu_ops._into(db_out, tot[:, -1])


KOPS = types.SimpleNamespace(dh1_layer1_workspace=cpu_ops.dh1_layer1_workspace,
                             dh1_layer1_backward=k_dh1)


@pytest.mark.parametrize("name", list(D.cases()))
def test_standins_meet_every_bound(name):
    c = D.cases()[name]
    D.run(cpu_ops, "cpu", c)
    if c.n <= 4357:  # (the stand-in walks 4 rows at a time in Python)
        D.run(KOPS, "cpu", c)


def test_sweeps_cover_what_they_claim():
    cs = D.cases()
    assert {c.n for c in cs.values()} >= set(D.SWEEP_N)
    assert {c.K for c in cs.values()} >= set(D.SWEEP_K)
    assert {c.M for c in cs.values()} >= set(D.SWEEP_M)
    assert {c.F for c in cs.values()} >= set(D.SWEEP_F)
    assert all(c.n % 64 for n, c in cs.items() if "_inf_" in n or "_nan_" in n)
    h = cs["mask_zeros"].h1
    assert (h == 0).any() and np.signbit(h[h == 0]).any() and not np.signbit(h[h == 0]).all()
    assert (cs["mask_on"].h1 > 0).all() and not (cs["mask_off"].h1 > 0).any()
    auto = [n for n, c in cs.items() if D.direct_auto(c.n, c.K, c.M, c.F)]
    assert auto == ["auto_many_tiles"]
    assert [n for n, c in cs.items() if not D.direct_fits(c.K, c.M, c.F)] == ["F32"]


@pytest.mark.parametrize("n,K,M,F", SHAPES + [(200000, 300, 400, 29), (13056, 300, 400, 29),
                                             (13057, 300, 400, 29), (16384, 300, 300, 2)])
def test_plan_info(n, K, M, F):
    from mepol_amd import ops

    from mepol_amd import _lib

    for mask, w2, form in ((True, True, "auto"), (True, False, "auto"), (False, False, "auto"),
                           (True, True, "lds"), (True, True, "direct"), (True, False, "direct"),
                           (False, False, "direct")):
        if form == "direct" and not (mask and D.direct_fits(K, M, F)):
            with pytest.raises(_lib.MepolError):
                ops.dh1_layer1_plan(n, K, M, F, mask=mask, w2=w2, form=form)
            continue
        p = ops.dh1_layer1_plan(n, K, M, F, mask=mask, w2=w2, form=form)
        direct = form == "direct" or (form == "auto" and mask and D.direct_auto(n, K, M, F))
        assert p["form"] == ("direct" if direct else "lds")
        assert p["nh"] == (F + 1 + 15) // 16
        assert p["row_blocks"] == (n + 255) // 256 and p["col_tiles"] == (M + 79) // 80
        assert p["threads"] == 64 * p["waves_per_block"]
        assert p["waves_per_block"] * p["rows_per_wave"] == 256
        assert (p["waves_per_block"], p["lds_bytes"]) == ((4, 40960 * p["nh"]) if direct
                                                          else (8, 86016))
        # two workgroups of the register-fed kernel share a CU's 160 KB of LDS
        assert not direct or 2 * p["lds_bytes"] <= 160 * 1024
        assert p["record_doubles"] == M * (F + 1)
        assert p["group_offset"] == p["row_blocks"] * p["record_doubles"] * 8
        assert p["ws_bytes"] == p["group_offset"] + 16 * p["record_doubles"] * 8


def test_plan_info_refuses_bad_arguments():
    from mepol_amd import _lib, ops

    for bad in ((0, 18, 82, 5), (5, 17, 82, 5), (5, 18, 0, 5), (5, 18, 82, 0), (5, 18, 82, 64)):
        with pytest.raises(_lib.MepolInputError):
            ops.dh1_layer1_plan(*bad)
    out = [ctypes.c_int() for _ in range(8)]
    big = [ctypes.c_int64(), ctypes.c_size_t(), ctypes.c_size_t()]
    refs = [ctypes.byref(v) for v in out + big]
    lib = _lib.load()
    assert lib.mepol_dh1_layer1_plan_info(5, 18, 82, 5, 1, 1, 0, *refs) == 0
    assert lib.mepol_dh1_layer1_plan_info(5, 18, 82, 5, 1, 1, 3, *refs) == 1001
    assert lib.mepol_dh1_layer1_plan_info(5, 18, 82, 5, 1, 1, 0, None, *refs[1:]) == 1001
    assert lib.mepol_dh1_layer1_plan_info(5, 18, 82, 32, 1, 1, 2, *refs) == 1003
    with pytest.raises(_lib.MepolInputError):
        ops.dh1_layer1_plan(5, 18, 81, 5, mask=True, w2=True)   # W2 as stored: hidden0 even
    with pytest.raises(_lib.MepolInputError):
        ops.dh1_layer1_plan(5, 18, 82, 5, mask=False, w2=True)  # W2 as stored: mask forms only
    assert _lib.load().mepol_abi_version() == 4


@pytest.mark.parametrize("n,K,M,F", SHAPES)
def test_workspace_query_is_what_the_launcher_checks(n, K, M, F):
    """mepol_dh1_layer1_workspace_size against the launchers' own check: with a workspace one byte
    short every form is refused (MEPOL_ERR_WORKSPACE, before anything is launched: the pointers
    here are never dereferenced) and the message names the size the query returned."""
    from mepol_amd import _lib, ops

    lib = _lib.load()
    need = ctypes.c_size_t()
    assert lib.mepol_dh1_layer1_workspace_size(n, M, F, ctypes.byref(need)) == 0
    assert need.value == ops.dh1_layer1_plan(n, K, M, F)["ws_bytes"]
    fake = ctypes.c_void_p(4096)  # non-null, 16-B aligned
    lib.mepol_last_error_string.restype = ctypes.c_char_p
    for fn in ("mepol_dh1_layer1_backward", "mepol_dh1_layer1_backward_masked",
               "mepol_dh1_layer1_backward_w2"):
        if fn.endswith("_w2") and M % 2:
            continue
        rc = getattr(lib, fn)(fake, n, K, fake, M, fake, fake, F, fake, fake, fake,
                              need.value - 1, None)
        assert rc == 1002, (fn, rc)
        got = re.search(r"workspace (\d+) < (\d+)", lib.mepol_last_error_string().decode())
        assert got and (int(got.group(1)), int(got.group(2))) == (need.value - 1, need.value)
    for form in (1, 2) if D.direct_fits(K, M, F) else (1,):
        rc = lib.mepol_dh1_layer1_backward_form(fake, n, K, fake, M, fake, fake, F, fake, fake, fake,
                                                need.value - 1, 1, form, None)
        assert rc == 1002, (form, rc)
