"""The cut kernel's case table (traj_cut_cases.py) reaches what it claims, its numpy restatement
does what the header says on a hand-written batch, and mepol_traj_cut / mepol_rollout_deep_plan_info
reject bad arguments on the host before any launch -- all without a GPU."""
import ctypes

import numpy as np

import traj_cut_cases as TC


def test_reference_on_a_hand_written_batch():
    done = np.array([[0, 0, 2, 1], [0, 0, 0, 0], [0x80, 0, 0, 0], [0, 0, 0, 1]], dtype=np.uint8)
    R = np.arange(1, 17, dtype=np.float32).reshape(4, 4)
    S = np.arange(1, 41, dtype=np.float32).reshape(4, 5, 2)
    A = np.arange(1, 17, dtype=np.float32).reshape(4, 4, 1)
    r, s, a, lens, dones = TC.cut_reference(done, R, S, A)
    assert lens.tolist() == [3, 4, 1, 4] and dones.tolist() == [1, 0, 1, 1]
    assert r.tolist() == [[1, 2, 3, 0], [5, 6, 7, 8], [9, 0, 0, 0], [13, 14, 15, 16]]
    assert a[..., 0].tolist() == r.tolist()
    # states keep the reached state, row len
    assert s[0, :4].tolist() == S[0, :4].tolist() and s[0, 4].tolist() == [0, 0]
    assert s[2, :2].tolist() == S[2, :2].tolist() and not s[2, 2:].any()
    assert np.array_equal(s[1], S[1]) and np.array_equal(s[3], S[3])
    assert np.array_equal(R, np.arange(1, 17, dtype=np.float32).reshape(4, 4))  # inputs untouched
    # bool done_step is read the same way
    assert TC.cut_reference(done != 0, R, S, A)[3].tolist() == [3, 4, 1, 4]


def test_table_reaches_every_edge():
    keys = TC.case_keys()
    assert {k[1] for k in keys} == set(TC.T_VALUES) == {1, 2, 63, 64, 65, 255, 256, 257, 513}
    assert {k[0] for k in keys} == {1, 3, 257} and {k[2] for k in keys} == {1, 2, 8}
    assert len(keys) == len(set(keys)) == 81
    kinds, firsts, byte_values = set(), set(), set()
    nan_kept = negzero_kept = filled = 0
    for key in keys:
        c = TC.case(*key)
        assert c.done.shape == (c.n, c.T) and c.A.shape == (c.n, c.T, c.a_dim)
        assert c.S.shape == (c.n, c.T + 1, TC.NF)
        kinds |= set(c.kinds)
        byte_values |= set(np.unique(c.done).tolist())
        Ru, Su, Au = (TC.bits(x) for x in (c.R, c.S, c.A))
        for i in range(c.n):
            L, hits = int(c.lens[i]), np.flatnonzero(c.done[i])
            if c.dones[i]:
                assert L == hits[0] + 1
                firsts.add((int(hits[0]), c.T, len(hits)))
            else:
                assert L == c.T and len(hits) == 0
                firsts.add((None, c.T, 0))
            nan_kept += int((Ru[i, :L] == TC.NAN_PAYLOAD).sum())
            negzero_kept += int((Ru[i, :L] == TC.NEG_ZERO).sum())
            # behind the end every word of all three buffers is the fill, in front of it none is
            assert (Ru[i, L:] == TC.FILL).all() and (Au[i, L:] == TC.FILL).all()
            assert (Su[i, L + 1:] == TC.FILL).all()
            assert np.isfinite(c.S[i, :L + 1]).all() and np.isfinite(c.A[i, :L]).all()
            filled += int(L < c.T)
    assert kinds == set(TC.KINDS)
    assert byte_values == {0, 1, 2, 0x80, 0xFF}
    assert nan_kept > 50 and negzero_kept > 50 and filled > 50
    first_t = {f for f, _, _ in firsts}
    assert {0, 255, 256, 257, None} <= first_t                      # t = 0, the seam, no hit
    assert all((T - 1, T, 1) in firsts for T in TC.T_VALUES)        # a single hit on the last step
    assert all((0, T, T) in firsts for T in TC.T_VALUES)            # a hit on every step
    assert any(f is not None and k == 2 and f < T - 1 for f, T, k in firsts)  # two: first wins
    # the late hit that a lower thread finds: steps 1 and 256, the first is step 1
    wrap = [c for k in keys for c in [TC.case(*k)] if "wrap" in c.kinds]
    assert wrap and all(c.lens[c.kinds.index("wrap")] == 2 for c in wrap)
    assert all(c.done[c.kinds.index("wrap"), TC.THREADS] != 0 for c in wrap)


def test_reference_on_the_table_is_idempotent_and_keeps_bits():
    for key in TC.case_keys()[::7]:
        c = TC.case(*key)
        r, s, a, lens, dones = TC.cut_reference(c.done, c.R, c.S, c.A)
        assert np.array_equal(lens, c.lens) and np.array_equal(dones, c.dones)
        for got, src in ((r, c.R), (s, c.S), (a, c.A)):
            g, o = TC.bits(got), TC.bits(src)
            assert ((g == o) | ((o == TC.FILL) & (g == 0))).all()
            assert not (g == TC.FILL).any()
        again = TC.cut_reference(c.done, r, s, a)
        assert all(np.array_equal(TC.bits(x), TC.bits(y)) for x, y in zip(again, (r, s, a, lens,
                                                                                  dones)))


def _host_buffers():
    """Non-null pointers for the argument checks: host memory, never dereferenced (a bad argument
    is refused before any launch)."""
    bufs = [ctypes.create_string_buffer(64) for _ in range(6)]
    return bufs, [ctypes.cast(b, ctypes.c_void_p) for b in bufs]


def test_traj_cut_rejects_bad_arguments_without_gpu():
    from mepol_amd import _lib

    lib = _lib.load()
    keep, (d, r, s, a, ln, dn) = _host_buffers()

    def cut(d=d, n=2, T=4, r=r, s=s, nf=2, a=a, a_dim=1, ln=ln, dn=dn):
        return lib.mepol_traj_cut(d, n, T, r, s, nf, a, a_dim, ln, dn, None)

    assert cut(n=0) == 0                                   # nothing to do: no launch
    assert cut(n=0, d=None, r=None, s=None, a=None, ln=None, dn=None) == 0
    for bad in (dict(d=None), dict(r=None), dict(s=None), dict(a=None), dict(ln=None),
                dict(dn=None), dict(T=0), dict(T=-1), dict(T=2 ** 31 - 1), dict(T=2 ** 31),
                dict(nf=0), dict(nf=-2), dict(a_dim=0), dict(a_dim=-1)):
        assert cut(**bad) == 1001, bad
        assert b"mepol_traj_cut" in lib.mepol_last_error_string()
    assert keep


def test_rollout_deep_plan_info_rejects_bad_arguments_without_gpu():
    from mepol_amd import _lib

    lib = _lib.load()
    wg = ctypes.c_int(-7)
    widths = (ctypes.c_int * 3)(64, 48, 64)

    def plan(env_id=1, n_hidden=3, w=widths, a_dim=2, out=ctypes.byref(wg)):
        return lib.mepol_rollout_deep_plan_info(env_id, n_hidden, w, a_dim, out)

    for bad in (dict(env_id=2), dict(env_id=-1), dict(n_hidden=2), dict(n_hidden=7), dict(w=None),
                dict(a_dim=0), dict(a_dim=9), dict(env_id=1, a_dim=1), dict(out=None),
                dict(w=(ctypes.c_int * 3)(64, 513, 64)), dict(w=(ctypes.c_int * 3)(64, 0, 64))):
        assert plan(**bad) == 1001, bad
        assert b"mepol_rollout_deep_plan_info" in lib.mepol_last_error_string()
    assert wg.value == -7                                  # a refused query writes nothing
