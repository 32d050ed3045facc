"""device_loop.capture_guard: the cyclic garbage collector stays out of a graph capture."""
import gc
import weakref


class _Node:
    pass


def _dead_cycle():
    a, b = _Node(), _Node()
    a.other, b.other = b, a
    return weakref.ref(a)


def test_capture_guard_collects_first_and_holds_the_collector_off():
    from mepol_amd.algorithms.device_loop import capture_guard

    assert gc.isenabled()
    before = _dead_cycle()
    with capture_guard():
        assert before() is None       # collected on entry, outside the capture
        assert not gc.isenabled()
        inside = _dead_cycle()
        with capture_guard():         # a second rank's capture in the same process
            assert not gc.isenabled()
        assert not gc.isenabled()     # the inner guard's end does not switch it back on
        for _ in range(3):            # allocation pressure that would otherwise trigger a pass
            junk = [[i] for i in range(20000)]
            del junk
        assert inside() is not None   # no collection ran inside the guard
    assert gc.isenabled()
    gc.collect()
    assert inside() is None


def test_capture_guard_restores_a_disabled_collector_and_survives_errors():
    from mepol_amd.algorithms.device_loop import capture_guard

    gc.disable()
    try:
        with capture_guard():
            pass
        assert not gc.isenabled()     # it was off before: it stays off
    finally:
        gc.enable()
    try:
        with capture_guard():
            raise RuntimeError("capture failed")
    except RuntimeError:
        pass
    assert gc.isenabled()
