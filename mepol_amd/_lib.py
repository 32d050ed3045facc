"""ctypes binding of the C ABI declared in include/mepol_amd.h (libmepol_amd.so, gfx950).

There is no CPU fallback: if the library is missing or cannot be loaded, every op raises.
Build it with ``make`` (or ``__graft_entry__.build()``).
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MEPOL_AMD_LIB", os.path.join(_HERE, "libmepol_amd.so"))

_c_i64 = ctypes.c_int64
_c_int = ctypes.c_int
_c_dbl = ctypes.c_double
_c_sz = ctypes.c_size_t
_c_vp = ctypes.c_void_p

ABI_VERSION = 4  # include/mepol_amd.h MEPOL_ABI_VERSION
MAZE_MAX_WALLS = 16  # MEPOL_MAZE_MAX_WALLS
GOAL_NONE, GOAL_BALL, GOAL_THRESHOLD = 0, 1, 2  # MEPOL_GOAL_*


class Maze(ctypes.Structure):
    """mepol_maze: the box maze the env 2 entry points take by pointer."""
    _fields_ = [("xlo", _c_dbl), ("xhi", _c_dbl), ("ylo", _c_dbl), ("yhi", _c_dbl),
                ("max_delta", _c_dbl), ("n_walls", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("walls", (_c_dbl * 4) * MAZE_MAX_WALLS)]


_c_mp = ctypes.POINTER(Maze)
_c_flt = ctypes.c_float
_c_ip = ctypes.POINTER(_c_int)

# name -> argtypes (restype is int unless listed in _RESTYPES)
SIGNATURES = {
    "mepol_last_error_string": [],
    "mepol_abi_version": [],
    "mepol_knn_workspace_size": [_c_i64, _c_i64, _c_int, _c_int, _c_int, ctypes.POINTER(_c_sz)],
    "mepol_knn_plan_info": [_c_i64, _c_i64, _c_int, _c_int, _c_int, ctypes.POINTER(_c_int),
                            ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)],
    "mepol_knn": [_c_vp, _c_i64, _c_vp, _c_i64, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp,
                  _c_vp, _c_sz, _c_vp],
    "mepol_knn_deferred": [_c_vp, _c_i64, _c_vp, _c_i64, _c_int, _c_int, _c_int, _c_vp, _c_vp,
                           _c_vp, _c_vp, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_knn_exact": [_c_vp, _c_i64, _c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp,
                        _c_vp],
    "mepol_iw_forward": [_c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp,
                         _c_vp],
    "mepol_iw_normalize": [_c_vp, _c_vp, _c_i64, _c_vp, _c_vp],
    "mepol_entropy_partials_size": [_c_i64],
    "mepol_entropy_gamma_partials_size": [_c_i64],
    "mepol_entropy_forward": [_c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_int, _c_int, _c_dbl, _c_dbl,
                              _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp],
    "mepol_entropy_forward_emit": [_c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_int, _c_int, _c_dbl, _c_dbl,
                              _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp],
    "mepol_iw_normalize_gathered": [_c_vp, _c_int, _c_i64, _c_int, _c_vp, _c_vp],
    "mepol_sharded_emit": [_c_vp, _c_int, _c_i64, _c_i64, _c_dbl, _c_i64, _c_vp, _c_vp, _c_vp],
    "mepol_csr_workspace_size": [_c_i64, _c_int, _c_i64, ctypes.POINTER(_c_sz)],
    "mepol_csr_build": [_c_vp, _c_i64, _c_int, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_sz,
                        _c_vp],
    "mepol_entropy_gamma": [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp],
    "mepol_entropy_reverse_scan": [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_i64, _c_i64,
                                   _c_vp, _c_vp, _c_vp],
    "mepol_head_forward": [_c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp,
                           _c_vp, _c_vp],
    "mepol_head_workspace_size": [_c_i64, _c_int, _c_int, ctypes.POINTER(_c_sz)],
    "mepol_head_backward": [_c_vp, _c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int,
                            _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_head_backward_phase": [_c_vp, _c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                  _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_sz, _c_int,
                                  _c_vp],
    "mepol_weight_grad_workspace_size": [_c_i64, _c_int, _c_int, ctypes.POINTER(_c_sz)],
    "mepol_weight_grad": [_c_vp, _c_i64, _c_int, _c_vp, _c_int, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_weight_grad_plan_info": [_c_i64, _c_int, _c_int] + [ctypes.POINTER(_c_int)] * 5 + [
        ctypes.POINTER(_c_i64)] * 2 + [ctypes.POINTER(_c_int)] * 5,
    "mepol_layer_forward": [_c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp],
    "mepol_layer_workspace_size": [_c_i64, _c_int, _c_int, ctypes.POINTER(_c_sz)],
    "mepol_layer_backward": [_c_vp, _c_vp, _c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_sz,
                             _c_vp],
    "mepol_policy_forward": [_c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int,
                             _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp,
                             _c_vp],
    "mepol_dh1_layer1_workspace_size": [_c_i64, _c_int, _c_int, ctypes.POINTER(_c_sz)],
    "mepol_dh1_layer1_backward_form": [_c_vp, _c_i64, _c_int, _c_vp, _c_int, _c_vp, _c_vp,
                                       _c_int, _c_vp, _c_vp, _c_vp, _c_sz, _c_int, _c_int, _c_vp],
    "mepol_dh1_layer1_plan_info": [_c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int] + [
        ctypes.POINTER(_c_int)] * 8 + [ctypes.POINTER(_c_i64)] + [ctypes.POINTER(_c_sz)] * 2,
    "mepol_dh1_layer1_backward": [_c_vp, _c_i64, _c_int, _c_vp, _c_int, _c_vp, _c_vp, _c_int,
                                  _c_vp, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_dh1_layer1_backward_masked": [_c_vp, _c_i64, _c_int, _c_vp, _c_int, _c_vp, _c_vp,
                                         _c_int, _c_vp, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_dh1_layer1_backward_w2": [_c_vp, _c_i64, _c_int, _c_vp, _c_int, _c_vp, _c_vp,
                                     _c_int, _c_vp, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_policy_forward_masked": [_c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp,
                                    _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp,
                                    _c_vp, _c_vp, _c_vp, _c_vp],
    "mepol_policy_forward_tiled": [_c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp,
                                   _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp,
                                   _c_vp, _c_vp, _c_vp, _c_int, _c_vp],
    "mepol_policy_forward_plan_info": [_c_i64, _c_int, _c_int, _c_int, ctypes.POINTER(_c_int)],
    "mepol_hidden_backward_workspace_size": [_c_i64, _c_int, ctypes.POINTER(_c_sz)],
    "mepol_hidden_backward": [_c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp,
                              _c_sz, _c_vp],
    "mepol_gemm_nt": [_c_vp, _c_i64, _c_int, _c_i64, _c_vp, _c_int, _c_i64, _c_vp, _c_int, _c_vp,
                      _c_i64, _c_int, _c_vp],
    "mepol_layer_tangent": [_c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp],
    "mepol_hidden_tangent": [_c_vp, _c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_vp, _c_int, _c_vp,
                             _c_vp, _c_vp, _c_int, _c_vp],
    "mepol_mean_tangent": [_c_vp, _c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int,
                           _c_vp, _c_vp],
    "mepol_mean_backward_workspace_size": [_c_i64, _c_int, _c_int, ctypes.POINTER(_c_sz)],
    "mepol_mean_backward": [_c_vp, _c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp,
                            _c_vp, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_step_mountaincar": [_c_vp, _c_vp, _c_i64, _c_i64, _c_vp],
    "mepol_step_gridworld": [_c_vp, _c_vp, _c_i64, _c_vp],
    "mepol_rollout_step": [_c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_int, _c_i64,
                           _c_i64, _c_vp, _c_vp, _c_vp, _c_vp],
    "mepol_rollout_mlp": [_c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp,
                          _c_int, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp,
                          _c_vp, _c_sz, _c_vp],
    "mepol_rollout_mlp_workspace_size": [_c_i64, _c_i64, _c_int, _c_int, _c_int,
                                         ctypes.POINTER(_c_sz)],
    "mepol_rollout_mlp_plan_info": [_c_i64, _c_int, _c_int, _c_int, ctypes.POINTER(_c_int),
                                    ctypes.POINTER(_c_int)],
    "mepol_rollout_deep": [_c_int, _c_int, ctypes.POINTER(_c_int), _c_vp, _c_vp, _c_vp, _c_vp,
                           _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_vp,
                           _c_vp, _c_vp, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_rollout_deep_workspace_size": [_c_i64, _c_i64, _c_int, ctypes.POINTER(_c_int), _c_int,
                                          ctypes.POINTER(_c_sz)],
    "mepol_rollout_deep_plan_info": [_c_int, _c_int, ctypes.POINTER(_c_int), _c_int,
                                     ctypes.POINTER(_c_int)],
    "mepol_rollout_goal": [_c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp,
                           _c_int, _c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_float, ctypes.c_float,
                           _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_rollout_goal_workspace_size": [_c_int, _c_i64, _c_i64, _c_int, _c_int, _c_int,
                                          ctypes.POINTER(_c_sz)],
    "mepol_rollout_goal_plan_info": [_c_i64, _c_int, _c_int, _c_int, ctypes.POINTER(_c_int),
                                     ctypes.POINTER(_c_int)],
    "mepol_rollout_deep_goal": [_c_int, _c_int, ctypes.POINTER(_c_int), _c_vp, _c_vp, _c_vp,
                                _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_i64, _c_i64,
                                ctypes.c_float, ctypes.c_float, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp,
                                _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_rollout_deep_goal_plan_info": [_c_int, ctypes.POINTER(_c_int), _c_int,
                                          ctypes.POINTER(_c_int)],
    "mepol_rollout_goal_threshold": [_c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_vp,
                                     _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64,
                                     _c_int, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                     _c_sz, _c_vp],
    "mepol_rollout_goal_threshold_workspace_size": [_c_int, _c_i64, _c_i64, _c_int, _c_int, _c_int,
                                                    ctypes.POINTER(_c_sz)],
    "mepol_rollout_goal_threshold_plan_info": [_c_int, _c_i64, _c_int, _c_int, _c_int,
                                               ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)],
    "mepol_rollout_deep_goal_threshold": [_c_int, _c_int, ctypes.POINTER(_c_int), _c_vp, _c_vp,
                                          _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp,
                                          _c_vp, _c_i64, _c_i64, _c_int, _c_dbl, _c_vp, _c_vp,
                                          _c_vp, _c_vp, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_rollout_deep_goal_threshold_plan_info": [_c_int, _c_int, ctypes.POINTER(_c_int), _c_int,
                                                    ctypes.POINTER(_c_int)],
    "mepol_step_maze": [_c_mp, _c_vp, _c_vp, _c_i64, _c_vp],
    "mepol_rollout_step_maze": [_c_mp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_int, _c_i64, _c_i64,
                                _c_vp, _c_vp, _c_vp, _c_vp],
    "mepol_rollout_maze_workspace_size": [_c_int, _c_i64, _c_i64, _c_int, _c_int, _c_int,
                                          ctypes.POINTER(_c_sz)],
    "mepol_rollout_maze_plan_info": [_c_int, _c_i64, _c_int, _c_int, _c_int, _c_ip, _c_ip],
    "mepol_rollout_maze": [_c_mp, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp,
                           _c_vp, _c_int, _c_vp, _c_vp, _c_i64, _c_i64, _c_flt, _c_flt, _c_int,
                           _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_sz,
                           _c_vp],
    "mepol_rollout_deep_maze_workspace_size": [_c_i64, _c_i64, _c_int, _c_ip, _c_int,
                                               ctypes.POINTER(_c_sz)],
    "mepol_rollout_deep_maze_plan_info": [_c_int, _c_int, _c_ip, _c_int, _c_ip],
    "mepol_rollout_deep_maze": [_c_mp, _c_int, _c_int, _c_ip, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_i64, _c_i64, _c_flt, _c_flt,
                                _c_int, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                _c_vp, _c_sz, _c_vp],
    "mepol_traj_budget": [_c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp],
    "mepol_traj_cut": [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_vp,
                       _c_vp],
    "mepol_gae": [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_dbl, _c_dbl, _c_vp,
                  _c_int, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp],
    "mepol_standardize_workspace_size": [_c_i64, ctypes.POINTER(_c_sz)],
    "mepol_standardize": [_c_vp, _c_i64, _c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_memcpy_async": [_c_vp, _c_vp, _c_sz, _c_vp],
    "mepol_optim_step": [_c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp],
    "mepol_optim_step_snapshot": [_c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                  _c_vp, _c_vp, _c_vp, _c_vp],
    "mepol_critic_fit_plan_info": [_c_int, _c_int, _c_int, _c_int] + [ctypes.POINTER(_c_int)] * 3,
    "mepol_critic_fit": [_c_vp, _c_vp, _c_i64, _c_vp, _c_i64, _c_int, _c_int, _c_int, _c_int,
                         _c_vp, _c_vp, _c_vp, _c_vp, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp],
}
_RESTYPES = {"mepol_last_error_string": ctypes.c_char_p}

_lib = None
_lock = threading.Lock()


class MepolError(RuntimeError):
    pass


class MepolInputError(MepolError, ValueError):
    """MEPOL_ERR_BAD_ARG: invalid input (e.g. non-finite particles); a ValueError like the
    reference's sklearn check_array rejection."""


def load():
    """Load libmepol_amd.so (once) and bind every exported symbol; raise if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise MepolError(
                    f"{LIB_PATH} not found: the MI355X kernels are not built (run `make` or "
                    "__graft_entry__.build()); there is no CPU fallback")
            lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
            for name, argtypes in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.argtypes = argtypes
                fn.restype = _RESTYPES.get(name, ctypes.c_int)
            got = lib.mepol_abi_version()
            if got != ABI_VERSION:
                raise MepolError(f"{LIB_PATH} has C ABI version {got}, this binding expects "
                                 f"{ABI_VERSION}: rebuild the library (make)")
            _lib = lib
    return _lib


def call(name, *args):
    """Invoke a C-ABI entry point; raise MepolError with the library's message on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.mepol_last_error_string()
        cls = MepolInputError if rc == 1001 else MepolError
        raise cls(f"{name} failed (rc={rc}): {msg.decode() if msg else ''}")
    return rc


def ptr(t):
    """Device pointer of a tensor (or None) as a ctypes void pointer."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())
