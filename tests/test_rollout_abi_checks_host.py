"""Argument checks of every rollout entry point of the C ABI, replayed from a recorded table
(tests/golden/rollout_abi_checks.json): the return code and the full mepol_last_error_string() of
each case are what the library gave when the table was recorded, so the order of the checks, the
codes and the texts are pinned.  The technique of test_rollout_deep_host.py: the pointers are host
memory and are never dereferenced, and every case is rejected or returns before a launch, so no
GPU is needed.  No case passes validation with n, T > 0 (it would launch), and none reaches an
occupancy query (the plan_info functions are only given arguments they refuse).

Before each case a sentinel call sets the error text, so a case that succeeds is recorded with the
sentinel's text: a success leaves the text alone.

`python tests/test_rollout_abi_checks_host.py --record` rewrites the table from the library at
hand; it drops any generated case that the library does not answer with 0 or 1001 .. 1003."""
import ctypes
import json
import os
import sys

import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                     "rollout_abi_checks.json")

_TWO = ["W1", "b1", "h0", "W2t", "b2", "h1", "Wm", "bm", "log_std", "a_dim"]
_DEEP = ["n_hidden", "widths", "W1", "b1", "Wt", "bt", "Wm", "bm", "log_std", "a_dim"]
_GOAL_OUT = ["rewards_rec", "len_out", "done_out"]
_WS = ["workspace", "workspace_bytes", "stream"]
_STEP = ["mean", "noise", "log_std", "n", "a_dim", "t", "T", "states_rec", "actions_rec",
         "policy_in", "stream"]
_MAZE_GOAL = ["goal_x", "goal_y", "coord", "goal_value", "states_rec", "actions_rec", "visited",
              "final_state"] + _GOAL_OUT + _WS

# entry point -> its parameter names, in order (the types are _lib.SIGNATURES')
PARAMS = {
    "mepol_rollout_step": ["env_id", "env_f64", "env_f32"] + _STEP,
    "mepol_rollout_step_maze": ["maze", "env_f32"] + _STEP,
    "mepol_step_maze": ["maze", "state", "action", "n", "stream"],
    "mepol_rollout_mlp": ["env_id"] + _TWO + ["init64", "init32", "noise", "n", "T", "states_rec",
                                              "actions_rec", "visited", "final_state"] + _WS,
    "mepol_rollout_mlp_plan_info": ["n", "h0", "h1", "a_dim", "out0", "out1"],
    "mepol_rollout_mlp_workspace_size": ["n", "T", "h0", "h1", "a_dim", "bytes"],
    "mepol_rollout_goal": ["env_id"] + _TWO + ["init32", "noise", "n", "T", "goal_x", "goal_y",
                                               "radius", "states_rec", "actions_rec"]
                          + _GOAL_OUT + _WS,
    "mepol_rollout_goal_plan_info": ["n", "h0", "h1", "a_dim", "out0", "out1"],
    "mepol_rollout_goal_workspace_size": ["env_id", "n", "T", "h0", "h1", "a_dim", "bytes"],
    "mepol_rollout_goal_threshold": ["env_id"] + _TWO + ["init64", "init32", "noise", "n", "T",
                                                         "coord", "threshold", "states_rec",
                                                         "actions_rec"] + _GOAL_OUT + _WS,
    "mepol_rollout_goal_threshold_plan_info": ["env_id", "n", "h0", "h1", "a_dim", "out0", "out1"],
    "mepol_rollout_goal_threshold_workspace_size": ["env_id", "n", "T", "h0", "h1", "a_dim",
                                                    "bytes"],
    "mepol_rollout_maze": ["maze", "goal_kind"] + _TWO + ["init32", "noise", "n", "T"] + _MAZE_GOAL,
    "mepol_rollout_maze_plan_info": ["goal_kind", "n", "h0", "h1", "a_dim", "out0", "out1"],
    "mepol_rollout_maze_workspace_size": ["goal_kind", "n", "T", "h0", "h1", "a_dim", "bytes"],
    "mepol_rollout_deep": ["env_id"] + _DEEP + ["init64", "init32", "noise", "n", "T",
                                                "states_rec", "actions_rec", "visited",
                                                "final_state"] + _WS,
    "mepol_rollout_deep_plan_info": ["env_id", "n_hidden", "widths", "a_dim", "out0"],
    "mepol_rollout_deep_workspace_size": ["n", "T", "n_hidden", "widths", "a_dim", "bytes"],
    "mepol_rollout_deep_goal": ["env_id"] + _DEEP + ["init32", "noise", "n", "T", "goal_x",
                                                     "goal_y", "radius", "states_rec",
                                                     "actions_rec"] + _GOAL_OUT + _WS,
    "mepol_rollout_deep_goal_plan_info": ["n_hidden", "widths", "a_dim", "out0"],
    "mepol_rollout_deep_goal_threshold": ["env_id"] + _DEEP + ["init64", "init32", "noise", "n",
                                                               "T", "coord", "threshold",
                                                               "states_rec", "actions_rec"]
                                         + _GOAL_OUT + _WS,
    "mepol_rollout_deep_goal_threshold_plan_info": ["env_id", "n_hidden", "widths", "a_dim",
                                                    "out0"],
    "mepol_rollout_deep_maze": ["maze", "goal_kind"] + _DEEP + ["init32", "noise", "n", "T"]
                               + _MAZE_GOAL,
    "mepol_rollout_deep_maze_plan_info": ["goal_kind", "n_hidden", "widths", "a_dim", "out0"],
    "mepol_rollout_deep_maze_workspace_size": ["n", "T", "n_hidden", "widths", "a_dim", "bytes"],
}

# what every case starts from; a table row holds only what it changes
BASE = {"env_id": 0, "goal_kind": 0, "h0": 8, "h1": 8, "a_dim": 1, "n": 4, "T": 3, "t": 0,
        "widths": [8, 8, 8], "goal_x": 0.5, "goal_y": 0.5, "radius": 0.1, "goal_value": 0.1,
        "threshold": 0.1, "coord": 0, "workspace_bytes": 256, "stream": "null", "maze": {}}
GOOD_MAZE = {"xlo": -1.0, "xhi": 1.0, "ylo": -1.0, "yhi": 1.0, "max_delta": 0.1, "n_walls": 1,
             "wall0": [-0.5, 0.5, -0.1, 0.1]}


def _num(v):
    return float(v) if isinstance(v, str) else v


def _call(lib, fn, over):
    """Calls `fn` with BASE changed by `over`; returns (rc, text, the size_t output or None)."""
    from mepol_amd import _lib

    buf = (ctypes.c_double * 64)()
    keep, size_out, args = [buf], None, []
    vals = dict(BASE, **over)
    if "n_hidden" not in over:
        vals["n_hidden"] = len(vals["widths"]) if vals["widths"] != "null" else 3
    for name, typ in zip(PARAMS[fn], _lib.SIGNATURES[fn]):
        v = vals.get(name, "p")
        if v == "null":
            arg = None
        elif typ is ctypes.c_void_p:
            arg = ctypes.addressof(buf)
        elif typ is _lib._c_mp:
            m, d = _lib.Maze(), dict(GOOD_MAZE, **v)
            for k in ("xlo", "xhi", "ylo", "yhi", "max_delta"):
                setattr(m, k, _num(d[k]))
            m.n_walls = d["n_walls"]
            for k in range(4):
                m.walls[0][k] = _num(d["wall0"][k])
            arg = ctypes.byref(m)
            keep.append(m)
        elif name == "widths":  # (8 words whatever n_hidden says: a refused count reads none)
            arg = (ctypes.c_int * 8)(*(list(v) + [8] * (8 - len(v))))
        elif typ is _lib._c_ip:
            arg = ctypes.pointer(ctypes.c_int())
        elif name == "bytes":
            size_out = ctypes.c_size_t()
            arg = ctypes.pointer(size_out)
        else:
            arg = _num(v)
        keep.append(arg)
        args.append(arg)
    # the sentinel: a refusal whose text every case starts from
    assert lib.mepol_rollout_deep_workspace_size(0, 0, 3, None, 1, None) == 1001
    rc = getattr(lib, fn)(*args)
    text = lib.mepol_last_error_string().decode()
    return rc, text, (size_out.value if size_out is not None and rc == 0 else None)


def _table():
    with open(TABLE) as f:
        return json.load(f)


def test_table_covers_every_rollout_entry_point():
    from mepol_amd import _lib

    t = _table()
    rollout = {k for k in _lib.SIGNATURES if k.startswith("mepol_rollout")} | {"mepol_step_maze"}
    assert set(t["cases"]) == set(PARAMS) == rollout
    for fn, rows in t["cases"].items():
        assert len(PARAMS[fn]) == len(_lib.SIGNATURES[fn]), fn
        assert len(rows) >= 10, fn
        assert any(rc == 1001 for _, rc, _, _ in rows), fn


@pytest.mark.parametrize("fn", sorted(PARAMS))
def test_argument_checks_match_the_recorded_table(fn):
    from mepol_amd import _lib

    lib = _lib.load()
    t = _table()
    wrong = []
    for over, rc, text, out in t["cases"][fn]:
        got = _call(lib, fn, over)
        if got != (rc, t["texts"][text], out):
            wrong.append((over, got, (rc, t["texts"][text], out)))
    assert not wrong, f"{len(wrong)} of {len(t['cases'][fn])} cases differ, the first: {wrong[0]}"


# ---- recording -----------------------------------------------------------------------------------
_MAZES = ["null", {"n_walls": 17}, {"n_walls": -1}, {"xlo": 1.0, "xhi": -1.0},
          {"ylo": 1.0, "yhi": -1.0}, {"wall0": [0.5, -0.5, 0.0, 0.0]}, {"max_delta": "nan"}]
SWEEP = {"env_id": [-1, 0, 1, 2, 3], "goal_kind": [-1, 0, 1, 2, 3], "a_dim": [0, 1, 2, 9],
         "h0": [0, 513], "h1": [0, 513], "n_hidden": [2, 7],
         "widths": [[8, 0, 8], [8, 513, 8], [513, 8, 8], [8, 8], [8] * 7, "null"],
         "goal_x": ["nan"], "goal_y": ["nan"], "radius": [-1.0, "nan"], "threshold": ["nan"],
         "goal_value": [-1.0, "nan"], "coord": [-1, 2], "T": [2 ** 31], "n": [-1], "t": [-1, 3],
         "workspace_bytes": [3, 255], "maze": _MAZES}


def _generate(fn):
    """Every case tried for `fn`: each base (env x a_dim, or goal kind) alone and with one argument
    swept, each of those as it is, with n = 0 and with T = 0."""
    from mepol_amd import _lib

    names = PARAMS[fn]
    if "env_id" in names:
        bases = [{"env_id": 0, "a_dim": 1}, {"env_id": 1, "a_dim": 2}]
    elif "goal_kind" in names:
        bases = [{"goal_kind": k, "a_dim": 2} for k in (0, 1, 2)]
    else:
        bases = [{"a_dim": 2}]
    single = [{}]
    for name, typ in zip(names, _lib.SIGNATURES[fn]):
        single += [{name: v} for v in SWEEP.get(name, [])]
        if name != "stream" and typ in (ctypes.c_void_p, _lib._c_ip, ctypes.POINTER(ctypes.c_size_t)):
            single.append({name: "null"})
    seen, out = set(), []
    for base in bases:
        for s in single:
            for nt in ({}, {"n": 0}, {"T": 0}):
                if any(k not in names or k in s for k in nt):
                    continue
                over = dict(base, **s, **nt)
                over = {k: v for k, v in over.items() if BASE.get(k, "p") != v}
                key = json.dumps(over, sort_keys=True)
                if key not in seen:
                    seen.add(key)
                    out.append(over)
    return out


def _record():
    from mepol_amd import _lib

    lib = _lib.load()
    texts, cases, dropped = [], {}, 0
    for fn in PARAMS:
        rows = []
        for over in _generate(fn):
            rc, text, out = _call(lib, fn, over)
            vals = dict(BASE, **over)
            launches = rc == 0 and vals["n"] > 0 and vals["T"] > 0 and "bytes" not in PARAMS[fn]
            if rc not in (0, 1001, 1002, 1003) or launches:
                dropped += 1  # it passed validation: a launch or an occupancy query
                continue
            if "bytes" in PARAMS[fn] and rc == 0 and vals["n"] > 0 and "widths" not in PARAMS[fn]:
                dropped += 1  # a two-layer size with n > 0 asks the device's occupancy
                continue
            if text not in texts:
                texts.append(text)
            rows.append([over, rc, texts.index(text), out])
        cases[fn] = rows
    with open(TABLE, "w") as f:
        f.write('{"texts": [\n' + ",\n".join(json.dumps(t) for t in texts) + '],\n"cases": {\n')
        f.write(",\n".join(json.dumps(fn) + ": [\n" + ",\n".join(json.dumps(r) for r in rows) + "]"
                           for fn, rows in cases.items()))
        f.write("}}\n")
    print(f"{sum(len(r) for r in cases.values())} cases recorded, {dropped} dropped")


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _record()
