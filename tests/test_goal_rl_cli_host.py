"""goal_rl's --hidden_sizes (a build extension, the MEPOL command line's): the parser, the width
check (which runs before the GPU check, so it is reachable here) and the reading of a
checkpoint's layer widths."""
import numpy as np

ARGS = ["--env", "GridGoal1", "--num_epochs", "1", "--batch_size", "10", "--traj_len", "5",
        "--kl_thresh", "0.001"]


def test_parser_takes_hidden_sizes():
    from mepol_amd.experiments.goal_rl import build_parser

    p = build_parser()
    assert p.parse_args(ARGS + ["--hidden_sizes", "300", "300", "300"]).hidden_sizes == [300, 300,
                                                                                         300]
    assert p.parse_args(ARGS).hidden_sizes is None


def test_non_positive_width_returns_4(capsys):
    from mepol_amd.experiments.goal_rl import main

    assert main(ARGS + ["--hidden_sizes", "0", "300"]) == 4
    assert "--hidden_sizes needs positive widths." in capsys.readouterr().out


def test_checkpoint_widths_follow_the_layer_order():
    """net.0, net.2, ... net.10: numeric order of the layer index, not the string order."""
    from mepol_amd.experiments.goal_rl import checkpoint_widths

    widths = [7, 300, 5, 64, 9, 11]
    sd, fan_in = {"log_std": np.zeros(2)}, 2
    for i, w in enumerate(widths):
        sd[f"net.{2 * i}.weight"] = np.zeros((w, fan_in))
        sd[f"net.{2 * i}.bias"] = np.zeros(w)
        fan_in = w
    sd["mean.weight"], sd["mean.bias"] = np.zeros((2, fan_in)), np.zeros(2)
    assert checkpoint_widths(sd) == widths
