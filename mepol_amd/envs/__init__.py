from .gridworld import GridWorldContinuous
from .maze import MAZE_MAX_WALLS, BoxMazeContinuous
from .mountain_car import MountainCarContinuous
from .spaces import Box
from .wrappers import (AnyGoal, BatchReward, BoxGoal, CustomRewardEnv, ErgodicEnv, GridGoal,
                       ThresholdGoal, unwrap)

__all__ = ["GridWorldContinuous", "MountainCarContinuous", "BoxMazeContinuous", "MAZE_MAX_WALLS",
           "Box", "ErgodicEnv",
           "CustomRewardEnv", "GridGoal", "ThresholdGoal", "BatchReward", "BoxGoal", "AnyGoal",
           "unwrap"]
