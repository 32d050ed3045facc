from .gridworld import GridWorldContinuous
from .mountain_car import MountainCarContinuous
from .spaces import Box
from .wrappers import (AnyGoal, BatchReward, BoxGoal, CustomRewardEnv, ErgodicEnv, GridGoal,
                       ThresholdGoal, unwrap)

__all__ = ["GridWorldContinuous", "MountainCarContinuous", "Box", "ErgodicEnv",
           "CustomRewardEnv", "GridGoal", "ThresholdGoal", "BatchReward", "BoxGoal", "AnyGoal",
           "unwrap"]
