"""`reth.algorithm` (reth/reth/algorithm/__init__.py:17-21): the DQN, DDPG and PPO solvers"""
from reth_amd.ddpg import DDPGSolver  # noqa: F401
from reth_amd.ppo import PPOSolver  # noqa: F401
from reth_amd.solver import DQNSolver, get_solver  # noqa: F401
