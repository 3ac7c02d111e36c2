"""`reth.algorithm.util` (reth/reth/algorithm/util.py:15-53)"""
from reth_amd.ddpg import soft_update  # noqa: F401
from reth_amd.ppo import calculate_discount_rewards, calculate_discount_rewards_with_dones  # noqa: F401
