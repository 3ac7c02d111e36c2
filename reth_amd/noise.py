"""Ornstein-Uhlenbeck exploration noise for continuous actions.

Reference: reth/reth/utils/noise.py (OUNoise) and reth/reth/utils/exploration.py:34-53
(OUNoiseExploration): action = solver.act(state) + eps * noise(), eps from a Schedule stepped per
act, no clipping; the worker resets the noise at every episode end.  The draws come from numpy's
global RandomState, as in the reference.
"""
import numpy as np

from .schedule import Schedule


class OUNoise:
    def __init__(self, action_dimension, mu=0, theta=0.15, sigma=0.2):
        self.action_dimension = action_dimension
        self.mu, self.theta, self.sigma = mu, theta, sigma
        self.reset()

    def reset(self):
        self.state = np.ones(self.action_dimension) * self.mu

    def noise(self):
        x = self.state
        self.state = x + (self.theta * (self.mu - x) + self.sigma * np.random.randn(len(x)))
        return self.state


class OUNoiseExploration:
    def __init__(self, solver, action_space, epsilon, **noise_kwargs):
        assert len(action_space.shape) == 1, action_space.shape
        self.solver, self.action_space = solver, action_space
        self.noise = OUNoise(action_space.shape[0], **noise_kwargs)
        self.schedule = Schedule.from_str(epsilon)

    def act(self, state):
        action = self.solver.act(state)
        eps = self.schedule.step()
        action += eps * self.noise.noise()
        return action

    def reset(self):
        self.noise.reset()
