"""Host environments -- gym and ALE are not part of this image.

CartPole restates gym's classic-control CartPole-v0/v1 dynamics (the reference's
examples/dqn/config.yaml names CartPole-v0; gym 0.17.3 is its pinned dependency): Euler
integration of the cart-pole ODE, terminal when |x| > 2.4 or |theta| > 12 degrees, reward
1 per step, TimeLimit 200 (v0) / 500 (v1).  Trajectories are not a parity claim (SURVEY
§8c: env dynamics are outside the path); the spaces and the step/reset contract are.
Acrobot (Acrobot-v1, TimeLimit 500) and MountainCar (MountainCar-v0, TimeLimit 200) restate
gym 0.17.3's definitions the same way; the three are the host definitions of the device envs
(csrc/env_actor.hpp), which follow them operation for operation.  Pendulum (Pendulum-v0, TimeLimit
200) is the continuous-control environment of the reference's examples/ddpg; it has no device
form yet and no discrete action set, so make() -- the envs of the DQN loops -- does not name it:
make_host() does, and is what the YAML factories (presets.get_env) and `reth.env.make` call.

Atari names (`<Game>NoFrameskip-v4`, the apex configs) give `SyntheticAtari`: the spaces of
the reference's wrapped env (env/util.py:281-297, wrap_deepmind + 4-frame stack: uint8
observations [4, 84, 84], the game's minimal action set) over synthetic frames with the
bench's reward / episode-end rates -- a stand-in so the reference's scripts build their
solver, trainer and workers; ALE emulation itself is out of scope.

Paddle ("Paddle-v0") is a small real pixel game with the same observation interface, the host
restatement of the device game the conv path's actors run (csrc/game.hpp).
"""
import math

import numpy as np

from .solver import Box, Discrete


class CartPole:
    gravity, masscart, masspole, length, force_mag, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
    theta_threshold = 12 * 2 * math.pi / 360
    x_threshold = 2.4

    def __init__(self, max_episode_steps=200, seed=None):
        high = np.array([self.x_threshold * 2, np.finfo(np.float32).max, self.theta_threshold * 2,
                         np.finfo(np.float32).max], dtype=np.float32)
        self.observation_space = Box(-high, high, (4,), np.float32)
        self.action_space = Discrete(2)
        self.max_episode_steps = max_episode_steps
        self.np_random = np.random.RandomState(seed)
        self.state = None
        self._t = 0

    def reset(self):
        self.state = self.np_random.uniform(low=-0.05, high=0.05, size=(4,))
        self._t = 0
        return np.array(self.state)

    def step(self, action):
        assert action in (0, 1), action
        x, x_dot, theta, theta_dot = self.state
        force = self.force_mag if action == 1 else -self.force_mag
        costheta, sintheta = math.cos(theta), math.sin(theta)
        total_mass = self.masspole + self.masscart
        polemass_length = self.masspole * self.length
        temp = (force + polemass_length * theta_dot ** 2 * sintheta) / total_mass
        thetaacc = (self.gravity * sintheta - costheta * temp) / (
            self.length * (4.0 / 3.0 - self.masspole * costheta ** 2 / total_mass))
        xacc = temp - polemass_length * thetaacc * costheta / total_mass
        x = x + self.tau * x_dot
        x_dot = x_dot + self.tau * xacc
        theta = theta + self.tau * theta_dot
        theta_dot = theta_dot + self.tau * thetaacc
        self.state = (x, x_dot, theta, theta_dot)
        self._t += 1
        done = bool(x < -self.x_threshold or x > self.x_threshold or theta < -self.theta_threshold
                    or theta > self.theta_threshold or self._t >= self.max_episode_steps)
        return np.array(self.state), 1.0, done, {}


class Acrobot:
    """gym 0.17.3's Acrobot-v1 (classic_control/acrobot.py, the "book" dynamics, no torque noise):
    state (theta1, theta2, omega1, omega2), torque a - 1, one classical RK4 step of dt, the angles
    wrapped into [-pi, pi] by repeated +-2 pi, the velocities clamped to +-4 pi / +-9 pi; terminal
    when -cos theta1 - cos(theta1 + theta2) > 1, reward 0 on a terminal step and -1 otherwise;
    observation (cos theta1, sin theta1, cos theta2, sin theta2, omega1, omega2).  Plain floats,
    every operation rounded once, left to right as written: the definition the device env
    (csrc/env_actor.hpp) follows operation for operation."""
    m1, m2, l1, lc1, lc2, I1, I2, g, dt = 1.0, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0, 9.8, 0.2
    max_vel_1, max_vel_2 = 4 * math.pi, 9 * math.pi

    def __init__(self, max_episode_steps=500, seed=None):
        high = np.array([1.0, 1.0, 1.0, 1.0, self.max_vel_1, self.max_vel_2], dtype=np.float32)
        self.observation_space = Box(-high, high, (6,), np.float32)
        self.action_space = Discrete(3)
        self.max_episode_steps = max_episode_steps
        self.np_random = np.random.RandomState(seed)
        self.state = None
        self._t = 0

    def _obs(self):
        t1, t2, w1, w2 = (float(v) for v in self.state)
        return np.array([math.cos(t1), math.sin(t1), math.cos(t2), math.sin(t2), w1, w2])

    def reset(self):
        self.state = self.np_random.uniform(low=-0.1, high=0.1, size=(4,))
        self._t = 0
        return self._obs()

    def _dsdt(self, y, tau):
        m1, m2, l1, lc1, lc2, I1, I2, g = self.m1, self.m2, self.l1, self.lc1, self.lc2, self.I1, self.I2, self.g
        t1, t2, w1, w2 = y
        c2, s2 = math.cos(t2), math.sin(t2)
        d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + 2.0 * l1 * lc2 * c2) + I1 + I2
        d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2
        phi2 = m2 * lc2 * g * math.cos(t1 + t2 - math.pi / 2.0)
        phi1 = (-m2 * l1 * lc2 * (w2 * w2) * s2 - 2.0 * m2 * l1 * lc2 * w2 * w1 * s2
                + (m1 * lc1 + m2 * l1) * g * math.cos(t1 - math.pi / 2.0) + phi2)
        a2 = (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * (w1 * w1) * s2 - phi2) / (m2 * lc2 * lc2 + I2 - d2 * d2 / d1)
        a1 = -(d2 * a2 + phi1) / d1
        return (w1, w2, a1, a2)

    def step(self, action):
        assert action in (0, 1, 2), action
        y0 = tuple(float(v) for v in self.state)
        tau = float(int(action) - 1)
        dt, dt2, dt6 = self.dt, self.dt / 2.0, self.dt / 6.0
        k1 = self._dsdt(y0, tau)
        k2 = self._dsdt(tuple(y0[j] + dt2 * k1[j] for j in range(4)), tau)
        k3 = self._dsdt(tuple(y0[j] + dt2 * k2[j] for j in range(4)), tau)
        k4 = self._dsdt(tuple(y0[j] + dt * k3[j] for j in range(4)), tau)
        t1, t2, w1, w2 = (y0[j] + dt6 * (k1[j] + 2.0 * k2[j] + 2.0 * k3[j] + k4[j]) for j in range(4))
        two_pi = 2.0 * math.pi
        while t1 > math.pi:
            t1 = t1 - two_pi
        while t1 < -math.pi:
            t1 = t1 + two_pi
        while t2 > math.pi:
            t2 = t2 - two_pi
        while t2 < -math.pi:
            t2 = t2 + two_pi
        w1 = -self.max_vel_1 if w1 < -self.max_vel_1 else (self.max_vel_1 if w1 > self.max_vel_1 else w1)
        w2 = -self.max_vel_2 if w2 < -self.max_vel_2 else (self.max_vel_2 if w2 > self.max_vel_2 else w2)
        self.state = (t1, t2, w1, w2)
        self._t += 1
        terminal = bool(-math.cos(t1) - math.cos(t2 + t1) > 1.0)
        return self._obs(), (0.0 if terminal else -1.0), bool(terminal or self._t >= self.max_episode_steps), {}


class MountainCar:
    """gym 0.17.3's MountainCar-v0 (classic_control/mountain_car.py): state (position, velocity),
    force (a - 1) * 0.001 against gravity 0.0025 cos(3 p), |v| <= 0.07, p in [-1.2, 0.6], the left
    wall inelastic; terminal when p >= 0.5 and v >= 0, reward -1 every step; the observation is
    the state.  The definition the device env (csrc/env_actor.hpp) follows."""
    min_position, max_position, max_speed, goal_position, goal_velocity = -1.2, 0.6, 0.07, 0.5, 0.0
    force, gravity = 0.001, 0.0025

    def __init__(self, max_episode_steps=200, seed=None):
        low = np.array([self.min_position, -self.max_speed], dtype=np.float32)
        high = np.array([self.max_position, self.max_speed], dtype=np.float32)
        self.observation_space = Box(low, high, (2,), np.float32)
        self.action_space = Discrete(3)
        self.max_episode_steps = max_episode_steps
        self.np_random = np.random.RandomState(seed)
        self.state = None
        self._t = 0

    def reset(self):
        self.state = np.array([self.np_random.uniform(low=-0.6, high=-0.4), 0.0])
        self._t = 0
        return np.array(self.state)

    def step(self, action):
        assert action in (0, 1, 2), action
        p, v = (float(x) for x in self.state)
        v = v + (float(int(action) - 1) * self.force + math.cos(3.0 * p) * (-self.gravity))
        v = -self.max_speed if v < -self.max_speed else (self.max_speed if v > self.max_speed else v)
        p = p + v
        p = self.min_position if p < self.min_position else (self.max_position if p > self.max_position else p)
        if p == self.min_position and v < 0.0:
            v = 0.0
        self.state = (p, v)
        self._t += 1
        terminal = bool(p >= self.goal_position and v >= self.goal_velocity)
        return np.array(self.state), -1.0, bool(terminal or self._t >= self.max_episode_steps), {}


class Pendulum:
    """gym 0.17.3's Pendulum-v0 (classic_control/pendulum.py): state (theta, theta_dot), the torque
    u = clip(action[0], -2, 2); theta_dot' = theta_dot + (-3 g / (2 l) sin(theta + pi) + 3 u / (m l^2)) dt,
    theta' = theta + theta_dot' dt, THEN theta_dot' clipped to +-8; reward -(angle_normalize(theta)^2 +
    0.1 theta_dot^2 + 0.001 u^2) of the state before the step; observation (cos theta, sin theta,
    theta_dot); reset uniform in [-pi, pi] x [-1, 1]; no terminal state, only the time limit."""
    max_speed, max_torque, dt, g, m, l = 8.0, 2.0, 0.05, 10.0, 1.0, 1.0

    def __init__(self, max_episode_steps=200, seed=None):
        high = np.array([1.0, 1.0, self.max_speed], dtype=np.float32)
        self.observation_space = Box(-high, high, (3,), np.float32)
        self.action_space = Box(-self.max_torque, self.max_torque, (1,), np.float32)
        self.max_episode_steps = max_episode_steps
        self.np_random = np.random.RandomState(seed)
        self.state = None
        self._t = 0

    def _obs(self):
        th, thdot = (float(v) for v in self.state)
        return np.array([math.cos(th), math.sin(th), thdot])

    def reset(self):
        high = np.array([math.pi, 1.0])
        self.state = self.np_random.uniform(low=-high, high=high)
        self._t = 0
        return self._obs()

    def step(self, action):
        th, thdot = (float(v) for v in self.state)
        u = float(np.clip(np.asarray(action, dtype=np.float64).reshape(-1)[0], -self.max_torque, self.max_torque))
        norm = ((th + math.pi) % (2.0 * math.pi)) - math.pi
        cost = norm ** 2 + 0.1 * thdot ** 2 + 0.001 * (u ** 2)
        newthdot = thdot + (-3.0 * self.g / (2.0 * self.l) * math.sin(th + math.pi)
                            + 3.0 / (self.m * self.l ** 2) * u) * self.dt
        newth = th + newthdot * self.dt
        newthdot = -self.max_speed if newthdot < -self.max_speed else (
            self.max_speed if newthdot > self.max_speed else newthdot)
        self.state = (newth, newthdot)
        self._t += 1
        return self._obs(), -cost, bool(self._t >= self.max_episode_steps), {}


# ALE minimal action-set sizes of the games the configs name (and a few common ones)
ATARI_ACTIONS = {"Pong": 6, "Breakout": 4, "BeamRider": 9, "Seaquest": 18, "SpaceInvaders": 6, "Qbert": 6,
                 "Enduro": 9, "MsPacman": 9, "Asterix": 9, "Boxing": 18, "Freeway": 3}


class SyntheticAtari:
    """the wrapped Atari env's interface (frame-stacked uint8 [4, 84, 84] observations, the
    minimal action set) over synthetic frames: each step shifts the stack and draws a new
    uniform frame; reward +-1 with probability p_reward, episode end with probability p_done"""

    def __init__(self, game, seed=None, p_reward=0.02, p_done=1.0 / 2000, frame_stack=4):
        self.game = game
        self.observation_space = Box(0, 255, (frame_stack, 84, 84), np.uint8)
        self.action_space = Discrete(ATARI_ACTIONS[game])
        self.p_reward, self.p_done = p_reward, p_done
        self.np_random = np.random.RandomState(seed)
        self._stack = None

    def _frame(self):
        return self.np_random.randint(0, 256, (84, 84), dtype=np.uint8)

    def reset(self):
        self._stack = np.stack([self._frame() for _ in range(self.observation_space.shape[0])])
        return self._stack.copy()

    def step(self, action):
        assert 0 <= int(action) < self.action_space.n, action
        self._stack = np.concatenate([self._stack[1:], self._frame()[None]])
        u = self.np_random.rand(2)
        r = float(np.sign(u[0] - 0.5)) if u[0] < self.p_reward or u[0] > 1 - self.p_reward else 0.0
        return self._stack.copy(), r, bool(u[1] < self.p_done), {}


class Paddle:
    """the host restatement of the device game of csrc/game.hpp (VecActors(env="paddle")): all
    integer, so the two agree bit for bit when fed the same draws.

    A ball (4x4, value 255) falls from the top with velocity (vx, vy), bouncing off the side
    walls; the paddle (12x3, value 160, rows 78..80) moves 4 px per step: action 0 stays, odd
    actions move right, even actions > 0 move left, clamped to [0, 72].  When the ball reaches
    the paddle rows (ball_y + 4 > 78) it is resolved: reward +1 if it overlaps the paddle's
    columns, else -1; after `balls_per_episode` balls the episode ends.  Observations are the
    last four 84x84 uint8 frames (reset: the first frame four times, env/util.py:179-209); the
    observation of a step is the render of the state after it -- the terminal state on done,
    the new ball after a spawn.

    state: int32[8] = ball_x, ball_y, vx, vy, paddle_x, balls_left, ep_return, ep_steps.
    draw(env, t) -> three uint32 (c0, c1, c2) for the spawn at step t / the reset at step t
    (t counts this object's step() calls and is not reset by reset(); the first reset is t = 0):
    ball_x = (c0 * 81) >> 32, vx = VX[(c1 * 6) >> 32], vy = VY[(c2 * 2) >> 32].  The device
    draws them from Philox(seed, env, t) on stream 8; the default here is a RandomState."""
    W, BALL, PAD_W, PAD_H, PAD_Y, PAD_SPEED, PAD_START = 84, 4, 12, 3, 78, 4, 36
    VX, VY = (-3, -2, -1, 1, 2, 3), (2, 3)

    def __init__(self, num_actions=6, balls_per_episode=5, seed=None, draw=None, env=0):
        if num_actions < 3 or balls_per_episode < 1:
            raise ValueError("Paddle: num_actions >= 3 (stay / right / left), balls_per_episode >= 1")
        self.observation_space = Box(0, 255, (4, self.W, self.W), np.uint8)
        self.action_space = Discrete(int(num_actions))
        self.balls_per_episode = int(balls_per_episode)
        self.np_random = np.random.RandomState(seed)
        self.draw = draw if draw is not None else self._draw
        self.env = int(env)
        self.t = 0
        self.state = None
        self._stack = None

    def _draw(self, env, t):
        return self.np_random.randint(0, 2 ** 32, 3, dtype=np.uint64).astype(np.uint32)

    def _spawn(self):
        c0, c1, c2 = (int(c) for c in self.draw(self.env, self.t))
        self.state[0:4] = (c0 * (self.W - self.BALL + 1)) >> 32, 0, self.VX[(c1 * 6) >> 32], self.VY[(c2 * 2) >> 32]

    def render(self, state=None):
        """the 84x84 uint8 frame of a state (default: the current one); the ball over the paddle"""
        bx, by, _, _, px = (int(v) for v in (self.state if state is None else state)[:5])
        f = np.zeros((self.W, self.W), np.uint8)
        f[self.PAD_Y:self.PAD_Y + self.PAD_H, px:px + self.PAD_W] = 160
        f[by:by + self.BALL, bx:bx + self.BALL] = 255
        return f

    def reset(self):
        self.state = np.zeros(8, np.int32)
        self.state[4:8] = self.PAD_START, self.balls_per_episode, 0, 0
        self._spawn()
        self._stack = np.repeat(self.render()[None], 4, axis=0)
        return self._stack.copy()

    def step(self, action):
        a = int(action)
        assert 0 <= a < self.action_space.n, action
        bx, by, vx, vy, px, balls, ret, steps = (int(v) for v in self.state)
        px = min(max(px + (0 if a == 0 else (self.PAD_SPEED if a & 1 else -self.PAD_SPEED)), 0), self.W - self.PAD_W)
        bx += vx
        if bx < 0:
            bx, vx = -bx, -vx
        elif bx > self.W - self.BALL:
            bx, vx = 2 * (self.W - self.BALL) - bx, -vx
        by += vy
        steps += 1
        self.t += 1
        reward, done = 0.0, False
        resolved = by + self.BALL > self.PAD_Y
        if resolved:
            reward = 1.0 if (bx + self.BALL > px and bx < px + self.PAD_W) else -1.0
            ret += int(reward)
            balls -= 1
            done = balls == 0
        self.state[:] = bx, by, vx, vy, px, balls, ret, steps
        if resolved and not done:
            self._spawn()
        self._stack = np.concatenate([self._stack[1:], self.render()[None]])
        return self._stack.copy(), reward, done, {}


def make(name, **kwargs):
    """reth.env.make (env/util.py:305-316) for the environments this build carries"""
    if name == "Paddle-v0":
        return Paddle(**kwargs)
    if name == "CartPole-v0":
        return CartPole(200, **kwargs)
    if name == "CartPole-v1":
        return CartPole(500, **kwargs)
    if name == "Acrobot-v1":
        return Acrobot(500, **kwargs)
    if name == "MountainCar-v0":
        return MountainCar(200, **kwargs)
    name = name.strip()
    if name.endswith("NoFrameskip-v4") and name[: -len("NoFrameskip-v4")] in ATARI_ACTIONS:
        return SyntheticAtari(name[: -len("NoFrameskip-v4")], **kwargs)
    raise NotImplementedError(f"environment {name!r}: gym/ALE are not part of this build (CartPole-v0/v1, Acrobot-v1 "
                              "and MountainCar-v0 are restated, Paddle-v0 is the device game's host form, Atari names get SyntheticAtari; "
                              "Atari observations: "
                              "reth_amd.atari.AtariPreprocessor)")


HOST_ONLY = {"Pendulum-v0": lambda **kwargs: Pendulum(200, **kwargs)}


def make_host(name, **kwargs):
    """make(), plus the environments that exist on the host alone (continuous actions, no device
    form): Pendulum-v0.  reth.env.make and the presets' get_env resolve names through this."""
    if name in HOST_ONLY:
        return HOST_ONLY[name](**kwargs)
    return make(name, **kwargs)
