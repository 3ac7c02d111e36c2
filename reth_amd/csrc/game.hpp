// "Paddle": a device-resident pixel game for the conv path's actors -- one instance per actor,
// all-integer rules, 84x84 uint8 frames rendered straight into the actors' frame ring.  Its reward
// and episode end follow from the action, so the closed Ape-X loop (act -> env -> n-step -> PER ->
// update -> weights slot -> actors) has something to learn; the synthetic env's do not.
// envs.Paddle restates these rules on the host, bit for bit.
//
// It honours the contract of the reference's host loop: reth/reth/presets/worker.py:128-155
// (Worker.step: act, env.step, env.reset() on done, the terminal observation kept as the done
// row's s1) and reth/reth/env/util.py:179-209 (FrameStack: reset = the first frame k times, step =
// drop the oldest frame, append the new one).
//
// Frame: background 0, ball 255 (4x4, top-left ball_x, ball_y), paddle 160 (12 wide x 3 high, rows
// 78..80, left edge paddle_x); the ball is drawn over the paddle.
// State: int32[8] = ball_x, ball_y, vx, vy, paddle_x, balls_left, ep_return, ep_steps.
//
// Step, in this order:
//   1. paddle: a == 0 stays, odd a moves +4, even a > 0 moves -4, clamped to [0, 72]
//   2. ball_x += vx; ball_x < 0: ball_x = -ball_x, vx = -vx; else ball_x > 80: ball_x = 160 -
//      ball_x, vx = -vx
//   3. ball_y += vy; ep_steps += 1
//   4. ball_y + 4 > 78: the ball is resolved -- reward +1 if ball_x + 4 > paddle_x and ball_x <
//      paddle_x + 12, else -1; ep_return += reward; balls_left -= 1; balls_left == 0: done, else a
//      new ball is spawned
//   5. otherwise reward 0
// The observation of a step is the render of the state after it: on done the terminal state (the
// ball at the paddle rows), after a spawn the new ball.
//
// Draws (a spawn at step t, the reset at t = 0 and at the step t whose episode ended; never both at
// one t): one Philox4x32-10 block per (seed, env i, t),
//     counter = {(uint32) i, (uint32) t, (uint32) (t >> 32), STREAM_GAME (= 8)}
//     key     = {(uint32) seed, (uint32) (seed >> 32)}
// (eps_explore_draw's layout), and of its output words c[k]:
//     ball_x = (c[0] * 81) >> 32, ball_y = 0, vx = {-3,-2,-1,1,2,3}[(c[1] * 6) >> 32],
//     vy = {2,3}[(c[2] * 2) >> 32].
// A reset also sets paddle_x = 36, balls_left = balls_per_episode, ep_return = ep_steps = 0.
#pragma once
#include "actor_shared.hpp"

namespace rth {

constexpr uint32_t STREAM_GAME = 8u;
constexpr int kGameW = 84, kGameBall = 4, kGamePadW = 12, kGamePadH = 3, kGamePadY = 78, kGamePadSpeed = 4;
constexpr int kGamePadMax = kGameW - kGamePadW, kGameBallMax = kGameW - kGameBall, kGamePadStart = 36;

struct GameState {
  int32_t bx, by, vx, vy, px, balls, ret, steps;
};

__device__ __forceinline__ GameState game_load(const int32_t *__restrict__ p) {
  const int4 a = reinterpret_cast<const int4 *>(p)[0], b = reinterpret_cast<const int4 *>(p)[1];
  return GameState{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

__device__ __forceinline__ void game_store(int32_t *__restrict__ p, const GameState &s) {
  reinterpret_cast<int4 *>(p)[0] = make_int4(s.bx, s.by, s.vx, s.vy);
  reinterpret_cast<int4 *>(p)[1] = make_int4(s.px, s.balls, s.ret, s.steps);
}

// a new ball from the block of (seed, env i, t)
__device__ inline void game_spawn(GameState &s, uint64_t seed, int64_t i, int64_t t) {
  uint32_t c[4] = {(uint32_t)i, (uint32_t)t, (uint32_t)((uint64_t)t >> 32), STREAM_GAME};
  philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int kx = (int)(((uint64_t)c[1] * 6u) >> 32);
  s.bx = (int32_t)(((uint64_t)c[0] * (uint64_t)(kGameBallMax + 1)) >> 32);
  s.by = 0;
  s.vx = kx < 3 ? kx - 3 : kx - 2;  // {-3,-2,-1,1,2,3}[kx]
  s.vy = 2 + (int)(((uint64_t)c[2] * 2u) >> 32);
}

__device__ inline GameState game_reset_state(uint64_t seed, int64_t i, int64_t t, int balls_per_episode) {
  GameState s;
  s.px = kGamePadStart, s.balls = balls_per_episode, s.ret = 0, s.steps = 0;
  game_spawn(s, seed, i, t);
  return s;
}

struct GameStep {
  int reward;
  bool done;
};

// the rules above on s, in place; on done s is the terminal state (the caller resets).  A pure
// function of its arguments: every lane of an env's workgroup may compute it.
__device__ inline GameStep game_step_one(GameState &s, int64_t action, uint64_t seed, int64_t i, int64_t t) {
  int px = s.px + (action <= 0 ? 0 : ((action & 1) ? kGamePadSpeed : -kGamePadSpeed));
  s.px = px < 0 ? 0 : (px > kGamePadMax ? kGamePadMax : px);
  int bx = s.bx + s.vx;
  if (bx < 0) {
    bx = -bx, s.vx = -s.vx;
  } else if (bx > kGameBallMax) {
    bx = 2 * kGameBallMax - bx, s.vx = -s.vx;
  }
  s.bx = bx;
  s.by += s.vy;
  s.steps += 1;
  if (s.by + kGameBall <= kGamePadY) return GameStep{0, false};
  const int reward = (bx + kGameBall > s.px && bx < s.px + kGamePadW) ? 1 : -1;
  s.ret += reward;
  s.balls -= 1;
  if (s.balls == 0) return GameStep{reward, true};
  game_spawn(s, seed, i, t);
  return GameStep{reward, false};
}

// the 16 bytes of chunk `chunk` (bytes 16 chunk .. 16 chunk + 15, row-major) of the state's frame
__device__ inline uint4 game_frame_bytes(const GameState &s, int chunk) {
  const int b0 = chunk * 16;
  int row = b0 / kGameW, col = b0 - row * kGameW;
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ball = (unsigned)(row - s.by) < (unsigned)kGameBall && (unsigned)(col - s.bx) < (unsigned)kGameBall;
      const bool pad = (unsigned)(row - kGamePadY) < (unsigned)kGamePadH && (unsigned)(col - s.px) < (unsigned)kGamePadW;
      word |= (ball ? 255u : (pad ? 160u : 0u)) << (8 * j);
      if (++col == kGameW) col = 0, ++row;
    }
    w[k] = word;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace rth
