// rth_cartpole_reset / rth_mlp_actor_step: the CartPole actors' entry points, kept for their
// callers, as adapters onto env_actor.hpp -- rth_mlp_actor_args is rth_env_actor_args without the
// env id and the return statistics.  They run the shared checks and launch
// k_env_reset<RTH_ENV_CARTPOLE> / k_env_actor_step<RTH_ENV_CARTPOLE> with ret_stats = NULL: what
// rth_env_reset / rth_env_actor_step compute for CartPole, bit for bit, minus those statistics.
#pragma once
#include "env_actor.hpp"

namespace rth {

inline int cartpole_actor_run(const char *fn, const rth_nstep *h, const rth_mlp_actor_args *m, bool step,
                              void *stream) {
  if (!m) return env_actor_run(fn, h, nullptr, step, false, stream);
  const rth_env_actor_args x{m->params, RTH_ENV_CARTPOLE, m->D,      m->H,        m->A,        m->state,  m->ep_steps,
                             m->t_dev,  m->stats,         nullptr,   m->obs_ring, m->cur_slot, m->eps,    m->action_in,
                             m->action, m->reward,        m->done,   m->s0_h,     m->s1_h,     m->emit,   m->row_s0,
                             m->row_a,  m->row_s1,        m->row_r,  m->row_done, m->row_obs0, m->row_obs1, m->q_out,
                             m->seed,   m->N,             m->ring,   m->max_episode_steps};
  return env_actor_run(fn, h, &x, step, false, stream);
}

}  // namespace rth

extern "C" {

int rth_cartpole_reset(const rth_mlp_actor_args *args, void *stream) {
  return rth::cartpole_actor_run("rth_cartpole_reset", nullptr, args, false, stream);
}

int rth_mlp_actor_step(rth_nstep *h, const rth_mlp_actor_args *args, void *stream) {
  return rth::cartpole_actor_run("rth_mlp_actor_step", h, args, true, stream);
}

}  // extern "C"
