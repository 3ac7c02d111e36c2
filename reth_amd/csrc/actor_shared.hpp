// Device functions of the actor side shared by actor.hip (the conv path's VecActors kernels) and
// the 1-D actor sets compiled into qnet.hip (env_actor.hpp, mlp_actor.hpp, ddpg_actor.hpp): the
// per-env Philox block, the ε-greedy draws, the per-actor n-step adder and its handle.  One
// definition, two translation units.
//
// Reference: reth/reth/utils/exploration.py:26-31 (RandomExploration.act),
// reth/reth/utils/nstep_adder.py:5-28 (NStepAdder).
#pragma once
#include "common.hpp"

namespace rth {

// ------------------------------------------------------------------ per-env draws
// c = the Philox4x32-10 block of (seed, env i, step t, stream word w), a pure function of the four:
// the reset draws and the OU normals of env_actor.hpp / ddpg_actor.hpp (their headers: the counter)
__device__ __forceinline__ void env_philox_block(uint64_t seed, int64_t i, int64_t t, uint32_t w, uint32_t (&c)[4]) {
  c[0] = (uint32_t)i, c[1] = (uint32_t)t, c[2] = (uint32_t)((uint64_t)t >> 32), c[3] = w;
  philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ------------------------------------------------------------------ epsilon-greedy
// the exploration draws of actor i at `counter`: the random action when u < eps_i, else -1 (act
// greedily).  u = Philox(seed, counter, lane i, STREAM_EXPLORE) as a 53-bit uniform; the random
// action = (c[0] * A) >> 32 of the block {i, counter lo, counter hi, STREAM_RANDACT}.
__device__ inline int64_t eps_explore_draw(int64_t i, int A, double eps_i, const double *__restrict__ u_in,
                                           const int64_t *__restrict__ ra_in, uint64_t seed, uint64_t counter) {
  const double u = u_in ? u_in[i] : philox_uniform(seed, counter, (uint32_t)i, STREAM_EXPLORE);
  if (!(u < eps_i)) return -1;
  if (ra_in) return ra_in[i];
  uint32_t c[4] = {(uint32_t)i, (uint32_t)counter, (uint32_t)(counter >> 32), STREAM_RANDACT};
  philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (int64_t)(((uint64_t)c[0] * (uint64_t)A) >> 32);  // uniform in [0, A)
}

// One lane per actor: A <= 18 for Atari, so the row argmax is a short in-register loop and
// the launch is one wave per 64 actors.
__device__ inline int64_t eps_greedy_one(const float *__restrict__ q, int64_t i, int A, int dueling,
                                         const double *__restrict__ eps, const double *__restrict__ u_in,
                                         const int64_t *__restrict__ ra_in, uint64_t seed, uint64_t counter) {
  const int64_t ra = eps_explore_draw(i, A, eps[i], u_in, ra_in, seed, counter);
  if (ra >= 0) return ra;
  float qr[kMaxActions];
  q_row(q + i * (A + dueling), A, dueling, qr);
  return argmax_first(qr, A);
}

// ------------------------------------------------------------------ n-step adder
// Per actor: a deque of up to n pending rows, position 0 = newest (appendleft), SoA in HBM.
struct NStepState {
  int32_t *count;
  int64_t *s0, *a, *s1;
  float *r, *done;
};

__device__ inline void nstep_push_one(const NStepState &st, int64_t i, int n, double gamma, int mode, int64_t s0,
                                      int64_t a, float rn, int64_t s1n, float done, int32_t *__restrict__ emit,
                                      int64_t *__restrict__ s0_out, int64_t *__restrict__ a_out,
                                      float *__restrict__ r_out, int64_t *__restrict__ s1_out,
                                      float *__restrict__ done_out) {
  const int64_t base = i * n;
  int count = st.count[i];
  int emitted = 0;
  if (count == n) {  // deque full: pop the oldest (nstep_adder.py:13-14)
    const int64_t k = base + count - 1;
    s0_out[i] = st.s0[k];
    a_out[i] = st.a[k];
    r_out[i] = st.r[k];
    s1_out[i] = st.s1[k];
    done_out[i] = st.done[k];
    --count;
    emitted = 1;
  }
  emit[i] = emitted;
  double t_gamma = gamma;
  for (int k = 0; k < count; ++k) {  // newest -> oldest (nstep_adder.py:16-25)
    const int64_t p = base + k;
    if (st.done[p] != 0.0f) break;
    if (mode == 0)  // numpy 1.19: f64 product, += casts back to the f32 row
      st.r[p] = (float)radd((double)st.r[p], rmul(t_gamma, (double)rn));
    else            // numpy 2 / NEP 50: the python float is weak, product stays f32
      st.r[p] = radd(st.r[p], rmul((float)t_gamma, rn));
    t_gamma = rmul(t_gamma, gamma);
    st.s1[p] = s1n;
  }
  for (int k = count; k > 0; --k) {  // appendleft
    const int64_t p = base + k;
    st.s0[p] = st.s0[p - 1];
    st.a[p] = st.a[p - 1];
    st.r[p] = st.r[p - 1];
    st.s1[p] = st.s1[p - 1];
    st.done[p] = st.done[p - 1];
  }
  st.s0[base] = s0;
  st.a[base] = a;
  st.r[base] = rn;
  st.s1[base] = s1n;
  st.done[base] = done;
  st.count[i] = count + 1;
}

}  // namespace rth

// rth_nstep (include/reth_hip.h): created and destroyed in actor.hip
struct rth_nstep {
  int64_t N;
  int32_t n;
  double gamma;
  int32_t mode;
  int device;
  void *mem;
  rth::NStepState st;
};
