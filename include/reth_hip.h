/*
 * reth_hip.h -- C ABI of libreth_hip.so, the MI355X (gfx950) hot path of Reth's Ape-X DQN
 * rollout -> prioritized replay -> update loop.
 *
 * Conventions
 *   - every call returns int: 0 (RTH_OK) or a negative RTH_ERR_*; rth_last_error() gives the
 *     message of the last failure on the calling thread.
 *   - pointers named *_dev are device (HBM) pointers; everything else is host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); all work
 *     is enqueued asynchronously on it, no call synchronises the device.
 *   - handles own their device storage; calls on one handle must be serialised by the
 *     caller (the reference's single-owner sampler process, server/sampler_loop.py:6-42).
 *   - index arrays are int64 (the reference mixes int32 appends, fifo_policy.py:13, and
 *     int64 updates; both widen losslessly).
 *
 * The reference is pure Python (numba/numpy/torch); each entry point names the Python
 * interface it replaces (paths relative to the sosp2021/Reth checkout).  The Python
 * binding (reth_amd/_lib.py, ctypes) re-exposes the reference's own signatures.
 */
#ifndef RETH_HIP_H
#define RETH_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTH_OK 0
#define RTH_ERR_INVALID -1   /* bad argument (the reference's `assert`s) */
#define RTH_ERR_HIP -2       /* a HIP runtime call failed */
#define RTH_ERR_NOMEM -3     /* device allocation failed */

/* element types of replay columns */
#define RTH_U8 0
#define RTH_I32 1
#define RTH_I64 2
#define RTH_F32 3
#define RTH_F64 4
#define RTH_MAX_COLS 8
/* priority "dtype" for the tree/replay update calls: float64 priorities stored as given,
 * without (w + 1e-6) ** alpha (NumbaSumTree.update; reth.buffer.PrioritizedBuffer.append) */
#define RTH_PRIO_RAW 16
/* in_dtype of a frame-stack column of a frame-store replay: each stored row is out_planes
 * int32 frame ids into the replay's frame store (rth_replay_frames_attach); row_elems is the
 * sampled stack (out_planes frames x frame bytes, out_dtype RTH_U8), assembled by the gather */
#define RTH_FRAMES 8

const char *rth_last_error(void);
/* how many tree-update top passes timed out waiting for their subtree workgroups since the
 * library was loaded (the concurrent top workgroup's bounded wait; a timed-out pass leaves the
 * levels above the subtree roots unwritten rather than maintaining them from stale sums).
 * Expected 0; the tests assert it. */
int rth_tree_update_timeouts(int64_t *out);
/* library build/ABI version (major*10000 + minor*100 + patch) */
int rth_version(void);
/* the source tree the library was compiled from: 40 hex digits, the SHA-1 over the lines
 * "<git blob id> <path>\n" of reth_amd/csrc/ and include/reth_hip.h in path order
 * (reth_amd._lib.source_build_id; reproducible from `git ls-tree -r HEAD`) */
const char *rth_build_id(void);
/* hipGraphUpload of a captured graph's executable on `stream` (plumbing for the captured
 * actor / learner blocks, reth_amd.apex.ApexDQN.upload_graphs: a graph's first launch then
 * carries no upload) */
int rth_graph_upload(void *graph_exec, void *stream);
/* The number of nodes the next operation captured on `stream` would depend on (0 at the start
 * of a capture and until something is captured), or -1 when the stream is not capturing:
 * ApexDQN's graph cuts skip a part that would be empty (two boundaries back to back). */
int rth_stream_capture_deps(void *stream);

/* ------------------------------------------------------------------------------------
 * In-order heap sum-tree, fp64, resident in HBM.
 * Replaces reth_buffer/reth_buffer/utils/sumtree.py:82-113 (NumbaSumTree and the numba
 * kernels _numba_maintain_node :5-21, _numba_maintain :24-31, _numba_find_index :34-58,
 * _numba_update :61-67, _numba_sample :70-79).  Bit-exact with the sequential reference.
 * ---------------------------------------------------------------------------------- */
typedef struct rth_sumtree rth_sumtree;
int rth_sumtree_create(int64_t capacity, int device, rth_sumtree **out); /* NumbaSumTree.__init__ :83-87 */
int rth_sumtree_destroy(rth_sumtree *t);
int rth_sumtree_clear(rth_sumtree *t, void *stream);                    /* NumbaSumTree.clear :98-101 */
/* NumbaSumTree.update :103-104 -> _numba_update: val[idx]=w, maintain, in order */
int rth_sumtree_update(rth_sumtree *t, const int64_t *idx_dev, const double *w_dev, int64_t n,
                       void *stream);
/* _numba_find_index :34-58, one target per element */
int rth_sumtree_find(rth_sumtree *t, const double *targets_dev, int64_t n, int64_t *idx_out_dev,
                     double *val_out_dev, void *stream);
/* NumbaSumTree.sample :112-113 -> _numba_sample :70-79.  uniforms_dev (n = batch) replaces
 * numba's internal np.random stream when non-NULL (the parity hook); when NULL the
 * uniforms come from Philox4x32-10(seed, counter). */
int rth_sumtree_sample(rth_sumtree *t, int64_t batch, const double *uniforms_dev, uint64_t seed,
                       uint64_t counter, int64_t *idx_out_dev, double *val_out_dev, void *stream);
/* out2_dev[0] = NumbaSumTree.sum() :106-107, out2_dev[1] = NumbaSumTree.min() :109-110 */
int rth_sumtree_stats(rth_sumtree *t, double *out2_dev, void *stream);
/* the three fp64 arrays of the reference layout (each [capacity], device) */
int rth_sumtree_export(rth_sumtree *t, double *sum_dev, double *min_dev, double *val_dev, void *stream);
int rth_sumtree_import(rth_sumtree *t, const double *sum_dev, const double *min_dev,
                       const double *val_dev, void *stream);
int64_t rth_sumtree_capacity(const rth_sumtree *t);

/* ------------------------------------------------------------------------------------
 * PER sampler on a sum-tree.  Replaces reth_buffer/reth_buffer/sampler/per_sampler.py:5-35.
 * Schedules (alpha/beta, utils/schedule.py) stay on the host; the current values are args.
 * ---------------------------------------------------------------------------------- */
/* PERSampler._normalize_weights :16-17: out = (w + 1e-6) ** alpha  (float32) */
int rth_per_normalize(const float *w_dev, int64_t n, float alpha, float *out_dev, void *stream);
/* PERSampler.update :34-35: tree.update(idx, _normalize_weights(td_abs)) fused in one pass.
 * td_abs_dev is float32 (td_dtype RTH_F32: normalised in f32 with (float)alpha, like numpy
 * on an f4 array) or float64 (RTH_F64: normalised in f64). */
int rth_per_update(rth_sumtree *t, const int64_t *idx_dev, const void *td_abs_dev, int32_t td_dtype,
                   int64_t n, double alpha, void *stream);
/* PERSampler.sample :24-28: (idx, (p / tree.min()) ** -beta) */
int rth_per_sample(rth_sumtree *t, int64_t batch, double beta, const double *uniforms_dev,
                   uint64_t seed, uint64_t counter, int64_t *idx_out_dev, double *isw_out_dev,
                   void *stream);

/* ------------------------------------------------------------------------------------
 * Replay shard in HBM: FIFO slot allocation + column storage + PER tree.
 * Replaces the reth_buffer service: append_loop (server/main_loop.py:21-61: deserialize,
 * FIFOPolicy.get_indices, LMDB put, forward to sampler), sampler_loop
 * (server/sampler_loop.py:6-42), Client.append / update_priorities (client/client.py:21-39)
 * and the loaders' row fetch (client/torch_cuda_loader.py:20-66, numpy_loader.py:27-51).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  int64_t row_elems;  /* elements per row (product of the per-row shape) */
  int32_t in_dtype;   /* storage type == type appended (RTH_U8 ... RTH_F64) */
  int32_t out_dtype;  /* type produced on sample: == in_dtype, or RTH_F32 from RTH_U8 */
  int32_t out_planes; /* 0: same element order; k > 0 (RTH_U8 -> RTH_F32 only): the row is k
                         planes (C,H,W) and is produced channels-last (H,W,C) */
  int32_t reserved;
} rth_col_desc;

/* a column source for an append: rows[i] (or i when rows_dev == NULL) of base_dev, rows
 * row_stride_bytes apart (0 = dense).  src_dtype: element type of the source rows; 0 or the
 * column's storage type = as stored; RTH_F32 into a RTH_U8 column narrows whole-number
 * pixels 0..255 (frames the reference's actors send as float32, test/apex-dqn/worker.py:46-50) */
typedef struct {
  const void *base_dev;
  const int64_t *rows_dev;
  int64_t row_stride_bytes;
  int32_t src_dtype;
  int32_t reserved;
} rth_src;

/* A PERSampler schedule (reth_buffer/reth_buffer/utils/schedule.py:4-52):
 * const: start; linear: start + (end - start) * k / max_steps;
 * exp: end - (end - start) * exp(-k / max_steps); k = steps taken, clamped to max_steps. */
#define RTH_SCHED_CONST 0
#define RTH_SCHED_LINEAR 1
#define RTH_SCHED_EXP 2
typedef struct {
  int32_t method;
  int32_t reserved;
  double start;
  double end;
  int64_t max_steps;
} rth_schedule;

typedef struct rth_replay rth_replay;
/* Samplers of a shard (reth_buffer/reth_buffer/sampler/):
 *   RTH_SAMPLER_PER      PERSampler (per_sampler.py:5-35): sum-tree, IS weights;
 *   RTH_SAMPLER_UNIFORM  UniformSampler (uniform_sampler.py:6-25): updates append their
 *                        indices to a list until it holds `capacity`; a sample draws
 *                        list[floor(u * len)], weights 1;
 *   RTH_SAMPLER_FIFO     FIFOSampler (fifo_sampler.py:8-29): updates push (index, weight)
 *                        into a queue of at most `capacity` (oldest dropped); a sample pops
 *                        the `batch` oldest, weights as pushed. */
#define RTH_SAMPLER_PER 0
#define RTH_SAMPLER_UNIFORM 1
#define RTH_SAMPLER_FIFO 2
/* The shard owns its sampler state (per_sampler.py:5-12): the alpha / beta schedules and
 * the step count, the FIFO tail, the sample-call counter and the uniform list / FIFO queue
 * live in device memory, so every launch below is argument-invariant from step to step
 * (HIP-graph replayable). */
int rth_replay_create(int64_t capacity, int32_t n_cols, const rth_col_desc *cols, int32_t sampler,
                      const rth_schedule *alpha, const rth_schedule *beta, int device, uint64_t seed,
                      rth_replay **out);
int rth_replay_destroy(rth_replay *h);
/* Client.append + append_loop + PERSampler.update: rows go to FIFO slots
 * tail, tail+1, ... mod capacity (FIFOPolicy :11-18), priorities (td_abs + 1e-6)**alpha
 * into the tree.  idx_out_dev (nullable) receives the slots. */
int rth_replay_append(rth_replay *h, const rth_src *srcs, const void *td_abs_dev, int32_t td_dtype,
                      int64_t n, int64_t *idx_out_dev, void *stream);
/* sampler_loop sample + loader gather: PER-sample `batch` rows (uniforms_dev nullable, see
 * rth_sumtree_sample) with the current beta, write IS weights, and gather every column into
 * out_cols_dev[c] ([batch, row] of out_dtype; NULL = no gather) -- TorchCudaLoader.sample's
 * (data, indices, weights).  The sampler's device call counter (the Philox counter of the
 * next sample) is advanced by the gather kernel; with out_cols_dev NULL, by the next
 * rth_replay_gather on this handle, or else by the next sample before it draws. */
int rth_replay_sample(rth_replay *h, int64_t batch, const double *uniforms_dev,
                      void *const *out_cols_dev, int64_t *idx_out_dev, double *isw_out_dev,
                      void *stream);
/* Client.update_priorities :37-39 -> sampler_loop :31-35: step != 0 advances the alpha/beta
 * schedules first (PERSampler.on_step), then PERSampler.update */
int rth_replay_update_priorities(rth_replay *h, const int64_t *idx_dev, const void *td_abs_dev,
                                 int32_t td_dtype, int64_t n, int32_t step, void *stream);
/* The same, deferred (PER shards): the update is recorded and applied by the shard's next
 * tree launch -- merged into the next rth_replay_append's (one launch instead of two), or on
 * its own before a sample / immediate update / rth_replay_flush -- which is the order the
 * reference's sampler applies its messages in.  idx_dev / td_abs_dev must stay valid (and
 * unmodified) until then.  Host counters are updated at once.  Call rth_replay_flush before
 * reading the tree through rth_replay_tree. */
int rth_replay_update_priorities_deferred(rth_replay *h, const int64_t *idx_dev, const void *td_abs_dev,
                                          int32_t td_dtype, int64_t n, int32_t step, void *stream);
int rth_replay_flush(rth_replay *h, void *stream);
/* NumpyLoader row fetch (numpy_loader.py:381-396) for explicit indices */
int rth_replay_gather(rth_replay *h, const int64_t *idx_dev, int64_t n, void *const *out_cols_dev,
                      void *stream);
/* host mirrors of the service counters: rows stored, FIFO tail, sampler cnt (appended +
 * re-prioritised, sampler_loop.py:36), sample calls issued, schedule steps taken, and the
 * sampler's own length (PER: rows stored; uniform: list length; FIFO: queued entries --
 * FIFOSampler.ready_sample is len > batch) */
int rth_replay_info(const rth_replay *h, int64_t *size, int64_t *tail, int64_t *cnt,
                    int64_t *sample_calls, int64_t *sched_steps, int64_t *sampler_len);
/* uniform row draw of NumpyBuffer.sample (reth/reth/buffer/buffer.py:88-90,
 * np.random.choice(size, batch)): idx[i] = floor(u_i * size), u_i = uniforms_dev[i] or
 * Philox(seed, counter (or *counter_dev), i) */
int rth_uniform_indices(int64_t size, int64_t batch, const double *uniforms_dev, uint64_t seed, uint64_t counter,
                        const int64_t *counter_dev, int64_t *idx_out_dev, void *stream);
rth_sumtree *rth_replay_tree(rth_replay *h);
/* Live per-kernel timing (the bench's in-loop HBM rooflines; no reference counterpart):
 * events[2k] / events[2k+1] (hipEvent_t, nullable) are recorded on the launch stream right
 * before / after the next launch of kind k of this handle, once, then disarmed:
 *   RTH_TIMING_TREE_UPDATE  the append's tree launch (k_tree_update_sub: the append's
 *                           priorities + a deferred update_priorities)
 *   RTH_TIMING_SAMPLE       the PER sample (k_tree_sample + IS weights)
 *   RTH_TIMING_GATHER       the gather (k_copy_rows into the learner batch)
 *   RTH_TIMING_INSERT       the append's row copy (k_copy_rows into the FIFO slots)
 * n = number of events given (<= RTH_TIMING_SLOTS); n = 0 disarms all.  fired_out (nullable)
 * receives the bit mask of the slots whose events were recorded since the previous call. */
#define RTH_TIMING_TREE_UPDATE 0
#define RTH_TIMING_SAMPLE 2
#define RTH_TIMING_GATHER 4
#define RTH_TIMING_INSERT 6
#define RTH_TIMING_SLOTS 8
int rth_replay_set_timing(rth_replay *h, void *const *events, int32_t n, int32_t *fired_out);
/* device pointer of column c's storage ([capacity, row] of in_dtype) */
void *rth_replay_column(rth_replay *h, int32_t c);
/* Frame de-duplicated storage (Breakout's 4 M rows are 225.9 GB as full uint8
 * rows, ~30 GB with each frame stored once).  The reference stores every row's two float32
 * stacks (test/apex-dqn/worker.py:44-51); here the RTH_FRAMES columns hold each stack as K
 * frame ids into a frame store of n_frames frames of frame_bytes, owned by the handle, and
 * the gather assembles the same uint8 stacks the full rows would hold.  store_out / head_out
 * (nullable): the store ([n_frames, frame_bytes]) and its device head (frames pushed).  The
 * store is a ring: it must hold every frame a live row references -- a row's oldest frame is
 * at most n + 4 actor steps older than the row, and a row lives capacity / N appends, and a
 * step pushes at most 2 N frames -- so n_frames >= 2 capacity + 2 (n + 16) N with N actors
 * covers every episode-end pattern (reth_amd.apex.ApexDQN.frame_store_frames, "hard").
 * *head_out = the device word holding the next frame id (a second word after it is internal). */
int rth_replay_frames_attach(rth_replay *h, int64_t n_frames, int64_t frame_bytes, void **store_out,
                             int64_t **head_out);
/* One vectorised actor step's frames into the store (VecActors, after the env step):
 * ring_dev = the actors' stack ring [N * ring_slots (+ extra), stack, frame], sid_dev = its
 * stack table ([same stacks, stack] int32 frame ids).  mode 0: stack s1_h[i] is stack s0_h[i]
 * shifted by one frame + a new frame (FrameStack.step, reth/reth/env/util.py:198-204): the new
 * frame enters the store, sid[s1] = sid[s0][1:] + [its id]; where done_dev[i], actor i's reset
 * stack (slot cur_slot_dev[i], one frame `stack` times: FrameStack.reset, :191-196) enters as one
 * frame.  mode 1: every actor's current stack (slot cur_slot_dev[i]) enters as `stack` frames
 * (the initial observations).  Then the device head advances past them. */
int rth_replay_push_frames(rth_replay *h, const uint8_t *ring_dev, int64_t n, int32_t ring_slots, int32_t stack,
                           const int64_t *s0_h_dev, const int64_t *s1_h_dev, const float *done_dev,
                           const int64_t *cur_slot_dev, int32_t *sid_dev, int32_t mode, void *stream);
/* Frames in place (r05): on = 1 makes the gathers (rth_replay_gather / _sample with out_cols)
 * write each frame-stack column's stored id tuple (int32 [n][4], 16-byte aligned output)
 * instead of the assembled stack; rth_conv1_frames_* read the frames from the store by
 * them.  4-frame stacks only.  on = 0 restores the stacks. */
int rth_replay_frames_ids_out(rth_replay *h, int32_t on);

/* ------------------------------------------------------------------------------------
 * Row copy / gather with optional uint8 -> float32 widening (the loaders' pinned copy +
 * H2D, torch_cuda_loader.py:43-62, as one HBM->HBM kernel).  src/dst row index arrays are
 * nullable (identity).  Strides in bytes.  out_planes as in rth_col_desc (channels-last out).
 * ---------------------------------------------------------------------------------- */
int rth_copy_rows(void *dst_dev, int64_t dst_stride, const int64_t *dst_rows_dev, const void *src_dev,
                  int64_t src_stride, const int64_t *src_rows_dev, int64_t n, int64_t row_elems,
                  int32_t in_dtype, int32_t out_dtype, int32_t out_planes, void *stream);

/* ------------------------------------------------------------------------------------
 * Actor side.
 * ---------------------------------------------------------------------------------- */
/* dueling (rth_eps_greedy, rth_td_huber): q rows hold the network's raw heads -- A
 * advantages then the state value -- and Q = (V + A) - mean(A) is formed in-kernel
 * (dqn_model.py:185-193); rth_td_huber's dq is then d(loss)/d(heads) [B, A+1].  A <= 32. */
/* RandomExploration.act (reth/reth/utils/exploration.py:26-31) over N actors:
 * u < eps[i] ? rand_action : argmax_a q[i, a] (first maximum, dqn_solver.py:126-131).
 * u_dev / rand_action_dev nullable -> Philox(seed, counter); counter_dev (nullable) supplies
 * the counter from device memory instead (graph replay). */
int rth_eps_greedy(const float *q_dev, int64_t N, int64_t A, int32_t dueling, const double *eps_dev,
                   const double *u_dev, const int64_t *rand_action_dev, uint64_t seed,
                   uint64_t counter, const int64_t *counter_dev, int64_t *action_out_dev,
                   void *stream);
/* *counter_dev += delta (device-resident step counters) */
int rth_counter_add(int64_t *counter_dev, int64_t delta, void *stream);

/* NStepAdder (reth/reth/utils/nstep_adder.py:5-28), one adder per actor, rows referencing
 * frame handles.  mode 0 = numpy 1.19 promotion (reference pin), 1 = numpy 2 / NEP 50. */
typedef struct rth_nstep rth_nstep;
int rth_nstep_create(int64_t n_actors, int32_t n_step, double gamma, int32_t mode, int device,
                     rth_nstep **out);
int rth_nstep_destroy(rth_nstep *h);
int rth_nstep_reset(rth_nstep *h, void *stream);
/* push one transition per actor; emit_dev[i] = 1 when actor i's oldest row was popped, its
 * fields in the *_out arrays (row i) */
int rth_nstep_push(rth_nstep *h, const int64_t *s0_dev, const int64_t *a_dev, const float *r_dev,
                   const int64_t *s1_dev, const float *done_dev, int32_t *emit_dev,
                   int64_t *s0_out_dev, int64_t *a_out_dev, float *r_out_dev,
                   int64_t *s1_out_dev, float *done_out_dev, void *stream);

/* Synthetic Pong-shaped environment (no ALE on the box): uint8 (4,84,84) frame stacks kept
 * in a per-actor ring of `ring` stacks.  Step t writes the next stack (shift + one fresh
 * frame) into slot (2t) % ring and, on done, a reset stack (one fresh frame x4, FrameStack
 * reset) into slot (2t+1) % ring.  reward in {-1,0,+1}, P(+-1) = p_reward/2 each;
 * done ~ Bernoulli(p_done).  cur_slot_dev is updated in place; s0/s1 handles
 * (actor*ring + slot) are written for the n-step adder.  Actions do not affect it.
 * t_dev (nullable) supplies t from device memory (graph replay). */
int rth_synth_env_step(uint8_t *frames_dev, int64_t n_actors, int32_t ring, int64_t t,
                       const int64_t *t_dev, int64_t *cur_slot_dev, const int64_t *action_dev, uint64_t seed,
                       float p_reward, float p_done, float *r_out_dev, float *done_out_dev,
                       int64_t *s0_handle_dev, int64_t *s1_handle_dev, void *stream);
/* The tail of one fused actor step, one workgroup per actor: rth_eps_greedy (dueling heads,
 * Philox draws at counter *t_dev) on q, the previous n-step rows' |td| (rth_td_huber with
 * target == online, isw = 1) from the per-stack heads cache -- heads of stack h at
 * qcache[h * (A + 1)] --, rth_synth_env_step at t = *t_dev and rth_nstep_push of the new
 * transition into the row outputs; every value equals the one of those separate calls.
 * td_abs (nullable) skips the rows' |td|. */
typedef struct rth_actor_tail_args {
  const float *q;          /* acting heads [N, A + 1] */
  const double *eps;       /* [N] */
  const int64_t *t_dev;    /* env step / Philox counter */
  int64_t *action;         /* out [N] */
  const float *qcache;
  const int64_t *prev_s0, *prev_a, *prev_s1;
  const float *prev_r, *prev_done;
  float *td_abs;           /* out [N] */
  uint8_t *frames;
  int64_t *cur_slot;
  float *r_out, *done_out; /* out [N] */
  int64_t *s0_h, *s1_h;    /* out [N] */
  uint64_t seed;           /* exploration and env seed */
  int64_t N;
  float gamma_n, p_reward, p_done;
  int32_t ring, A;
  int32_t ext_frames;      /* 1: the env step writes no frame bytes -- rth_atari_env_step fills the
                            * step's stacks from raw frames right after (Atari env mode) */
} rth_actor_tail_args;
/* The fused actor step's first launch (reth_amd/actors.py step_fused): *t_dev += 1 (the
 * step counter rth_actor_tail's ε-greedy and env step read) and rows_out[i] = i * ring +
 * cur_slot[i], the acting stacks' frame-ring rows the torso forward reads (i < n). */
int rth_actor_prologue(int64_t *t_dev, const int64_t *cur_slot_dev, int64_t n, int64_t ring, int64_t *rows_out_dev,
                       void *stream);
int rth_actor_tail(rth_nstep *h, const rth_actor_tail_args *args, int32_t *emit_dev, int64_t *s0_out_dev,
                   int64_t *a_out_dev, float *r_out_dev, int64_t *s1_out_dev, float *done_out_dev, void *stream);
/* initial reset of every actor into slot 1 (t = 0) */
int rth_synth_env_reset(uint8_t *frames_dev, int64_t n_actors, int32_t ring, uint64_t seed,
                        int64_t *cur_slot_dev, void *stream);
/* "Paddle": a device-resident pixel game as the env of the same frame ring (csrc/game.hpp: the
 * exact integer rules, the Philox draws on stream 8 and the render; reth_amd.envs.Paddle restates
 * them on the host bit for bit).  One instance per actor; reward and episode end follow from the
 * action.  It honours the host loop's contract -- reth/reth/presets/worker.py:128-155 (Worker.step:
 * env.step, env.reset() on done, the terminal observation kept as the done row's s1) and
 * reth/reth/env/util.py:179-209 (FrameStack: reset = the first frame x4, step = shift in the new
 * frame) -- with rth_synth_env_step's slot arithmetic: step t writes the next stack into slot
 * (2t) % ring and, on done, the reset stack into (2t + 1) % ring; cur_slot and the s0 / s1 handles
 * are written the same way, so the heads cache, rth_compact_flagged and rth_replay_push_frames work
 * unchanged.  The game's tensors are the caller's; env i's state and stats rows are written by its
 * own workgroup only (no atomics, nothing zero-filled per step). */
typedef struct rth_game_args {
  int32_t *state;            /* [N, 8] ball_x, ball_y, vx, vy, paddle_x, balls_left, ep_return, ep_steps;
                              * 16-byte aligned */
  int64_t *stats;            /* [N, 4] episodes finished, sum of their returns, last return, last length */
  const int64_t *action_in;  /* [N] nullable, rth_game_actor_tail only: overrides the ε-greedy choice */
  uint64_t seed;             /* spawn / reset draws */
  int64_t N;
  int32_t balls_per_episode; /* >= 1 */
  int32_t reserved;
} rth_game_args;
/* env.reset() of every env at t = 0: state from Philox(seed, env, 0), stats = 0, the reset stack
 * (the reset state's frame x4) into ring slot 1, cur_slot = 1.  frames_dev 16-byte aligned. */
int rth_game_reset(const rth_game_args *game, uint8_t *frames_dev, int64_t n_actors, int32_t ring,
                   int64_t *cur_slot_dev, void *stream);
/* one game step per actor with the given actions (any int64: 0 and below stay, odd right, even
 * left), the counterpart of rth_synth_env_step: reward in {-1, 0, +1}, done, handles, the shifted
 * stack with the render of the state after the step (the terminal state on done) and, on done, the
 * reset stack; the env is reset (Philox(seed, env, t)) and its stats row updated. */
int rth_game_env_step(const rth_game_args *game, uint8_t *frames_dev, int64_t n_actors, int32_t ring, int64_t t,
                      const int64_t *t_dev, int64_t *cur_slot_dev, const int64_t *action_dev, float *r_out_dev,
                      float *done_out_dev, int64_t *s0_handle_dev, int64_t *s1_handle_dev, void *stream);
/* rth_actor_tail with the game as the env (p_reward / p_done unused, ext_frames = 0): ε-greedy (or
 * game->action_in; args->q may then be NULL), the previous rows' |td|, rth_game_env_step at
 * t = *t_dev with the chosen action, rth_nstep_push; every value equals the one of those separate
 * calls. */
int rth_game_actor_tail(rth_nstep *h, const rth_actor_tail_args *args, const rth_game_args *game, int32_t *emit_dev,
                        int64_t *s0_out_dev, int64_t *a_out_dev, float *r_out_dev, int64_t *s1_out_dev,
                        float *done_out_dev, void *stream);
/* stream compaction for variable-size device batches: out[0..k) = vals[i] for the i < n with
 * flag[i] != 0, in order of i (at most cap of them), out[k..cap) = fill, *count_out = base + k.
 * The actors use it to list the terminal stacks of the episodes that just ended (flag = done,
 * vals = the step's next-observation handles) behind the next acting batch. */
int rth_compact_flagged(const float *flag_dev, const int64_t *vals_dev, int64_t n, int64_t *out_dev, int64_t cap,
                        int64_t fill, int64_t base, int64_t *count_out_dev, void *stream);

/* ------------------------------------------------------------------------------------
 * Learner: DQNSolver TD error + Huber (reth/reth/algorithm/dqn/dqn_solver.py:68-124).
 * td = q_s0[a] - (r + (gamma_n * q_tgt(s1)[a*]) * (1 - done)),  a* = argmax q_online(s1)
 * (double_q) or argmax q_tgt(s1); loss = mean(smooth_l1(td) * w); dq = dloss/dq_s0.
 * Every output pointer is nullable.  isw_dev is the sampler's fp64 IS weight (cast to f32
 * like ensure_tensor, :105-106), nullable = no weights.
 * ---------------------------------------------------------------------------------- */
int rth_td_huber(const float *q_s0_dev, const float *q_s1_online_dev, const float *q_s1_target_dev,
                 const int64_t *a_dev, const float *r_dev, const float *done_dev,
                 const double *isw_dev, int64_t B, int64_t A, float gamma_n, int32_t double_q,
                 int32_t dueling, float *td_out_dev, float *td_abs_out_dev, float *loss_elem_dev,
                 float *loss_out_dev, float *dq_out_dev, void *stream);

/* ------------------------------------------------------------------------------------
 * Q-network conv epilogue (reth/reth/algorithm/dqn/dqn_model.py:14-20: Conv2d -> ReLU),
 * on channels-last (NHWC) contiguous fp32 activations of `rows` = N*H*W rows x C channels.
 * rth_bias_relu: y = relu(y + bias[c]) in place (the convolution runs without bias).
 * rth_relu_bias_grad: gy = (y > 0) ? g : 0 (threshold_backward) and db[c] = sum of gy over
 * the rows, deterministic; `workspace` holds rth_relu_bias_grad_workspace(C) bytes of
 * per-block partial sums (scratch, no initialisation).  C a power of 2 in [4, 256].
 * db = NULL: only the slabs are written (finished by rth_conv_relu_wgrad_ex).
 * ---------------------------------------------------------------------------------- */
int rth_bias_relu(float *y_dev, const float *bias_dev, int64_t rows, int32_t C, void *stream);
int64_t rth_relu_bias_grad_workspace(int32_t C);
/* Merged dueling heads (dqn_model.py:22-43 fc_adv / fc_value): params = {adv.0.weight [H,F],
 * value.0.weight [H,F], adv.0.bias, value.0.bias, adv.2.weight [A,H], value.2.weight [1,H],
 * adv.2.bias [A], value.2.bias [1]} -> w1 [2H,F] (FC1 of both branches; with C > 0 its
 * columns follow the NHWC flatten of a C x P feature map), b1 [2H], w2 [A+1,2H]
 * (block diagonal), b2 [A+1].  rth_heads_split_grad maps the four gradients back onto the
 * eight parameters (grads in the same order).
 * C = RTH_HEADS_FC2_ONLY: only the second layer (w2, b2 / their gradients); w1, b1, gw1, gb1
 * and params / grads 0-3 may be NULL -- for a model whose two FC1 branches are row slices of
 * one merged [2H, F] storage (reth_amd/model.py), which FC1 reads and writes in place. */
#define RTH_HEADS_FC2_ONLY (-1)
int rth_heads_merge(const float *const *params_dev, int64_t H, int64_t F, int64_t A, int32_t C, int32_t P,
                    float *w1_dev, float *b1_dev, float *w2_dev, float *b2_dev, void *stream);
int rth_heads_split_grad(const float *gw1_dev, const float *gb1_dev, const float *gw2_dev, const float *gb2_dev,
                         int64_t H, int64_t F, int64_t A, int32_t C, int32_t P, float *const *grads_dev,
                         void *stream);
int rth_relu_bias_grad(const float *g_dev, const float *y_dev, float *gy_dev, float *db_dev, void *workspace_dev,
                       int64_t rows, int32_t C, void *stream);
/* rth_relu_bias_grad for an NCHW activation (the last conv's output written with
 * RTH_CONV_OUT_NCHW: g and y are [n, C, P]); gy is written channels-last [n, P, C] for the
 * data / weight gradients that follow.  Same workspace and slab layout (a deferred job with
 * rows = n * P finishes it); C a power of 2 in [4, 256], C * (P + 1) <= 3200. */
int rth_relu_bias_grad_nchw(const float *g_dev, const float *y_dev, float *gy_dev, float *db_dev,
                            void *workspace_dev, int64_t n, int32_t C, int32_t P, void *stream);
/* Backward of the merged heads' second layer, heads = h @ w2^T + b2 with h = relu(FC1) [B, H2]
 * (row stride ldh), from d(loss)/d(heads) dq [B, A1] (rth_td_huber, dueling): replaces the
 * addmm backward (two GEMMs + a column sum) and threshold_backward of torch.autograd at
 * dqn_solver.py:116 (loss.backward()).  Writes gh = (h > 0) ? dq @ w2 : 0 [B, H2],
 * gw2 = dq^T @ h [A1, H2], gb2 [A1], gb1 = column sums of gh [H2] (the FC1 bias gradient);
 * deterministic.  td_abs_dev / td_acc_dev (nullable): td_acc[0] += mean(td_abs[0..B)), the
 * Trainer's mean_error accumulator (reth/reth/presets/trainer.py:64-69).  H2 % 16 == 0. */
int rth_heads_backward(const float *dq_dev, const float *h_dev, int64_t ldh, const float *w2_dev, int64_t B,
                       int32_t H2, int32_t A1, float *gh_dev, float *gw2_dev, float *gb2_dev, float *gb1_dev,
                       const float *td_abs_dev, float *td_acc_dev, void *stream);
/* rth_td_huber (dueling heads, want dq) + rth_heads_backward in one launch, for
 * B * (A + 1) <= 16384: writes |td| [B], the loss [1] and the heads' gradients as above;
 * td_acc_dev (nullable) += mean |td|.  |td| and the gradients equal the two-launch path's. */
int rth_td_heads_backward(const float *q_s0_dev, const float *q_s1_online_dev, const float *q_s1_target_dev,
                          const int64_t *a_dev, const float *r_dev, const float *done_dev, const double *isw_dev,
                          int64_t B, int64_t A, float gamma_n, int32_t double_q, const float *h_dev, int64_t ldh,
                          const float *w2_dev, int32_t H2, float *td_abs_dev, float *loss_out_dev, float *gh_dev,
                          float *gw2_dev, float *gb2_dev, float *gb1_dev, float *td_acc_dev, void *stream);
/* The same two kernels with the second layer in the reference's branch form: fc2_params =
 * {adv.2.weight [A, H], value.2.weight [1, H], ...} read in place instead of a merged
 * block-diagonal w2, fc2_grads = {adv.2.weight, value.2.weight, adv.2.bias, value.2.bias}
 * gradients written in place (the off-diagonal blocks of gw2 are not produced); H2 = 2H,
 * H a multiple of 16.  Replaces rth_heads_merge / rth_heads_split_grad for the second layer. */
int rth_heads_backward_branches(const float *dq_dev, const float *h_dev, int64_t ldh, const float *const *fc2_params_dev,
                                int32_t H, int64_t B, int64_t A, float *gh_dev, float *const *fc2_grads_dev,
                                float *gb1_dev, const float *td_abs_dev, float *td_acc_dev, void *stream);
int rth_td_heads_backward_branches(const float *q_s0_dev, const float *q_s1_online_dev, const float *q_s1_target_dev,
                                   const int64_t *a_dev, const float *r_dev, const float *done_dev,
                                   const double *isw_dev, int64_t B, int64_t A, float gamma_n, int32_t double_q,
                                   const float *h_dev, int64_t ldh, const float *const *fc2_params_dev, int32_t H,
                                   float *td_abs_dev, float *loss_out_dev, float *gh_dev,
                                   float *const *fc2_grads_dev, float *gb1_dev, float *td_acc_dev, void *stream);
/* The dueling heads' second layer forward (dqn_model.py:22-43 fc_adv[2] / fc_value[2] on the
 * ReLU'd FC1 output h [n, 2H], row stride ldh): heads [n, A+1] = (adv.2(h[:, :H]),
 * value.2(h[:, H:])), the raw heads the TD / epsilon-greedy kernels consume; fc2_params =
 * {adv.2.weight, value.2.weight, adv.2.bias, value.2.bias} read in place. */
int rth_heads_fc2(const float *h_dev, int64_t ldh, int64_t n, int32_t H, int32_t A, const float *const *fc2_params_dev,
                  float *heads_dev, void *stream);
/* rth_heads_fc2 over a device-counted batch (the actors' acting + terminal stacks,
 * test/apex-dqn/worker.py:46 act and :55-60 calc_loss): only rows r < min(*n_dev, n_max) are
 * computed; cache_dev (nullable) [stacks, A+1] additionally receives row r at cache_rows_dev[r]
 * (the per-stack heads cache the deduplicated calc_loss reads) -- one launch instead of two. */
int rth_heads_fc2_upto(const float *h_dev, int64_t ldh, int64_t n_max, const int64_t *n_dev, int32_t H, int32_t A,
                       const float *const *fc2_params_dev, float *heads_dev, float *cache_dev,
                       const int64_t *cache_rows_dev, void *stream);
/* y[r] = relu(x[r] . w^T + b) for rows r0 <= r < min(*n_dev, n_max) (dqn_model.py:22-43, the
 * heads' first Linear -> ReLU): the device-counted tail of a batch whose first r0 rows a
 * library GEMM covers -- the actors' terminal stacks, absent in most steps (every workgroup
 * exits at once).  x [*, F] row stride ldx, w [O, F], y row stride ldy; F, ldx multiples of 4,
 * x and w 16-byte aligned.  Deterministic (fixed-order sums). */
int rth_linear_relu_rows_upto(const float *x_dev, int64_t ldx, int64_t r0, int64_t n_max, const int64_t *n_dev,
                              const float *w_dev, const float *b_dev, int64_t F, int64_t O, float *y_dev, int64_t ldy,
                              void *stream);

/* ------------------------------------------------------------------------------------
 * Q-network convolution torso forward (reth/reth/algorithm/dqn/dqn_model.py:14-20: each
 * Conv2d -> ReLU of `features`): y = relu(conv2d(x, w) + bias) in one launch, implicit GEMM
 * on the fp32 MFMA, output NHWC fp32 [n, hout, wout, cout].  `packed` is the Conv2d weight
 * in the kernel's fragment order, made by rth_conv_pack from the OHWI weight (a channels_last
 * [cout, cin, kh, kw] parameter) into rth_conv_packed_bytes(shape) bytes -- once per weight
 * version, so every launch stages it into LDS with one coalesced copy.  16-byte aligned.
 *   input RTH_CONV_F32_NHWC: x = [n, hin, win, cin] fp32 (channels-last activations);
 *   input RTH_CONV_U8_CHW:   x = uint8 frame stacks [cin, hin, win] (the reference's float32
 *       frames hold exactly these integers); sample i reads stack rows_dev[i] when rows_dev
 *       is given (replay rows, actor frame-ring handles), else stack i -- no f32 copy of the
 *       observations is made.
 * Built geometries: the Nature-DQN torso on 4 x 84 x 84 stacks (conv1 either input form,
 * conv2 32x20x20 -> 64 k4 s2, conv3 64x9x9 -> 64 k3 s1); rth_conv_supported says whether
 * a shape is one of them.  Replaces MIOpen's forward + the separate rth_bias_relu pass.
 * ---------------------------------------------------------------------------------- */
#define RTH_CONV_F32_NHWC 0
#define RTH_CONV_U8_CHW 1
/* flag OR'ed into `input` of rth_conv_bias_relu(_upto): write y NCHW [n, cout, hout, wout]
 * (the last conv, whose output FC1 reads in the reference's (C, H, W) flatten order); the
 * fp32-MFMA kernels only (not the uint8 conv1, which feeds conv2) */
#define RTH_CONV_OUT_NCHW 16
/* rth_conv_pack_many only: the job packs the flipped data-gradient kernel of this FORWARD
 * shape (rth_conv_dgrad_workspace(shape) bytes) for rth_conv_dgrad_prepacked */
#define RTH_CONV_PACK_DGRAD 32
typedef struct rth_conv_shape {
  int32_t input; /* RTH_CONV_F32_NHWC | RTH_CONV_U8_CHW [| RTH_CONV_OUT_NCHW] */
  int32_t cin, hin, win, cout, kh, kw, stride;
} rth_conv_shape;
int rth_conv_supported(const rth_conv_shape *shape);
/* which kernel rth_conv_bias_relu runs for a shape and n samples: RTH_CONV_IMPL_F32
 * (k_conv_bias_relu, fp32 MFMA), RTH_CONV_IMPL_BF16X3 (k_conv1_u8_share: conv1 on uint8 stacks,
 * the weights split into three exact bf16 terms), RTH_CONV_IMPL_X9 (k_conv_x9: both operands split into three exact bf16
 * terms, nine bf16 MFMAs per fp32 product; *nsamp_out = samples per workgroup); 0 = not built.
 * Diagnostics (bench.py's roofline labels), no launch. */
#define RTH_CONV_IMPL_F32 1
#define RTH_CONV_IMPL_BF16X3 2
#define RTH_CONV_IMPL_X9 3
int rth_conv_impl(const rth_conv_shape *shape, int64_t n, int32_t *nsamp_out);
int64_t rth_conv_packed_bytes(const rth_conv_shape *shape);
int rth_conv_pack(const rth_conv_shape *shape, const float *w_ohwi_dev, float *packed_dev, void *stream);
/* rth_conv_pack for n <= 6 layers in one launch (a network's torso, both conv1 forms, and
 * with RTH_CONV_PACK_DGRAD in a job's shape->input the packed data-gradient kernels of the
 * same weights: the learner packs everything its forward and backward read in one launch) */
int rth_conv_pack_many(int32_t n, const rth_conv_shape *shapes, const float *const *w_ohwi_dev,
                       float *const *packed_dev, void *stream);
int rth_conv_bias_relu(const rth_conv_shape *shape, const void *x_dev, const int64_t *rows_dev, int64_t n,
                       const float *packed_dev, const float *bias_dev, float *y_dev, void *stream);
/* rth_conv_bias_relu over the first min(n_max, *n_dev) samples, the count read on the device
 * (graph replay of a variable-size batch: the actors' acting stacks plus the terminal stacks
 * of the episodes that just ended); outputs past the count are left untouched. */
int rth_conv_bias_relu_upto(const rth_conv_shape *shape, const void *x_dev, const int64_t *rows_dev, int64_t n_max,
                            const int64_t *n_dev, const float *packed_dev, const float *bias_dev, float *y_dev,
                            void *stream);
/* Data gradient of conv2d(x, w) (the backward through conv3 / conv2 of the learner's torso,
 * reth/reth/algorithm/dqn/dqn_solver.py:117 loss.backward() on dqn_model.py:14-20; replaces
 * MIOpen's backward-data solver and its zero fill): gx = [n, hin, win, cin] fp32 NHWC from
 * gy = [n, hout, wout, cout] fp32 NHWC and w = the OHWI weight (a channels_last Conv2d
 * parameter, read directly: no packing).  Every element of gx is written exactly once.
 * `shape` is the FORWARD convolution's (input RTH_CONV_F32_NHWC); built: conv2 and conv3 of
 * the Nature-DQN torso (rth_conv_dgrad_supported).  16-byte aligned buffers. */
int rth_conv_dgrad_supported(const rth_conv_shape *shape);
int rth_conv_dgrad(const rth_conv_shape *shape, const float *gy_dev, int64_t n, const float *w_ohwi_dev,
                   float *gx_dev, void *stream);
/* The same with a caller-owned workspace for the flipped kernel the exact-split path packs
 * each launch (rth_conv_dgrad_workspace bytes, 16-byte aligned; 0 bytes: none needed).
 * rth_conv_dgrad uses one internal workspace per device, so two learners in one process whose
 * backward passes run on different streams (or are replayed from different graphs) must each
 * pass their own: the pack and the convolution of one call are stream-ordered, two calls on
 * two streams are not. */
int64_t rth_conv_dgrad_workspace(const rth_conv_shape *shape);
/* rth_conv_dgrad from a kernel packed beforehand: `packed_dev` = the RTH_CONV_PACK_DGRAD job of
 * rth_conv_pack_many for this shape and the weights of the forward (no pack launch here; same
 * result as rth_conv_dgrad_ws on those weights, bit for bit).  Built where
 * rth_conv_dgrad_workspace(shape) > 0. */
int rth_conv_dgrad_prepacked(const rth_conv_shape *shape, const float *gy_dev, int64_t n, const void *packed_dev,
                             float *gx_dev, void *stream);
/* rth_conv_dgrad_prepacked for conv3's geometry (rth_conv_dgrad_relu_supported) with the layer
 * below's ReLU applied in the same launch (r05): gx = the data gradient where y_dev (the layer
 * below's output, [n, 9, 9, 64] NHWC) > 0, else 0 -- what rth_relu_bias_grad makes of the plain
 * data gradient -- and that layer's bias-gradient slab partials written to bias_ws_dev (a
 * rth_relu_bias_grad workspace of C = 64, finished later by a rth_bias_deferred job whose
 * `slabs` is *slabs_out).  Reference: the backward of dqn_model.py:14-20 (Conv2d + ReLU). */
int rth_conv_dgrad_relu_supported(const rth_conv_shape *shape);
int rth_conv_dgrad_relu_prepacked(const rth_conv_shape *shape, const float *gy_dev, int64_t n, const void *packed_dev,
                                  const float *y_dev, float *gx_dev, void *bias_ws_dev, int64_t *slabs_out,
                                  void *stream);
/* rth_conv_dgrad_relu_prepacked reading FC1's data gradient where it lies (r15; conv3's geometry,
 * rth_conv_dgrad_relu_nchw_supported): g_dev and y_dev are NCHW [n, 64, 7, 7], FC1's data
 * gradient and conv3's own forward output.  The data-gradient launch does rth_relu_bias_grad_nchw's
 * mask pass too: gy_dev [n, 7, 7, 64] NHWC = g where y > 0, else 0 (for the weight gradient),
 * gx_dev = the data gradient of gy where y_below_dev (conv2's output, [n, 9, 9, 64] NHWC) > 0,
 * else 0, and conv2's bias-gradient slabs in bias_ws_below_dev, finished by a rth_bias_deferred
 * job whose `slabs` is *slabs_out -- all as rth_conv_dgrad_relu_prepacked writes them.  A second,
 * small launch sums conv3's own bias-gradient slabs from gy_dev into bias_ws_dev in
 * rth_relu_bias_grad_nchw's slab layout and order (finished by a job with `slabs` 0 and rows =
 * n * 49).  Every output has the bits of rth_relu_bias_grad_nchw followed by
 * rth_conv_dgrad_relu_prepacked.  Both workspaces are rth_relu_bias_grad workspaces of C = 64.
 * Same preconditions as rth_conv_dgrad_relu_prepacked (16-byte alignment, n * 49 * 64 * 4 bytes
 * < 2 GiB, at most 2048 slabs).  Reference: the backward of dqn_model.py:14-20 (Conv2d + ReLU,
 * Flatten). */
int rth_conv_dgrad_relu_nchw_supported(const rth_conv_shape *shape);
int rth_conv_dgrad_relu_nchw_prepacked(const rth_conv_shape *shape, const float *g_dev, const float *y_dev, int64_t n,
                                       const void *packed_dev, const float *y_below_dev, float *gy_dev, float *gx_dev,
                                       void *bias_ws_dev, void *bias_ws_below_dev, int64_t *slabs_out, void *stream);
/* FC1 of the dueling heads (the first Linear + ReLU of both branches, dqn_model.py:38-47, as
 * one [N, K] weight) on the exact-split bf16 MFMA: y [M, N] = act(x [M, K] w^T + b), x
 * row-major with row stride ldx, w row-major [N, K] (the Linear weight as stored), act = ReLU
 * when relu != 0, bias may be NULL; M % 64 == 0, N % 128 == 0, K % 32 == 0
 * (rth_fc_x9_supported).  Fixed-order split-K partials in `workspace` (rth_fc_x9_workspace
 * bytes, NULL when that is 0): run-to-run deterministic.  M and N multiples of 128 run on a
 * 128 x 128 workgroup tile (late r05), others on a 64 x 128 tile; the tile and the k splits
 * are fixed functions of (M, N, K), so the workspace size is too.  Replaces the hipBLASLt GEMM
 * + bias + ReLU epilogue (torch._addmm_activation) of every FC1 forward in the loop (r06: the
 * actors', the target pass's and the learner's). */
int rth_fc_x9_supported(int64_t M, int64_t N, int64_t K);
int64_t rth_fc_x9_workspace(int64_t M, int64_t N, int64_t K);
int rth_fc_x9(const float *x_dev, int64_t ldx, int64_t M, const float *w_dev, int64_t N, int64_t K,
              const float *bias_dev, int32_t relu, float *y_dev, void *workspace_dev, void *stream);
/* The actors' counted FC1 (r05): y [n_max, N] rows [0, M) = rth_fc_x9 (ReLU, M % 64 == 0) and
 * rows [M, min(*n_dev, n_max)) = rth_linear_relu_rows_upto (the device-counted terminal stacks),
 * the split-K reduce and the counted rows in one launch; y row stride N; the same bits as
 * those two calls. */
int rth_fc_x9_rows_upto(const float *x_dev, int64_t ldx, int64_t M, int64_t n_max, const int64_t *n_dev,
                        const float *w_dev, int64_t N, int64_t K, const float *bias_dev, float *y_dev,
                        void *workspace_dev, void *stream);
/* FC1 -> FC2 of the dueling heads in two launches (r06; dqn_model.py:38-47, 59-71 forward
 * under dqn_solver.py:77-98 _calc_td_error / the target pass): rth_fc_x9's GEMM into its split-K
 * workspace, then one launch reducing it (+ b1 + ReLU, rth_fc_x9's order) and running the second
 * layer of both branches from the parameters in place (fc2_params = {adv weight [A, H], value
 * weight [1, H], adv bias [A], value bias [1]}, rth_heads_fc2's order): heads [M, A + 1] (raw
 * advantages then value) bit-identical to rth_fc_x9 + rth_heads_fc2; h1_out (nullable) [M, N]
 * receives relu(FC1).  N = 2H <= 512; workspace = rth_fc_x9_workspace(M, N, K) bytes. */
int rth_fc1_heads_supported(int64_t M, int64_t N, int64_t K, int32_t A);
int rth_fc1_heads(const float *x_dev, int64_t ldx, int64_t M, const float *w1_dev, int64_t N, int64_t K,
                  const float *b1_dev, int32_t A, const float *const *fc2_params, float *heads_dev, float *h1_out_dev,
                  void *workspace_dev, void *stream);
/* The same FC1 on the fp32 MFMA with no LDS (r05): the arguments, the workspace protocol and
 * the determinism of rth_fc_x9; any M >= 1 (ragged actor batches), N % 128 == 0, K % 32 == 0
 * (rth_fc_f32_supported).  Not used by the loop (the x9 form is faster there); kept as the
 * fp32-MFMA reference form, tested against it. */
int rth_fc_f32_supported(int64_t M, int64_t N, int64_t K);
int64_t rth_fc_f32_workspace(int64_t M, int64_t N, int64_t K);
int rth_fc_f32(const float *x_dev, int64_t ldx, int64_t M, const float *w_dev, int64_t N, int64_t K,
               const float *bias_dev, int32_t relu, float *y_dev, void *workspace_dev, void *stream);
/* FC1's backward (r07; the backward of dqn_model.py:38-47, the first Linear of both branches as
 * one [N, K] weight, under dqn_solver.py:116-117 loss.backward()) on the exact-split bf16 MFMA,
 * both gradients in one launch: gx [B, K] = gy w and gw [N, K] = gy^T x, from gy [B, N] (the
 * gradient of the Linear's output, already ReLU-masked; row-major, row stride ldg), x [B, K] (the
 * Linear's input; row-major, row stride ldx) and w [N, K] (row-major, contiguous); gx and gw are
 * written contiguous, every element, with no zero fill expected.  gx_dev and gw_dev are each
 * nullable: a NULL gradient is not computed and its operand (w for gx, x for gw) may be NULL;
 * both NULL is an error; a gradient's bits do not depend on whether the other is asked for.
 * B % 64 == 0, N % 128 == 0, K % 64 == 0 (rth_fc_bwd_supported); strides multiples of 4 floats,
 * buffers 16-byte aligned.  The tiles and the k splits are fixed functions of (B, N, K), so
 * rth_fc_bwd_workspace (bytes; 0 where nothing is split, then workspace_dev may be NULL) is too;
 * the workspace needs no initialisation.  No atomics: fixed-order split partials and one reduce
 * launch, run-to-run bit-identical.  Launches on one stream are ordered; two calls sharing a
 * workspace on two streams are not (as rth_conv_dgrad_ws).  Replaces the two hipBLASLt GEMMs of
 * the learner's FC1 backward where model.FC1_BWD = "hip". */
int rth_fc_bwd_supported(int64_t B, int64_t N, int64_t K);
int64_t rth_fc_bwd_workspace(int64_t B, int64_t N, int64_t K);
int rth_fc_bwd(const float *gy_dev, int64_t ldg, const float *x_dev, int64_t ldx, const float *w_dev, int64_t B,
               int64_t N, int64_t K, float *gx_dev, float *gw_dev, void *workspace_dev, void *stream);
int rth_conv_dgrad_ws(const rth_conv_shape *shape, const float *gy_dev, int64_t n, const float *w_ohwi_dev,
                      float *gx_dev, void *workspace_dev, void *stream);
/* Weight gradient of conv2d(x, w) for the fp32 channels-last layers (conv2 and conv3 of the
 * torso; the backward of dqn_model.py:14-20 under dqn_solver.py:117 loss.backward(); replaces
 * MIOpen's weight-gradient solver and its zero fill): gw [cout, kh, kw, cin] (OHWI, the
 * channels_last parameter layout) = sum over output pixels of gy[p][co] * x-window[p], from
 * x = [n, hin, win, cin] and gy = [n, hout, wout, cout] (already ReLU-masked), on the fp32
 * MFMA; every sum has a fixed order (deterministic).  `shape` is the forward convolution's
 * (input RTH_CONV_F32_NHWC); workspace = rth_conv_wgrad_f32_workspace(shape) bytes. */
/* The same on the bf16 MFMA with both operands split into three exact bf16 terms (nine
 * products per fp32 product, exact in the fp32 accumulator: the fp32 path's products in
 * another fixed summation order); workspace = rth_conv_wgrad_x9_workspace(shape) bytes. */
int rth_conv_wgrad_x9_supported(const rth_conv_shape *shape);
int64_t rth_conv_wgrad_x9_workspace(const rth_conv_shape *shape);
int rth_conv_wgrad_x9(const rth_conv_shape *shape, const float *x_dev, int64_t n, const float *gy_dev, float *gw_dev,
                      void *workspace_dev, void *stream);
int rth_conv_wgrad_f32_supported(const rth_conv_shape *shape);
int64_t rth_conv_wgrad_f32_workspace(const rth_conv_shape *shape);
int rth_conv_wgrad_f32(const rth_conv_shape *shape, const float *x_dev, int64_t n, const float *gy_dev, float *gw_dev,
                       void *workspace_dev, void *stream);
/* rth_conv_wgrad_f32's partial launch alone (r06): *job_out describes the fixed-order reduce that
 * finishes gw_dev -- handed to conv1's weight-gradient reduce launch (rth_conv_relu_wgrad_ex and
 * its frame-id / norm forms, `wdeferred`), which runs it in its own workgroups; the result is
 * bit-identical to rth_conv_wgrad_f32's. */
typedef struct rth_wgrad_deferred {
  const float *partial; /* the workspace holding the split partials */
  float *gw;            /* OHWI output */
  int32_t splits, elems, nb, K;
} rth_wgrad_deferred;
int rth_conv_wgrad_f32_partials(const rth_conv_shape *shape, const float *x_dev, int64_t n, const float *gy_dev,
                                float *gw_dev, void *workspace_dev, rth_wgrad_deferred *job_out, void *stream);
/* Backward of relu(conv2d(x, w) + b) for the weights and bias, on uint8 stacks (conv1, whose
 * input needs no gradient): gy = (y > 0) ? g : 0, gw = sum over output pixels of gy times the
 * input window (OHWI [cout, kh, kw, cin], the layout of a channels_last weight), gb = sum of
 * gy.  g, y: NHWC fp32 [n, hout, wout, cout] (upstream gradient, forward output).  Summed in
 * a fixed order (deterministic); workspace = rth_conv_wgrad_workspace(shape) bytes.  Built
 * for the uint8 conv1 geometry; replaces rth_relu_bias_grad + MIOpen's weight gradient. */
int64_t rth_conv_wgrad_workspace(const rth_conv_shape *shape);
int rth_conv_relu_wgrad(const rth_conv_shape *shape, const void *x_dev, const int64_t *rows_dev, int64_t n,
                        const float *g_dev, const float *y_dev, float *gw_dev, float *gb_dev, void *workspace_dev,
                        void *stream);
/* rth_conv_relu_wgrad that also finishes up to 4 deferred bias gradients in its reduce launch
 * (one launch fewer per layer): each a rth_relu_bias_grad called with db = NULL on
 * `workspace`, over `rows` rows of C channels, earlier on the same stream; and up to 2 deferred
 * weight gradients (rth_conv_wgrad_f32_partials jobs, earlier on the same stream). */
typedef struct rth_bias_deferred {
  const void *workspace; /* the rth_relu_bias_grad workspace holding the slabs */
  float *db;             /* [C] output */
  int64_t rows;
  int32_t C;
  int32_t slabs; /* the slab count; 0 = rth_relu_bias_grad's for `rows` (rth_conv_dgrad_relu_prepacked
                  * reports its own) */
} rth_bias_deferred;
int rth_conv_relu_wgrad_ex(const rth_conv_shape *shape, const void *x_dev, const int64_t *rows_dev, int64_t n,
                           const float *g_dev, const float *y_dev, float *gw_dev, float *gb_dev, void *workspace_dev,
                           const rth_bias_deferred *deferred, int32_t ndeferred,
                           const rth_wgrad_deferred *wdeferred, int32_t nwdeferred, void *stream);
/* Frames in place (r05): conv1 (4x84x84 uint8 -> 32, k8 s4) forward and weight gradient
 * reading each sample's 4 frames straight from a replay's frame store (the
 * rth_replay_frames_attach store, 84*84-byte frames) by the int32 [n][4] frame ids a
 * rth_replay_frames_ids_out gather wrote (16-byte aligned), instead of from gathered stacks:
 * results bit-identical to rth_conv_bias_relu / rth_conv_relu_wgrad_ex on the stacks
 * rth_replay_gather would have assembled from the same ids, without that copy. */
int rth_conv1_frames_bias_relu(const rth_conv_shape *shape, const uint8_t *store_dev, const int32_t *ids_dev,
                               int64_t n, const float *packed_dev, const float *bias_dev, float *y_dev, void *stream);
int rth_conv1_frames_relu_wgrad_ex(const rth_conv_shape *shape, const uint8_t *store_dev, const int32_t *ids_dev,
                                   int64_t n, const float *g_dev, const float *y_dev, float *gw_dev, float *gb_dev,
                                   void *workspace_dev, const rth_bias_deferred *deferred, int32_t ndeferred,
                                   const rth_wgrad_deferred *wdeferred, int32_t nwdeferred, void *stream);

/* ------------------------------------------------------------------------------------
 * Atari observation preprocessing (reth/reth/env/util.py:121-209, 281-297): per actor, the
 * max of the last two raw RGB frames of the skip window (MaxAndSkipEnv), cv2 RGB2GRAY +
 * INTER_AREA resize to out_h x out_w (WarpFrame; OpenCV's 8-bit algorithms restated, cv2
 * being absent), pushed onto the actor's frame stack (FrameStack, ImageToPyTorch layout).
 *   raw_dev    [n, 2, in_h, in_w, 3] uint8 (for a reset: the reset frame twice)
 *   frames_dev the actors' stack ring [n * ring, stack, out_h, out_w] uint8 (nullable):
 *              slot new_slot[i] <- slot prev_slot[i] shifted by one frame + the new frame,
 *              or the new frame `stack` times when reset_dev[i] != 0 (reset_dev nullable)
 *   out_frame_dev (nullable) [n, out_h, out_w]: the preprocessed frames alone
 * ---------------------------------------------------------------------------------- */
typedef struct rth_atari rth_atari;
int rth_atari_create(int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, int device, rth_atari **out);
int rth_atari_destroy(rth_atari *h);
int rth_atari_step(rth_atari *h, const uint8_t *raw_dev, int64_t n, uint8_t *frames_dev, int32_t ring, int32_t stack,
                   const int64_t *prev_slot_dev, const int64_t *new_slot_dev, const uint8_t *reset_dev,
                   uint8_t *out_frame_dev, void *stream);
/* the Ape-X actors' Atari env mode (after rth_actor_tail with ext_frames = 1): per actor i the
 * raw pair raw_dev[i] (MaxAndSkip max, gray, INTER_AREA) becomes the new top frame of stack
 * s1_h[i] = stack s0_h[i] shifted by one (FrameStack.step), and where done_dev[i] != 0 the
 * reset observation -- env.reset()'s screen reset_raw_dev[i] ([n, in_h, in_w, 3], read only
 * where done; MaxAndSkip.reset returns it without a pair max, util.py:129-130), warped, `stack`
 * times (FrameStack.reset, util.py:191-196) -- goes into actor i's slot cur_slot_dev[i].
 * Handles index frames_dev's stacks; slots are per-actor ring slots. */
int rth_atari_env_step(rth_atari *h, const uint8_t *raw_dev, int64_t n, uint8_t *frames_dev, int32_t ring,
                       int32_t stack, const int64_t *s0_h_dev, const int64_t *s1_h_dev, const float *done_dev,
                       const int64_t *cur_slot_dev, const uint8_t *reset_raw_dev, void *stream);
/* synthetic raw emulator screens (the stand-in for ALE's output, ALE being absent): nbytes of
 * device Philox (seed, step *t_dev), 16-byte aligned and a multiple of 16 bytes */
int rth_atari_synth_raw(uint8_t *raw_dev, int64_t nbytes, uint64_t seed, const int64_t *t_dev, void *stream);
/* synthetic reset screens: frame i of reset_raw_dev ([n, frame_bytes]) from device Philox
 * (seed, step *t_dev, its own stream), written only where done_dev[i] != 0 */
int rth_atari_synth_reset(uint8_t *reset_raw_dev, int64_t n, int64_t frame_bytes, uint64_t seed, const int64_t *t_dev,
                          const float *done_dev, void *stream);

/* ------------------------------------------------------------------------------------
 * Learner optimizer step (reth/reth/algorithm/dqn/dqn_solver.py:118-121):
 * torch.nn.utils.clip_grad_norm_(params, max_norm) then torch.optim.Adam.step() over up to
 * RTH_MAX_PARAM_TENSORS fp32 tensors in two launches (norm partials, then the update).
 * max_norm < 0 skips clipping.  step_dev (int64, device) is Adam's step count, incremented on
 * the device; workspace_dev holds rth_clip_adam_workspace() bytes, zero-filled once before the
 * first call; one workspace per optimizer.  total_norm_out_dev (nullable) receives the pre-clip
 * 2-norm (clip_grad_norm_'s return).
 * Every tensor has 1 <= n < 2^29 elements (n * 4 bytes is the 32-bit record count of the buffer
 * resource the kernels read it through); rth_clip_adam and rth_adam_prenormed return
 * RTH_ERR_INVALID for a larger one and launch nothing.
 * Workspace layout: [32,768 doubles: the norm partials, summed in index order]
 * [16 B: float coef, step_size, bc2_sqrt, total_norm -- the last update's scalars, written by the
 * update] [8 B: float step_size, bc2_sqrt -- the bias corrections lr / (1 - beta1^t) and
 * sqrt(1 - beta2^t) of step t, written with the step count and read by the update] [the rest
 * unused].  A caller of rth_adam_prenormed fills the first nparts partials and the bias
 * corrections; rth_adam_prenormed does not advance step_dev.
 * ---------------------------------------------------------------------------------- */
#define RTH_MAX_PARAM_TENSORS 32
typedef struct rth_param_tensor {
  float *param;
  const float *grad;
  float *exp_avg;    /* Adam state["exp_avg"] */
  float *exp_avg_sq; /* Adam state["exp_avg_sq"] */
  int64_t n;
} rth_param_tensor;
int64_t rth_clip_adam_workspace(void);
int rth_clip_adam(const rth_param_tensor *tensors, int32_t n_tensors, double lr, double beta1, double beta2,
                  double eps, double max_norm, int64_t *step_dev, void *workspace_dev, float *total_norm_out_dev,
                  void *stream);
/* The same step with clip_grad_norm_'s partials produced by the learner's backward (r06, one
 * rank: the gradients are final there).  rth_conv1_relu_wgrad_norm is rth_conv_relu_wgrad_ex
 * (rows_dev != NULL: stacks by row; fids_dev != NULL: rth_conv1_frames_relu_wgrad_ex's frame
 * ids, x_dev the frame store; neither: x_dev the stacks) whose reduce launch also writes the
 * fp64 sum-of-squares partials clip_grad_norm_ reduces: extra workgroups over the gradients of
 * `sq` (every parameter but conv1's weight and bias and the deferred bias and weight gradients,
 * which the launch finishes itself and adds right behind them; only .grad and .n are read), the first of
 * them advancing step_dev and writing the step's bias corrections as rth_clip_adam's first
 * launch does, all into adam_workspace_dev (rth_clip_adam_workspace's layout);
 * *nparts_out = the partial count.  rth_adam_prenormed(..., nparts, ...) is then
 * rth_clip_adam's second launch alone: the same update, the norm summed in partial order. */
int rth_conv1_relu_wgrad_norm(const rth_conv_shape *shape, const void *x_dev, const int64_t *rows_dev,
                              const int32_t *fids_dev, int64_t n, const float *g_dev, const float *y_dev,
                              float *gw_dev, float *gb_dev, void *workspace_dev, const rth_bias_deferred *deferred,
                              int32_t ndeferred, const rth_wgrad_deferred *wdeferred, int32_t nwdeferred,
                              const rth_param_tensor *sq, int32_t n_sq, double lr, double beta1,
                              double beta2, int64_t *step_dev, void *adam_workspace_dev, int32_t *nparts_out,
                              void *stream);
int rth_adam_prenormed(const rth_param_tensor *tensors, int32_t n_tensors, double lr, double beta1, double beta2,
                       double eps, double max_norm, int32_t nparts, int64_t *step_dev, void *workspace_dev,
                       float *total_norm_out_dev, void *stream);

/* ------------------------------------------------------------------------------------
 * The MLP Q-network (dqn_model.py:59-71, the network of every 1-D observation: CartPole):
 * Linear(D,H) -> ReLU -> Linear(H,H) -> ReLU -> Linear(H,A) as fused fp32 kernels (mlp.hpp).
 * `params` (`online`, `target`, `grads`) is a HOST array of six device pointers in torch layout,
 * read in place: {nn.0.weight [H,D], nn.0.bias [H], nn.2.weight [H,H], nn.2.bias [H],
 * nn.4.weight [A,H], nn.4.bias [A]}.  Built for H = 128, D in 1..64, A in 1..18, any n, B >= 1;
 * other shapes return RTH_ERR_INVALID and launch nothing.  Every product is one fp32 fmaf and a
 * dot product has one fixed summation order, so the Q of a row does not depend on n, on the
 * row's position or on the entry point; the gradients sum over the batch in a fixed order (no
 * atomics).  All launches go to `stream`, without host synchronisation or allocation.
 * ---------------------------------------------------------------------------------- */
int rth_mlp_supported(int64_t D, int64_t H, int64_t A);            /* 1 where built, else 0 */
int64_t rth_mlp_workspace(int64_t B, int64_t D, int64_t H, int64_t A); /* bytes for rth_mlp_dqn_grads; < 0: error */
/* Q[n,A] = net(x[n,D]) (row stride ldx floats); argmax_dev nullable: first index of the row max
 * (torch.argmax's tie rule, dqn_solver.py:126-131).  One launch. */
int rth_mlp_q(const float *const *params, const float *x_dev, int64_t ldx, int64_t n, int64_t D, int64_t H, int64_t A,
              float *q_dev, int32_t *argmax_dev, void *stream);
/* dqn_solver.py:68-117 for the MLP: Q(s0), Q(s1) online (only if double_q), Q_tgt(s1), the TD /
 * Huber / IS-weight arithmetic of rth_td_huber (same operation order; isw fp64 cast to f32,
 * nullable) and the backward through the online net into grads[6] (same order and shapes as
 * params; every element written, nothing accumulated).  grads == NULL: no backward (calc_loss).
 * td_abs_dev [B], loss_dev [1] (mean) nullable.  workspace_dev: rth_mlp_workspace(B, D, H, A)
 * bytes.  At most two launches. */
int rth_mlp_dqn_grads(const float *const *online, const float *const *target, const float *s0_dev, int64_t lds0,
                      const float *s1_dev, int64_t lds1, const int64_t *a_dev, const float *r_dev,
                      const float *done_dev, const double *isw_dev, int64_t B, int64_t D, int64_t H, int64_t A,
                      float gamma_n, int32_t double_q, float *const *grads, float *td_abs_dev, float *loss_dev,
                      void *workspace_dev, void *stream);

/* ------------------------------------------------------------------------------------
 * Device-resident vectorised CartPole actors on the MLP kernels: N gym CartPole-v0/v1
 * environments stepped by one launch, without host synchronisation.  Replaces the host actor loop
 * of reth/reth/presets/worker.py:128-155 (Worker.step: act, env.step, env.reset on done) and what
 * it calls: utils/exploration.py:26-31 (RandomExploration.act), algorithm/dqn/dqn_solver.py:126-131
 * (act = argmax Q) and utils/nstep_adder.py:11-28.  All pointers are device memory except `params`
 * (a host array of six device pointers, as rth_mlp_q's).  Built for D = 4, H = 128, A = 2.
 * These two entry points are adapters (csrc/mlp_actor.hpp) onto the classic-control kernels below
 * (csrc/env_actor.hpp) with env = RTH_ENV_CARTPOLE and no return statistics: one step kernel and
 * one reset kernel serve all four entry points.
 * ---------------------------------------------------------------------------------- */
typedef struct rth_mlp_actor_args {
  const float *const *params; /* the acting network (rth_mlp_q layout); unused by the reset */
  int64_t D, H, A;
  double *state;              /* [N, 4] fp64 env state (x, x_dot, theta, theta_dot) */
  int32_t *ep_steps;          /* [N] steps taken in the running episode */
  int64_t *t_dev;             /* [N] env steps taken, one (equal) copy per env: the Philox counter */
  int64_t *stats;             /* [N, 3] finished episodes, sum of their lengths, last length */
  float *obs_ring;            /* [N * ring + 1, 4] f32 observations, 16-byte aligned; last row: zero sink */
  int64_t *cur_slot;          /* [N] ring slot of the observation acted on next */
  const double *eps;          /* [N] exploration rates, read every step */
  const int64_t *action_in;   /* [N] nullable: overrides the ε-greedy choice (tests) */
  int64_t *action;            /* out [N]: this step's transition ... */
  float *reward, *done;       /* out [N] */
  int64_t *s0_h, *s1_h;       /* out [N]: observation handles env * ring + slot */
  int32_t *emit;              /* out [N]: 1 where the adder emitted a row; its fields: */
  int64_t *row_s0, *row_a, *row_s1;
  float *row_r, *row_done;
  float *row_obs0, *row_obs1; /* out [N, 4]: the emitted row's observations by value (16-byte aligned) */
  float *q_out;               /* out [N, A] nullable: the acting Q rows (equal to rth_mlp_q's) */
  uint64_t seed;              /* exploration and reset seed */
  int64_t N;
  int32_t ring;               /* slots per env: >= 4 and >= 2 (n_step + 2) */
  int32_t max_episode_steps;  /* TimeLimit: 200 (v0) / 500 (v1) */
} rth_mlp_actor_args;
/* env.reset() of every env (worker.py:144-145): states from Philox(seed, env, t = 0) -- the counter
 * layout is documented in csrc/env_actor.hpp --, ep_steps / t_dev / stats = 0, the observation into
 * ring slot 1, cur_slot = 1.  Uses state, ep_steps, t_dev, stats, obs_ring, cur_slot, seed, N, ring.
 * Arguments are checked before anything is launched (RTH_ERR_INVALID, rth_last_error). */
int rth_cartpole_reset(const rth_mlp_actor_args *args, void *stream);
/* One env step of all N actors (Worker.step, worker.py:128-155), one launch: Q of the current observations
 * (rth_mlp_q's values), ε-greedy with rth_eps_greedy's draws at counter t = t_dev + 1
 * (exploration.py:26-31, dqn_solver.py:126-131), CartPole dynamics in fp64, reward 1, done on
 * |x| > 2.4, |theta| > 12 degrees or ep_steps reaching max_episode_steps; a finished episode's env
 * is reset (Philox(seed, env, t)); next observation to ring slot (2t) % ring, reset observation
 * to (2t + 1) % ring; the transition is pushed into the adder `h` (nstep_adder.py:11-28, as
 * rth_nstep_push) and an emitted row is written as handles and by value.  args->N must equal the
 * adder's.  Arguments are checked before anything is launched. */
int rth_mlp_actor_step(rth_nstep *h, const rth_mlp_actor_args *args, void *stream);

/* ------------------------------------------------------------------------------------
 * Device-resident classic-control actors on the MLP kernels (csrc/env_actor.hpp): one launch per
 * env step, one kernel templated on the env, for a family of gym 0.17.3 classic-control
 * environments, each at its own network shape (H = 128):
 *   RTH_ENV_CARTPOLE     CartPole-v0/v1   D = 4, A = 2, reward 1
 *   RTH_ENV_ACROBOT      Acrobot-v1       D = 6, A = 3, reward -1 (0 on the terminal step)
 *   RTH_ENV_MOUNTAINCAR  MountainCar-v0   D = 2, A = 3, reward -1
 * The dynamics are those of reth_amd/envs.py's host classes in fp64, in their operation order.
 * rth_mlp_actor_args' fields keep their meaning; what differs is noted.  rth_cartpole_reset /
 * rth_mlp_actor_step launch these kernels' RTH_ENV_CARTPOLE instance, so the four entry points
 * agree bit for bit on CartPole (pinned by tests/test_classic_actors_gpu.py::
 * test_generic_cartpole_equals_the_cartpole_actors); only these two keep ret_stats, which they
 * require.
 * ---------------------------------------------------------------------------------- */
enum { RTH_ENV_CARTPOLE = 0, RTH_ENV_ACROBOT = 1, RTH_ENV_MOUNTAINCAR = 2 };
typedef struct rth_env_actor_args {
  const float *const *params;
  int64_t env;                /* RTH_ENV_* */
  int64_t D, H, A;            /* must be the env's */
  double *state;              /* [N, 4] fp64 env state; columns the env does not use stay 0 */
  int32_t *ep_steps;
  int64_t *t_dev;
  int64_t *stats;             /* [N, 3] finished episodes, sum of their lengths, last length */
  double *ret_stats;          /* [N, 3] fp64: running return, sum of finished returns, last finished return */
  float *obs_ring;            /* [N * ring + 1, LD] f32, LD = D rounded up to 4 (pad floats 0), 16-byte aligned;
                                 last row: zero sink */
  int64_t *cur_slot;
  const double *eps;
  const int64_t *action_in;   /* nullable */
  int64_t *action;
  float *reward, *done;
  int64_t *s0_h, *s1_h;
  int32_t *emit;
  int64_t *row_s0, *row_a, *row_s1;
  float *row_r, *row_done;
  float *row_obs0, *row_obs1; /* out [N, D] dense: the emitted row's observations by value (16-byte aligned) */
  float *q_out;               /* out [N, A] nullable */
  uint64_t seed;
  int64_t N;
  int32_t ring;               /* slots per env: >= 4 and >= 2 (n_step + 2) */
  int32_t max_episode_steps;  /* TimeLimit: CartPole-v0 / MountainCar-v0 200, CartPole-v1 / Acrobot-v1 500 */
} rth_env_actor_args;
/* env.reset() of every env: states from Philox(seed, env, t = 0) on the env's stream (mapping:
 * csrc/env_actor.hpp), ep_steps / t_dev / stats / ret_stats = 0, the observation into ring slot 1,
 * cur_slot = 1.  Arguments are checked before anything is launched (RTH_ERR_INVALID, rth_last_error). */
int rth_env_reset(const rth_env_actor_args *args, void *stream);
/* One env step of all N actors, one launch: the step rth_mlp_actor_step describes, with the env's
 * dynamics, reward, terminal rule and observation map, and the return statistics.  args->N must equal the adder's.
 * Arguments are checked before anything is launched. */
int rth_env_actor_step(rth_nstep *h, const rth_env_actor_args *args, void *stream);

/* ------------------------------------------------------------------------------------
 * DDPG's actor and critic (ddpg_model.py:76-122) as fused fp32 kernels (ddpg.hpp):
 *   actor   fc1 (D -> H1), ReLU, fc2 (H1 -> H2), ReLU, fc3 (H2 -> Ad), tanh
 *   critic  fc1 (D -> H1), ReLU, fc2 (H1 + Ad -> H2) on cat(relu(fc1(s)), a), ReLU, fc3 (H2 -> 1)
 * A network is a HOST array of six device pointers in torch layout, read in place: {fc1.weight,
 * fc1.bias, fc2.weight, fc2.bias, fc3.weight, fc3.bias}; gradients have the same order and shapes
 * (every element written, nothing accumulated).  Built for D in 1..64, Ad in 1..8, H1 and H2
 * multiples of 4 in 4..512, any n, B >= 1; other shapes return RTH_ERR_INVALID and launch nothing.
 * Every product is one fp32 fmaf and a dot product has one fixed summation order, so a row's
 * action or Q does not depend on n, on the row's position or on the entry point; the gradients
 * sum over the batch in a fixed order (no atomics).  tanh is evaluated in fp64 and rounded once.
 * Inputs are fp32 matrices with unit column stride and the given row strides (in floats).  All
 * launches go to `stream`, without host synchronisation or allocation.
 * ---------------------------------------------------------------------------------- */
int rth_ddpg_supported(int64_t D, int64_t Ad, int64_t H1, int64_t H2); /* 1 where built, else 0 */
/* bytes for rth_ddpg_critic_grads / rth_ddpg_actor_grads (one size serves both); < 0: error */
int64_t rth_ddpg_workspace(int64_t B, int64_t D, int64_t Ad, int64_t H1, int64_t H2);
/* act_out[n, Ad] = actor(x[n, D]), dense rows.  One launch (ddpg_solver.py:112-118). */
int rth_ddpg_act(const float *const *actor, const float *x_dev, int64_t ldx, int64_t n, int64_t D, int64_t Ad,
                 int64_t H1, int64_t H2, float *act_out_dev, void *stream);
/* ddpg_solver.py:79-94: a1 = actor_target(s1), y = r + ((1 - done) * gamma) * critic_target(s1, a1),
 * td = critic(s0, a) - y, loss = mean(td^2 * isw) (isw fp32, nullable) and the backward into the
 * critic's grads[6].  grads == NULL: no backward (calc_loss).  td_abs_dev [B] = |td|, loss_dev [1]
 * nullable.  At most two launches. */
int rth_ddpg_critic_grads(const float *const *critic, const float *const *actor_target,
                          const float *const *critic_target, const float *s0_dev, int64_t lds0, const float *a_dev,
                          int64_t lda, const float *r_dev, const float *done_dev, const float *s1_dev, int64_t lds1,
                          const float *isw_dev, int64_t B, int64_t D, int64_t Ad, int64_t H1, int64_t H2, float gamma,
                          float *const *grads, float *td_abs_dev, float *loss_dev, void *workspace_dev, void *stream);
/* ddpg_solver.py:98-101: loss = -mean(critic(s0, actor(s0))) and its backward into the ACTOR's
 * grads[6]: through the critic's fc3, fc2's ReLU and the action columns [H1, H1 + Ad) of its
 * fc2.weight, through 1 - tanh^2 and the actor's three layers.  The critic is only read and no
 * critic gradient is produced.  loss_dev [1] nullable.  Afterwards the first B * Ad floats of the
 * workspace hold the actions actor(s0) -- rth_ddpg_act's values, bit for bit.  Two launches. */
int rth_ddpg_actor_grads(const float *const *actor, const float *const *critic, const float *s0_dev, int64_t lds0,
                         int64_t B, int64_t D, int64_t Ad, int64_t H1, int64_t H2, float *const *grads,
                         float *loss_dev, void *workspace_dev, void *stream);
/* Polyak update (algorithm/util.py:15-24) of n_tensors <= 16 tensors in one launch; target, source
 * and numel are HOST arrays.  Per element fl(fl(t * (float)(1 - tau)) + fl(p * (float)tau)): two
 * fp32 products and one fp32 sum, never contracted -- what torch computes for
 * target * (1.0 - tau) + param * tau. */
int rth_soft_update(float *const *target, const float *const *source, const int64_t *numel, int32_t n_tensors,
                    double tau, void *stream);

/* ------------------------------------------------------------------------------------
 * PPO's actor and value network (ppo_model.py:6-40) as fused fp32 kernels (ppo.hpp):
 *   actor  Linear (D -> H), tanh, Linear (H -> H), tanh, Linear (H -> A), softmax
 *   value  Linear (D -> H), tanh, Linear (H -> H), tanh, Linear (H -> 1)
 * A network is a HOST array of six device pointers in torch layout, read in place (rth_mlp_q's
 * `params`: {0.weight, 0.bias, 2.weight, 2.bias, 4.weight, 4.bias} of the Sequential); gradients
 * have the same order and shapes (every element written, nothing accumulated).  Built for H = 64,
 * D in 1..64, A in 2..18, any n (rth_ppo_act: up to 2^32), B >= 1; every entry point returns
 * RTH_ERR_INVALID for another shape or a row stride below D and launches nothing.
 * Every product is one fp32 fmaf and a dot product has one fixed summation order; the last layer's
 * 64 products are summed in fp64 (increasing k, then the bias) and the logit or value rounded once,
 * as a trained policy's logits reach the hundreds; tanh, exp and log are evaluated in fp64 and
 * rounded once.  The policy is the log-softmax of the logits z: with
 * m = max_j z_j and s = sum_j exp(z_j - m) (fp64, increasing j), logp_j = fl32((z_j - m) - log s)
 * and p_j = fl32(exp(logp_j)).  The reference builds Categorical(probs = softmax(z)), which clamps
 * the probabilities to [1.19e-7, 1 - 1.19e-7] before taking their logarithm; this form has no
 * such clamp, so the two differ where a probability leaves that range (and nowhere else beyond
 * rounding).  One forward and one log-softmax serve both entry points: a row's log-probability
 * does not depend on n, on the row's position, on the row stride or on the entry point.
 * Inputs are fp32 matrices with unit column stride and the given row stride (in floats).  All
 * launches go to `stream`, without host synchronisation or allocation.
 * ---------------------------------------------------------------------------------- */
int rth_ppo_supported(int64_t D, int64_t H, int64_t A); /* 1 where built, else 0 */
int64_t rth_ppo_workspace(int64_t B, int64_t D, int64_t H, int64_t A); /* bytes for rth_ppo_grads; < 0: error */
/* ppo_solver.py:102-109 for n states, one launch: probs = actor(x) (probs_dev [n, A] dense,
 * nullable), one Categorical draw per row by inverse CDF -- c_j = fl32(c_{j-1} + p_j) in increasing
 * j, action = the first j with (double) c_j > u, or A - 1 if there is none -- and logprob =
 * logp_action.  u = uniforms_dev[row] (double in [0, 1)) where given, else the Philox4x32-10
 * uniform (53 bits, csrc/common.hpp philox_uniform) of (seed, counter, lane = row, stream word 13). */
int rth_ppo_act(const float *const *actor, const float *x_dev, int64_t ldx, int64_t n, int64_t D, int64_t H, int64_t A,
                const double *uniforms_dev, uint64_t seed, uint64_t counter, int64_t *action_dev, float *logprob_dev,
                float *probs_dev, void *stream);
/* One epoch of ppo_solver.py:72-96 for both networks.  With v_b = value(s_b), adv_b = ret_b - v_b,
 * rho_b = exp(logp_b[a_b] - old_logprob_b), H_b = -sum_j p_bj logp_bj and mse = (1/B) sum_b
 * (v_b - ret_b)^2:
 *   loss_b = -min(rho_b adv_b, clamp(rho_b, 1 - eps_clip, 1 + eps_clip) adv_b) + vf_coef mse - ent_coef H_b
 * (the reference: vf_coef = 0.5, ent_coef = 0.01); loss_abs_dev [B] = |loss_b|, loss_mean_dev [1]
 * (nullable) = the mean of loss_b.  The backward of that mean goes into actor_grads[6] -- through
 * d/d(logits) = (1/B) [k_b (onehot(a_b) - p_b) + ent_coef p_b (logp_b + H_b)], k_b = -rho_b adv_b
 * where the unclipped term is the minimum or rho_b lies inside the clip range, else 0 -- and into
 * value_grads[6] -- through d/dv_b = 2 vf_coef (v_b - ret_b) / B; the advantage carries no gradient.
 * Both gradient arrays NULL: evaluate only (loss_abs, loss_mean and the workspace are written,
 * nothing else); one of them NULL is an error.  Actions (int64) must lie in [0, A).  Afterwards
 * the first B floats of the workspace hold the new log-probabilities logp_b[a_b] -- rth_ppo_act's
 * logprob for that network, row and action, bit for bit.  Two launches: the tile pass, then the
 * batch reductions in a fixed order (no atomics), which also finish the per-row loss. */
int rth_ppo_grads(const float *const *actor, const float *const *value, const float *s_dev, int64_t lds,
                  const int64_t *a_dev, const float *ret_dev, const float *old_logprob_dev, int64_t B, int64_t D,
                  int64_t H, int64_t A, float eps_clip, float vf_coef, float ent_coef, float *const *actor_grads,
                  float *const *value_grads, float *loss_abs_dev, float *loss_mean_dev, void *workspace_dev,
                  void *stream);
/* rth_ppo_grads for a batch whose row count is known only on the device: B is the CAPACITY (the
 * workspace is laid out for it: rth_ppo_workspace(B, ...); loss_abs_dev holds B floats) and the
 * batch is the first n = min(n_dev[0], B) rows, read on the device.  Gradients, loss_abs[0, n),
 * loss_mean and the workspace's log-probabilities equal rth_ppo_grads' with B = n on those rows bit
 * for bit (one code path); rows at n and beyond are neither read nor written.  n = 0: every
 * gradient element and loss_mean are written 0. */
int rth_ppo_grads_n(const float *const *actor, const float *const *value, const float *s_dev, int64_t lds,
                    const int64_t *a_dev, const float *ret_dev, const float *old_logprob_dev, int64_t B, int64_t D,
                    int64_t H, int64_t A, float eps_clip, float vf_coef, float ent_coef, float *const *actor_grads,
                    float *const *value_grads, float *loss_abs_dev, float *loss_mean_dev, void *workspace_dev,
                    const int64_t *n_dev, void *stream);
/* rth_ppo_grads_n with the advantage as an input: the surrogate uses adv_b = adv_dev[b] (float [B])
 * where rth_ppo_grads forms ret_b - v_b; the value loss and its gradient still use ret_dev.  n_dev
 * is nullable here: NULL means n = B.  Everything else -- workspace, loss_abs, loss_mean, two
 * launches, no atomics, the checks before any launch -- is rth_ppo_grads' (one code path: with
 * adv_b = fl32(ret_b - v_b) the results are rth_ppo_grads' bit for bit).  Rows of adv_dev at n and
 * beyond are not read. */
int rth_ppo_grads_adv(const float *const *actor, const float *const *value, const float *s_dev, int64_t lds,
                      const int64_t *a_dev, const float *ret_dev, const float *adv_dev, const float *old_logprob_dev,
                      int64_t B, int64_t D, int64_t H, int64_t A, float eps_clip, float vf_coef, float ent_coef,
                      float *const *actor_grads, float *const *value_grads, float *loss_abs_dev, float *loss_mean_dev,
                      void *workspace_dev, const int64_t *n_dev, void *stream);
/* Advantage normalisation, one launch (one workgroup), in place over the first n = min(n_dev[0], B)
 * rows (n_dev NULL: n = B): adv_b = (float) (((double) adv_b - mean) / (std + 1e-8)), mean and the
 * population standard deviation of the fp32 advantages summed in fp64 in a fixed order (lane t of
 * 1024 sums rows t, t + 1024, ... in increasing order, then a tree over the lanes).  n = 0 writes
 * nothing, n = 1 writes 0.  Rows at n and beyond are neither read nor written. */
int rth_ppo_adv_normalize(float *adv_dev, int64_t B, const int64_t *n_dev, void *stream);
/* Shuffled minibatches (csrc/ppo_shuffle.hpp): a counter-based random permutation of the batch's
 * first n = min(max(n_dev[0], 0), B) rows (n_dev NULL: n = B), drawn on the device, and the batch
 * laid out as K dense minibatches.  With M = ceil(n / K) (0 when n = 0) and the pitch Mcap =
 * ceil(B / K):
 *   key_i   = keys_in[i] (uint64 [B]) where given, else c[0] | (uint64) c[1] << 32 of Philox4x32-10 on
 *             the block {lane = i, (uint32) c, (uint32) (c >> 32), stream word 14}, c = counter_dev[0],
 *             key (seed lo, seed hi)
 *   perm    = the STABLE argsort of key[0..n): perm_dev[q] = i where q = #{j < n : key_j < key_i, or
 *             key_j == key_i and j < i}; perm_dev[n..B) is not written
 *   gather  position q < n is minibatch m = q / M, place j = q % M: row perm[q] of every column goes,
 *           bits unchanged, to row m * Mcap + j of the mb_* columns (mb_s_dev: [K * Mcap, D] dense; the
 *           source has row stride lds >= D); rows that are no position's destination are neither read
 *           nor written
 *   mb_n_dev[m] = clamp(n - m * M, 0, M), m < K
 * and afterwards counter_dev[0] += 1, with keys_in or without (in the second launch; the first one
 * reads it).  adv_dev and mb_adv_dev are both given or both NULL.  Minibatch m is then the batch
 * (mb_s_dev + m * Mcap * D, ...) of capacity Mcap and device row count mb_n_dev + m for
 * rth_ppo_grads_n / rth_ppo_grads_adv.  B in 1..65,536, D in 1..64, K in 1..64 and K <= B; the
 * workspace holds the keys (rth_ppo_shuffle_workspace(B) bytes).  Two launches, no atomics, no host
 * synchronisation or allocation; the checks come before any launch (RTH_ERR_INVALID). */
int64_t rth_ppo_shuffle_workspace(int64_t B); /* bytes; < 0: error */
int rth_ppo_shuffle(const float *s_dev, int64_t lds, const int64_t *a_dev, const float *ret_dev, const float *adv_dev,
                    const float *old_logprob_dev, int64_t B, const int64_t *n_dev, int64_t D, int64_t K, uint64_t seed,
                    int64_t *counter_dev, const uint64_t *keys_in, float *mb_s_dev, int64_t *mb_a_dev,
                    float *mb_ret_dev, float *mb_adv_dev, float *mb_logprob_dev, int64_t *mb_n_dev, int32_t *perm_dev,
                    void *workspace_dev, void *stream);

/* ------------------------------------------------------------------------------------
 * Device-resident PPO actors on the fused actor above (csrc/ppo_actor.hpp): the on-policy rollout
 * of reth/examples/ppo/run.py for N envs of the classic-control family (RTH_ENV_*: CartPole
 * D = 4, A = 2; Acrobot D = 6, A = 3; MountainCar D = 2, A = 3; H = 64), kept in HBM.
 * Step, one launch: per env the acting forward and log-softmax (rth_ppo_act's probabilities, bit
 * for bit), t = t_dev[i] + 1, one Categorical draw by rth_ppo_act's inverse CDF on u =
 * uniforms_in[i] or the Philox uniform of (seed, counter = t, lane = i, stream word 13), or
 * action_in[i]; logprob of the action taken; the env's fp64 dynamics, time limit and reset
 * (csrc/env_actor.hpp); and the row (s0, a, r, done, logp) appended to the env's rollout segment:
 * columns [N, cap, .] dense, fill[i] rows stored, the first complete[i] of them in finished
 * episodes.  A full segment stores nothing and counts the row in dropped[i]; nothing is written
 * outside a buffer.  complete is int32 [2, N]: the live slot of env i is gen[i] & 1 (the finish
 * reads one slot of every env and zeroes the other of its own, then gen[i] += 1).
 * No host synchronisation, no atomics; graph-capturable.
 * ---------------------------------------------------------------------------------- */
typedef struct rth_ppo_actor_args {
  const float *const *actor;  /* the actor: HOST array of six device pointers (the step only) */
  int64_t env;                /* RTH_ENV_* */
  int64_t D, H, A;            /* must be the env's D and A; H = 64 */
  double *state;              /* [N, 4] fp64 env state; columns the env does not use stay 0 */
  int32_t *ep_steps;          /* [N] steps of the running episode */
  int64_t *t_dev;             /* [N] env steps taken (the Philox counter) */
  int64_t *stats;             /* [N, 3] finished episodes, sum of their lengths, last length */
  double *ret_stats;          /* [N, 3] fp64: running return, sum of finished returns, last finished return */
  float *cur_obs;             /* [N, LD] f32, LD = D rounded up to 4 (pad floats 0), 16-byte aligned: the
                                 observation each env acts on next */
  const int64_t *action_in;   /* [N] nullable: overrides the drawn action */
  const double *uniforms_in;  /* [N] nullable: replaces the Philox uniform (double in [0, 1)) */
  int64_t *action;            /* out [N]: the step's action */
  float *logprob;             /* out [N]: its log-probability */
  float *seg_s;               /* [N, cap, D] the observations acted on */
  int64_t *seg_a;             /* [N, cap] */
  float *seg_r, *seg_done, *seg_logp; /* [N, cap] each */
  int32_t *fill;              /* [N] rows stored */
  int32_t *complete;          /* [2, N] rows of finished episodes; env i's live slot: gen[i] & 1 */
  int32_t *gen;               /* [N] finishes so far */
  int64_t *dropped;           /* [N] rows not stored because the segment was full */
  uint64_t seed;
  int64_t N;
  int32_t cap;                /* rows per env, 1..4096 */
  int32_t max_episode_steps;  /* TimeLimit */
} rth_ppo_actor_args;
/* env.reset() of every env: states from Philox(seed, env, t = 0), ep_steps / t_dev / stats /
 * ret_stats / fill / complete / gen / dropped = 0, the observation into cur_obs.  Arguments are
 * checked before anything is launched (RTH_ERR_INVALID, rth_last_error). */
int rth_ppo_env_reset(const rth_ppo_actor_args *args, void *stream);
/* One env step of all N actors, one launch.  Arguments are checked before anything is launched. */
int rth_ppo_actor_step(const rth_ppo_actor_args *args, void *stream);
/* The end of a rollout, one launch, one workgroup per env.  Rows [0, complete[i]) of env i are whole
 * episodes; each episode's returns are algorithm/util.py:27-40 on that episode alone, in fp64:
 * backwards, run = run * gamma + r_t (one product, one sum), d_t = (float) run, a done row 0; then
 * ret_t = (float) ((d_t - mean) / (sqrt(var) + 1e-7)) with the episode's own mean and population
 * variance of the fp32 d_t, summed in increasing t.  The rows (s, a, ret, logp) go to the dense
 * batch (batch_s [., D], the others [.]; N * cap rows hold any rollout) env-major, then in time
 * order, n_dev[0] = their count; batch rows at n and beyond are left as they were.  The rows of
 * the episode still running move to the front of the segment with their old log-probabilities:
 * fill[i] -= complete[i], complete[i] = 0.  Arguments are checked before anything is launched. */
int rth_ppo_rollout_finish(const rth_ppo_actor_args *args, double gamma, float *batch_s_dev, int64_t *batch_a_dev,
                           float *batch_ret_dev, float *batch_logprob_dev, int64_t *n_dev, void *stream);
/* The end of a rollout with GAE(lambda) and a value bootstrap at the rollout's edge: the other
 * estimator on the segments the step leaves.  `value` is the value network (HOST array of six
 * device pointers); args->cur_obs is read (the step's other state buffers are not).  Env i
 * contributes all of its T = fill[i] rows (0..cap): v_t = value(s_t) and v_last = value(cur_obs[i]),
 * by the forward of rth_ppo_grads (the value that entry point computes for the row with the same
 * weights, bit for bit), then in fp64, every operation rounded once and none contracted, backwards
 * over t = T-1 .. 0 with run = 0:
 *   nt    = 1 - done_t
 *   nv    = (t == T-1) ? v_last : v_{t+1}
 *   delta = (r_t + (gamma * nv) * nt) - v_t
 *   run   = delta + ((gamma * lam) * nt) * run
 *   adv_t = (float) run,   ret_t = (float) (run + (double) v_t)
 * A done row is a terminal state whether the time limit or the dynamics ended the episode: nothing
 * is bootstrapped through it.  The rows (s, a, ret, adv, v, logp) go to the dense batch (batch_s
 * [., D], the others [.]; N * cap rows hold any rollout) at offset sum_{k<i} fill[k] -- env-major,
 * then in time order -- and n_dev[0] = sum_k fill[k]; batch rows at n and beyond are left as they
 * were.  Then fill[i] = 0, both complete slots of env i = 0 and gen[i] += 1: there is no carry.
 * Two launches on `stream` (one workgroup per env, then the counters -- no workgroup may empty a
 * fill another still has to sum); no atomics, no host synchronisation, graph-capturable.  gamma and
 * lam in 0..1; arguments are checked before anything is launched. */
int rth_ppo_gae_finish(const rth_ppo_actor_args *args, const float *const *value, double gamma, double lam,
                       float *batch_s_dev, int64_t *batch_a_dev, float *batch_ret_dev, float *batch_adv_dev,
                       float *batch_v_dev, float *batch_logprob_dev, int64_t *n_dev, void *stream);
/* rth_ppo_actor_step that also records why an episode ended and what it ended on.  With the row it
 * stores (0 <= fill[i] < cap; a dropped row writes neither column):
 *   seg_trunc[row] = (steps >= max_episode_steps && !terminal) ? 1 : 0    [N, cap] f32
 * where `terminal` is the dynamics' own end: an end with both causes on one step is terminal, not
 * truncated.  On a truncated row only, seg_term_s[row * D .. + D) ([N, cap, D] f32) gets the
 * observation of the post-dynamics state, taken before the reset draw replaces it; other rows of
 * seg_term_s are not written.  Every other output -- action, logprob, state, stats, cur_obs, the
 * five segment columns, fill / complete / dropped -- equals rth_ppo_actor_step's bit for bit.  One
 * launch, no atomics, graph-capturable; arguments are checked before anything is launched. */
int rth_ppo_actor_step_tl(const rth_ppo_actor_args *args, float *seg_trunc_dev, float *seg_term_s_dev, void *stream);
/* rth_ppo_gae_finish that bootstraps through time-limit ends.  Per env, after v_t and v_last, vterm_t
 * = value(seg_term_s[t]) for the rows with seg_trunc[t] != 0, by the same forward, and the scan
 * selects its operands:
 *   nt    = 1 - done_t
 *   nb    = trunc_t ? 1 : nt
 *   nv    = trunc_t ? vterm_t : ((t == T-1) ? v_last : v_{t+1})
 *   delta = (r_t + (gamma * nv) * nb) - v_t
 *   run   = delta + ((gamma * lam) * nt) * run
 *   adv_t = (float) run,   ret_t = (float) (run + (double) v_t)
 * in fp64, every operation rounded once and none contracted.  The lambda-chain is still cut at every
 * done row; a truncated row (done flags are 0 or 1) bootstraps from the value of the state its
 * episode ended on.  With seg_trunc all zero every output equals rth_ppo_gae_finish's bit for bit;
 * rows of seg_term_s whose seg_trunc is 0 are never read.  Row order, n_dev, the counters, the two
 * launches and the checks are rth_ppo_gae_finish's; both new columns are required (not NULL). */
int rth_ppo_gae_finish_tl(const rth_ppo_actor_args *args, const float *const *value, double gamma, double lam,
                          float *batch_s_dev, int64_t *batch_a_dev, float *batch_ret_dev, float *batch_adv_dev,
                          float *batch_v_dev, float *batch_logprob_dev, int64_t *n_dev, const float *seg_trunc_dev,
                          const float *seg_term_s_dev, void *stream);

/* ------------------------------------------------------------------------------------
 * Device-resident continuous-control actors on DDPG's fused actor (csrc/ddpg_actor.hpp): one
 * launch per env step of N envs, one kernel templated on the env:
 *   RTH_DDPG_ENV_PENDULUM  Pendulum-v0  D = 3, Ad = 1, reward -cost, no terminal state
 * Per env: the acting forward (rth_ddpg_act's action, bit for bit), Ornstein-Uhlenbeck noise on
 * counter-based normal draws (utils/noise.py, utils/exploration.py:34-53; the draws' mapping is
 * documented in csrc/ddpg_actor.hpp), action = (float) ((double) act_det + eps * x') without
 * clipping, the dynamics of reth_amd/envs.py's host class in fp64 in its operation order, the
 * time limit, the reset of a finished episode (env state from Philox(seed, env, t), noise back to
 * mu) and the transition as a dense row.  eps = eps_start + (eps_end - eps_start) * k / eps_steps,
 * k = min(t, eps_steps), t = t_dev[i] + 1 the env's own act count: the schedule advances once per
 * launch.  No host synchronisation, no atomics; graph-capturable.
 * ---------------------------------------------------------------------------------- */
enum { RTH_DDPG_ENV_PENDULUM = 0 };
typedef struct rth_ddpg_actor_args {
  const float *const *actor;  /* the actor: HOST array of six device pointers (unused by the reset) */
  int64_t env;                /* RTH_DDPG_ENV_* */
  int64_t D, Ad, H1, H2;      /* D, Ad must be the env's; the shape one rth_ddpg_supported builds */
  double *state;              /* [N, 4] fp64 env state; columns the env does not use stay 0 */
  int32_t *ep_steps;          /* [N] steps of the running episode */
  int64_t *t_dev;             /* [N] env steps taken (the Philox counter, the schedule's step) */
  int64_t *stats;             /* [N, 3] finished episodes, sum of their lengths, last length */
  double *ret_stats;          /* [N, 3] fp64: running return, sum of finished returns, last finished return */
  double *noise;              /* [N, Ad] fp64 OU state */
  float *cur_obs;             /* [N, LD] f32, LD = D rounded up to 4 (pad floats 0), 16-byte aligned: the
                                 observation each env acts on next */
  const float *action_in;     /* [N, Ad] nullable: overrides the noisy action (the noise still advances) */
  float *act_det;             /* out [N, Ad] nullable: the noise-free action */
  float *row_s0, *row_a, *row_r, *row_s1, *row_done; /* out, dense f32: [N, D], [N, Ad], [N], [N, D], [N] */
  uint64_t seed;
  int64_t N;
  double mu, theta, sigma;    /* OUNoise */
  double eps_start, eps_end;  /* the noise scale's linear schedule */
  int64_t eps_steps;          /* >= 1 */
  int32_t max_episode_steps;  /* TimeLimit: Pendulum-v0 200 */
  int32_t reserved;
} rth_ddpg_actor_args;
/* env.reset() of every env: states from Philox(seed, env, t = 0), ep_steps / t_dev / stats /
 * ret_stats = 0, noise = mu, the observation into cur_obs.  Arguments are checked before anything
 * is launched (RTH_ERR_INVALID, rth_last_error). */
int rth_ddpg_env_reset(const rth_ddpg_actor_args *args, void *stream);
/* One env step of all N actors, one launch.  Arguments are checked before anything is launched. */
int rth_ddpg_actor_step(const rth_ddpg_actor_args *args, void *stream);

/* ------------------------------------------------------------------------------------
 * Learner -> actor weights: a device-resident latest-wins slot with a device version.
 * Replaces perwez's PUB/SUB CONFLATE weights channel (perwez/perwez/client/socket.py:19-122,
 * 302-328: SendSocket.send / RecvSocket.recv / RecvSocket.empty) as used by
 * test/apex-dqn/trainer.py:38-41 (publish every send_weights_interval updates) and
 * worker.py:37-41 (load when > recv_weights_interval steps passed and a message waits).
 * Segments: the parameter tensors, 4-byte aligned, in a fixed order (<= 64).
 * ---------------------------------------------------------------------------------- */
typedef struct rth_weights rth_weights;
int rth_weights_create(int64_t bytes, int device, rth_weights **out);
int rth_weights_destroy(rth_weights *h);
int64_t rth_weights_bytes(const rth_weights *h);
/* SendSocket.send: copy the n segments into the slot, then version += 1 (stream order) */
int rth_weights_publish(rth_weights *h, int32_t n, const void *const *src_dev, const int64_t *bytes, void *stream);
/* the slot's initial contents without a message (version unchanged): what a subscriber that
 * connects before the first send holds -- the reference's SUB socket delivers nothing until
 * the trainer's first send (test/apex-dqn/trainer.py:38-41) */
int rth_weights_fill(rth_weights *h, int32_t n, const void *const *src_dev, const int64_t *bytes, void *stream);
/* RecvSocket.empty + recv, decided on the device: if version > *seen_dev (and, with a step
 * counter, *step_dev - *prev_dev > interval) copy the slot into the n segments, set
 * *seen_dev = version, *prev_dev = *step_dev and *loaded_dev = 1; else *loaded_dev = 0.
 * step_dev / prev_dev / loaded_dev may be NULL.  Graph-capturable (no host decision). */
int rth_weights_acquire(rth_weights *h, int32_t n, void *const *dst_dev, const int64_t *bytes, int64_t *seen_dev,
                        const int64_t *step_dev, int64_t *prev_dev, int64_t interval, int32_t *loaded_dev,
                        void *stream);
int rth_weights_version(const rth_weights *h, int64_t *out);        /* synchronous read */
int rth_weights_version_ptr(rth_weights *h, int64_t **out_dev);     /* the device counter */

/* ------------------------------------------------------------------------------------
 * LZ4 frames (host code) for compressed wire messages: Client.append(..., compress=True)
 * (reth_buffer/reth_buffer/utils/pack.py:62-84 lz4.frame.compress / :147-164 decompress),
 * what test/apex-dqn/worker.py:60 sends.  Host pointers.
 * ---------------------------------------------------------------------------------- */
int rth_lz4_frame_bound(const uint8_t *src, int64_t n, int64_t *bound);
int rth_lz4_frame_decompress(const uint8_t *src, int64_t n, uint8_t *dst, int64_t cap, int64_t *out_len);
int64_t rth_lz4_frame_compress_bound(int64_t n);
int rth_lz4_frame_compress(const uint8_t *src, int64_t n, uint8_t *dst, int64_t cap, int64_t *out_len);
uint32_t rth_xxh32(const uint8_t *src, int64_t n, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif
