/*
 * pantheon_hip.h -- C ABI of libpantheon_hip.so: the MI355X (gfx950) rollout-buffer / GAE / PPO-update
 * engine behind PantheonRL's OnPolicyAgent surface.
 *
 * The reference (Stanford-ILIAD/PantheonRL) is pure Python and delegates this path to
 * stable-baselines3==1.7.0 (reference setup.py:17).  Every entry point below replaces one reference call
 * site; the citation names it (paths relative to the reference root).  The reference-side binding a
 * maintainer would add is a ctypes stub -- see INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  Unless a parameter says "host", every pointer is a DEVICE
 *     pointer (HBM) owned by the caller; the library never frees caller memory and only allocates its own
 *     scratch inside ph_ctx (released by ph_ctx_destroy).
 *   - every call is asynchronous on the context's HIP stream (ph_ctx_set_stream); ph_ctx_sync() waits.
 *   - return value: 0 = ok, non-zero = error; ph_last_error() gives the thread-local message.  Nothing
 *     here calls abort().  No re-entrancy on one ph_ctx.
 *   - all floating point is IEEE float32 ("f32"), actions are stored float32 in the rollout buffer like
 *     SB3 does, and handed to environments as int32.
 *
 * Rollout buffer layout in HBM (same as SB3 RolloutBuffer): time-major (T, E, ...) row-major
 * float32 arrays; the PPO minibatch index n in [0, T*E) is SB3's env-major "swap_and_flatten" index
 * n = e*T + t and is translated to the physical row t*E + e inside the kernels (no flattened copy is made).
 *
 * Parameter vector layout (float32, P = ph_layout.P entries; H = 64), weights input-major [in][out]
 * (the transpose of torch.nn.Linear.weight):
 *   pi_W1[F][H] pi_b1[H] pi_W2[H][H] pi_b2[H]  vf_W1[F][H] vf_b1[H] vf_W2[H][H] vf_b2[H]
 *   act_W[H][L] act_b[L]  val_W[H] val_b[1]  (Box action spaces: + log_std[A], and L = A)
 */
#ifndef PANTHEON_HIP_H
#define PANTHEON_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PH_ABI_VERSION 7   /* 2: + ph_agent_*, ph_bc_*, ph_adap_*, ph_scripted_rollout, ph_liar_selfplay_rollout, ph_roundrobin_env_step,
                                  ph_buffer_compact_columns (additions only: every v1 signature is unchanged)
                              3: + ph_selfplay_rollout_persistent, PH_STEP_FIX_ILLEGAL / _MASK_ENV_ONLY, ph_modular_*, ph_roundrobin_*_iteration
                                  (additions only)
                              4: + ph_selfplay_rollout_persistent_capacity, ph_ppo_train's gradient pack (no signature changed)
                              5: + ph_policy_act_host, ph_buffer_add_reward_const, ph_adapmult_*, ph_ctx_set_joint_reward_rule (additions only)
                              6: + ph_bench_train_kernels, ph_debug_split_oh_tables, ph_ctx_step_errors (additions only)
                              7: ph_spec.act may be PH_SPACE_BOX on ph_layout_of / ph_policy_forward / ph_ppo_minibatch_grad / ph_ppo_train
                                  (an error before; no signature or struct changed)
                                 still 7: + ph_block_reset / _step / _obs, ph_block_selfplay_step, ph_block_replay_host (additions only)
                                 still 7: + ph_bc_train_path (addition only)
                                 still 7: + ph_adap_rows, ph_adap_context_draw, ph_adap_vec_host, ph_liar_selfplay_step_adap (additions only)
                                 still 7: + ph_block_scripted_actions / _host, ph_block_group_forward, ph_block_xplay_step (additions only)
                                 still 7: + ph_block_pool_forward, ph_block_pool_step (additions only) */
#define PH_HIDDEN 64     /* SB3 MlpPolicy default net_arch pi=[64,64], vf=[64,64] (modular/policies.py:112-114) */
#define PH_MAX_COMP 256  /* max MultiDiscrete components per space */
#define PH_MAX_LOGITS 64 /* max total policy logits L */
#define PH_MAX_BOX_ACT 16 /* max dimensions of a Box (continuous) action space: DiagGaussian head, general kernels */
#define PH_NSTAT 8       /* per-minibatch stats record, see ph_ppo_train */
#define PH_MOD_MAX 8     /* max partner modules of a ModularPolicy (ph_modular_*) */
#define PH_MAX_RANKS 16   /* ranks of one node in the peer-to-peer exchange layouts */

#define PH_SPACE_BOX 0      /* gym.spaces.Box, flattened length n                        */
#define PH_SPACE_DISCRETE 1 /* Discrete(k) (n=1, nvec={k}) or MultiDiscrete(nvec) (n=len) */

typedef struct ph_ctx ph_ctx;

typedef struct ph_space {
  int kind;              /* PH_SPACE_*                                                      */
  int n;                 /* Box: length.  Discrete family: number of components             */
  int nvec[PH_MAX_COMP]; /* Discrete family: categories per component                       */
} ph_space;

typedef struct ph_spec { /* observation_space / action_space of one agent (multiagentenv.py:72-79) */
  ph_space obs;
  ph_space act; /* PH_SPACE_DISCRETE: the categorical family PPO uses in every BASELINE config (every entry point).
                   PH_SPACE_BOX (n <= PH_MAX_BOX_ACT): SB3's DiagGaussianDistribution -- the head's n outputs are the means, log_std[n]
                   follows val_b in the parameter vector (ph_layout.P counts it); actions are float32 rows, clipped to the Box by the caller
                   (pantheonrl/common/util.py:84-99); ph_policy_forward, ph_ppo_minibatch_grad and ph_ppo_train only -- every other entry
                   point refuses the spec */
} ph_spec;

typedef struct ph_layout {
  int D; /* stored obs length per transition   */
  int F; /* feature length after one-hot       */
  int A; /* stored action length               */
  int L; /* total logits                       */
  int P; /* parameter count                    */
  int pi_W1, pi_b1, pi_W2, pi_b2, vf_W1, vf_b1, vf_W2, vf_b2, act_W, act_b, val_W, val_b; /* offsets */
} ph_layout;

typedef struct ph_rollout { /* SB3 RolloutBuffer storage; call sites agents.py:123-130,157,172-179,196-198 */
  int T, E;
  float *observations;   /* (T,E,D) */
  float *actions;        /* (T,E,A) */
  float *rewards;        /* (T,E)   */
  float *episode_starts; /* (T,E)   */
  float *values;         /* (T,E)   */
  float *log_probs;      /* (T,E)   */
  float *advantages;     /* (T,E)   */
  float *returns;        /* (T,E)   */
} ph_rollout;

typedef struct ph_ppo_hyper { /* SB3 PPO defaults mirrored at adap_learn.py:90-103; Adam eps modular/policies.py:84-88 */
  float learning_rate;      /* 3e-4 */
  float clip_range;         /* 0.2  */
  float clip_range_vf;      /* < 0 : None */
  float ent_coef;           /* 0.0  */
  float vf_coef;            /* 0.5  */
  float max_grad_norm;      /* 0.5  */
  float target_kl;          /* < 0 : None */
  int normalize_advantage;  /* 1    */
  float adam_beta1, adam_beta2, adam_eps; /* 0.9, 0.999, 1e-5 */
} ph_ppo_hyper;

typedef struct ph_opt_state {
  float *params; /* (P) */
  float *adam_m; /* (P) exp_avg    */
  float *adam_v; /* (P) exp_avg_sq */
  int *step;     /* (1) device counter: optimizer steps applied so far */
} ph_opt_state;

/* ---- library / context ------------------------------------------------------------------------------ */
int ph_abi_version(void);
const char *ph_last_error(void);
int ph_device_count(int *n_out /* host */);
/* create on HIP device `device`; fails (non-zero) when no gfx950 device is visible. <- PPO.__init__(device=) trainer.py:110,197 */
int ph_ctx_create(int device, ph_ctx **out /* host */);
int ph_ctx_destroy(ph_ctx *ctx);
int ph_ctx_set_stream(ph_ctx *ctx, void *hip_stream /* hipStream_t, may be NULL = default */);
int ph_ctx_sync(ph_ctx *ctx);
/* hipGraph capture of everything enqueued between begin/end on the ctx stream (launch-bound rollout loops) */
int ph_graph_begin(ph_ctx *ctx);
int ph_graph_end(ph_ctx *ctx, int *graph_id_out /* host */);
int ph_graph_launch(ph_ctx *ctx, int graph_id);
/* nodes of a captured graph = everything that was enqueued between begin/end: kernel launches, and memcpy / memset nodes where a
 * call enqueues one (hipGraphGetNodes counts them all); a step that only launches kernels has one node per launch.  An addition for
 * the launch-count tests; PH_ABI_VERSION unchanged */
int ph_graph_nodes(ph_ctx *ctx, int graph_id, int *nodes_out /* host */);
/* Device-resident RNG epoch.  Philox counters and permutation seeds are launch arguments, so a captured graph would
 * replay the same random numbers; when an epoch word (one device uint64, caller-owned) is attached, every random
 * stream is additionally keyed by *epoch, and ph_rng_epoch_advance enqueues *epoch += 1 (capturable). */
int ph_ctx_set_rng_epoch(ph_ctx *ctx, unsigned long long *epoch_dev /* device, or NULL to detach */);
int ph_rng_epoch_advance(ph_ctx *ctx);
/* Debug: while a buffer is attached, workgroup (bx,by) of policy_fwd / ppo_grad writes the shader clock at up to 16
 * phase boundaries to stamps[((by*gridDim.x)+bx)*16 + phase] (caller sizes it: 16 * workgroups int64).  NULL detaches. */
int ph_debug_set_profile_buffer(ph_ctx *ctx, long long *stamps_dev);
/* debug: how many elements of the context's pre-split weight image (the fragments gemm_mode 2's gradient kernel loads; kept in
 * step with the parameters by the optimizer kernel) differ from what `params` (device, P floats) split to right now.
 * *mismatches (host) = -1 when the context holds no image.  Synchronises the context's stream. */
int ph_debug_weight_image_mismatches(ph_ctx *ctx, const ph_spec *spec, const float *params, int *mismatches);
/* Scheduling hint: nothing else runs on this context's device while its training launches do (one learner per GPU --
 * north_star's "one agent per GPU", BASELINE config 5).  The slab reduction between two gradient launches then uses 1024-lane
 * blocks (it sits on the critical path) instead of the 256-lane blocks sized to run BESIDE another learner's gradient launch;
 * both walk the same summation tree, so results do not depend on the hint.  Default 0. */
int ph_set_exclusive_device(ph_ctx *ctx, int exclusive);
/* The one-launch reduce + clip + Adam step an exclusive learner uses (ppo_step_kernel) makes its blocks wait for each other's
 * partial results; a wait that runs into its bound (~2 s: never on a healthy, truly exclusive device) leaves that block's
 * parameters unchanged, marks the minibatch's statistics record (stats[7] = -1) and counts here.  *count_out = waits that expired
 * since the context was created; a non-zero count means an optimizer step was applied only in part: treat the run as invalid.
 * Synchronises the context's stream. */
int ph_ctx_step_errors(ph_ctx *ctx, unsigned int *count_out /* host */);
/* HIP-event timing on the ctx stream (bench.py roofline: events must sit on the stream the kernels run on) */
int ph_timer_start(ph_ctx *ctx);
int ph_timer_stop(ph_ctx *ctx, float *ms_out /* host */); /* synchronises */

/* ---- shapes --------------------------------------------------------------------------------------------- */
int ph_layout_of(const ph_spec *spec /* host */, ph_layout *out /* host */);
/* debug, host only (no device touched): the tables of gemm_mode 2's gradient kernel for `spec` -- slab_map[net * 8960 + position]
 * = parameter index held at that position of a workgroup's gradient slab (-1 = padding), image_map[2 * p + {0, 1}] = element
 * index (plane 0) of the weight-fragment image backed by parameter p (-1 = none).  *eligible = 0 (tables untouched) for specs
 * the kernel does not take. */
int ph_debug_split_tables(const ph_spec *spec, int *slab_map, int *image_map, int *eligible);
/* the same for the one-hot-observation kernel of gemm_mode 2 (ppo_grad_split_oh_kernel): *slab_len_out = ints slab_map needs
 * (a slab's floats, both nets), *image_elems_out = bf16 elements of its weight image; slab_map / image_map may be NULL (sizes only) */
int ph_debug_split_oh_tables(const ph_spec *spec, int *slab_map, int *image_map, int *slab_len_out, int *image_elems_out,
                             int *eligible);

/* ---- K1: rollout buffer writes --------------------------------------------------------------------------- */
/* RolloutBuffer.add(obs, action, reward=0, episode_start, value, log_prob) at row `pos` <- agents.py:172-179.
 * Inputs are copied (SB3 copies too), so callers may reuse them. */
int ph_buffer_add(ph_ctx *ctx, const ph_spec *spec, const ph_rollout *rb, int pos, const float *obs /* (E,D) */,
                  const float *actions /* (E,A) f32 */, const float *episode_start /* (E) */,
                  const float *values /* (E) */, const float *log_probs /* (E) */);
/* buf.rewards[pos][e] += reward[e] for e with env_mask[e] != 0 (NULL = all) <- Agent.update, agents.py:198 */
int ph_buffer_add_reward(ph_ctx *ctx, const ph_rollout *rb, int pos, const float *reward /* (E) */,
                         const unsigned char *env_mask /* (E) or NULL */);
/* Agent.update(reward, done) with a SCALAR reward (agents.py:198: buf.rewards[pos - 1][0] += reward; every environment of the
 * row receives it): the value travels as a kernel argument -- no host array, no copy, nothing to wait for. */
int ph_buffer_add_reward_const(ph_ctx *ctx, const ph_rollout *rb, int pos, float reward);
/* How the joint action of a SimultaneousEnv step enters every agent's reward in ph_buffer_add_reward_joint, ph_policy_step_multi,
 * ph_selfplay_rollout_* (multiagentenv.py:395-409 hands each agent ITS reward of the step).  A setting of the context:
 *   PH_JOINT_MATCH_BONUS (default): + bonus * [own action == partner's]   -- the synthetic driver's shared coordination term
 *   PH_JOINT_RPS:                   + bonus * rock-paper-scissors payoff of (own, partner's): (own - partner's + 3) % 3 == 1 wins,
 *                                     == 2 loses, 0 draws (rps.py:41-45; zero-sum: the partner's reward is the negative) -- a
 *                                     device-resident RPS self-play is the exchange rollout under this rule (bonus = 1, base reward 0,
 *                                     every step ends its episode) */
#define PH_JOINT_MATCH_BONUS 0
#define PH_JOINT_RPS 1
int ph_ctx_set_joint_reward_rule(ph_ctx *ctx, int rule);

/* Agent-per-GPU SimultaneousEnv step (multiagentenv.py:149-170 with the actions all-gathered over RCCL): seat `seat`
 * receives rewards[pos][e] += base_reward[e] + bonus * (joint[seat][e] == joint[*partner_seat][e]) -- the shared
 * coordination term of the synthetic transition, consuming the JOINT action.  joint_actions is (n_seats, E) int32;
 * partner_seat is a DEVICE int so the round-robin pairing (kept in Python) can change between graph replays. */
int ph_buffer_add_reward_joint(ph_ctx *ctx, const ph_rollout *rb, int pos, const float *base_reward /* (E) */,
                               const int *joint_actions, int n_seats, int seat, const int *partner_seat /* device */,
                               float bonus);
/* One-agent-per-GPU round-robin layout (BASELINE config 4: ego vs K OnPolicy partners, exactly one partner active per episode):
 * the synthetic 2-player SimultaneousEnv transition of n environments on the ego's rank <- MultiAgentEnv.step / reset,
 * multiagentenv.py:149-243, with the per-environment partner id the reference keeps in `partnerids` (:105-125).
 *   joint_actions (1 + n_partners, n) int32: row 0 the ego's actions, row 1 + k partner k's (all-gathered over RCCL)
 *   partnerid (n) int32 in/out: the partner of each environment; where done[e] != 0 it advances to (id + 1) % n_partners --
 *       resample_round_robin at that environment's own reset (:118-125,224)
 *   reward_out (n): base_reward[e] + bonus * [ego action == its partner's action] (Overcooked's reward is shared, so this is
 *       both players' reward); alt_action_out (n) or NULL: the partner action each environment consumed
 *   next_block (n, block_ld) f32 or NULL: header columns 0..2 of the next step's routing block are written --
 *       [partner id of the next step | reward_out | done] -- the block the ego's rank sends to the partner ranks together
 *       with the partner-seat observations in columns 3.. */
int ph_roundrobin_env_step(ph_ctx *ctx, const int *joint_actions, int *partnerid, const float *base_reward,
                           const float *done, float *reward_out, int *alt_action_out, float *next_block, int block_ld,
                           int n_partners, float bonus, int n);
/* The same layout with ONE native call per iteration and rank (no host tensor op, collective call or synchronisation per
 * environment step).  Every rank owns a fine-grained receive area (ph_p2p_alloc) that the others map through HIP IPC
 * (ph_p2p_open): [64 stamp words | slot 0 | slot 1], ph_rr_area_bytes() long; a partner's slot holds the block's header rows
 * (n, 4) = [partner id | reward | done | -] followed by the observations (n, D), rank 0's slot the actions (1 + K, n).  Per step t of iteration i (stamp i * T + t + 1):
 *   rank 0 : ego forward + rollout-buffer row (its actions land in row 0 of its own slot t & 1) -> the routing block of step t
 *            stored into every partner's slot t & 1, then the partner's block stamp -> wait for the K action stamps -> the
 *            transition of ph_roundrobin_env_step (writes the header of block t + 1)            multiagentenv.py:149-243
 *   rank 1+k: wait for the block stamp -> Agent.update of the previous step where it acted, this step's record mask, room and
 *            episode_start (agents.py:186-203,176) -> ph_policy_forward_ragged -> advance the write rows, store its actions into
 *            row 1 + k of rank 0's slot, then its action stamp.
 * A step is ping-pong between rank 0 and each partner, so two slots suffice.  Waits are bounded; a timeout bumps *error.
 * The caller (roundrobin.py) credits the ego's last reward, runs the learners' updates and decides ONCE per iteration whether a
 * partner whose columns are full trains (the reference's partner checks before every action, agents.py:126). */
typedef struct ph_rr_link {
  int n_partners, rank;                 /* rank 0 = ego, 1 + k = partner k */
  int n, block_ld;                      /* environments; floats per routing-block row (3 + D) */
  void *area[PH_MAX_RANKS];             /* [r] rank r's receive area as mapped in this process (own one included) */
  unsigned long long *error;            /* local device word */
  unsigned long long timeout_cycles;    /* bound of one wait, wall_clock64() ticks (100 MHz) */
} ph_rr_link;
typedef struct ph_rr_ego {
  const ph_spec *spec;                  /* host */
  const float *params;
  const float *obs_seq;                 /* (T, n, D) the ego's observations */
  const float *base_reward_seq;         /* (T, n) */
  const float *done_seq;                /* (T, n) */
  float *blocks;                        /* (T, n, block_ld): observation columns prefilled, headers written step by step */
  int *partnerid;                       /* (n) in/out */
  float *rewards;                       /* (T, n) out */
  int *alt_actions;                     /* (T, n) out */
  int *partner_trace;                   /* (T, n) out */
  const float *episode_start0;          /* (n) */
  unsigned long long seed, counter0;
  float *values, *log_probs;            /* (n) */
  const ph_rollout *rb;                 /* host; rows 0 .. T-1 */
  float bonus;
} ph_rr_ego;
typedef struct ph_rr_partner {
  const ph_spec *spec;                  /* host */
  const float *params;
  float *obs_scratch;                   /* unused (the forward reads the observations from the receive slot); may be NULL */
  float *es_scratch;                    /* (n) */
  unsigned char *can_scratch;           /* (n) */
  int *pos;                             /* (n) per-environment write rows, in/out */
  unsigned char *boundary, *term, *open, *prev_mask;   /* (n) RaggedVecOnPolicyAgent's book-keeping, in/out */
  unsigned long long seed, counter0;
  int *actions;                         /* (n) */
  float *values, *log_probs;            /* (n) */
  const ph_rollout *rb;                 /* host */
} ph_rr_partner;
int ph_rr_area_bytes(int n_partners, int n, int block_ld, size_t *bytes_out /* host */);
int ph_roundrobin_ego_iteration(ph_ctx *ctx, const ph_rr_link *link, const ph_rr_ego *ego, int T, unsigned long long iteration);
int ph_roundrobin_partner_iteration(ph_ctx *ctx, const ph_rr_link *link, const ph_rr_partner *partner, int T,
                                    unsigned long long iteration);
/* RolloutBuffer.reset() <- agents.py:157 : zero-fills every array */
int ph_buffer_reset(ph_ctx *ctx, const ph_spec *spec, const ph_rollout *rb);

/* ---- K2: GAE ------------------------------------------------------------------------------------------------ */
/* RolloutBuffer.compute_returns_and_advantage(last_values, dones) <- agents.py:127-130.
 * gamma / gae_lambda are doubles because the reference multiplies them as Python floats before the
 * float32 array arithmetic (gamma*gae_lambda is rounded to f32 once).
 * mode 0 = auto, 1 = serial-in-T / one lane per env (summation order and rounding identical to the numpy
 * loop: bit-exact), 2 = chunked wavefront suffix scan over T, any T (fp32 tolerance). */
int ph_gae(ph_ctx *ctx, const ph_rollout *rb, const float *last_values /* (E) */, const float *dones /* (E) */,
           double gamma, double gae_lambda, int mode);

/* ---- K4: policy forward --------------------------------------------------------------------------------------- */
/* ActorCriticPolicy.forward(obs) -> (actions, values, log_probs) <- util.py:63-81 (action_from_policy), agents.py:162.
 *  action_mask (n,L) u8 or NULL : logits -= 30*(1-mask)  (modular/policies.py:330-333)
 *  uniforms (n,A) or NULL       : teacher-forced inverse-CDF sampling; NULL = Philox4x32-10 keyed (seed, counter, row, comp)
 *  given_actions (n,A) f32 or NULL : evaluate these instead of sampling (evaluate_actions, modular/policies.py:364-383)
 *  deterministic != 0           : argmax
 * Box action spaces (spec->act.kind == PH_SPACE_BOX; SB3 DiagGaussianDistribution, L = A): the head's outputs are the means,
 *  action = mean + exp(log_std) * eps with eps ~ N(0, 1) -- `uniforms` (n,A) then carries the STANDARD-NORMAL draws eps (NULL:
 *  Box-Muller over two Philox uniforms per dimension), deterministic = the mean, log_prob / entropy = Normal's summed over the
 *  dimensions; actions leave through actions_f32 only (UNclipped: the caller clips for the environment, util.py:84-99),
 *  `logits` returns the means, action_mask must be NULL.
 * Outputs (any may be NULL): actions_i32 (n,A), actions_f32 (n,A), values (n), log_probs (n), entropy (n), logits (n,L).
 * When rb != NULL the transition is also written at row `pos` of the rollout buffer (fused RolloutBuffer.add with
 * reward 0 and episode_start = episode_start_in) -- n must equal rb->E; if pending_reward (E) is also given, it is
 * added to row pos-1's rewards in the same launch (the previous step's Agent.update, agents.py:198, folded in).
 * params must be 16-byte aligned. */
int ph_policy_forward(ph_ctx *ctx, const ph_spec *spec, const float *params, const float *obs, int n,
                      const unsigned char *action_mask, const float *uniforms, const float *given_actions,
                      unsigned long long seed, unsigned long long counter, int deterministic, int *actions_i32,
                      float *actions_f32, float *values, float *log_probs, float *entropy, float *logits,
                      const ph_rollout *rb, int pos, const float *episode_start_in, const float *pending_reward,
                      int gemm_mode);

/* The same call for an environment that lives on the HOST (the reference's own situation: one get_action per environment step,
 * the action needed back before the environment can move -- agents.py:111-184, util.py:63-81): observations, episode starts and
 * the three results are HOST arrays; the call stages them through pinned, device-visible memory of the context that the forward
 * kernel reads and writes directly (with the fused rollout-buffer write when rb != NULL, as above) and returns when the kernel
 * has finished.  One call, one launch and one wait per environment step instead of several tensor operations; the sampled
 * actions are bitwise those of ph_policy_forward with the same (seed, counter).  A launch of one 16-row tile (n <= 16, the
 * 16-row forward's shape class) signals its end through two words in the same pinned memory, stored by the policy and the value
 * workgroup after their last output, and the call polls those (bounded: 50 ms, then the stream wait) instead of synchronising
 * the stream.  Either way every write of the launch, the rollout-buffer row included, is complete when the call returns.
 *   obs_host (n, D) f32; episode_start_host (n) f32 or NULL (required with rb); actions_host (n, A) i32; values_host (n);
 *   log_probs_host (n) -- any output may be NULL. */
int ph_policy_act_host(ph_ctx *ctx, const ph_spec *spec, const float *params, const float *obs_host, int n,
                       const float *episode_start_host, unsigned long long seed, unsigned long long counter,
                       int deterministic, int *actions_host, float *values_host, float *log_probs_host,
                       const ph_rollout *rb, int pos, int gemm_mode);

/* One environment step of SEVERAL local agents in one launch (agent-per-GPU self-play hosts two learners per GPU).
 * Each record is one agent's ph_policy_forward call with the fused rollout-buffer write; optionally the PREVIOUS step's
 * late reward (Agent.update, agents.py:198) is applied to row pos-1 in the same launch:
 *   rewards[pos-1][e] += pending_reward[e] + (joint_actions ? bonus * [joint[seat][e] == joint[*partner_seat][e]] : 0)
 * where joint_actions (n_seats, n) int32 is the all-gathered action matrix of that previous step.
 * All records must have the same n and the same padded logit count; n_calls <= 4. */
typedef struct ph_step_call {
  const ph_spec *spec;               /* host */
  const float *params;
  const float *obs;                  /* (n, D) */
  int n;
  const unsigned char *action_mask;  /* (n, L) or NULL */
  unsigned long long seed, counter;
  int deterministic;                 /* bit 0: argmax instead of sampling; PH_STEP_FIX_ILLEGAL / PH_STEP_MASK_ENV_ONLY: see below */
  int *actions_i32;                  /* (n, A) */
  float *values;                     /* (n) */
  float *log_probs;                  /* (n) */
  const ph_rollout *rb;              /* host; required */
  int pos;
  const float *episode_start_in;     /* (n) */
  const float *pending_reward;       /* (n) or NULL */
  const int *joint_actions;          /* (n_seats, n) or NULL */
  int n_seats, seat;
  const int *partner_seat;           /* device int; required when joint_actions != NULL */
  float bonus;
} ph_step_call;
/* Flags in `deterministic` besides bit 0, for a record with an action mask (single Discrete heads of <= 8 logits):
 *  PH_STEP_FIX_ILLEGAL: actions_i32 -- what the environment and the action exchange consume -- is the ENV-SIDE fix-up of an
 *      illegal sample (first legal index: pettingzoo.py:81-82 does this inside the environment, before base_env.step), while
 *      the rollout-buffer row and the log-prob keep the sampled action, as the reference's agent does (it is never told).
 *  PH_STEP_MASK_ENV_ONLY: the mask is NOT applied to the logits.  That is the reference's plain PPO agent: OnPolicyAgent
 *      hands its policy obs.obs only (agents.py:162; action_from_policy util.py:63-81), so only ModularPolicy
 *      (modular/policies.py:330-333) ever offsets logits; everyone else samples unmasked and the environment repairs. */
#define PH_STEP_FIX_ILLEGAL 2
#define PH_STEP_MASK_ENV_ONLY 4
int ph_policy_step_multi(ph_ctx *ctx, int n_calls, const ph_step_call *calls /* host */);

/* ---- agent-per-GPU action exchange over RCCL ------------------------------------------------------
 * What MultiAgentEnv._get_actions does in-process (multiagentenv.py:149-170) across ranks: every rank contributes the actions
 * of its local agents for the current step, every rank receives the joint action.  librccl.so is loaded on first use
 * (dlopen) -- a build or a node without it still loads this library and gets an error from these calls only.
 *  ph_comm_unique_id: ncclGetUniqueId on the calling rank (rank 0); the 128 bytes travel to the other ranks through the
 *      caller's rendezvous (torch.distributed's store).
 *  ph_comm_init:      ncclCommInitRank for this context (one process per GPU).
 *  ph_all_gather_i32: joint[r*count .. (r+1)*count) <- rank r's local[0..count), on the context's stream, no host sync.
 *      Without a communicator (single process) it degenerates to a device copy.
 *  ph_selfplay_rollout: T environment steps back to back -- step t = ph_policy_step_multi(calls + t*n_calls) followed by
 *      the all-gather of the step's actions -- in ONE host call: the per-step host work is two native enqueues. */
#define PH_COMM_ID_BYTES 128
int ph_comm_unique_id(unsigned char *id_out /* host, PH_COMM_ID_BYTES */);
int ph_comm_init(ph_ctx *ctx, const unsigned char *id /* host */, int world, int rank);
int ph_comm_destroy(ph_ctx *ctx);
int ph_all_gather_i32(ph_ctx *ctx, const int *local /* (count) */, int *joint /* (world*count) */, int count);
int ph_selfplay_rollout(ph_ctx *ctx, int n_calls, const ph_step_call *calls /* host, [T][n_calls] */, int T,
                        const int *local, int *joint, int count);

/* ---- the same exchange as direct peer-to-peer stores over xGMI -------------------------------------------------------
 * The per-step message is KB-sized, so the collective's cost is its latency.  Here every rank owns a fine-grained
 * (uncached, cross-device coherent) receive area that all ranks map through HIP IPC; after the step's forward launch a
 * one-workgroup kernel stores the local actions straight into every peer's receive area (slot = step parity), fences at
 * system scope and publishes a monotonic step stamp in the peer's flag array; the consumer is a one-wave kernel that waits
 * for all stamps (bounded: a timeout raises the error word instead of hanging the device).
 *  ph_p2p_alloc / ph_p2p_open / ph_p2p_close / ph_p2p_free: the shareable buffer and its 64-byte IPC handle.
 *  ph_p2p: the exchange as seen from one rank -- peers' receive areas and flag arrays as mapped here (own ones included).
 *  ph_p2p_push(t): joint[t&1][peer][rank*count ..] <- local[0..count) for every peer; flags[peer][rank] <- stamp(t).
 *  ph_p2p_wait(t): until flags_local[src] >= stamp(t) for every src.   stamp(t) = (*epoch) * T + t + 1.
 *  ph_selfplay_rollout_p2p: T x { ph_policy_step_multi, push, wait } in one host call.  When every call fits the 16-row
 *      step kernel the exchange is folded INTO the step launch with the stamp in-band: a policy workgroup stores each row's
 *      action as ONE 8-byte word (stamp << 32 | action) into every rank's `ll` area (slot = t mod ll_slots; 8-byte stores are
 *      single-copy atomic, so no fence, flag or arrival counter is needed), and the value workgroups of the next step poll
 *      exactly the two words they consume (own seat, partner seat) until the stamp matches.  A rank therefore waits for
 *      its partner's rank only and can run up to world-1 steps ahead of some other rank: ll_slots must be >= T so that no
 *      slot is reused inside an iteration (the unpack of step T-1 waits for every rank, which bounds the skew per iteration).  After the last step the
 *      words of step T-1 are unpacked into this rank's plain receive slot for ordinary consumers. */
#define PH_IPC_HANDLE_BYTES 64
typedef struct ph_p2p {
  int world, rank, count, T;
  int *joint[2][PH_MAX_RANKS];                 /* [parity][peer] -> that peer's (world*count) int32 receive slot */
  unsigned long long *flags[PH_MAX_RANKS];     /* [peer] -> that peer's (world) stamp array */
  unsigned long long *ll[PH_MAX_RANKS];        /* [peer] -> that peer's ll_slots x (world*count) stamp-in-band words */
  int ll_slots;                                /* slot of step t = t mod ll_slots; >= T (see above) */
  const unsigned long long *epoch;             /* device word advanced once per iteration (ph_rng_epoch_advance) */
  unsigned long long *error;                   /* local device word: number of timed-out waits */
  unsigned long long timeout_cycles;           /* bound of one wait in wall_clock64() ticks (100 MHz) */
} ph_p2p;
int ph_p2p_alloc(ph_ctx *ctx, size_t bytes, void **ptr_out, unsigned char *handle_out /* host, 64 */);
int ph_p2p_open(ph_ctx *ctx, const unsigned char *handle /* host, 64 */, void **ptr_out);
int ph_p2p_close(ph_ctx *ctx, void *ptr);
int ph_p2p_free(ph_ctx *ctx, void *ptr);
int ph_p2p_push(ph_ctx *ctx, const ph_p2p *x, const int *local, int t);
int ph_p2p_wait(ph_ctx *ctx, const ph_p2p *x, int t);
/* stamp-in-band variant as separate launches (what the fused step launch does per row; used by the route self-test):
 * ll_push stores (stamp(t) << 32 | local[i]) into every rank's word area, ll_unpack waits for step t's words of every rank
 * and writes their low halves to this rank's plain receive slot of parity t & 1 */
int ph_p2p_ll_push(ph_ctx *ctx, const ph_p2p *x, const int *local, int t);
int ph_p2p_ll_unpack(ph_ctx *ctx, const ph_p2p *x, int t);
int ph_selfplay_rollout_p2p(ph_ctx *ctx, int n_calls, const ph_step_call *calls /* host, [T][n_calls] */, int T,
                            const int *local, const ph_p2p *x);

/* The same T steps as ONE launch (the N > 1 counterpart of ph_scripted_rollout): when every local agent's observations,
 * base rewards and done flags of the rollout already sit in HBM (the synthetic rollout driver of SURVEY.md 8d), the only thing
 * that has to cross a step boundary is what multiagentenv.py:149-170 hands between agents -- each seat's action.  Here that
 * hand-off happens INSIDE the launch: the policy workgroup of 16 environments stores each sampled action as one stamped
 * 8-byte word into every rank's `ll` area (as ph_selfplay_rollout_p2p's fused step does), and the value workgroup of step
 * t + 1 polls the two words it consumes (own seat, partner seat) before it credits step t's reward
 *   rewards[t][e] += rew_seq[t][e] + bonus * [joint[seat][e] == joint[*partner_seat][e]]
 * (the last step's reward is credited at the end of the launch).  Bitwise the launch-per-step walk of
 * ph_selfplay_rollout_p2p followed by ph_buffer_add_reward_joint for step T - 1 (tests/test_gpu_parity.py).
 *   Word slots: step t of an iteration whose epoch word reads e uses slot (e & 1) * x->T + t (x->T >= T), so x->ll_slots must be
 *   >= 2 x->T (a
 *   launch's policy workgroups run ahead of its value workgroups; alternating halves keep a faster peer's next iteration
 *   from overwriting words this rank has not consumed).  After the launch the words of step T - 1 are unpacked into the plain
 *   receive slot of parity (T - 1) & 1, which also makes this rank wait for every peer once per iteration.
 *   Every workgroup of the launch must be resident at once (value workgroups poll; policy workgroups never wait):
 *   n_calls * 2 * ceil(n / 16) workgroups, times `ranks_on_device` when several ranks share one GPU, must not exceed
 *   what ph_selfplay_rollout_persistent_capacity reports -- the runtime's occupancy answer for the rollout kernel on this
 *   device (workgroups per CU x CUs, one workgroup per CU held back where the answer is not bounded by LDS: the occupancy API
 *   can be one high there) -- otherwise the call refuses (use ph_selfplay_rollout_p2p).  Shapes of the 16-row forward only. */
typedef struct ph_rollout_call {
  const ph_spec *spec;               /* host */
  const float *params;
  const float *obs_seq;              /* (T, n, D) */
  const float *rew_seq;              /* (T, n) base reward of every step */
  const float *done_seq;             /* (T, n) */
  const unsigned char *mask_seq;     /* (T, n, L) action masks or NULL */
  int n;
  const float *episode_start0;       /* (n) */
  unsigned long long seed, counter0; /* step t samples with counter0 + t */
  int mask_mode;                     /* with mask_seq: 0 = policy-side logit offset only, 1 = offset + env-side fix-up
                                        (PH_STEP_FIX_ILLEGAL), 2 = env-side fix-up only (+ PH_STEP_MASK_ENV_ONLY) */
  int *actions_i32;                  /* (n) the last step's environment-side actions */
  float *values;                     /* (n) */
  float *log_probs;                  /* (n) */
  const ph_rollout *rb;              /* host; rows 0 .. T-1 are written */
  int n_seats, seat;
  const int *partner_seat;           /* device int */
  float bonus;
} ph_rollout_call;
int ph_selfplay_rollout_persistent(ph_ctx *ctx, int n_calls, const ph_rollout_call *calls /* host */, int T,
                                   const ph_p2p *x, int ranks_on_device);
/* workgroups of the exchange rollout kernel the device keeps resident at once (hipOccupancyMaxActiveBlocksPerMultiprocessor,
 * not a formula): the bound ph_selfplay_rollout_persistent checks its grid against.  Callers that must agree across ranks
 * (vec.FusedSelfPlayRollout) read it, decide, and all-reduce the decision. */
int ph_selfplay_rollout_persistent_capacity(ph_ctx *ctx, int *workgroups_out);

/* Ragged rollout buffers for vectorised TURN-BASED games ("per-env pos"): a partner does not act in
 * every env at every step, so each env e has its own write row pos_env[e] (device int32, caller-owned).
 *  ph_policy_forward_ragged: forward for all n = rb->E envs; the transition of env e is recorded at row pos_env[e] iff
 *      record_mask[e] != 0 and pos_env[e] < rb->T; `values` (n) is only updated for recorded envs (it caches V of the
 *      last recorded action, the bootstrap OnPolicyAgent hands to GAE -- agents.py:127-130,183).
 *  ph_buffer_add_reward_ragged: rewards[pos_env[e]-1][e] += reward[e] for env_mask[e] != 0 with pos_env[e] >= 1.
 *  ph_ragged_advance: pos_env[e] += 1 for record_mask[e] != 0 while pos_env[e] < rb->T (call after the forward). */
int ph_policy_forward_ragged(ph_ctx *ctx, const ph_spec *spec, const float *params, const float *obs,
                             const unsigned char *action_mask, unsigned long long seed, unsigned long long counter,
                             int deterministic, int *actions_i32, float *values, float *log_probs,
                             const ph_rollout *rb, const int *pos_env, const unsigned char *record_mask,
                             const float *episode_start_in);
int ph_buffer_add_reward_ragged(ph_ctx *ctx, const ph_rollout *rb, const int *pos_env, const float *reward,
                                const unsigned char *env_mask);
int ph_ragged_advance(ph_ctx *ctx, const ph_rollout *rb, int *pos_env, const unsigned char *record_mask);
/* ph_buffer_compact_columns: dst (T, n, .) <- columns cols[0..n) (device int32, environment indices, any order) of src
 * (T, E, .), all eight arrays.  A partner whose environments reach it at different rates (turn-based games, round-robin
 * partner selection) trains on the columns that are full -- the E-environment reading of "train once n_steps of its own
 * transitions are in the buffer" (agents.py:126) -- instead of waiting for every environment. */
int ph_buffer_compact_columns(ph_ctx *ctx, const ph_spec *spec, const ph_rollout *src, const ph_rollout *dst,
                              const int *cols /* device (n) */, int n);

/* env-side illegal-action fix-up: action not legal -> first legal index <- pettingzoo.py:81-82.  Integer, bit-exact. */
int ph_fix_illegal_actions(ph_ctx *ctx, int *actions /* (n) in/out */, const unsigned char *action_mask /* (n,L) */,
                           int n, int L);

/* ---- vectorised integer game rules ------------------------------------------------------ */
/* RPSEnv.multi_step <- pantheonrl/envs/rpsgym/rps.py:41-45 for n environments: rewards (ego, partner) as f32 */
int ph_rps_step(ph_ctx *ctx, const int *ego_actions, const int *alt_actions, float *ego_reward, float *alt_reward, int n);
/* LiarEnv.player_step <- pantheonrl/envs/liargym/liar.py:58-83 (sanitize_action, eval_bluff, getObs) for every env with
 * active[e] != 0 (NULL = all).  hands (n,12) int32 = ego histogram then partner histogram; history (n,24) int32 moves
 * newest first, nmoves (n) int32 -- both updated in place; actions (n,2) int32 raw (side, count-1) of the mover,
 * is_ego (n) u8 = who moves.  Outputs: obs_next (n,30) f32 observation of the OTHER player, rewards (n,2) f32
 * (ego, partner), done (n) u8.  hands / history must be 16-byte aligned, actions / obs / rewards 8-byte aligned (the
 * kernels move a table's state with 16-byte accesses); the same holds for ph_liar_reset / ph_liar_obs and the arrays
 * of ph_liar_selfplay. */
int ph_liar_step(ph_ctx *ctx, const int *hands, int *history, int *nmoves, const int *actions,
                 const unsigned char *is_ego, const unsigned char *active, float *obs_next, float *rewards,
                 unsigned char *done, int n);

/* LiarEnv.multi_reset <- liar.py:96-102 for every env with reset_mask[e] != 0 (NULL = all): dice from Philox4x32-10
 * keyed (seed, counter [+ the context's RNG epoch word << 32, when one is attached], env, die/4; die%4 selects the word),
 * empty history; ego_first (n) u8 <- first mover ~ Bernoulli(probegostart)
 * (TurnBasedEnv.n_reset, multiagentenv.py:323-326). */
int ph_liar_reset(ph_ctx *ctx, int *hands, int *history, int *nmoves, const unsigned char *reset_mask,
                  unsigned char *ego_first, unsigned long long seed, unsigned long long counter, float probegostart,
                  int n);
/* LiarEnv.getObs(isego) <- liar.py:53-56: observation (n,30) f32 of the player is_ego[e] selects, active envs only */
int ph_liar_obs(ph_ctx *ctx, const int *hands, const int *history, const int *nmoves, const unsigned char *is_ego,
                const unsigned char *active, float *obs_out, int n);

/* One vectorised MultiAgentEnv.step of n Liar's Dice tables with a PPO ego and a PPO partner, entirely on the device
 * (multiagentenv.py:149-215 + TurnBasedEnv.n_step/n_reset :307-327 + LiarEnv, liar.py:53-102), as ONE host call that
 * enqueues ~15 launches and keeps every mask on the device: ego forward (recorded at row ego_pos of its rectangular
 * buffer) -> player_step -> partner credited / flagged (Agent.update) -> partner forward where the game goes on (ragged
 * rows) -> player_step -> both credited, ego observation, episode flags -> finished tables re-dealt -> where the partner
 * opens the new game it moves once -> every table is back at the ego's turn.  With deal_only != 0 only the re-deal half
 * runs, for the tables flagged in `done` (the initial deal).  RNG counters: ego forward `counter`, partner forwards
 * 2*counter and 2*counter+1, dice `counter`.  All pointers are device pointers owned by the caller. */
typedef struct ph_liar_selfplay {
  int n;
  const ph_spec *spec;                       /* LiarsDice spaces (both seats) */
  int *hands, *history, *nmoves;             /* (n,12) (n,24) (n) game state */
  unsigned char *ego_first;                  /* (n) */
  unsigned long long dice_seed;
  float probegostart;
  /* ego: rectangular rollout buffer */
  const float *ego_params;
  const ph_rollout *ego_rb;
  int *ego_actions;                          /* (n,2) */
  float *ego_values, *ego_log_probs;         /* (n) */
  float *ego_episode_start;                  /* (n) in: flags of the previous step; out: this step's done */
  unsigned long long ego_seed;
  /* partner: ragged rollout buffer */
  const float *alt_params;
  const ph_rollout *alt_rb;
  int *alt_actions;                          /* (n,2) */
  float *alt_values, *alt_log_probs;         /* (n) */
  int *alt_pos;                              /* (n) per-table write row */
  unsigned char *alt_boundary, *alt_term, *alt_open, *alt_acted;   /* (n) OnPolicyAgent book-keeping per table */
  unsigned long long alt_seed;
  /* observations of whoever moves next */
  float *obs_ego, *obs_alt;                  /* (n,30) */
  unsigned long long *episodes;              /* finished games */
  /* scratch */
  float *obs_next, *rew1, *rew2, *es_alt;    /* (n,30) (n,2) (n,2) (n) */
  unsigned char *done1, *done2, *running, *can, *alt_opens, *ego_opens, *done;   /* (n) */
  const unsigned char *zeros8, *ones8;       /* (n) constants */
} ph_liar_selfplay;
int ph_liar_selfplay_step(ph_ctx *ctx, const ph_liar_selfplay *s, int ego_pos, unsigned long long counter, int deal_only);
/* n_steps of those vectorised steps -- ego rows ego_pos .. ego_pos + n_steps - 1, step t with counter + t -- in ONE persistent
 * launch: tables are independent, so one workgroup owns up to 16 tables (as few as spreads n over the CUs) for the whole rollout
 * and runs the three forwards and the book-keeping of every step with workgroup barriers in place of kernel boundaries.  The
 * game state, observations, both rollout buffers, the partner's book-keeping, the cached values and the episode count are
 * bitwise the result of n_steps calls of ph_liar_selfplay_step(deal_only = 0).  A partner forward that none of a workgroup's
 * tables asks for (no game running after the ego's move; no fresh game opened by the partner) is not executed: the scratch
 * outputs such a forward would have left for tables that do not move (partner action / log-prob cache entries nothing reads)
 * are then stale.  Needs the 16-row one-hot forward's shape class (<= 64 observation components, <= 32 logits). */
int ph_liar_selfplay_rollout(ph_ctx *ctx, const ph_liar_selfplay *s, int ego_pos, int n_steps, unsigned long long counter);

/* ---- Liar's Dice against a pool of partners (csrc/ph_pool.h): seat 1 of table e is held by member partnerid[e] of K <=
 * PH_MAX_POOL members, resampled at that table's own re-deal (MultiAgentEnv.add_partner_agent / resample_round_robin /
 * resample_random, multiagentenv.py:92-147).  A member is a learner (its own ragged rollout buffer and per-table book-keeping
 * vectors, as the partner block of ph_liar_selfplay), a frozen policy (samples like any forward, records nothing) or the
 * scripted player (LiarDefaultAgent, integer rule).  All members share the Liar's Dice spaces; learners and frozen members play
 * the 64-64 policy.  A clone (PH_POOL_CLONE; an addition, PH_ABI_VERSION unchanged) plays the shared-trunk FeedForward32Policy of
 * behavioural cloning: `params` is a ph_bc_layout vector for the step's spec (ph_bc_layout_of must succeed for it) and `seed` its
 * Philox key; rb, pos, boundary, term, open, values and log_probs are ignored and may be NULL.  Like a frozen member it records
 * nothing.  ph_pool_forward, ph_liar_pool_step and ph_liar_xplay_step accept it.  A learner or a frozen member -- and the pool's
 * ego -- may instead play the towers of a run-time shape (ph_arch): through ph_pool_forward_arch, ph_liar_pool_step_arch and
 * ph_liar_xplay_step_arch, declared with the towers below. */
#define PH_MAX_POOL 8
#define PH_POOL_LEARNER 0
#define PH_POOL_FROZEN 1
#define PH_POOL_SCRIPTED 2
#define PH_POOL_CLONE 3
#define PH_POOL_ROBIN 0    /* partnerid <- (partnerid + 1) % K at every deal of the table */
#define PH_POOL_RANDOM 1   /* partnerid <- (uint64(w) * K) >> 32, w = word 0 of Philox block 101 keyed (pool_seed, deal counter, table) */
typedef struct ph_pool_member {
  int kind;                                  /* PH_POOL_* */
  const float *params;                       /* learner, frozen: ph_layout vector; clone: ph_bc_layout vector */
  const ph_rollout *rb;                      /* learner: (T, n) ragged buffer; NULL otherwise */
  int *pos;                                  /* (n) learner: per-table write row */
  unsigned char *boundary, *term, *open;     /* (n) learner: OnPolicyAgent book-keeping per table */
  float *values, *log_probs;                 /* (n) learner: caches of the last recorded forward; frozen: optional */
  unsigned long long seed;                   /* learner, frozen, clone: Philox key of its forwards */
} ph_pool_member;
/* The grouped forward on its own: ONE launch behind a bucket pass (stable counting sort of the tables with active[e] != 0 by
 * partnerid[e], 16-row tiles per member).  A workgroup runs one tile with its member's weights: rows of a learner are recorded
 * at pos[e] of its buffer where the column has room (episode_start_in[e] goes into the row; values cached for recorded rows
 * only), rows of a frozen member write actions only, rows of the scripted member follow ph_liar_default_actions.  Row e draws
 * with the Philox key (member seed, counter, e) -- what ph_policy_forward_ragged / ph_policy_forward use -- and stores its
 * action into actions (n, 2); rows that are not active are not touched.  A clone's row e draws philox_uniform(member seed,
 * counter, e, component) -- exactly what ph_bc_forward draws for row e -- and its action is bitwise the one ph_bc_forward(params,
 * obs, n, seed, counter) samples for that row; it writes actions only.  Clone tiles run in a launch of their own behind the grouped
 * one, made only when the member table holds a clone (and alone when it holds nothing else).  The spec must run on the 16-row one-hot forward
 * (<= 64 observation components, <= 32 logits). */
int ph_pool_forward(ph_ctx *ctx, const ph_spec *spec, const ph_pool_member *members, int n_members, const float *obs,
                    const int *partnerid, const unsigned char *active, unsigned long long counter, int *actions,
                    const float *episode_start_in, int n);
/* LiarDefaultAgent.get_action for the rows with active[e] != 0 (NULL = all): obs (n, 30) f32, actions (n, 2) int32 */
int ph_liar_default_actions(ph_ctx *ctx, const float *obs, const unsigned char *active, int *actions, int n);
/* ph_liar_selfplay with the partner block replaced by the pool.  RNG counters of step c: ego forward c, member forwards 2c and
 * 2c + 1 (each member under its own seed), dice c, resample c. */
typedef struct ph_liar_pool {
  int n;
  const ph_spec *spec;
  int *hands, *history, *nmoves;
  unsigned char *ego_first;
  unsigned long long dice_seed;
  float probegostart;
  const float *ego_params;
  const ph_rollout *ego_rb;
  int *ego_actions;
  float *ego_values, *ego_log_probs;
  float *ego_episode_start;
  unsigned long long ego_seed;
  const ph_pool_member *members;             /* host array [n_members] */
  int n_members;
  int *partnerid;                            /* (n) member of every table */
  int resample;                              /* PH_POOL_ROBIN / PH_POOL_RANDOM */
  unsigned long long pool_seed;
  int *alt_actions;                          /* (n,2) shared by the members */
  unsigned char *alt_acted;                  /* (n) the table's member has moved in the current game */
  float *obs_ego, *obs_alt;
  unsigned long long *episodes;
  float *obs_next, *rew1, *rew2, *es_alt;
  unsigned char *done1, *done2, *running, *can, *alt_opens, *ego_opens, *done;
} ph_liar_pool;
/* One vectorised step (deal_only: only the re-deal half, for the tables flagged in `done`): ego forward, book-keeping, bucket
 * pass + ONE grouped forward for the replies, book-keeping + re-deal + resample, bucket pass + ONE grouped forward for the
 * openers, book-keeping: 8 launches (10 when the members are clones and others).  No host synchronisation; capturable once it ran outside capture.  The context keeps ONE
 * device-side member table, uploaded (with a stream synchronisation) whenever the members passed in differ from it: a captured step
 * replays against the table uploaded last, so pools that are replayed from graphs should not share a context. */
int ph_liar_pool_step(ph_ctx *ctx, const ph_liar_pool *pool, int ego_pos, unsigned long long counter, int deal_only);

/* ---- cross-play evaluation of Liar's Dice (csrc/ph_xplay.h; additions, PH_ABI_VERSION unchanged): tester.py:41-63 -- play a
 * fixed ego against a fixed partner for a number of games and report the ego's returns -- for n tables at once.  BOTH seats are
 * held by members of one table of 1..PH_MAX_POOL frozen / cloned / scripted members (a learner is refused): table e plays the ordered pair
 * pairs[e % n_pairs] = (seat 0, seat 1) for the whole evaluation, exactly episodes_per_table games, and then goes idle: it is
 * masked out of every forward and pass, and its state and logs do not change again.  A game's return is the sum of the ego rewards
 * MultiAgentEnv.step returns over the game (the ego's own transition plus the reply's, multiagentenv.py:201-202), accumulated in
 * f32; its length is the number of ego moves.  RNG counters of step c >= 1: seat 0's forward 3c, the reply 3c + 1, the opening
 * 3c + 2 (each member under its own seed, row = table; the same member may hold both seats of a table, so the seats' counters are
 * disjoint), dice c; the first deal uses dice counter 0 and opening counter 2. */
typedef struct ph_liar_xplay {
  int n;
  const ph_spec *spec;
  int *hands, *history, *nmoves;
  unsigned char *ego_first;
  unsigned long long dice_seed;
  float probegostart;
  const ph_pool_member *members;             /* host array [n_members]: PH_POOL_FROZEN / PH_POOL_CLONE / PH_POOL_SCRIPTED */
  int n_members;
  const int *pairs;                          /* host array [n_pairs][2]: (member at seat 0, member at seat 1) */
  int n_pairs;                               /* 1..n */
  int episodes_per_table;                    /* G >= 1 */
  const int *ego_id, *alt_id;                /* (n) device: pairs[e % n_pairs][0] / [1]; a table whose index is out of range does not move */
  int *ego_actions, *alt_actions;            /* (n,2) */
  float *obs_ego, *obs_alt;                  /* (n,30) */
  int *games;                                /* (n) games finished */
  unsigned char *playing;                    /* (n) 1 while games[e] < G */
  int *tables_left;                          /* [1] tables with budget left */
  float *ep_return;                          /* (n) return of the game in progress */
  int *ep_length;                            /* (n) ego moves of the game in progress */
  float *returns;                            /* (n,G) log: ego return of game g of table e */
  int *lengths;                              /* (n,G) log: ego moves of game g of table e */
  float *obs_next, *rew1, *rew2;             /* scratch (n,30) (n,2) (n,2) */
  unsigned char *done1, *done2, *running, *alt_opens, *ego_opens, *done;   /* scratch (n) */
} ph_liar_xplay;
/* One MultiAgentEnv.step of every playing table (tester.py:41-63): grouped forward of seat 0 by ego_id, book-keeping, grouped
 * forward of seat 1 by alt_id where the game goes on, book-keeping (end of game: log, games += 1, then the next deal, or
 * tables_left -= 1 when the budget is spent), grouped forward of seat 1 where it opens, book-keeping: 9 launches (12 when the members
 * are clones and others).  deal_only: the
 * first deal of the tables flagged in `done` (the caller has set games = 0, playing = 1, tables_left = n and cleared ep_return /
 * ep_length), the openings and seat 0's first observation.  No host synchronisation; capturable once it ran outside capture (the
 * context's one member table, see ph_liar_pool_step). */
int ph_liar_xplay_step(ph_ctx *ctx, const ph_liar_xplay *xp, unsigned long long counter, int deal_only);
/* The statistics tester.py:41-63 prints, per pair: stats (n_pairs,4) f64 = count, sum, sum of squares, sum of lengths over the
 * logged games (games[e] of them) of the tables p, p + n_pairs, ... in ascending table and game order, one lane per pair, no atomics:
 * two runs give the same bits.  Mean and population standard deviation follow on the host.  stats is 16-byte aligned. */
int ph_xplay_stats(ph_ctx *ctx, const float *returns, const int *lengths, const int *games, int n, int episodes_per_table,
                   int n_pairs, double *stats);

/* ---- episode returns and lengths of device-resident training, per pool member (csrc/ph_episode.h; additions, PH_ABI_VERSION
 * unchanged).  Stands for what the reference reads out of SB3's Monitor records: OnPolicyAgent logs rollout/ep_rew_mean and
 * rollout/ep_len_mean from model.ep_info_buffer (pantheonrl/common/agents.py:132-158; SB3 Monitor / ep_info_buffer) -- here over
 * ALL episodes that ended, not a deque of the last 100.  Nothing is added to a step: the statistics are ONE launch behind the
 * rollout, over what it left in the ego's rectangular buffer.  An episode of table e ends at row t iff episode_starts[t + 1][e] is
 * set (t + 1 < T) or last_dones[e] is (t = T - 1); row 0's own start flag is never read.  Its return is the f32 sum of
 * rewards[.][e] over its rows, added in ascending row order with the carry first (bitwise a sequential NumPy f32 loop); its
 * length is its number of rows (one row = one ego move, ph_liar_xplay's meaning).  Games span rollouts: (carry_return,
 * carry_length) hold the game in progress between calls, and carry_valid[e] == 0 drops the game in progress when it ends (it began
 * before the statistics were attached) and is set from then on.  With n_members > 1 the member at seat 1 is replayed: an episode
 * that ends at row t is credited to member[e], then member[e] <- the pool's resample rule (PH_POOL_ROBIN / PH_POOL_RANDOM) under
 * (pool_seed, deal counter counter0 + t, table e) -- the context's RNG epoch word, when one is attached, is the counter's high half
 * exactly as in ph_liar_pool_step -- so after a scan member[] equals the pool's partnerid[].  stats (n_members, PH_EPISODE_NSTAT)
 * f64 = count, sum of returns, sum of squared returns, sum of lengths per member, ACCUMULATED INTO (zeroed: one rollout's figures;
 * kept: running totals), summed in a fixed order without floating-point atomics: two runs on the same inputs give the same bits.
 * No host synchronisation and no allocation once its workspace exists: capturable after one call outside capture. */
#define PH_EPISODE_NSTAT 4
typedef struct ph_episode_scan {
  const ph_rollout *rb;                      /* host; rewards and episode_starts rows 0 .. T-1 are read, nothing is written */
  int T;                                     /* rows filled, 1 .. rb->T */
  const float *last_dones;                   /* (E) the end flags of row T-1 */
  float *carry_return;                       /* (E) in/out */
  int *carry_length;                         /* (E) in/out */
  unsigned char *carry_valid;                /* (E) in/out: 0 = drop the game in progress */
  int n_members;                             /* 1 .. PH_MAX_POOL; 1 = no attribution (member may be NULL) */
  int *member;                               /* (E) in/out: the member at seat 1 of the game in progress */
  int resample;                              /* PH_POOL_ROBIN / PH_POOL_RANDOM */
  unsigned long long pool_seed, counter0;    /* row t was step counter0 + t */
  double *stats;                             /* (n_members, PH_EPISODE_NSTAT) device, 8-byte aligned, accumulated into */
} ph_episode_scan;
int ph_episode_stats(ph_ctx *ctx, const ph_episode_scan *scan);

/* ---- a move log of the vectorised Liar's Dice step on the device (csrc/ph_record.h; additions, PH_ABI_VERSION unchanged): the rows
 * TurnBasedRecorder (wrappers.py:82-160) produces for each table, [obs 30 | action 2 | flag] f32 with flag 0 ego moved, 1 partner
 * moved, + 2 where that move ended the game.  A step logs up to three moves per table, in the table's own order: the ego's move,
 * the reply where the game goes on, seat 1's opening of a freshly dealt game (flag 1: an opening never ends a game).  Table e owns
 * rows[e] and its cursors; a move that finds count[e] == cap is dropped and counted in dropped[e], so the table's log stays a
 * prefix of its stream and nothing is written past rows[e].  member[e][r] (optional) names who moved: in cross-play ego_id /
 * alt_id, in the pool partnerid[e] for seat 1 (the opening's is read behind the deal's resample), otherwise 0.  The caller zeroes
 * count / count_alt / dropped and fills pending with -1 before attaching. */
typedef struct ph_liar_record {
  int n;                                     /* tables: the n of the steps that record */
  int cap;                                   /* rows per table, >= 1 */
  float *rows;                               /* (n,cap,33) device, 16-byte aligned */
  int *member;                               /* (n,cap) device, or NULL */
  int *count;                                /* (n) rows logged */
  int *count_alt;                            /* (n) ... of which seat 1's */
  int *dropped;                              /* (n) moves that found the table full */
  int *pending;                              /* (n) row of the reply whose flag is still to come within a step, else -1 */
} ph_liar_record;
/* Attach a recorder to the context (the struct is copied; rec == NULL detaches), in the manner of ph_ctx_set_rng_epoch.  While one
 * is attached, every ph_liar_selfplay_step / _step_arch / ph_liar_pool_step / ph_liar_xplay_step of this context with n == rec->n
 * launches two record kernels besides its own launches (a deal-only call: one); a step with another n is refused.  Cross-play
 * tables that are not `playing` log nothing.  Refused inside graph capture; a step with a recorder attached is capturable like
 * the plain one.  ph_liar_selfplay_rollout is refused while a recorder is attached. */
int ph_liar_record_attach(ph_ctx *ctx, const ph_liar_record *rec);
/* offsets (n+1) int64 device = exclusive scan of the per-table counts of the rows `seat` selects: -1 every row, 0 seat 0's
 * (flag % 2 == 0), 1 seat 1's (count_alt).  With rows_out != NULL also the selected rows, table-major and in each table's own
 * order, into rows_out (out_cap,33) f32 and -- where member_out != NULL -- who moved into member_out (out_cap) int32; rows at or
 * past out_cap are not written.  Call it once with rows_out == NULL, read offsets[n], allocate, call it again.  `rec` need not be
 * attached. */
int ph_liar_record_export(ph_ctx *ctx, const ph_liar_record *rec, int seat, long long *offsets, float *rows_out, int *member_out,
                          long long out_cap);

/* ---- the block worlds: BlockEnv-v0 (variant 0, simpleblockworld.py:36-131) and BlockEnv-v1 (variant 1, blockworld.py:34-83,
 * gridutils.py:8-64).  The planner (ego) always moves first; the constructor is the partner.  A table is PH_BLOCK_STATE_WORDS
 * int32 words, 16-byte aligned (layout: csrc/ph_block.h).  Observations are the raw integer components as f32:
 *   planner  (n,98) target grid then built grid      | (n,40) true blocks then the constructor's view (orientation, y, x, colour)
 *   constructor (n,50) last token then built grid    | (n,21) last token then its view of the blocks
 * Actions int32: planner (n) one token; constructor (n,3) = (x, orientation, colour - 1) | (n,2) = (block, colour). */
#define PH_BLOCK_STATE_WORDS 12
/* multi_reset of every table with reset_mask[e] != 0 (NULL = all): a world from Philox4x32-10 keyed (seed, counter [+ the context's
 * RNG epoch word << 32, when one is attached], table, draw); one Philox block per draw in the reference's draw order, draws that
 * do not fit discarded, at most 64 draws, then a deterministic placement (never seen in practice; the loop is bounded) */
int ph_block_reset(ph_ctx *ctx, int variant, int *state, const unsigned char *reset_mask, unsigned long long seed,
                   unsigned long long counter, int n);
/* ego_step (is_ego != 0: actions (n) tokens) or alt_step (actions (n,3) | (n,2)) of every table with active[e] != 0 (NULL = all):
 * obs_next = the OTHER seat's observation, rewards (n,2) (ego, partner), done (n) u8.  Only the last token ends a game; the reward
 * is then 2 tp / (built cells + target cells) as one f32 division | 100 * correctly coloured blocks / 5. */
int ph_block_step(ph_ctx *ctx, int variant, int *state, const int *actions, int is_ego, const unsigned char *active,
                  float *obs_next, float *rewards, unsigned char *done, int n);
/* get_obs(is_ego) of the active tables */
int ph_block_obs(ph_ctx *ctx, int variant, const int *state, int is_ego, const unsigned char *active, float *obs_out, int n);

/* One vectorised MultiAgentEnv.step of n block-world tables with a PPO planner and a PPO constructor, entirely on the device, as ONE
 * host call of four launches and no host synchronisation: the ego's forward (recorded at row ego_pos) -> token played, partner
 * credited where it moved in this game, ego reward / episode flag / episode count, finished tables regenerated (world counter =
 * `counter`), both observation rows, the partner's record mask -> the partner's ragged forward -> its move where the game goes on,
 * the ego's next observation.  The seats have different spaces: two specs.  RNG counters: both forwards and the worlds `counter`. */
typedef struct ph_block_selfplay {
  int n, variant;
  const ph_spec *ego_spec, *alt_spec;        /* planner / constructor spaces */
  int *state;                                /* (n, PH_BLOCK_STATE_WORDS) */
  unsigned long long world_seed;
  /* ego: rectangular rollout buffer */
  const float *ego_params;
  const ph_rollout *ego_rb;
  int *ego_actions;                          /* (n) */
  float *ego_values, *ego_log_probs;         /* (n) */
  float *ego_episode_start;                  /* (n) in: flags of the previous step; out: this step's done */
  unsigned long long ego_seed;
  /* partner: ragged rollout buffer */
  const float *alt_params;
  const ph_rollout *alt_rb;
  int *alt_actions;                          /* (n,3) | (n,2) */
  float *alt_values, *alt_log_probs;         /* (n) */
  int *alt_pos;                              /* (n) per-table write row */
  unsigned char *alt_boundary, *alt_term, *alt_open, *alt_acted;   /* (n) OnPolicyAgent book-keeping per table */
  unsigned long long alt_seed;
  float *obs_ego, *obs_alt;                  /* planner / constructor observation of every table */
  unsigned long long *episodes;              /* finished games */
  /* scratch */
  float *es_alt;                             /* (n) */
  unsigned char *running, *can, *done;       /* (n); done = tables whose game ended in this step */
} ph_block_selfplay;
int ph_block_selfplay_step(ph_ctx *ctx, const ph_block_selfplay *s, int ego_pos, unsigned long long counter);
/* Host only (no context, no device): the same rule text on the CPU.  With do_reset != 0 every table e of `state` (host, (n,12)) is
 * first generated from (seed, counter, e) -- the full counter, there is no epoch word -- with at most max_draws draws (< 0: the
 * device's 64; 0 reaches the deterministic placement at once).  Then `rounds` rounds are played, every one whether or not a game
 * ended: ego_step(tokens[r][e]) -> alt_obs_out[r][e], rewards_out[r][e][2], done_out[r][e]; alt_step(alt_actions[r][e]) ->
 * ego_obs_out[r][e].  Output pointers may be NULL. */
int ph_block_replay_host(int variant, int n, int rounds, int *state, const int *tokens, const int *alt_actions, float *alt_obs_out,
                         float *rewards_out, unsigned char *done_out, float *ego_obs_out, int do_reset, unsigned long long seed,
                         unsigned long long counter, int max_draws);

/* ---- cross-play evaluation of the block worlds (csrc/ph_block.h, ph_block.hip; additions, PH_ABI_VERSION unchanged): every
 * planner of a population with every constructor, frozen or scripted, n tables at once.
 *
 * The scripted constructors (envs/blockworld.py) as one integer rule of a constructor observation row: variant 1 with
 * PH_BLOCK_RULE_DEFAULT is DefaultConstructorAgent; variant 0 with PH_BLOCK_RULE_DEFAULT is SBWDefaultAgent and with
 * PH_BLOCK_RULE_EASY SBWEasyPartner (EASY exists for variant 0 only).  The reference's quirks are kept: a red-range token whose
 * row is done looks at row token - 8, counted from the bottom; the pass move is (0, colour of block 0); SBWEasyPartner halves tokens
 * above 10.  One stated deviation: where SBWEasyPartner answers the negative block index token - 8 (tokens 6, 7, 12-15), which the
 * host game reads from the end of its list, the rule gives the index modulo 5 (-2 -> 3, -1 -> 4): the move the host game makes,
 * inside the action space.  obs (n,50) | (n,21) f32, actions (n,3) | (n,2) int32; rows with active[e] == 0 (NULL = all) are not
 * touched.  The _host form runs the same text on the CPU: no context, host pointers. */
#define PH_BLOCK_RULE_DEFAULT 0
#define PH_BLOCK_RULE_EASY 1
int ph_block_scripted_actions(ph_ctx *ctx, int variant, int rule, const float *obs, const unsigned char *active, int *actions, int n);
int ph_block_scripted_actions_host(int variant, int rule, const float *obs, int *actions, int n);
/* The grouped forward for any categorical spec whose padded logit count is 32 (n < 16384; not the 16-row dense class of one
 * Discrete head of <= 8 logits over one feature chunk): ONE bucket pass (ph_pool_forward's: a stable counting sort of the rows with
 * active[e] != 0 by member_of[e], 16-row tiles per member) and ONE launch in which a workgroup runs one tile's policy net with its
 * member's parameters and seed, read from a member table in device memory.  Members are PH_POOL_FROZEN (params: a ph_layout vector of
 * `spec`, 16-byte aligned; seed: its Philox key; the other fields are ignored) or PH_POOL_SCRIPTED (a block-world constructor spec
 * only; `seed` holds the PH_BLOCK_RULE_*).  A PH_POOL_LEARNER or PH_POOL_CLONE member, a spec with Box actions and a rule the
 * variant does not have are refused before anything is launched.  Row e of a frozen member draws with (member seed, counter, e) and
 * its action is bitwise what ph_policy_forward(spec, member params, obs, n, seed, counter) with gemm_mode 0 samples for row e in the
 * same process: a tile runs the body ph_policy_forward picks for the spec -- the 16-row one-hot body or the general 32-row body, half
 * empty.  Scripted members' rows follow ph_block_scripted_actions, in a launch of their own, made only when the table holds a
 * scripted member.  Only actions[e] of active rows is written.  The context keeps two member tables besides the Liar's Dice one:
 * one for specs that are a block-world constructor's, one for every other spec (the planners'); each is uploaded, with a stream
 * synchronisation, when the members passed in differ from it. */
int ph_block_group_forward(ph_ctx *ctx, const ph_spec *spec, const ph_pool_member *members, int n_members, const float *obs,
                           const int *member_of, const unsigned char *active, unsigned long long counter, int *actions, int n);
/* n tables, 1..PH_MAX_POOL planners and 1..PH_MAX_POOL constructors: table e plays pairs[e % n_pairs] = (planner, constructor) for
 * exactly episodes_per_table games and then goes idle -- masked out of every launch, its state and logs frozen.  A game's return is
 * the f32 sum of the ego rewards, its length the number of planner tokens.  Only the planner's last token ends a game, so nothing
 * bounds one: the caller runs steps in chunks, reads tables_left between them and stops at a cap of its own; ph_xplay_stats covers
 * the logged games (games[e] of table e). */
typedef struct ph_block_xplay {
  int n, variant;
  const ph_spec *ego_spec, *alt_spec;        /* planner / constructor spaces of the variant */
  int *state;                                /* (n, PH_BLOCK_STATE_WORDS) */
  unsigned long long world_seed;
  const ph_pool_member *planners;            /* host array [n_planners]: PH_POOL_FROZEN */
  int n_planners;
  const ph_pool_member *constructors;        /* host array [n_constructors]: PH_POOL_FROZEN / PH_POOL_SCRIPTED (seed = rule) */
  int n_constructors;
  const int *pairs;                          /* host array [n_pairs][2]: (planner, constructor) */
  int n_pairs;                               /* 1..n */
  int episodes_per_table;                    /* G >= 1 */
  const int *ego_id, *alt_id;                /* (n) device: pairs[e % n_pairs][0] / [1] */
  int *ego_actions;                          /* (n) */
  int *alt_actions;                          /* (n,3) | (n,2) */
  float *obs_ego, *obs_alt;                  /* planner / constructor observation of every table */
  int *games;                                /* (n) games finished */
  unsigned char *playing;                    /* (n) 1 while games[e] < G */
  int *tables_left;                          /* [1] tables with budget left */
  float *ep_return;                          /* (n) return of the game in progress */
  int *ep_length;                            /* (n) planner tokens of the game in progress */
  float *returns;                            /* (n,G) log */
  int *lengths;                              /* (n,G) log */
  unsigned char *running;                    /* scratch (n): tables whose game goes on behind the planner's token */
} ph_block_xplay;
/* One step: grouped planner forward over the playing tables -> after_ego (the token played; on the end token the game logged at
 * [e, games[e]], games += 1, then the next world and its planner observation, or tables_left -= 1 when the budget is spent;
 * otherwise the constructor's observation) -> grouped constructor forward over the running tables -> after_alt (the move played,
 * the planner's observation).  Six launches, seven when a constructor is scripted, whatever the number of members; no host
 * synchronisation.  RNG counters of step c >= 1: planner forward 2c, constructor forward 2c + 1, worlds c.  first != 0: nothing is
 * played -- every table gets its first world (world counter 0) and its planner observation; the caller has set games = 0,
 * playing = 1, tables_left = n and cleared ep_return / ep_length. */
int ph_block_xplay_step(ph_ctx *ctx, const ph_block_xplay *xp, unsigned long long counter, int first);

/* ---- the block worlds against a pool of constructors (additions, PH_ABI_VERSION unchanged): ph_block_selfplay with the partner
 * block replaced by the pool, as ph_liar_pool is ph_liar_selfplay's.  Seat 1 of table e is held by member partnerid[e] of 1..PH_MAX_POOL
 * members -- PH_POOL_LEARNER (its own (T, n) ragged buffer and per-table book, as the partner block of ph_block_selfplay), PH_POOL_FROZEN
 * or PH_POOL_SCRIPTED (`seed` holds the PH_BLOCK_RULE_*) -- resampled where the table's game ends.
 *
 * The grouped constructor forward on its own: ph_block_group_forward's bucket pass and launches for a table that may hold learners.
 * A learner (rb with E = n, pos, boundary, term, open, values, log_probs) records row e at pos[e] where active[e] != 0 and the column
 * has room: episode_start_in[e] goes into the row, the value is cached for recorded rows only, pos is not advanced.  Row e of a learner
 * is bitwise what ph_policy_forward_ragged(spec, member params, obs, seed, counter, ..., rb, pos, active, episode_start_in) leaves for
 * that row -- action, cached value and log-prob, every recorded plane; a frozen member's row is ph_policy_forward's, a scripted
 * member's ph_block_scripted_actions'.  When the table holds a learner ONE launch of grid (tiles, 2) runs the learners' and the frozen
 * members' tiles; otherwise the launches are ph_block_group_forward's.  Learner tiles exist on the 16-row one-hot body only: a table
 * with a learner whose spec is not in that class is refused before anything is launched, as are a PH_POOL_CLONE member and a learner
 * without episode_start_in. */
int ph_block_pool_forward(ph_ctx *ctx, const ph_spec *spec, const ph_pool_member *members, int n_members, const float *obs,
                          const int *member_of, const unsigned char *active, unsigned long long counter, int *actions,
                          const float *episode_start_in, int n);
typedef struct ph_block_pool {
  int n, variant;
  const ph_spec *ego_spec, *alt_spec;        /* planner / constructor spaces of the variant */
  int *state;                                /* (n, PH_BLOCK_STATE_WORDS) */
  unsigned long long world_seed;
  /* ego: rectangular rollout buffer */
  const float *ego_params;
  const ph_rollout *ego_rb;
  int *ego_actions;                          /* (n) */
  float *ego_values, *ego_log_probs;         /* (n) */
  float *ego_episode_start;                  /* (n) in: flags of the previous step; out: this step's done */
  unsigned long long ego_seed;
  /* the pool at the constructor's seat */
  const ph_pool_member *members;             /* host array [n_members] */
  int n_members;
  int *partnerid;                            /* (n) member of every table */
  int resample;                              /* PH_POOL_ROBIN / PH_POOL_RANDOM */
  unsigned long long pool_seed;
  int *alt_actions;                          /* (n,3) | (n,2) shared by the members */
  unsigned char *alt_acted;                  /* (n) the table's member has moved in the current game */
  float *obs_ego, *obs_alt;                  /* planner / constructor observation of every table */
  unsigned long long *episodes;              /* finished games */
  /* scratch */
  float *es_alt;                             /* (n) */
  unsigned char *running, *can, *done;       /* (n); done = tables whose game ended in this step */
} ph_block_pool;
/* One vectorised step: the ego's forward, recorded at ego_pos -> after_ego (token played, the member that has acted in this game
 * credited, ego reward / episode flag / episode count; a finished table: its next world, alt_acted cleared, partnerid resampled, the
 * planner's observation; a running one: the constructor's observation and what its member's forward records) -> a bucket pass by
 * partnerid over `running` -> the grouped forward -> the scripted members' rows, only when the table holds one -> after_alt (commit,
 * the move, the planner's observation).  Five launches, six with a scripted member, whatever the number of members; no host
 * synchronisation; capturable once it ran outside capture (the member table is uploaded only when it changed, never inside capture).
 * RNG counters of step c: the ego's forward c, a member's forward c under its own seed, worlds c, the resample c (with the context's
 * epoch word, as the worlds): ph_block_selfplay_step's, so a pool of one learner is that step bit for bit.  first != 0: nothing is
 * played -- every table gets world counter 0, a resample under counter 0 (PH_POOL_ROBIN from 0: 1 % n_members) and its planner
 * observation; the caller has zeroed partnerid. */
int ph_block_pool_step(ph_ctx *ctx, const ph_block_pool *pool, int ego_pos, unsigned long long counter, int first);

/* n_steps vectorised agent steps against a SCRIPTED environment -- observations, rewards and dones of every step already
 * resident on the device (the synthetic rollout driver of SURVEY.md 8d; a recorded trajectory being replayed) -- in ONE launch:
 * a workgroup stages the network once and walks the steps of its 16 environments.  Exactly, bit for bit,
 *     for t in 0 .. n_steps-1:  ph_policy_forward(obs_seq[t], counter0 + t, rb, pos0 + t,
 *                                                 episode_start_in = t ? done_seq[t-1] : episode_start0,
 *                                                 pending_reward   = t ? rew_seq[t-1]  : NULL)
 *     ph_buffer_add_reward(rb, pos0 + n_steps - 1, rew_seq[n_steps-1], NULL)
 * i.e. OnPolicyAgent.get_action / update per step (agents.py:111-203) with the launch boundaries removed; actions / values /
 * log_probs (n, .) end up holding the last step's outputs, as after the per-step calls.  obs_seq (n_steps, n, D), rew_seq and
 * done_seq (n_steps, n) f32.  Shapes of the 16-row forward only (one feature chunk, one Discrete head of <= 8 logits,
 * n < 16384); anything else is an error, not a slower path. */
int ph_scripted_rollout(ph_ctx *ctx, const ph_spec *spec, const float *params, const float *obs_seq, const float *rew_seq,
                        const float *done_seq, int n, int n_steps, const float *episode_start0, unsigned long long seed,
                        unsigned long long counter0, int *actions_i32, float *values, float *log_probs, const ph_rollout *rb,
                        int pos0, int gemm_mode);

/* Frame stack as a device ring buffer <- HistoryQueue.add / reset, wrappers.py:37-71, applied to
 * n environments: stack (n, numframes*D) f32 holds the last numframes observations NEWEST FIRST; for envs with
 * reset_mask[e] != 0 the history is first refilled with default_obs (D, NULL = zeros), then obs (n, D) is pushed. */
int ph_framestack_push(ph_ctx *ctx, float *stack, const float *obs, const unsigned char *reset_mask,
                       const float *default_obs, int n, int D, int numframes);

/* ---- K3+K5+K6: PPO.train() ------------------------------------------------------------------------------------ */
/* PPO.train() <- agents.py:155 (SB3 semantics SURVEY.md A.3; in-tree witness adap_learn.py:229-371).
 * For each epoch, for each consecutive slice of `batch_size` indices (last may be short): gather by index,
 * advantage normalisation, clipped surrogate + value + entropy loss, backward, global-norm clip, Adam.
 *   perms      (n_epochs, T*E) int32 env-major indices (teacher-forced np.random.permutation) or NULL = a keyed
 *              Feistel permutation of [0,T*E) per epoch generated in-kernel from perm_seed.
 *   stats      (n_epochs * ceil(T*E/batch_size), PH_NSTAT) f32 or NULL: per minibatch
 *              {policy_loss, value_loss, entropy_loss, clip_fraction, approx_kl, loss, grad_norm, applied}.
 *   gemm_mode  how the 64x64x64 products are computed:
 *              0 = v_mfma_f32_32x32x2_f32, exact float32 (bit-for-bit the k-ordered fmaf chain);
 *              1 = VALU fmaf chain with the same tile order (debug cross-check of 0, bitwise equal to it);
 *              2 = float32 operands carried as three bf16 planes (x = h + m + l, 24 significand bits), each product six
 *                  v_mfma_f32_16x16x32_bf16 terms accumulated in float32 (ppo_grad_split_kernel): float32 accuracy -- against a
 *                  float64 gradient its error is not larger than mode 0's (tests/test_gpu_parity.py) -- at 6/16 of the matrix
 *                  cycles, beside the vector ALU instead of on it.  Applies to the gradient launches of specs that kernel
 *                  takes (Box observations, <= 64 features, one Discrete head of <= 8 logits); everywhere else 2 means 0.
 * target_kl early stop is evaluated on the device; later minibatches become no-ops (applied = 0). */
int ph_ppo_train(ph_ctx *ctx, const ph_spec *spec, const ph_opt_state *opt, const ph_rollout *rb,
                 const ph_ppo_hyper *hyper /* host */, int n_epochs, int batch_size, const int *perms,
                 unsigned long long perm_seed, float *stats, int gemm_mode);
/* The same call for several independent learners at once (trainer.py: `PPO PPO` self-play keeps two PPO objects, each
 * with its own buffer, policy and optimizer <- trainer.py:126,203; README.md:6).  Every learner's launches go to its own
 * context's stream exactly as ph_ppo_train would issue them -- results are bit-identical -- but the gradient launches of
 * the learners are chained round-robin with events, so that one learner's small reduce / Adam launches overlap the next
 * learner's device-filling gradient launch instead of all learners alternating between "everyone computes gradients" and
 * "everyone reduces".  Streams may be captured into one hipGraph (fork / join is the caller's). */
#define PH_MAX_TRAIN_CALLS 8
typedef struct ph_train_call {
  ph_ctx *ctx;
  const ph_spec *spec;
  const ph_opt_state *opt;
  const ph_rollout *rb;
  const ph_ppo_hyper *hyper;
  int n_epochs, batch_size;
  const int *perms;
  unsigned long long perm_seed;
  float *stats;
  int gemm_mode;
} ph_train_call;
int ph_ppo_train_multi(const ph_train_call *calls, int n_calls);

/* gradient of ONE minibatch (indices given, (nb) int32 env-major) without touching the optimizer state:
 * grad_out (P) = d loss / d params before clipping; stats_out (PH_NSTAT) as above.  For parity tests. */
int ph_ppo_minibatch_grad(ph_ctx *ctx, const ph_spec *spec, const float *params, const ph_rollout *rb,
                          const ph_ppo_hyper *hyper /* host */, const int *indices, int nb, float *grad_out,
                          float *stats_out, int gemm_mode);

/* ---- ADAP: PPO.train() with the context term ("ADAP loss terms as fused-update variants") ------------
 * ADAP.train() <- pantheonrl/algos/adap/adap_learn.py:229-371 is PPO.train() whose minibatch loss gains
 *     context_loss_coeff * get_context_kl_loss(...)                         adap_learn.py:313-320, adap/util.py:97-131
 * The rollout rows carry the context in their LAST context_size components (adap_learn.py:448-452, agent.py:117-121) and
 * AdapPolicy is the MlpPolicy over features ++ context (adap/policies.py:104-119, 136-146), so `spec->obs` is the Box of
 * length (environment observation + context_size).  Per minibatch: min(num_state_samples, nb) states of the minibatch
 * (th.randperm(B)[:num_state_samples]) are re-evaluated under num_context_samples sampled contexts; the term is the mean
 * over context pairs (a before b, itertools.combinations) of mean_s exp(-KL(pi(.|s,a) || pi(.|s,b))).
 *   state_idx   device (n_minibatches, num_state_samples) int32 positions WITHIN each minibatch (teacher-forced
 *               randperm; only the first min(num_state_samples, nb) of a row are read) or NULL = the head of a keyed
 *               Feistel permutation of [0, nb) drawn in the kernel from (seed, rng epoch, minibatch number)
 *   contexts    device (n_minibatches, num_context_samples, context_size) f32 (teacher-forced sampler) or NULL = drawn in
 *               the kernel from a Philox stream keyed the same way, through `sampler` (adap/util.py:42-77)
 *   context_loss, used_state_idx, used_contexts   device outputs with the shapes above ((n_minibatches) for the loss) or
 *               NULL: the raw term and the samples each minibatch actually used
 * n_minibatches = n_epochs * ceil(T*E / batch_size) for ph_adap_train, 1 for ph_adap_minibatch_grad.
 * stats[.][5] (loss) includes the term; the gradient norm, the clip and the Adam step see the gradient of the whole loss.
 * Box observations and categorical action families only; 2 <= num_context_samples <= 16. */
#define PH_CTX_L2 0              /* "l2": uniform in [-1,1)^n scaled to unit length      util.py:42-51 */
#define PH_CTX_UNIT_SQUARE 1     /* "unit_square": uniform in [-1,1)^n                   util.py:54-59 */
#define PH_CTX_POSITIVE_SQUARE 2 /* "positive_square": uniform in [0,1)^n                util.py:62-67 */
#define PH_CTX_CATEGORICAL 3     /* "categorical": one-hot                               util.py:70-77 */
#define PH_CTX_NATURAL_NUMBERS 4 /* "natural_numbers": ONE integer in [0, ctx_size); ctx_size must be 1   util.py:80-89 */
typedef struct ph_adap_loss {     /* defaults: ADAP.__init__ adap_learn.py:111-116 */
  int context_size;               /* 3    */
  int num_context_samples;        /* 5    */
  int num_state_samples;          /* 32   */
  int sampler;                    /* PH_CTX_L2 */
  float context_loss_coeff;       /* 0.1  */
  const int *state_idx;
  const float *contexts;
  unsigned long long seed;
  float *context_loss;
  int *used_state_idx;
  float *used_contexts;
} ph_adap_loss;
int ph_adap_train(ph_ctx *ctx, const ph_spec *spec, const ph_opt_state *opt, const ph_rollout *rb,
                  const ph_ppo_hyper *hyper /* host */, int n_epochs, int batch_size, const int *perms,
                  unsigned long long perm_seed, float *stats, int gemm_mode, const ph_adap_loss *adap /* host */);
/* ph_ppo_minibatch_grad with the context term: grad_out = d (ppo loss + coeff * context loss) / d params */
int ph_adap_minibatch_grad(ph_ctx *ctx, const ph_spec *spec, const float *params, const ph_rollout *rb,
                           const ph_ppo_hyper *hyper /* host */, const int *indices, int nb, float *grad_out,
                           float *stats_out, int gemm_mode, const ph_adap_loss *adap /* host */);

/* ---- AdapPolicyMult (pantheonrl/algos/adap/policies.py:136-283): AdapPolicy with MultModel as its extractor -----------------
 * Rows are features ++ context like AdapPolicy's (adap_learn.py:448-452); per net (policies.py:239-264)
 *   x = tanh(W1 o + b1)  (o = the row without its context),  x_a = tanh(Ws x + bs) viewed as (64, C),
 *   latent = tanh(W2 (x + x_a @ ctx) + b2),  then action_net / value_net.
 * spec: obs = Box(features + context_size) with features <= 64, context_size <= 4; act = Discrete(<= 8).
 * Parameter vector (input-major, like ph_layout): pi {W1 [Fo][64], b1, Ws [64][64 C] (column j C + c), bs, W2 [64][64], b2},
 * vf {the same}, act_W [64][L], act_b, val_W [64], val_b.  The entry points mirror ph_policy_forward / ph_ppo_minibatch_grad /
 * ph_adap_train (same argument meaning; `adap` may be NULL in the gradient call = PPO loss only); the network runs as a chain of
 * small launches over dense intermediates (csrc/ph_adapmult.hip), exact float32. */
typedef struct ph_adapmult_layout {
  int Fo, C, L, P;
  int pi_W1, pi_b1, pi_Ws, pi_bs, pi_W2, pi_b2;
  int vf_W1, vf_b1, vf_Ws, vf_bs, vf_W2, vf_b2;
  int act_W, act_b, val_W, val_b;
} ph_adapmult_layout;
int ph_adapmult_layout_of(const ph_spec *spec, int context_size, ph_adapmult_layout *out /* host */);
int ph_adapmult_forward(ph_ctx *ctx, const ph_spec *spec, int context_size, const float *params, const float *obs, int n,
                        const unsigned char *action_mask, const float *uniforms, const float *given_actions,
                        unsigned long long seed, unsigned long long counter, int deterministic, int *actions_i32,
                        float *actions_f32, float *values, float *log_probs, float *entropy, float *logits,
                        const ph_rollout *rb, int pos, const float *episode_start_in);
int ph_adapmult_minibatch_grad(ph_ctx *ctx, const ph_spec *spec, int context_size, const float *params, const ph_rollout *rb,
                               const ph_ppo_hyper *hyper /* host */, const int *indices, int nb, float *grad_out,
                               float *stats_out, const ph_adap_loss *adap /* host, or NULL */);
int ph_adapmult_train(ph_ctx *ctx, const ph_spec *spec, int context_size, const ph_opt_state *opt, const ph_rollout *rb,
                      const ph_ppo_hyper *hyper /* host */, int n_epochs, int batch_size, const int *perms,
                      unsigned long long perm_seed, float *stats, const ph_adap_loss *adap /* host */);

/* Measurement hook for bench.py's roofline: enqueue ONLY the ppo_grad kernel (the dominant kernel of PPO.train) `reps`
 * times between two HIP events on the ctx stream; *avg_ms_out = mean launch duration.  Launch i takes minibatch
 * i mod ceil(T*E / batch) of one in-kernel permutation of the buffer (size min(batch_size, T*E)), as the launches of an epoch do:
 * consecutive launches read DIFFERENT rows, so the figure does not flatter the kernel with rows the previous launch left in
 * the L2.  Optimizer state is not touched.  Synchronises. */
int ph_bench_ppo_grad(ph_ctx *ctx, const ph_spec *spec, const float *params, const ph_rollout *rb,
                      const ph_ppo_hyper *hyper /* host */, int batch_size, int reps, int gemm_mode,
                      float *avg_ms_out /* host */);
/* same for the GAE kernel (mode as in ph_gae); advantages/returns are overwritten with the same values each rep */
int ph_bench_gae(ph_ctx *ctx, const ph_rollout *rb, const float *last_values, const float *dones, double gamma,
                 double gae_lambda, int mode, int reps, float *avg_ms_out /* host */);

/* Measurement hook for bench.py's HBM-side roofline lines (K1 buffer write, K3 minibatch gather, K6 reduction):
 * the kernels of one PPO.train() call OTHER than the gradient kernel, each enqueued `reps` times between two HIP events on the ctx
 * stream; us_out[slot] = mean launch duration in microseconds (0 = the kernel does not run for this spec).  Runs the preparation of
 * a train() call with the in-kernel permutation, one gradient launch (so that the slabs hold a real minibatch), then the timed
 * launches; `opt` must be a SCRATCH copy of the optimizer state -- the reduction / Adam launches advance it.  Synchronises. */
enum {
  PH_BENCH_WEIGHT_IMAGE = 0, /* weight_image_kernel (split gradient kernel only) */
  PH_BENCH_OBS_PLANES = 1,   /* obs_planes_kernel: the call's observation planes + per-row scalar table (split only) */
  PH_BENCH_ADV_STATS = 2,    /* adv_stats_kernel + adv_finalize_kernel: all n_epochs x n_minibatches of the call */
  PH_BENCH_REDUCE = 3,       /* ppo_reduce_kernel, the shape used beside another learner's gradient launch */
  PH_BENCH_REDUCE_WIDE = 4,  /* ppo_reduce_kernel, the 16-byte-load shape of a learner alone on its device */
  PH_BENCH_ADAM = 5,         /* ppo_adam_kernel */
  PH_BENCH_STEP_FUSED = 6,   /* ppo_step_kernel (reduce + clip + Adam as one launch), 0 if its grid is not resident at once */
  PH_BENCH_BUFFER_ADD = 7,   /* buffer_add_kernel: RolloutBuffer.add of one step (row 1 <- row 0) */
  PH_BENCH_SLAB_FLOATS = 8,  /* not a time: floats of gradient slabs one minibatch writes (and the reduction reads) */
  PH_BENCH_NKERN = 9
};
int ph_bench_train_kernels(ph_ctx *ctx, const ph_spec *spec, const ph_opt_state *scratch_opt, const ph_rollout *rb,
                           const ph_ppo_hyper *hyper /* host */, int n_epochs, int batch_size, int reps, int gemm_mode,
                           float *us_out /* host, PH_BENCH_NKERN */);

/* Host-side evaluation of the keyed Feistel permutation ph_ppo_train uses when perms == NULL: writes
 * out[i] = perm_epoch(start + i) for i < count (env-major indices in [0, n)).  Pure CPU, needs no device;
 * the kernels run the identical integer code, so this is the bit-exact statement of the minibatch order. */
int ph_feistel_indices(int n, unsigned long long perm_seed, int epoch, int start, int count, int *out /* host */);

/* ---- ModularAlgorithm / ModularPolicy (pantheonrl/algos/modular) -----------------------------------------
 * ModularPolicy (modular/policies.py:243-395): the ordinary MlpPolicy ("main") plus one module per partner -- a 64-64 policy
 * tower and a 64-64 value tower that BOTH read the main policy latent (policies.py:254,281), an action head and a value head.
 * Logits = main + partner logits (the partner's alone with `nomain`, policies.py:325-328), value = main + partner value
 * (policies.py:286).  `baseline` shares one module between all partners (policies.py:255-257).
 * Parameter vector: the main network in ph_layout order (P_main floats), then module m at P_main + m * P_module in the ph_layout
 * order of a (Box(64), same action space) network.  Single Discrete head of <= 8 logits, <= 64 features.
 *   ph_modular_layout  : both layouts and the total length.
 *   ph_modular_forward : ModularPolicy.forward / evaluate_actions / get_action_logits_from_obs for partner `partner_idx`
 *       (policies.py:271-288,364-395): arguments as ph_policy_forward, plus the two logit vectors the marginal regulariser reads.
 *   ph_modular_train   : ModularAlgorithm.train (modular/learn.py:221-351): partner by partner over that partner's rollout buffer
 *       (rbs[k], learn.py:134-144), n_epochs passes each; every minibatch is the PPO loss on the composed heads with ALWAYS
 *       normalised advantages (learn.py:260-261) + marginal_reg_coef * marginal regularisation loss (learn.py:298-318), one
 *       clip_grad_norm_ over the main network and every module, one Adam step (torch's per-parameter step counts: mod_first);
 *       the target-KL test runs after a whole epoch on the mean of its KLs (learn.py:320-334) and ends that partner's epochs.
 *       stats: (num_partners * n_epochs * n_minibatches, PH_NSTAT) = policy_loss, value_loss, entropy_loss, clip_fraction,
 *       approx_kl (mean(old_log_prob - log_prob), learn.py:327), loss, grad_norm, marginal_reg; rows of skipped minibatches 0.
 *   ph_modular_minibatch_grad : the gradient of one minibatch's loss w.r.t. every parameter (tests). */
typedef struct ph_modular {
  int num_partners;
  int n_modules;               /* distinct modules: num_partners, or 1 with `baseline` */
  int module_of[PH_MOD_MAX];   /* partner -> module */
  int nomain;
} ph_modular;
int ph_modular_layout(const ph_spec *spec /* host */, const ph_modular *mod /* host */, ph_layout *main_out /* host */,
                      ph_layout *module_out /* host */, int *p_total_out /* host */);
int ph_modular_forward(ph_ctx *ctx, const ph_spec *spec, const ph_modular *mod, const float *params, int partner_idx,
                       const float *obs, int n, const unsigned char *action_mask, const float *uniforms,
                       const float *given_actions, unsigned long long seed, unsigned long long counter, int deterministic,
                       int *actions_i32, float *actions_f32, float *values, float *log_probs, float *entropy,
                       float *logits_main /* (n, L) or NULL */, float *logits_partner /* (n, L) or NULL */,
                       const ph_rollout *rb, int pos, const float *episode_start_in, const float *pending_reward,
                       int gemm_mode);
int ph_modular_train(ph_ctx *ctx, const ph_spec *spec, const ph_modular *mod, const ph_opt_state *opt,
                     int *mod_first /* device (n_modules): -1 until the module's value side first received a gradient */,
                     const ph_rollout *rbs /* host, [num_partners] */, const ph_ppo_hyper *hyper, int n_epochs, int batch_size,
                     const int *perms /* device (num_partners, n_epochs, T*E) or NULL */, unsigned long long perm_seed,
                     float *stats, float marginal_reg_coef, int gemm_mode);
int ph_modular_minibatch_grad(ph_ctx *ctx, const ph_spec *spec, const ph_modular *mod, const float *params, int partner_idx,
                              const ph_rollout *rb, const ph_ppo_hyper *hyper, const int *indices /* device (nb) */, int nb,
                              float marginal_reg_coef, float *grad_out /* device (P_total) */,
                              float *stats_out /* device (PH_NSTAT) or NULL */, int gemm_mode);

/* ---- behavioural cloning --------------------------------------------------------------------------
 * BC <- pantheonrl/algos/bc.py:180-366 on FeedForward32Policy <- pantheonrl/common/util.py:114-123: SB3 ActorCriticPolicy with
 * net_arch = [32, 32], ONE shared tanh trunk feeding action_net and value_net.  Parameter vector (float32, input-major):
 *   W1[F][32] b1[32] W2[32][32] b2[32] act_W[32][L] act_b[L] val_W[32] val_b[1]
 *  ph_bc_forward: policy.forward / evaluate_actions of that architecture (argument meaning as ph_policy_forward).
 *  ph_bc_train:   BC.train (bc.py:305-353): for every epoch, for every consecutive slice of `batch_size` entries of that epoch's
 *      visiting order (the last may be short; DataLoader(shuffle=True) draws one permutation per epoch -- `order` teacher-forces
 *      it): loss = -mean(log_prob) - ent_weight * mean(entropy) + l2_weight * sum(w^2) / 2 (bc.py:291-303), backward, one
 *      torch.optim.Adam step (no gradient clipping).  max_batches > 0 stops after that many minibatches (`n_batches` mode).
 *      The whole chain runs inside ONE launch of one persistent workgroup (parameters resident in LDS).
 *      stats (minibatches, PH_BC_NSTAT) or NULL: {neglogp, entropy, ent_loss, prob_true_act, l2_norm, l2_loss, loss, rows}
 *      (bc.py:305-313).  Limit: parameters, their gradient and one 32-row tile must fit the CU's 160 KiB of LDS (F <= ~500). */
#define PH_BC_HIDDEN 32
#define PH_BC_NSTAT 8
typedef struct ph_bc_layout {
  int D, F, A, L, P;
  int W1, b1, W2, b2, act_W, act_b, val_W, val_b; /* offsets */
} ph_bc_layout;
typedef struct ph_bc_hyper { /* BC defaults: bc.py:189-191; torch.optim.Adam defaults */
  float learning_rate; /* 1e-3  */
  float adam_beta1, adam_beta2, adam_eps; /* 0.9, 0.999, 1e-8 */
  float ent_weight;    /* 1e-3  */
  float l2_weight;     /* 0.0   */
} ph_bc_hyper;
int ph_bc_layout_of(const ph_spec *spec /* host */, ph_bc_layout *out /* host */);
/* host only, no launch: which kernel ph_bc_train runs for the spec -- 0 none (ph_bc_train refuses: the working set exceeds the LDS),
 * 1 bc_train_kernel (VALU loops), 2 bc_train_mfma_kernel<false> (MFMA tiles, Adam moments through L2), 3 bc_train_mfma_kernel<true>
 * (moments in LDS).  ph_bc_train dispatches through the same function; PH_BC_MFMA=0 (read once per process) leaves 0 and 1. */
int ph_bc_train_path(const ph_spec *spec /* host */, int *out /* host */);
int ph_bc_forward(ph_ctx *ctx, const ph_spec *spec, const float *params, const float *obs, int n,
                  const unsigned char *action_mask, const float *uniforms, const float *given_actions,
                  unsigned long long seed, unsigned long long counter, int deterministic, int *actions_i32, float *values,
                  float *log_probs, float *entropy, float *logits);
int ph_bc_train(ph_ctx *ctx, const ph_spec *spec, const ph_opt_state *opt, const float *obs /* (N,D) */,
                const float *acts /* (N,A) f32 */, const int *order /* (n_epochs, N) int32 */, int N, int batch_size,
                int n_epochs, int max_batches, const ph_bc_hyper *hyper /* host */, float *stats);

/* ---- MLP towers of a run-time shape (policy_kwargs net_arch; kernels: ph_arch.hip) ---------------------------------------
 * SB3's MlpPolicy with net_arch = [dict(pi = W, vf = W)]: both towers the same list W of one to PH_ARCH_MAX_LAYERS widths, every
 * width a multiple of 32 in [32, PH_ARCH_MAX_WIDTH], Tanh after every layer (the extractor loop is reference
 * pantheonrl/algos/adap/policies.py:152-200), categorical heads.  Parameter vector, float32, input-major like ph_layout: policy
 * tower W1 b1 .. Wn bn, value tower the same, act_W[w_n][L], act_b[L], val_W[w_n], val_b:
 *   P = 2 * sum_l (in_l * w_l + w_l) + w_n * L + L + w_n + 1;  at widths (64, 64) every offset equals ph_layout_of's.
 * The entry points take the arguments of ph_policy_forward / ph_ppo_minibatch_grad / ph_ppo_train plus the arch, and mean the same.
 * gemm_mode: 0 = f32 MFMA, 1 = the same kernel's VALU fmaf instantiation (bitwise the same results), 2 = answered by mode 0.
 * Gradient slabs are P floats per workgroup in parameter order; their allocation is capped (256 MiB per context), and the
 * workgroup count of a gradient launch follows from the cap.  Box action spaces are refused. */
#define PH_ARCH_MAX_LAYERS 3
#define PH_ARCH_MAX_WIDTH 256
typedef struct ph_arch {
  int n_layers;
  int width[PH_ARCH_MAX_LAYERS];   /* of both towers */
} ph_arch;
typedef struct ph_arch_layout {
  int D, F, A, L, P;
  int pi_W[PH_ARCH_MAX_LAYERS], pi_b[PH_ARCH_MAX_LAYERS], vf_W[PH_ARCH_MAX_LAYERS], vf_b[PH_ARCH_MAX_LAYERS];
  int act_W, act_b, val_W, val_b;
} ph_arch_layout;
int ph_arch_layout_of(const ph_spec *spec /* host */, const ph_arch *arch /* host */, ph_arch_layout *out /* host */);
/* dynamic LDS bytes of the gradient launch (rows_out: its tile height, 64 or 32) and of the forward launch for this spec and arch;
 * host only */
int ph_arch_lds_bytes(const ph_spec *spec /* host */, const ph_arch *arch /* host */, int *grad_bytes_out, int *grad_rows_out,
                      int *fwd_bytes_out);
/* 0 when the tower kernels can run this spec and arch; otherwise the status and ph_last_error text with which every ph_arch entry
 * point refuses the pair (a bad arch; a 32-row LDS carve above the CU's LDS: "... LDS tile ...").  Host only, no context: for
 * callers that want the refusal when an agent is built, not at its first step (the reference has no such limit: its
 * MlpExtractor is a chain of torch.nn.Linear, stable_baselines3/common/torch_layers.py) */
int ph_arch_fits(const ph_spec *spec /* host */, const ph_arch *arch /* host */);
int ph_arch_forward(ph_ctx *ctx, const ph_spec *spec, const ph_arch *arch /* host */, const float *params, const float *obs, int n,
                    const unsigned char *action_mask, const float *uniforms, const float *given_actions,
                    unsigned long long seed, unsigned long long counter, int deterministic, int *actions_i32,
                    float *actions_f32, float *values, float *log_probs, float *entropy, float *logits,
                    const ph_rollout *rb /* or NULL */, int pos, const float *episode_start_in,
                    const float *pending_reward /* or NULL */, int gemm_mode);
int ph_arch_minibatch_grad(ph_ctx *ctx, const ph_spec *spec, const ph_arch *arch /* host */, const float *params,
                           const ph_rollout *rb, const ph_ppo_hyper *hyper /* host */, const int *indices, int nb,
                           float *grad_out, float *stats_out, int gemm_mode);
int ph_arch_train(ph_ctx *ctx, const ph_spec *spec, const ph_arch *arch /* host */, const ph_opt_state *opt, const ph_rollout *rb,
                  const ph_ppo_hyper *hyper /* host */, int n_epochs, int batch_size, const int *perms,
                  unsigned long long perm_seed, float *stats, int gemm_mode);
/* The towers in the device-resident paths (additions; PH_ABI_VERSION unchanged).
 *  ph_arch_forward_ragged: ph_policy_forward_ragged with a tower of run-time shape -- OnPolicyAgent.get_action of the partner seat
 *      of a vectorised turn-based game (agents.py:111-184 per table: forward for all n = rb->E tables, the transition of table e
 *      recorded at row pos_env[e] iff record_mask[e] != 0 and pos_env[e] < rb->T, `values` updated for recorded tables only).
 *      Actions, values and log-probs are bitwise ph_arch_forward's for the same (seed, counter). */
int ph_arch_forward_ragged(ph_ctx *ctx, const ph_spec *spec, const ph_arch *arch /* host */, const float *params, const float *obs,
                           const unsigned char *action_mask, unsigned long long seed, unsigned long long counter,
                           int deterministic, int *actions_i32, float *values, float *log_probs, const ph_rollout *rb,
                           const int *pos_env, const unsigned char *record_mask, const float *episode_start_in, int gemm_mode);
/*  ph_liar_selfplay_step_arch: ph_liar_selfplay_step -- one vectorised MultiAgentEnv.step of n Liar's Dice tables
 *      (multiagentenv.py:149-215 + TurnBasedEnv.n_step / n_reset :307-327) -- with either seat's policy a tower: ego_arch / alt_arch
 *      describe the parameter vectors s->ego_params / s->alt_params; NULL keeps that seat on the 64-wide kernels (mixed pairings),
 *      and (NULL, NULL) is bit for bit ph_liar_selfplay_step.  Same launch sequence, same RNG counters (ego forward `counter`,
 *      partner forwards 2*counter and 2*counter + 1, dice `counter`). */
int ph_liar_selfplay_step_arch(ph_ctx *ctx, const ph_liar_selfplay *s, const ph_arch *ego_arch /* host or NULL */,
                               const ph_arch *alt_arch /* host or NULL */, int ego_pos, unsigned long long counter, int deal_only);
/*  ph_block_selfplay_step_arch: the same for ph_block_selfplay_step (one MultiAgentEnv.step of n block-world tables,
 *      multiagentenv.py:149-215); both forwards and the worlds draw with `counter`. */
int ph_block_selfplay_step_arch(ph_ctx *ctx, const ph_block_selfplay *s, const ph_arch *ego_arch /* host or NULL */,
                                const ph_arch *alt_arch /* host or NULL */, int ego_pos, unsigned long long counter);
/*  Towers as members of the Liar's Dice pool and of cross-play (additions; PH_ABI_VERSION unchanged; ph_pool_member, ph_liar_pool
 *      and ph_liar_xplay keep their layouts: the archs travel beside them).  member_archs: NULL, or a host array [n_members] whose
 *      entry k is NULL -- member k stays what its kind says, on today's kernels -- or the arch of the towers that a PH_POOL_LEARNER
 *      or PH_POOL_FROZEN member's `params` (a ph_arch_layout vector, 16-byte aligned) describe.  With every arch NULL each entry
 *      point is bit for bit the one it extends (which is that call).  Refused with nothing launched: an arch on a scripted member
 *      or a clone, an arch ph_arch_fits refuses for the spec, misaligned params.
 *  ph_pool_forward_arch: a tower member's tiles of the bucket pass run in ONE launch of their own behind the grouped one
 *      (pool_tower_kernel: one workgroup per (tile, net), the 32-row tower forward over the tile's <= 16 tables, dynamic LDS the
 *      largest carve over the table's tower members), made only when the member table holds a tower; the 64-wide launch is left out
 *      when the table holds neither a 64-wide nor a scripted member.  Row e of a frozen tower is bitwise ph_arch_forward's row e
 *      for (member seed, counter), row e of a learner tower ph_arch_forward_ragged's with the member's rows as record mask.  Only
 *      the MFMA instantiation (gemm_mode 0) is built: the grouped forward takes no gemm_mode.
 *  ph_liar_pool_step_arch: ph_liar_pool_step with tower members and / or a tower ego (ego_arch describes pool->ego_params; NULL: the
 *      64-wide ego).  8 launches as ph_liar_pool_step when every member is a tower or none is; a table that holds towers beside
 *      other members adds one launch per grouped forward: 10 (12 with clones as well).
 *  ph_liar_xplay_step_arch: ph_liar_xplay_step with tower members.  9 launches when every member is a tower or none is, else one
 *      more per grouped forward: 12 (15 with clones as well).
 *  A recorder logs a tower member's moves like any member's. */
int ph_pool_forward_arch(ph_ctx *ctx, const ph_spec *spec, const ph_pool_member *members, int n_members, const float *obs,
                         const int *partnerid, const unsigned char *active, unsigned long long counter, int *actions,
                         const float *episode_start_in, int n, const ph_arch *const *member_archs /* host or NULL */);
int ph_liar_pool_step_arch(ph_ctx *ctx, const ph_liar_pool *pool, const ph_arch *ego_arch /* host or NULL */,
                           const ph_arch *const *member_archs /* host or NULL */, int ego_pos, unsigned long long counter,
                           int deal_only);
int ph_liar_xplay_step_arch(ph_ctx *ctx, const ph_liar_xplay *xp, const ph_arch *const *member_archs /* host or NULL */,
                            unsigned long long counter, int deal_only);
/*  ph_arch_scripted_rollout: ph_scripted_rollout for towers -- OnPolicyAgent.get_action / update per step (agents.py:111-203)
 *      against a scripted environment with the launch boundaries removed: ONE launch in which a workgroup owns 32 rows of one net
 *      for all n_steps.  Exactly, bit for bit,
 *          for t in 0 .. n_steps-1:  ph_arch_forward(obs_seq[t], counter0 + t, rb, pos0 + t,
 *                                                    episode_start_in = t ? done_seq[t-1] : episode_start0,
 *                                                    pending_reward   = t ? rew_seq[t-1]  : NULL)
 *          ph_buffer_add_reward(rb, pos0 + n_steps - 1, rew_seq[n_steps-1], NULL)
 *      for every spec / arch pair ph_arch_forward takes.  n must equal rb->E; rows pos0 .. pos0 + n_steps - 1 must lie in rb. */
int ph_arch_scripted_rollout(ph_ctx *ctx, const ph_spec *spec, const ph_arch *arch /* host */, const float *params,
                             const float *obs_seq, const float *rew_seq, const float *done_seq, int n, int n_steps,
                             const float *episode_start0, unsigned long long seed, unsigned long long counter0, int *actions_i32,
                             float *values, float *log_probs, const ph_rollout *rb, int pos0, int gemm_mode);

/* ---- ADAP seats in the device-resident games (csrc/ph_adap_vec.h; additions, PH_ABI_VERSION unchanged) -------------------------
 * An AdapPolicy (adap/policies.py:21-146) is, for the engine, the MLP over a Box row  features(observation) ++ context  of F + C
 * floats.  On the device-resident paths the row is built on the device and every table owns a context that is redrawn there when
 * the seat's episode ends (AdapAgent.update, adap/agent.py:147-151; ADAP.collect_rollouts, adap_learn.py:457-461).
 *  ph_adap_rows: rows[e] = one_hot(obs[e]) ++ contexts[e]  (env_obs_space PH_SPACE_DISCRETE: SB3's one-hot in component order, a
 *      component outside [0, nvec_i) clamped)  or  obs[e] ++ contexts[e]  (PH_SPACE_BOX: F = n).  One launch, float accesses only
 *      (F + C may be odd); rows of tables with active[e] == 0 are left untouched.
 *  ph_adap_context_draw: contexts[e] <- sampler's draw from philox_uniform(seed ^ salt, counter + (rng epoch word << 32), e,
 *      component) for every table with redraw[e] != 0 (NULL: every table).  One launch.  context_size <= 64; PH_CTX_NATURAL_NUMBERS
 *      needs context_size == 1.
 *  ph_adap_vec_host: the same two functions on the CPU over HOST arrays; no context, no device.  do_draw != 0: contexts are drawn
 *      first (at `counter`, no epoch word); rows != NULL: rows are built from obs and contexts.  Misuse is reported through
 *      ph_last_error. */
int ph_adap_rows(ph_ctx *ctx, const ph_space *env_obs_space /* host */, int context_size, const float *obs /* (n,D) */,
                 const float *contexts /* (n,C) */, const unsigned char *active /* (n) or NULL */, float *rows /* (n,F+C) */, int n);
int ph_adap_context_draw(ph_ctx *ctx, int sampler, int context_size, unsigned long long seed, unsigned long long counter,
                         const unsigned char *redraw /* (n) or NULL */, float *contexts /* (n,C) */, int n);
int ph_adap_vec_host(const ph_space *env_obs_space /* or NULL when rows is NULL */, int context_size, int sampler, int do_draw,
                     unsigned long long seed, unsigned long long counter, const unsigned char *redraw /* (n) or NULL */,
                     float *contexts /* (n,C) */, const float *obs /* (n,D) or NULL */, const unsigned char *active /* (n) or NULL */,
                     float *rows /* (n,F+C) or NULL */, int n);
/*  ph_liar_selfplay_step_adap: ph_liar_selfplay_step with an ADAP learner in either seat.  A NULL seat stays on the kernels it has
 *      today (its parameters are s->ego_params / s->alt_params under s->spec); (NULL, NULL) is bit for bit ph_liar_selfplay_step.
 *      The launch sequence is that step's with two additions:
 *        - each forward of an ADAP seat is preceded by its row build (ph_adap_rows' launch) from the observation plane the forward
 *          would have read (s->obs_ego; for seat 1 the reply's obs_next under `running`, the opening's obs_alt under `alt_opens`)
 *          and the seat's contexts; the forward then runs on `rows` under the seat's Box spec and records `rows` into its buffer;
 *        - behind the pass that ends games (after_reply) one redraw launch per drawing seat gives a new context, drawn at `counter`,
 *          to every table in which that seat just received `done`.  For the ego that is every table whose game ended (s->done).
 *          For the partner it is the tables where _update_players pays it with done, i.e. where it moved in that game -- which in
 *          Liar's Dice is again every ended game: sanitize_action turns a call on the opening move into a bid (liar.py:58-67), so a
 *          game never ends before both seats have moved.  A deal-only call redraws nothing: the first contexts of a run are the
 *          caller's, drawn at counter 0.
 *      shared != 0 (--share-latent, adap/agent.py:72-73): the seat reads the OTHER seat's `contexts` of the same table and never
 *      draws; the other seat must then be an ADAP seat of the same context_size.  Both seats draw at the step's `counter`; their
 *      keys differ because their seeds differ.  Refused with nothing launched: a seat whose spec is not a Box of F + C components
 *      over the Liar's Dice observation, a rollout buffer of another row length, a context_size the sampler does not take, a
 *      missing plane, misaligned parameters. */
typedef struct ph_adap_seat {
  const ph_spec *spec;      /* host: Box(F + C) observations, the seat's action space */
  int context_size, sampler;
  float *contexts;          /* (n, C) */
  float *rows;              /* (n, F + C) scratch: the rows of the seat's latest forward */
  unsigned long long seed;  /* the learner's policy seed: the draws' key is seed ^ salt */
  int shared;
} ph_adap_seat;
int ph_liar_selfplay_step_adap(ph_ctx *ctx, const ph_liar_selfplay *s, const ph_adap_seat *ego /* host or NULL */,
                               const ph_adap_seat *alt /* host or NULL */, int ego_pos, unsigned long long counter, int deal_only);
/*  Frozen ADAP checkpoints as members of the Liar's Dice pool and of cross-play (additions; PH_ABI_VERSION unchanged; ph_pool_member,
 *      ph_liar_pool and ph_liar_xplay keep their layouts: the descriptions travel beside them, as the archs do).  This is the
 *      reference's FIXED '{"type":"ADAP","location":...,"latent_val":[...]}' partner (trainer.py:140-147: ADAP.load, then
 *      policy.set_context(latent_val)) over n tables.  member_adaps: NULL, or a host array [n_members] whose entry k is NULL -- member k
 *      stays what its kind and arch say -- or the description of the additive AdapPolicy a PH_POOL_FROZEN member plays: the member's
 *      `params` are the 64-64 parameters under `spec` (Box(270 + C) observations, the step's action space), `seed` its Philox key, and
 *      table e's row is one_hot(observation e) ++ contexts[e].
 *        stated   draw == 0: the caller filled every row of `contexts` with the latent; nothing ever writes it.
 *        sampled  draw != 0: every table owns a context of this member; one ph_adap_context_draw launch per sampling member and step,
 *                 behind the pass that ends games, redraws it in every table that pass has dealt (alt_opens | ego_opens: in the pool
 *                 exactly the tables of `done`; in an evaluation the ended games of tables that play on -- a retired table keeps its
 *                 last context) -- key member seed ^ salt, counter the step's (+ the epoch word), block the table.  A deal-only call
 *                 draws for the tables it deals (all of them at the first deal).  Two sampling members must be given different seeds,
 *                 or their contexts are one stream.
 *      A member's move for table e is bitwise ph_adap_rows over the observation and contexts[e], then ph_policy_forward under `spec`
 *      with (member seed, counter); only actions[e] is written: a frozen member records nothing, values / log_probs are ignored.
 *      Its tiles of the bucket pass run in ONE launch of their own behind the others (pool_adap_kernel: one workgroup per tile, the
 *      general 32-row forward half empty, its X chunks built in LDS from the tile's 30 components and contexts: no row matrix in
 *      global memory), made only when the member table holds an ADAP member, and the only launch when it holds nothing else.  With
 *      every entry NULL each entry point is bit for bit and launch for launch its `_arch` counterpart (which is that call).
 *      Refused with nothing launched: NULL contexts, context_size outside 1..64, a spec whose observation is not a Box of
 *      270 + context_size or whose heads are not the step's (A, L) = (2, 19), a description on a member that is not PH_POOL_FROZEN
 *      (a PH_POOL_LEARNER: ADAP learners do not sit in a pool), an arch beside it, PH_CTX_NATURAL_NUMBERS with context_size != 1. */
typedef struct ph_pool_adap {
  const ph_spec *spec;      /* host: Box(270 + C) observations, the step's action space */
  int context_size, sampler;
  float *contexts;          /* (n, C) device */
  int draw;                 /* != 0: redrawn on the device with `sampler` where a game ends */
} ph_pool_adap;
int ph_pool_forward_adap(ph_ctx *ctx, const ph_spec *spec, const ph_pool_member *members, int n_members, const float *obs,
                         const int *partnerid, const unsigned char *active, unsigned long long counter, int *actions,
                         const float *episode_start_in, int n, const ph_arch *const *member_archs /* host or NULL */,
                         const ph_pool_adap *const *member_adaps /* host or NULL */);
int ph_liar_pool_step_adap(ph_ctx *ctx, const ph_liar_pool *pool, const ph_arch *ego_arch /* host or NULL */,
                           const ph_arch *const *member_archs /* host or NULL */,
                           const ph_pool_adap *const *member_adaps /* host or NULL */, int ego_pos, unsigned long long counter,
                           int deal_only);
int ph_liar_xplay_step_adap(ph_ctx *ctx, const ph_liar_xplay *xp, const ph_arch *const *member_archs /* host or NULL */,
                            const ph_pool_adap *const *member_adaps /* host or NULL */, unsigned long long counter, int deal_only);

/* ---- owning handle: one agent = its rollout buffer, weights and Adam state on the device ----------------------------------
 *   The pointer-level entry points above take device memory owned by the caller (the Python host uses torch
 * allocations).  This layer is the same path for a binder that has NO device runtime of its own: the handle owns every device
 * allocation, every array crossing the boundary is a HOST array (copied in / out), every call is complete on return.
 * Mapping to the reference's call sites:
 *   ph_agent_create / destroy        <- PPO.__init__(env, n_steps, gamma, gae_lambda, seed, device)    trainer.py:108-126,196-203
 *   ph_agent_set/get_params          <- policy.load_state_dict / state_dict (flat layout: ph_layout)    trainer.py:140-157,419-432
 *   ph_agent_set/get_optimizer       <- policy.optimizer.state_dict()
 *   ph_agent_buffer_reset            <- rollout_buffer.reset()                                          agents.py:157
 *   ph_agent_act(record=1)           <- policy.forward(obs) + rollout_buffer.add(..., reward = 0, ...)  util.py:63-81, agents.py:162-179
 *   ph_agent_act(record=0)           <- policy.forward(obs) alone (StaticPolicyAgent)                   agents.py:54-79
 *   ph_agent_add_reward              <- rollout_buffer.rewards[pos - 1] += reward                       agents.py:198
 *   ph_agent_gae                     <- rollout_buffer.compute_returns_and_advantage(last_values, dones) agents.py:127-130
 *   ph_agent_train                   <- model.train()                                                   agents.py:155
 *   ph_agent_export / import_buffer  <- the buffer's arrays as SB3 lays them out, (T, E, ...) float32
 * Errors: non-zero return, message from ph_agent_last_error() (thread-local). */
typedef struct ph_agent ph_agent;
const char *ph_agent_last_error(void);
int ph_agent_create(int device, const ph_spec *spec /* host */, int n_envs, int n_steps, double gamma, double gae_lambda,
                    unsigned long long seed, ph_agent **out /* host */);
int ph_agent_destroy(ph_agent *agent);
int ph_agent_layout(const ph_agent *agent, ph_layout *out /* host */);
int ph_agent_set_params(ph_agent *agent, const float *params /* host (P) */);
int ph_agent_get_params(ph_agent *agent, float *params_out /* host (P) */);
int ph_agent_set_optimizer(ph_agent *agent, const float *adam_m /* host (P) */, const float *adam_v /* host (P) */, int step);
int ph_agent_get_optimizer(ph_agent *agent, float *adam_m_out, float *adam_v_out, int *step_out /* host, any may be NULL */);
int ph_agent_buffer_reset(ph_agent *agent);
int ph_agent_pos(const ph_agent *agent, int *pos_out /* host */);
/* obs (E,D) host; action_mask (E,L) u8 or NULL; uniforms (E,A) or NULL (NULL = Philox keyed by the handle's seed and call
 * counter); record != 0 writes the transition at the buffer's write row with episode_start (E) and advances it.
 * Outputs (host, any may be NULL): actions (E,A) int32, values (E), log_probs (E). */
int ph_agent_act(ph_agent *agent, const float *obs, const unsigned char *action_mask, const float *uniforms,
                 int deterministic, int record, const float *episode_start, int *actions_out, float *values_out,
                 float *log_probs_out);
int ph_agent_add_reward(ph_agent *agent, const float *reward /* host (E) */, const unsigned char *env_mask /* host (E) or NULL */);
int ph_agent_gae(ph_agent *agent, const float *last_values /* host (E) */, const float *dones /* host (E) */, int mode);
/* perms (n_epochs, T*E) host int32 or NULL (keyed Feistel order from perm_seed); stats_out host
 * (n_epochs * ceil(T*E / batch_size), PH_NSTAT) or NULL */
int ph_agent_train(ph_agent *agent, const ph_ppo_hyper *hyper /* host */, int n_epochs, int batch_size, const int *perms,
                   unsigned long long perm_seed, float *stats_out);
int ph_agent_export_buffer(ph_agent *agent, float *observations, float *actions, float *rewards, float *episode_starts,
                           float *values, float *log_probs, float *advantages, float *returns /* host, any may be NULL */);
int ph_agent_import_buffer(ph_agent *agent, const float *observations, const float *actions, const float *rewards,
                           const float *episode_starts, const float *values, const float *log_probs, const float *advantages,
                           const float *returns /* host, any may be NULL */, int pos);

#ifdef __cplusplus
}
#endif
#endif /* PANTHEON_HIP_H */
