/*
 * ctr_reach_amd.h -- C ABI of libctr_reach_amd.so, the MI355X (gfx950) batched
 * concentric-tube-robot reach environment.
 *
 * Every entry point is extern "C", takes plain pointers and sizes, and is asynchronous
 * and stream-ordered: it enqueues HIP kernels on `stream` and returns without a device
 * synchronisation.  All device buffers are allocated and owned by the caller (PyTorch);
 * the library allocates nothing on the hot path.  Pointers marked "device" must be
 * device memory; structs themselves are read from host memory at call time.
 *
 * Return codes: 0 = ok, CTR_EINVAL (-1) = bad argument, CTR_EHIP (-2) = HIP launch error.
 * ctr_last_error() returns a thread-local description of the last failure.
 * Per-environment numeric faults (ODE step-size underflow, sampler exhaustion) are
 * reported through per-lane `status` words, never by aborting.
 *
 * Reference interfaces each entry point replaces (reference = keshaviyengar/gym-ctr-reach,
 * paths relative to ctr_reach_envs/):
 *   ctr_fk              Model.forward_kinematics(joint, system)          envs/model.py:30-70
 *                       (+ Segment envs/CTR_Python/Segment.py:6-61, ode_eq model.py:72-117,
 *                        ctr_model model.py:119-174, scipy solve_ivp RK45)
 *   ctr_set_action      Obs.set_action(action, system) x n_substeps       envs/obs.py:166-183,
 *                                                                          envs/ctr_reach_env.py:134-135
 *   ctr_step            CtrReachEnv.step(action)                          envs/ctr_reach_env.py:124-158
 *   ctr_reset           CtrReachEnv.reset(goal=None, system=None)         envs/ctr_reach_env.py:70-114
 *                       (+ Obs.sample_goal envs/obs.py:185-207, get_obs obs.py:136-164)
 *   ctr_compute_reward  CtrReachEnv.compute_reward(ag, dg, info)          envs/ctr_reach_env.py:160-170
 *   ctr_fk_tables       Model.forward_kinematics with per-row tube tables  envs/model.py:30-70
 *   ctr_fk_shape        Model.forward_kinematics + Model.r / r1 / r2 / r3  envs/model.py:30-70,119-174
 *   ctr_jacobian        CTR_Model.jac (finite differences)             envs/CTR_Python/CTR_Model.py:251-262
 *   ctr_ik_dls          dls_ik_position_only(model, q0, P_d, lam, num, tol) src/jacobian_controller.py:19-73
 *                       (and its use along the line / circle / helix waypoint paths of src/)
 *   ctr_actor / ctr_rollout
 *                       model.predict(obs, deterministic=True) of the stable-baselines DDPG MlpPolicy
 *                       actor in the evaluation loops of src/ (the loops behind evaluations*.csv),
 *                       ctr_rollout together with the env.step calls of those loops
 *   ctr_actor_load      the learner's parameters into that actor after a policy update of the
 *                       training pipeline (stable-baselines shares them inside one TensorFlow graph)
 *   ctr_critic / ctr_her_sample_td
 *                       the target-Q part of stable-baselines DDPG's _setup_target_network_updates /
 *                       _train_step: r + gamma (1 - done) Q'(s', pi'(s')) from the target networks,
 *                       ctr_her_sample_td together with the replay draw that feeds it
 *                       (ctr_critic_load: the Polyak-updated target parameters into the critic's blob)
 *   ctr_polyak          the target update of that DDPG (ddpg.py get_target_updates: target <-
 *                       (1 - tau) target + tau online after every training step) together with the
 *                       refresh of the target networks' blobs, one launch for all of them
 *   ctr_her_sample_td3 / ctr_td3_critic_step
 *                       no counterpart in the reference, which trains DDPG: the TD3 variant of the two
 *                       (Fujimoto et al. 2018; stable-baselines' TD3 defaults): the clipped double-Q
 *                       target on a noise-smoothed target action, and both critics' regression
 *   ctr_gauss_act / ctr_sac_actor_step / ctr_her_sample_sac
 *                       no counterpart in the reference either: stable-baselines' third model class
 *                       for a continuous action space, SAC (Haarnoja et al. 2018), with its defaults:
 *                       the tanh-Gaussian policy's sample and log-probability, the policy's update
 *                       under the smaller of two critics with the learned temperature, and the
 *                       entropy-regularised target together with the replay draw that feeds it;
 *                       ctr_collect_gauss: ctr_collect with that policy's samples as the actions
 *   ctr_explore / ctr_collect
 *                       the data collection of the reference's training pipeline, stable-baselines
 *                       DDPG under HER: NormalActionNoise clipped to the action box and
 *                       random_exploration on the policy's action; ctr_collect together with the
 *                       env.step calls and the replay wrapper's add() of that loop
 *   ctr_set_goal / ctr_follow
 *                       the policy side of the path-following comparisons of src/ (a trained policy
 *                       against dls_ik_position_only along line / circle / helix waypoints): the
 *                       goal moved from waypoint to waypoint between the env.step calls
 *   ctr_domain_params   Model.current_sys_parameters after randomize_parameters
 *                                                                          envs/model.py:20-28, model_utils.py:5-35
 *   ctr_her_open / ctr_her_record / ctr_her_sample
 *                       the replay side of the reference's training pipeline: stable-baselines 2
 *                       HER (HindsightExperienceReplayWrapper.add / _store_episode /
 *                       _sample_achieved_goal, ReplayBuffer.sample) with the reference's
 *                       settings goal_selection_strategy 'future', n_sampled_goal 4
 *                       (saved_policies/.../her/CTR-Generic-Reach-v0_1/CTR-Generic-Reach-v0/
 *                       config.yml), fed by CtrReachEnv.compute_reward (ctr_reach_env.py:160-170)
 */
#ifndef CTR_REACH_AMD_H
#define CTR_REACH_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_ABI_VERSION 17
#define CTR_MAX_SYSTEMS 8
#define CTR_POOL_MAX 192          /* ctr_batch_t.pool_depth limit (reset slots per environment) */
#define CTR_EINVAL (-1)
#define CTR_EHIP (-2)

/* per-lane status bits */
#define CTR_STATUS_STEP_UNDERFLOW 1u   /* scipy "Required step size is less than spacing" */
#define CTR_STATUS_SAMPLER_STUCK  2u   /* obs.py:204 "Stuck sampling goals..." (>1000 tries) */
#define CTR_STATUS_NAN            4u   /* model.py:69 assert not any(isnan(r)) */
#define CTR_STATUS_TOO_LONG       8u   /* fixed-step RK4: a segment needs > 2^20 steps (joints far
                                           outside the action box); the tip is NaN          */
#define CTR_STATUS_POOL_MISS     16u   /* CTR_AUTORESET_POOLED step: a done env found no pooled
                                           reset (the caller's no-miss promise was broken); the
                                           env stays done and is reset on a later step       */

/* ctr_step / ctr_step_her autoreset argument */
#define CTR_AUTORESET_OFF    0   /* done environments are left as they are                          */
#define CTR_AUTORESET_SWEEP  1   /* done environments are reset in the same call: from the reset pool
                                    if it holds their next reset, else by a miss sweep (a second,
                                    small launch that computes the missing resets)                  */
#define CTR_AUTORESET_POOLED 2   /* as SWEEP, but the caller guarantees every done environment finds
                                    its reset in the pool, so no sweep is launched: true when at most
                                    pool_depth steps have run since the last ctr_pool_refill (each
                                    step takes at most one reset per environment, and a refill leaves
                                    every environment's next pool_depth resets precomputed)          */

/* One 3-tube system (index 0 = innermost tube), derived on the host from the
 * registration kwargs exactly as Tube.__init__ (envs/CTR_Python/Tube.py:7-19):
 * EI = E * pi (d_o^4 - d_i^4) / 64, GJ = G * pi (d_o^4 - d_i^4) / 32. */
typedef struct ctr_system_t {
    double L[3];       /* tube length                        (Tube.L)    */
    double Lc[3];      /* pre-curved length                  (Tube.L_c)  */
    double EI[3];      /* bending stiffness  E * I                       */
    double GJ[3];      /* torsional stiffness G * J                      */
    double Ux[3];      /* pre-curvature x    (Tube.U_x)                  */
    double Uy[3];      /* pre-curvature y    (Tube.U_y)                  */
} ctr_system_t;

/* Raw tube inputs of Tube.__init__ (envs/CTR_Python/Tube.py:7-19) for one system, needed only
 * by domain randomisation, which re-samples them every reset (envs/model_utils.py:5-35). */
typedef struct ctr_tube_raw_t {
    double Din[3];     /* diameter_inner                                 */
    double Dout[3];    /* diameter_outer                                 */
    double E[3];       /* stiffness                                      */
    double G[3];       /* torsional_stiffness                            */
} ctr_tube_raw_t;

/* Integrator selection */
#define CTR_INTEGRATOR_RK45_SCIPY 0    /* scipy solve_ivp RK45 emulation, rtol 1e-3 atol 1e-6 (parity) */
#define CTR_INTEGRATOR_RK4        1    /* fixed-step classical RK4 of the same ODE (throughput)       */

/* Mechanics model */
#define CTR_MODEL_COMPLIANT 0          /* torsionally compliant (the reference, model.py:72-117)        */
#define CTR_MODEL_RIGID     1          /* torsionally rigid: GJ -> infinity, tube angles constant       */

/* Environment configuration (registration kwargs, ctr_reach_envs/__init__.py:6-94). */
typedef struct ctr_env_config_t {
    int32_t n_systems;          /* len(select_systems), 1..CTR_MAX_SYSTEMS              */
    int32_t n_substeps;         /* n_substeps (10)                                       */
    int32_t max_steps;          /* max_steps_per_episode (150)                           */
    int32_t constrain_alpha;    /* constrain_alpha                                       */
    int32_t egocentric;         /* joint_representation == 'egocentric'                  */
    int32_t resample_joints;    /* resample_joints                                       */
    int32_t integrator;         /* CTR_INTEGRATOR_*                                      */
    int32_t rk4_steps_per_m;    /* RK4 only: steps per metre of arclength (> 0)          */
    int32_t model;              /* CTR_MODEL_*                                           */
    int32_t obs_f64;            /* observation buffers (ctr_step_out_t.obs / terminal_obs,
                                   ctr_reset's obs): 0 = float32 [n][obs_dim], 1 = float64
                                   [n][obs_dim], the reference's dtype (obs.py:153-156).
                                   The values are computed in float64 either way.        */
    double  tol;                /* goal_tolerance.get_tol()                              */
    uint64_t seed;              /* Philox key for resets                                 */
    ctr_system_t systems[CTR_MAX_SYSTEMS];
    /* Domain randomisation (domain_rand kwarg; Model.randomize_parameters, model.py:20-28, called
     * by reset, ctr_reach_env.py:80).  0 = off.  Otherwise every reset draws, per tube, d_in,
     * d_out, E, G and U_x uniformly in v * [1 - domain_rand, 1 + domain_rand] (L, L_c, U_y are
     * kept) from Philox stream 3 keyed (seed, global env id, reset number), and the episode's
     * FKs use the tube table derived from them.  raw[] holds the unrandomised inputs. */
    double domain_rand;
    double domain_pad;
    ctr_tube_raw_t raw[CTR_MAX_SYSTEMS];
} ctr_env_config_t;

/* Device-resident batch state, row-major per environment ([n][k]). */
/* One precomputed reset of the pool (ABI 15): 128 B, one cache line when the pool is 128-B
 * aligned, so a pooled auto-reset reads one line (the ABI-14 [P][n][k] arrays spread it over 7). */
typedef struct ctr_pool_slot_t {
    double   dg[3];              /* desired goal                   bytes   0 -  23 */
    double   ag[3];              /* start position (its FK tip)            24 -  47 */
    float    qd[6];              /* desired joints                         48 -  71 */
    float    q0[6];              /* start joints                           72 -  95 */
    int32_t  sys;                /* system index                           96      */
    uint32_t stat;               /* CTR_STATUS_* of the precomputation    100      */
    uint32_t r;                  /* reset number held (0 = empty)         104      */
    uint32_t pad[5];             /*                                       108 - 127 */
} ctr_pool_slot_t;

typedef struct ctr_batch_t {
    int64_t   n;                 /* environments in this shard                        */
    int64_t   env_base;          /* global id of environment 0 (RNG key; sharding)    */
    float    *joints;            /* [n][6] f32 [b0,b1,b2,a0,a1,a2] (Obs.joints)       */
    double   *desired_goal;      /* [n][3]                                            */
    double   *achieved_goal;     /* [n][3] tip after the last step / reset            */
    int32_t  *t;                 /* [n] steps taken in the episode                    */
    int32_t  *system;            /* [n] index into config.systems                     */
    uint32_t *epoch;             /* [n] resets taken so far (RNG counter)             */
    float    *desired_joints;    /* [n][6] or NULL (info q_desired)                   */
    float    *starting_joints;   /* [n][6] or NULL (info q_starting)                  */
    double   *starting_position; /* [n][3] or NULL                                    */
    int32_t  *work;              /* [n+2] auto-reset miss list: 2 counters, then ids  */
    int32_t   work_parity;       /* host toggles 0/1 every ctr_step: which counter   */
    int32_t   work_pad;
    /* Reset pool (optional, pool_depth 0 disables it).  Resets are a deterministic function of
     * (seed, global env id, reset number), so they can be computed ahead of time: slot (r mod P)
     * of env e holds reset number r (ctr_pool_slot_t.r), precomputed by ctr_pool_refill; an
     * auto-reset consumes it with a copy instead of two forward-kinematics solves.  A missing
     * slot falls back to computing the reset in the same ctr_step call.  Layout [P][n] of
     * 128-B slots (ABI 15; one cache line per reset, was [P][n][k] per field). */
    int32_t   pool_depth;        /* P (0 = no pool, at most CTR_POOL_MAX)             */
    int32_t   pool_pad;
    ctr_pool_slot_t *pool;       /* [P][n] slots, 128-B aligned, zero-initialised     */
    int32_t  *refill;            /* [2 + 2 refill_cap]: count, (env, reset number) pairs,
                                    then a completion ticket (zero-initialised)          */
    int64_t   refill_cap;
    /* Resumable refill (optional, carry NULL disables it; scipy RK45 on either model, and
     * fixed-step RK4 on the compliant model -- the rigid model's RK4 segment maps ignore it).
     * A reset at least
     * refill_lead resets ahead of its environment (r - epoch - 1 >= refill_lead at the time of
     * the refill) runs at most refill_budget iterations (segment start + RK45 attempt; one RK4
     * step) of each of its two FKs in one ctr_pool_refill; an unfinished one is suspended
     * into the carry list and resumed by the next ctr_pool_refill, which writes its pool slot
     * once both FKs are done.  The result is bit-identical; only the refill a reset lands in
     * changes.  With refill_lead >= the steps between refills, no reset is due before it lands
     * (after every refill, the resets fewer than refill_lead ahead are in the pool).  */
    void     *carry;             /* ctr_refill_carry_bytes(carry_cap) B, zero-initialised */
    int64_t   carry_cap;         /* resets each of its two lists holds                 */
    int32_t   refill_budget;     /* iterations (RK4 steps) per FK and refill (0 = none) */
    int32_t   refill_lead;
} ctr_batch_t;

typedef struct ctr_gather_push_t ctr_gather_push_t;   /* defined with the push gather below */

/* Per-step outputs (device). obs_dim = 13, or 14 when n_systems > 1 (obs.py:153-156). */
typedef struct ctr_step_out_t {
    void     *obs;               /* [n][obs_dim]   observation after the step (after auto-reset);
                                    float32, or float64 with cfg->obs_f64                         */
    float    *reward;            /* [n]            0 or -1                                       */
    uint8_t  *done;              /* [n]                                                          */
    uint8_t  *success;           /* [n]            info['is_success']                            */
    float    *error;             /* [n]            info['error'] = ||dg - ag||                   */
    void     *terminal_obs;      /* [n][obs_dim] or NULL: pre-reset observation of done envs
                                    (the dtype of obs)                                           */
    double   *terminal_achieved; /* [n][3] or NULL: achieved goal of the terminal step           */
    uint32_t *status;            /* [n] or NULL: CTR_STATUS_* bits                               */
    uint32_t *nfev;              /* [n] or NULL: RHS evaluations spent in the step's FK          */
    float    *packed;            /* [n][4] (16-B aligned) or NULL: the step's outputs packed for
                                    the optional all-gather of a single-process trainer: tip x, y,
                                    z (float32; the terminal achieved goal of a done env) and
                                    done | success << 1 | (reward == -1) << 2 as a float (the
                                    reward is -1 or 0).  Written by k_step itself, so gathering
                                    costs no packing launch.                                      */
    uint32_t  packed_seq;        /* != 0 (with packed): k_step also writes row n of packed as
                                    (packed_seq, 0, 0, 0) as uint32 bits, the step's sequence word
                                    that ctr_copy_list pushes after the rows (packed then holds
                                    n + 1 rows).  0: row n is not touched.                        */
    uint32_t  packed_pad;
    const ctr_gather_push_t *gather;      /* device or NULL: the fused push gather of step
                                             gather_seq (descriptor of its slot) -- k_step also
                                             stores each env's packed row (as in `packed`) into
                                             every rank's receive slot, gather->dst[p] + e for
                                             p < gather->world (IPC-mapped peer memory), after
                                             every rank has released that slot (flow control,
                                             see "Push all-gather"), as system-scope stores the
                                             storing wave waits for.  The first
                                             lanes also release this rank's slot of step
                                             gather_seq + 1 - depth to every producer          */
    const ctr_gather_push_t *gather_prev; /* device or NULL: the first lanes of k_step publish
                                             gather_prev_seq to every gather_prev->seqw[p]
                                             (system scope) -- the previous gathered
                                             step, whose launch has completed (so its row stores
                                             are performed at system scope) before this one
                                             starts                                              */
    uint32_t  gather_prev_seq;
    uint32_t  gather_seq;        /* the step pushed with `gather` (wraps modulo 2^32)            */
    int32_t   gather_wait_prev;  /* != 0 (with gather, depth >= 3): k_step also waits until every
                                    rank's rows of step gather_seq - 1 are published in this
                                    rank's ring (gather->wait_seqw), so after this launch the
                                    previous step's gathered slot is readable on the stream (the
                                    fused consumer wait; errors in gather->err)                  */
    int32_t   gather_pad;
} ctr_step_out_t;

/* ---------------------------------------------------------------------------------------
 * HER replay feed (device).  Episodes are recorded where the environments run and relabelled
 * with stable-baselines 2 HER semantics:
 *   - an episode enters the replay store when it ends (HindsightExperienceReplayWrapper.add
 *     stores on done); its L transitions become L real rows plus, per transition t, k relabelled
 *     rows (FUTURE: none for the last transition), in _store_episode's order;
 *   - a relabelled row of transition t takes the achieved goal of obs_sel, the observation
 *     before transition sel (_sample_achieved_goal returns selected_transition[0]'s
 *     achieved_goal): FUTURE sel ~ U{t+1 .. L-1}, FINAL sel = L-1, EPISODE sel ~ U{0 .. L-1};
 *     its reward is compute_reward(achieved goal of obs_{t+1}, goal) at the tolerance in force
 *     when the episode ended, its done is 0; only the desired_goal slots change (the
 *     'observation' part, which holds dg - ag, is kept, as the wrapper keeps it);
 *   - ctr_her_sample draws rows uniformly with replacement over all stored rows
 *     (ReplayBuffer.sample) and returns them in HERGoalEnvWrapper's flat layout
 *     [observation, achieved_goal, desired_goal].
 * Storage: each environment owns `slots` episode slots used round-robin (slot of episode r of
 * env e = e * slots + r mod slots), so the store keeps each env's last slots - 1 finished
 * episodes (first-in first-out per env; stable-baselines drops the globally oldest rows).
 * The sel draws are a pure function of (seed, global env id, reset number, t, j) (Philox
 * stream 4): they are fixed per row, as the wrapper fixes them when it stores the episode. */
#define CTR_HER_FUTURE  0
#define CTR_HER_FINAL   1
#define CTR_HER_EPISODE 2

typedef struct ctr_her_t {
    int32_t  obs_dim;          /* 13 or 14                                                  */
    int32_t  t_max;            /* longest episode (max_steps_per_episode), <= 65535          */
    int32_t  n_sampled_goal;   /* k (4), <= 255                                              */
    int32_t  strategy;         /* CTR_HER_*                                                  */
    int64_t  n;                /* environments                                               */
    int64_t  env_base;         /* global id of environment 0 (keys the relabel draws)       */
    int32_t  slots;            /* episode slots per environment (>= 2)                      */
    int32_t  pad;
    uint64_t seed;             /* Philox key of the relabel draws                            */
    /* episode store, E = n * slots slots (device) */
    /* slot id = env * slots + s.  Rows are env-minor ([slots][t][n]) so the lanes of a wave,
     * consecutive envs mostly at the same (slot, t), write one contiguous span, and 16-B
     * aligned so every row is whole dwordx4 stores; a sampled row is one or two cache lines. */
    float    *state;           /* [slots][t_max + 1][n][24], 96-B rows: floats 0 .. obs_dim-1 =
                                  obs_t (obs_0 .. obs_L), floats 16 .. 21 = its achieved goal
                                  as 3 doubles                                                */
    float    *step;            /* [slots][t_max][n][8], 32-B rows: action 0..5, reward 6      */
    double   *dg;              /* [E][3]                   the episode's desired goal         */
    double   *tol;             /* [E]                      tolerance when the episode ended   */
    int32_t  *len;             /* [E]   L of a stored episode; 0 = empty, -1 = being recorded */
    uint32_t *epoch;           /* [E]   reset number of the episode in the slot              */
    /* per environment (device) */
    int32_t  *cur_t;           /* [n]   transitions recorded in the open episode; -1 = none  */
    uint32_t *cur_epoch;       /* [n]   reset number of the open episode                     */
    /* sampler scratch (device), CTR_HER_CDF_LEN(n * slots) int64: every ctr_her_sample call
     * rebuilds the prefix sums of the stored rows per slot here, so a draw is one search */
    int64_t  *cdf;
} ctr_her_t;

#define CTR_HER_SCAN_TILE 1024     /* slots per scan tile of the sampler's prefix sums */
#define CTR_HER_CDF_LEN(E) ((E) + ((E) + CTR_HER_SCAN_TILE - 1) / CTR_HER_SCAN_TILE + 1)

/* Flat sampled batch (device), d = obs_dim + 6. */
typedef struct ctr_her_batch_t {
    float   *obs;              /* [B][d]  [observation_t, achieved_goal_t, desired_goal]      */
    float   *action;           /* [B][6]                                                      */
    float   *reward;           /* [B]                                                         */
    float   *next_obs;         /* [B][d]  [observation_t+1, achieved_goal_t+1, desired_goal]  */
    float   *done;             /* [B]     1 for the last real transition of an episode        */
    int32_t *index;            /* [B][3] or NULL: (slot, t, j), j = 0 real, 1..k relabelled;
                                  slot -1: the store holds no rows (the row is zeros)        */
} ctr_her_batch_t;

/* Opens an episode for the environments with mask[i] != 0 (NULL = all) from the batch's
 * current state (after ctr_reset): obs_0 = obs [n][obs_dim], its achieved goal, the desired
 * goal and the reset number.  An episode still open in that env is discarded. */
int ctr_her_open(const ctr_her_t *her, const ctr_batch_t *batch, const float *obs, const uint8_t *mask,
                 void *stream);

/* Records the step that ctr_step (autoreset on) just made: action [n][6], out's reward / done /
 * obs / terminal_obs / terminal_achieved (terminal_* required).  A done env's episode is closed
 * with the tolerance tol and stored; the env's next episode is opened from the post-reset
 * state. */
int ctr_her_record(const ctr_her_t *her, const ctr_batch_t *batch, const float *actions,
                   const ctr_step_out_t *out, double tol, void *stream);

/* ctr_step + ctr_her_record in one pass: k_step writes the step's transition into the store as
 * it finishes each env (no second launch, no re-read of the step outputs), and opens the next
 * episode of every env it auto-resets (the miss sweep does it for the envs it resets).  Same
 * arguments and outputs as ctr_step; terminal_obs / terminal_achieved may be NULL here. */
int ctr_step_her(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const float *actions,
                 const ctr_step_out_t *out, int32_t autoreset, const ctr_her_t *her, void *stream);

/* Draws B rows uniformly with replacement over the stored rows: one uniform integer u per row
 * (keyed seed, counter, row) below the stored-row count, mapped to its (slot, row) through the
 * per-slot prefix sums this call rebuilds in her->cdf (exact inverse CDF: no retries, no
 * misses whatever the episode lengths). */
int ctr_her_sample(const ctr_her_t *her, int64_t batch_size, uint64_t seed, uint64_t counter,
                   const ctr_her_batch_t *out, void *stream);

int ctr_abi_version(void);
const char *ctr_last_error(void);

/* Batched Model.forward_kinematics: joints [n][6] f32 -> tip [n][3] f64.
 * sys_idx: [n] or NULL (all system 0).  stats: [n][4] or NULL = {RHS evaluations, accepted
 * RK steps, rejected RK attempts, integrated segments}.  Fixed-step RK4 never rejects; there
 * stats[1] counts the steps taken stage by stage and stats[2] the executed work of the segments
 * run as segment maps (matrix powers: every segment of the rigid model, the trailing segments of
 * the compliant model where tube 0 is alone): maps << 16 | square-and-multiply compositions.
 * stats[0] counts 4 RHS per RK4 step, mapped or not (the oracle's count).  status: [n] or NULL.
 * (device) */
int ctr_fk(const float *joints, const int32_t *sys_idx, int64_t n, const ctr_env_config_t *cfg,
           double *tip, uint32_t *stats, uint32_t *status, void *stream);

/* Model.forward_kinematics with one tube table per row: tables [n] (device), e.g. the
 * domain-randomised tables from ctr_domain_params (the reference integrates with
 * Model.current_sys_parameters, model.py:13,30).  cfg supplies the integrator and model. */
int ctr_fk_tables(const float *joints, const ctr_system_t *tables, int64_t n, const ctr_env_config_t *cfg,
                  double *tip, uint32_t *stats, uint32_t *status, void *stream);

/* Model.forward_kinematics with the backbone shape (Model.r, model.py:66-68 and ctr_model
 * model.py:119-174): besides the tip, r at the 30 sorted linspace points of every segment
 * (solve_ivp t_eval, RK45 dense output) and their arclengths s (ctr_model's Length), row-major
 * r [n][cap][3], s [n][cap]; npts [n] = 30 x segments (points past cap are not stored).
 * cap = 270 always suffices (<= 9 segments).  tables [n] or NULL: per-row tube tables as in
 * ctr_fk_tables (sys_idx is then ignored).  Needs integrator rk45_scipy.  (device) */
int ctr_fk_shape(const float *joints, const int32_t *sys_idx, const ctr_system_t *tables, int64_t n,
                 const ctr_env_config_t *cfg, int32_t cap, double *tip, double *r, double *s, int32_t *npts,
                 uint32_t *status, void *stream);

/* Forward-difference tip Jacobian d tip / d q over float64 joints [n][6] (device):
 * jac[n][3][6] = (tip(q + eps e_i) - tip(q)) / eps, the scheme of CTR_Model.jac
 * (envs/CTR_Python/CTR_Model.py:251-262, eps 1e-4 there) applied to Model.forward_kinematics;
 * the 7 FKs of an env run on 7 lanes.  tip [n][3] (the unperturbed FK) and status may be NULL;
 * status bits are OR-ed in. */
int ctr_jacobian(const double *joints, const int32_t *sys_idx, int64_t n, const ctr_env_config_t *cfg, double eps,
                 double *tip, double *jac, uint32_t *status, void *stream);

/* Damped-least-squares position IK on that Jacobian (ABI 17), the loop of dls_ik_position_only
 * (src/jacobian_controller.py:19-73) for n targets in ONE launch.  Per target and waypoint, at
 * most num times:
 *     p, J = FK(q), (FK(q + eps e_c) - FK(q)) / eps           (ctr_jacobian's arithmetic)
 *     e    = p_d - p
 *     e or J not finite: err = NaN, stop (q and iters unchanged: the last finite iterate)
 *     q   += J^T (J J^T + lam I)^-1 e ;  err = |e| ;  iters += 1 ;  stop once |e| < tol
 * (the stop is checked after the update, as the reference does).  With waypoints = K > 1 a target
 * follows a path: waypoint k starts from the q waypoint k - 1 ended with (q0 for k = 0), also
 * after a NaN stop; err starts at +inf and iters at 0 for every waypoint, so num = 0 returns
 * q0, +inf, 0.  The 7 FKs of a target run on 7 lanes of one wave, which owns its 9 targets
 * from q0 to the last waypoint: a target costs FKs only while its wave still has one running.
 * A target's result does not depend on n or on its place in the batch.
 * One launch runs at most waypoints * num <= CTR_IK_MAX_ITERS iterations per target; longer paths
 * are cut at waypoint boundaries by the caller (the next call's q0 = the last waypoint's q).
 * Every mode ctr_jacobian supports.  Nothing is allocated; stream-ordered; the struct is read at
 * the call.  A refused argument is CTR_EINVAL before any HIP call; n = 0 is a no-op. */
#define CTR_IK_MAX_ITERS 8192
typedef struct ctr_ik_t {
    int64_t n;                 /* targets                                                        */
    int32_t waypoints;         /* K >= 1                                                         */
    int32_t num;               /* iterations per waypoint, >= 0, K * num <= CTR_IK_MAX_ITERS     */
    double  lam, tol, eps;     /* lam > 0 finite; tol >= 0 (not NaN); eps finite, != 0           */
    const double  *targets;    /* [n][K][3]  device                                              */
    const double  *q0;         /* [n][6]     device, must not overlap q                          */
    const int32_t *sys_idx;    /* [n] or NULL (system 0)                                         */
    double   *q;               /* [n][K][6]  q at the end of each waypoint                       */
    double   *err;             /* [n][K]                                                         */
    int32_t  *iters;           /* [n][K]                                                         */
    uint32_t *status;          /* [n] or NULL: CTR_STATUS_* of every FK run, OR-ed in            */
} ctr_ik_t;
int ctr_ik_dls(const ctr_env_config_t *cfg, const ctr_ik_t *ik, void *stream);

/* n_substeps x Obs.set_action, in place on joints [n][6] (device). */
int ctr_set_action(const ctr_env_config_t *cfg, float *joints, const int32_t *sys_idx,
                   const float *actions, int64_t n, void *stream);

/* One CtrReachEnv.step for every environment of the batch; actions [n][6] f32 (device).
 * autoreset (CTR_AUTORESET_*) != 0: done environments are reset in the same call (VecEnv
 * semantics) and their pre-reset observation goes to out->terminal_obs. */
int ctr_step(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const float *actions,
             const ctr_step_out_t *out, int32_t autoreset, void *stream);

/* k consecutive ctr_step calls in one launch (ABI 16): afterwards the batch state and the output
 * buffers are exactly what ctr_step with actions->a[0], ..., actions->a[k - 1] (each [n][6] f32,
 * device), the same autoreset and batch->work_parity toggled after every step would have left
 * (terminal_obs / terminal_achieved: the rows of every step an env was done in, the last such
 * step winning; the other outputs: the last step's).  One kernel runs the period: the tables are
 * staged once and each wave takes its 64 environments through all k steps, with no device-wide
 * join between the steps (a step of an environment reads only that environment's own state and
 * its action row; the refill queue is append-only).  The entries of the queue may come in another
 * order than k launches leave them; ctr_pool_refill's result does not depend on it.
 * The pointer table is copied into the kernel arguments at the call: the caller's struct need not
 * outlive it.  Nothing is allocated; stream-ordered like ctr_step.
 * Supported: the one-environment-per-lane modes (every mode but the rigid model's fixed-step RK4,
 * which runs on 8-lane groups, and the compliant model's fixed-step RK4 without y pre-curvature,
 * which runs on lane pairs), autoreset CTR_AUTORESET_OFF or CTR_AUTORESET_POOLED, and
 * out->packed, out->gather, out->gather_prev all NULL.  Anything else, k outside
 * 1..CTR_STEP_MANY_MAX or a NULL entry in a[0..k-1] is CTR_EINVAL, before any HIP call.
 * The caller keeps CTR_AUTORESET_POOLED's promise for all k steps (no refill falls inside). */
#define CTR_STEP_MANY_MAX 64
typedef struct ctr_action_seq_t {
    const float *a[CTR_STEP_MANY_MAX];
} ctr_action_seq_t;
int ctr_step_many(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const ctr_action_seq_t *actions,
                  int32_t k, const ctr_step_out_t *out, int32_t autoreset, void *stream);

/* A whole refill period in one call (an entry point added within ABI 17: no existing entry point
 * or struct changes, so the number stays; a caller that needs it looks the symbol up): ctr_step_many(..., CTR_AUTORESET_POOLED, ...) followed
 * by ctr_pool_refill, with the refill's work done in the tail of the step kernel.  A wave that
 * has taken its 64 environments through the k steps does not append their consumed resets to
 * batch->refill; it goes straight on to the refill: it claims resets the previous refill suspended
 * (chunks of the carry list, one atomic per chunk) until none are left, then computes the new
 * resets of its own environments, with ctr_pool_refill's arithmetic and the same refill_budget /
 * refill_lead rule, suspending onto the same carry list.  No wave waits for another.  The last
 * workgroup to finish flips the carry lists; a second, small kernel follows, which as a rule exits
 * at once: it finishes the resets ctr_pool_refill would not have suspended where the waves could
 * not know that (the budget rule counts the whole period's resets; a wave may read another wave's
 * epoch before that environment's last reset of the period).
 * Afterwards the batch, the outputs, the pool and the set of suspended resets are what
 * ctr_step_many and ctr_pool_refill leave (the carry lists' order aside), batch->refill is empty,
 * and a ctr_pool_refill that follows finds nothing to do.  It interoperates with ctr_step,
 * ctr_pool_refill, ctr_pool_requeue and checkpoints of the batch like ctr_pool_refill.
 * The caller's promises: batch->refill is empty at the call (the call starts a period: the last
 * launch on the batch was a refill), and CTR_AUTORESET_POOLED's promise holds for all k steps.
 * Refused (CTR_EINVAL, before any HIP call) wherever ctr_step_many is -- which includes the two
 * modes whose refill is not the two-lane resumable one, the rigid model's fixed-step RK4 (8-lane
 * groups) and the compliant model's without y pre-curvature (lane pairs) -- without a reset pool,
 * and for the compliant model's scipy RK45 with a y pre-curvature (that kernel would not fit the
 * register file without scratch; use ctr_step_many and ctr_pool_refill).  Stream-ordered; nothing is allocated. */
int ctr_step_period(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const ctr_action_seq_t *actions,
                    int32_t k, const ctr_step_out_t *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * MLP actor (entry points added within ABI 17: no existing entry point or struct changes, so the
 * number stays; a caller that needs them looks the symbols up).  A deterministic policy on the
 * device: the reference's stable-baselines DDPG MlpPolicy actor on HERGoalEnvWrapper's flat row
 * x = [observation, achieved_goal, desired_goal] (in_dim = obs_dim + 6 floats, the layout of
 * ctr_her_batch_t.obs).  1..3 hidden layers, widths multiples of 32 up to 256:
 *     x_hi = bf16(x);  x_lo = bf16(x - float(x_hi))        (round to nearest even; x - x_hi in f32)
 *     z1   = W1 x_hi + W1 x_lo                             (bf16 weights, f32 accumulation)
 *     h1   = bf16(relu(z1 + b1))                           (f32 bias; relu(z) = z > 0 ? z : 0)
 *     hl   = bf16(relu(Wl h(l-1) + bl))                    the further hidden layers
 *     y    = Wout hL + bout                                6 "logits", f32
 *     a_i  = scale_i * tanhf(y_i)
 * An env's action depends on its own row and the weights only (not on n or on its neighbours).
 * The weights live in one packed device blob (ctr_actor_pack), staged into LDS once per launch:
 * per layer l = 0..n_hidden (the last one the 6-row output layer, padded to 32 rows), per 32-row
 * tile T, per k-step S (2 for layer 0, whose in_dim inputs are padded to 32; width[l-1] / 16 after),
 * 64 lane fragments of 8 bf16 (16 B each): fragment (T, S, lane) starts at byte
 * w_off[l] + ((T * ksteps + S) * 64 + lane) * 16, w_off[0] = 0, the layers back to back; its element
 * j is bf16(W[l][32 T + (lane & 31)][k]) (0 past the matrix) with, for h = lane >> 5,
 *     layer 0:  k = 16 S + 8 h + j
 *     others:   k = 32 (S >> 1) + 16 (S & 1) + 8 (j >> 2) + 4 h + (j & 3)
 * (the order in which the matrix cores hand a layer's result to the next).  The f32 biases follow
 * the last fragment, layer after layer, each padded with zeros to its whole 32-row tiles.
 * [128,128,128] packs to 81 920 B of weights + 1 664 B of biases, the largest network supported. */
#define CTR_ACTOR_MAX_HIDDEN 3
#define CTR_ACTOR_MAX_WIDTH  256
#define CTR_ACTOR_MAX_BYTES  98304
typedef struct ctr_actor_t {
    int32_t in_dim;                 /* obs_dim + 6: 19 or 20                         */
    int32_t n_hidden;               /* 1..CTR_ACTOR_MAX_HIDDEN                       */
    int32_t width[CTR_ACTOR_MAX_HIDDEN]; /* multiples of 32, <= CTR_ACTOR_MAX_WIDTH  */
    int32_t pad;
    float   scale[6];               /* finite                                        */
    const void *blob;               /* device, 16-B aligned, ctr_actor_blob_bytes()  */
} ctr_actor_t;

/* Bytes of the packed blob; -1 on a refused shape (ctr_last_error: which, with the byte counts
 * where the network exceeds CTR_ACTOR_MAX_BYTES).  scale and blob are not read. */
int64_t ctr_actor_blob_bytes(const ctr_actor_t *a);
/* Host only, no HIP call: row-major f32 W[l] [out][in], b[l] [out] (l = 0..n_hidden, the last one
 * the 6-row output layer) -> the packed blob in host memory, which the caller copies to the
 * device.  The weights are rounded to bf16 here, once.  scale and blob are not read. */
int ctr_actor_pack(const ctr_actor_t *a, const float *const *W, const float *const *b, void *blob_host);
/* The device-side ctr_actor_pack: W[l] / b[l] (l = 0..n_hidden) are DEVICE pointers to contiguous
 * float32 [out, in] weights and [out] biases; a->blob (device, 16-B aligned, ctr_actor_blob_bytes())
 * is overwritten with the same bytes ctr_actor_pack would give for those values, padding included.
 * One launch on `stream`, nothing read back, no allocation: it can be captured into a graph, and a
 * replay packs whatever the parameters hold then.  The caller orders it against launches that read
 * the blob (the same stream does).  scale is not read.  (Added within ABI 17.) */
int ctr_actor_load(const ctr_actor_t *a, const float *const *W, const float *const *b, void *stream);
/* rows [n][in_dim] f32 -> actions [n][6] f32; logits [n][6] (the pre-tanh y) or NULL.  (device) */
int ctr_actor(const ctr_actor_t *a, const float *rows, int64_t n, float *actions, float *logits, void *stream);

/* Closed-loop ctr_step_many: k steps in one launch, each step's action computed by the actor from
 * the observation the step before left.  Afterwards the batch, the outputs, the pool and the refill
 * queue are exactly what k rounds of
 *     row = [(float)out->obs, (float)batch->achieved_goal, (float)batch->desired_goal]
 *     ctr_actor(actor, row, ...);  ctr_step(cfg, batch, actions, out, autoreset, ...)
 * with batch->work_parity toggled after every step would have left, bit for bit.  The caller
 * promises that out->obs holds the batch's current observation (the last call on the batch was
 * ctr_reset, ctr_step* or ctr_rollout).  The blob is staged into LDS once; no wave waits for another
 * after that.  aux (NULL, or any of its pointers NULL: not wanted) records the actions and
 * accumulates per-env episode statistics: each env's lane adds to its own row in every step the
 * env is done in.
 * Refused (CTR_EINVAL, before any HIP call) wherever ctr_step_many is, with its messages; when
 * actor->in_dim != obs_dim + 6; for a refused actor; for the statistics arrays without
 * CTR_AUTORESET_POOLED (a done env would stay done and be counted at every step); and when the
 * blob, the kernel's static LDS and the domain-randomisation tables together exceed the 160 KB of
 * LDS of a workgroup (the message has the byte counts: use ctr_actor + ctr_step there).  n = 0
 * is a no-op. */
typedef struct ctr_rollout_aux_t {   /* every pointer device, or NULL */
    float    *actions;      /* [k][n][6] the action applied in each step                    */
    uint32_t *episodes;     /* [n] += 1 at every step the env is done in                    */
    uint32_t *successes;    /* [n] += success of that step                                   */
    double   *error_sum;    /* [n] += (double)error of that step (the f32 `error` output)    */
    uint32_t *length_sum;   /* [n] += t of the terminal step                                 */
} ctr_rollout_aux_t;
int ctr_rollout(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const ctr_actor_t *actor, int32_t k,
                const ctr_step_out_t *out, int32_t autoreset, const ctr_rollout_aux_t *aux, void *stream);

/* ---------------------------------------------------------------------------------------
 * Exploration noise and data collection (entry points added within ABI 17: no existing entry point
 * or struct changes, so the number stays; a caller that needs them looks the symbols up).
 *
 * The reference trains with stable-baselines HER + DDPG: Gaussian action noise, clipped to the box
 * (clip(action + NormalActionNoise, -1, 1) in the normalised box, rescaled), and with probability
 * random_exploration a uniformly random action (action_space.sample()) instead of the policy's.
 * Here an env's six actions are perturbed as a pure function of (explore->seed, the global env id
 * genv = batch->env_base + e, the env's reset number `epoch`, its clock t before the step): not of
 * the launch, the lane, the shard, or of how the steps are cut into launches.
 *   draws   two Philox4x32-10 blocks blk = 0, 1 of stream 6: counter {t | blk << 16, epoch,
 *           (uint32)genv, (uint32)(genv >> 32) ^ (6u << 24)}, key {(uint32)seed, (uint32)(seed >> 32)};
 *           their words w0..w3 | w4..w7; u_i = (float)(w_i >> 8) * 2^-24 (exact in f32, in [0, 1));
 *           w7 is not used
 *   random  if u6 < random_eps (f32):  a_i = scale_i * (2 u_i - 1), i = 0..5 (2 u_i - 1 is exact, so
 *           one f32 rounding, the product's)
 *   else    (z_2j, z_2j+1) = sqrtf(-2 logf(1 - u_2j)) * (cosf, sinf)(2 pi u_2j+1), j = 0..2 (Box-Muller;
 *           1 - u is exact and in (0, 1]; 2 pi u = 6.2831855f * u, one f32 product)
 *           a_i = min(max(fmaf(sigma_i * |scale_i|, z_i, a_i), -|scale_i|), |scale_i|)
 *           (sigma_i * |scale_i| one f32 product, then ONE fused multiply-add; all f32)
 *   no-op   sigma all zero and random_eps zero: the actions keep their bits (nothing is computed)
 * logf, sinf, cosf and sqrtf are the device library's f32 functions: the Gaussian branch matches a
 * float64 restatement to their error, the random branch and the choice between the two bit for bit. */
typedef struct ctr_explore_t {
    uint64_t seed;              /* the noise stream's key                                       */
    float    sigma[6];          /* finite, >= 0: the Gaussian's std in units of |scale_i|       */
    float    random_eps;        /* in [0, 1]: probability of a uniformly random action          */
    int32_t  pad;
} ctr_explore_t;

/* actions [n][6] f32 (device), perturbed in place with the batch's current t, epoch and env_base:
 * what ctr_collect applies inside its kernel, as a launch of its own (for use with ctr_step*).
 * Refused (CTR_EINVAL, before any HIP call): NULL arguments where n > 0, a non-finite or negative
 * sigma, random_eps outside [0, 1], a non-finite scale. */
int ctr_explore(const ctr_batch_t *batch, const ctr_explore_t *explore, const float *scale, float *actions,
                void *stream);

/* ctr_rollout that collects training data: every step's action is perturbed by `explore` (NULL: no
 * noise, the branch is skipped wave-uniformly) with actor->scale as the box, and every transition
 * is recorded into the HER store as ctr_step_her records it.  Afterwards the batch, the outputs,
 * the pool, the refill queue, every buffer of the HER store, aux->actions (the applied, noisy
 * actions) and the statistics are exactly what k rounds of
 *     ctr_actor(actor, row, ...);  ctr_explore(batch, explore, actor->scale, actions, ...);
 *     ctr_step_her(cfg, batch, actions, out, autoreset, her, ...)
 * with batch->work_parity toggled after every step would have left, bit for bit.
 * Refused (CTR_EINVAL, before any HIP call) wherever ctr_rollout is, with its messages (so also
 * for the compliant model's scipy RK45 with a y pre-curvature, whose kernel would spill, and for
 * the lane-pair and 8-lane group modes); where ctr_step_her is (a NULL or malformed store,
 * her->t_max != cfg->max_steps, her->n or her->env_base different from the batch's); and where
 * ctr_explore is. */
int ctr_collect(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const ctr_actor_t *actor,
                const ctr_explore_t *explore, const ctr_her_t *her, int32_t k, const ctr_step_out_t *out,
                int32_t autoreset, const ctr_rollout_aux_t *aux, void *stream);

/* ctr_collect for SAC (a symbol added within ABI 17: no existing entry point or struct changes):
 * every step's action is the tanh-Gaussian policy's own sample ("SAC" below: ctr_gauss_act), and
 * there is no ctr_explore_t, the policy's noise being the exploration.  `policy` is the 12-row blob
 * of ctr_gauss_pack / ctr_gauss_load with its action box in scale; seed is the noise key and counter
 * the draw of the call's first step.  Afterwards the batch, the outputs, the pool, the refill queue,
 * every buffer of the HER store, aux->actions (the applied actions) and the statistics are exactly
 * what k rounds i = 0..k-1 of
 *     ctr_gauss_act(policy, row, n, seed, counter + i, batch->env_base, 0, actions, NULL, NULL, NULL, ...);
 *     ctr_step_her(cfg, batch, actions, out, autoreset, her, ...)
 * with `row` the environments' flat rows [observation, achieved_goal, desired_goal] before the step
 * and batch->work_parity toggled after every step would have left, bit for bit.  counter + i is a
 * 64-bit sum (modulo 2^64) whose low and high halves are the noise counter's words, and the row word
 * is the global env id batch->env_base + e: an env's action in a step is a pure function of its
 * row, the weights and (seed, counter + i, global env id), not of the launch, the lane, the shard
 * or of how the steps are cut into calls.  One launch; nothing is read back or allocated, so it can
 * be captured into a graph.  There is no deterministic flag: ctr_collect with explore = NULL and
 * the 6-row actor built from the head's first six rows already is the deterministic policy, bit for
 * bit.
 * Refused (CTR_EINVAL, before any HIP call, ctr_last_error names ctr_collect_gauss): wherever
 * ctr_rollout is, with the policy's shape judged as ctr_gauss_act judges it (the blob has the 6-row
 * actor's size, so the LDS budget and its message are ctr_rollout's; the compliant model's scipy
 * RK45 with a y pre-curvature, whose kernel would spill to scratch, is refused by name: use
 * ctr_gauss_act + ctr_step_her there); where ctr_step_her is (a NULL or malformed store,
 * her->t_max != cfg->max_steps, her->n or her->env_base different from the batch's);
 * batch->env_base < 0 or batch->env_base + n above 2^32 (the env id is the key's 32-bit row word,
 * as ctr_gauss_act's row_base + row).  n = 0 is a no-op. */
int ctr_collect_gauss(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const ctr_actor_t *policy,
                      uint64_t seed, uint64_t counter, const ctr_her_t *her, int32_t k,
                      const ctr_step_out_t *out, int32_t autoreset, const ctr_rollout_aux_t *aux, void *stream);

/* ---------------------------------------------------------------------------------------
 * Retargeting and waypoint following (entry points added within ABI 17: no existing entry point or
 * struct changes, so the number stays; a caller that needs them looks the symbols up).  The policy
 * side of the reference's line / circle / helix path comparisons of src/, whose IK side is
 * ctr_ik_dls.
 *
 * ctr_set_goal: a new desired goal for the environments with mask[e] != 0 (mask NULL = all), the
 * joints kept (ctr_reset with a goal draws them anew).  For each such env
 *     batch->desired_goal[e][k] = goal[e][k]                                    (k = 0..2, f64)
 *     obs[e][9 + k]             = goal[e][k] - batch->achieved_goal[e][k]
 * one f64 subtraction each, stored as every observation is: rounded once to f32, or kept as f64
 * with cfg->obs_f64.  Nothing else changes: not the joints, t, epoch, system, the other observation
 * slots, the reward / done / success / error rows or the pool.  goal [n][3] f64, obs [n][obs_dim]
 * (device).  Refused (CTR_EINVAL, before any HIP call): a NULL argument other than mask, a
 * missing batch buffer, a batch size out of range.  n = 0 is a no-op. */
int ctr_set_goal(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const uint8_t *mask, const double *goal,
                 void *obs, void *stream);

/* ctr_follow: ctr_rollout (CTR_AUTORESET_OFF, no statistics) in which every env walks its own list
 * of K waypoints.  Per-env state: the cursor c (the waypoint the env is on, K = past the end) and
 * held (steps spent on waypoint c); both read when the launch starts and written back, so launches
 * chain.  Each env, on each of the k steps:
 *   1. if c < K and held == 0: the env is retargeted to waypoints[c][e] as ctr_set_goal does it
 *      (the desired_goal row and observation slots 9..11 are stored); the actor's row of this step
 *      has (float)(g - ag) in slots 9..11 and (float)g in its goal slots
 *   2. a = actor(row), then the step, exactly as ctr_rollout takes it with CTR_AUTORESET_OFF
 *   3. if c < K: held += 1; the env advances if held >= hold, or if reach is set and the step's
 *      success is set.  On an advance tip[c][e] = achieved goal (3 x f64), err[c][e] = the step's
 *      f32 error, steps[c][e] = held, reached[c][e] = success; then c += 1, held = 0
 *   4. an env with c == K keeps stepping towards its last waypoint and records nothing
 * Afterwards the batch, the step outputs, cursor, held, the four per-waypoint arrays and `actions`
 * are exactly what k rounds of
 *     ctr_set_goal(mask = (c < K && held == 0), goal = waypoints[c]);  ctr_actor(actor, row, ...);
 *     ctr_step(cfg, batch, actions, out, CTR_AUTORESET_OFF, ...);  the bookkeeping of 3.
 * would have left, bit for bit.  No auto-reset, no noise and no HER in a follow; entries of the
 * per-waypoint arrays whose waypoint no env left in this call are not written.
 * Refused (CTR_EINVAL, before any HIP call) wherever ctr_rollout is, with its messages (so also for
 * the compliant model's scipy RK45 with a y pre-curvature, for the lane-pair and 8-lane group modes,
 * with packed rows or the gather, on an in_dim mismatch and when the LDS does not suffice, with the
 * byte counts); for a NULL follow, waypoints, cursor or held; K < 1, hold < 1, reach not 0 or 1.
 * n = 0 is a no-op. */
typedef struct ctr_follow_t {
    const double *waypoints;    /* [K][n][3] device: env-minor, so a wave whose lanes share a    */
                                /* cursor loads one span                                         */
    int32_t K, hold, reach, pad;
    int32_t *cursor, *held;     /* [n] device, in and out; cursor in 0..K, held in 0..hold-1    */
    double  *tip;               /* [K][n][3] or NULL: the tip when the env left the waypoint     */
    float   *err;               /* [K][n]    or NULL: the f32 error of that step                 */
    int32_t *steps;             /* [K][n]    or NULL: the steps the env spent on the waypoint    */
    uint8_t *reached;           /* [K][n]    or NULL: that step's success                        */
} ctr_follow_t;
int ctr_follow(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const ctr_actor_t *actor,
               const ctr_follow_t *follow, int32_t k, const ctr_step_out_t *out,
               float *actions /* [k][n][6] or NULL */, void *stream);

/* ---------------------------------------------------------------------------------------
 * MLP critic and the TD target (entry points added within ABI 17: no existing entry point or struct
 * changes, so the number stays; a caller that needs them looks the symbols up).  The Q-network of
 * the reference's stable-baselines DDPG on x = [row, a] (in_dim = obs_dim + 12 floats): row is
 * HERGoalEnvWrapper's flat row [observation, achieved_goal, desired_goal] (the layout of
 * ctr_her_batch_t.obs) and a the six actions in the normalised box [-1, 1], as that critic sees
 * them (the caller divides by the action scale; no entry point here applies one).  The arithmetic
 * is the actor's, with a one-row output layer and no tanh:
 *     x_hi = bf16(x);  x_lo = bf16(x - float(x_hi))        (round to nearest even; x - x_hi in f32)
 *     h1   = bf16(relu(W1 x_hi + W1 x_lo + b1))            (bf16 weights, f32 accumulation, f32 bias)
 *     hl   = bf16(relu(Wl h(l-1) + bl))                    the further hidden layers
 *     q    = Wout hL + bout                                f32
 * A row's q depends on that row and the weights only.  The blob's layout is exactly the actor's
 * ("MLP actor" above): the same fragment order, layer 0 with 2 k-steps over the in_dim inputs
 * padded to 32, the biases behind the fragments, each padded to whole 32-row tiles; the output
 * layer has 1 row where the actor has 6.  The byte limit is CTR_ACTOR_MAX_BYTES. */
typedef struct ctr_critic_t {
    int32_t in_dim;                       /* obs_dim + 12: 25 or 26                        */
    int32_t n_hidden;                     /* 1..CTR_ACTOR_MAX_HIDDEN                       */
    int32_t width[CTR_ACTOR_MAX_HIDDEN];  /* multiples of 32, <= CTR_ACTOR_MAX_WIDTH       */
    int32_t pad;
    const void *blob;                     /* device, 16-B aligned, ctr_critic_blob_bytes() */
} ctr_critic_t;
/* As ctr_actor_blob_bytes, ctr_actor_pack (host only) and ctr_actor_load (one launch that writes
 * every byte of c->blob, padding included) are for the actor; the last layer is the 1-row output
 * layer.  ctr_critic_blob_bytes and ctr_critic_pack do not read blob. */
int64_t ctr_critic_blob_bytes(const ctr_critic_t *c);
int ctr_critic_pack(const ctr_critic_t *c, const float *const *W, const float *const *b, void *blob_host);
int ctr_critic_load(const ctr_critic_t *c, const float *const *W, const float *const *b, void *stream);
/* rows [n][in_dim - 6] f32, actions [n][6] f32 -> q [n] f32.  (device)  Refused (CTR_EINVAL, before
 * any HIP call): a refused shape, a NULL or misaligned blob, n out of range, a NULL array where
 * n > 0.  n = 0 is a no-op. */
int ctr_critic(const ctr_critic_t *c, const float *rows, const float *actions, int64_t n, float *q, void *stream);

/* ctr_her_sample that also hands the learner the DDPG target of the rows it drew.  It writes
 * everything ctr_her_sample writes for the same (her, batch_size, seed, counter), bit for bit, and
 * in the same launch, for each sampled row,
 *     a'     = tanhf(y),  y = the target policy's logits on the f32 row stored to out->next_obs
 *                         (ctr_actor's arithmetic; actor->scale is not read)
 *     q      = critic([next_obs row, a'])                  (ctr_critic's arithmetic)
 *     target = done != 0 ? reward : (gamma * q) + reward   (two f32 roundings, no fused multiply-add)
 * A zero row (empty store: index slot -1) goes through the networks like any other row.  The two
 * blobs take turns in one LDS region beside the sampler's row staging, so every supported actor
 * works with every supported critic.  Three launches (the sampler's two scans, then this kernel);
 * stream-ordered, nothing allocated, nothing read back.
 * Refused (CTR_EINVAL, before any HIP call): whatever ctr_her_sample refuses; a NULL td or
 * td->target; a refused actor or critic; actor->in_dim != her->obs_dim + 6; critic->in_dim !=
 * her->obs_dim + 12; a non-finite gamma.  batch_size = 0 is a no-op. */
typedef struct ctr_her_td_t {
    const ctr_actor_t  *actor;    /* target policy; its scale is not read                  */
    const ctr_critic_t *critic;   /* target critic                                         */
    float   gamma;                /* finite                                                */
    int32_t pad;
    float  *target;               /* [B] device, required                                  */
    float  *q_next;               /* [B] or NULL: Q'(s', pi'(s'))                          */
    float  *next_action;          /* [B][6] or NULL: pi'(s') = tanhf(y), in [-1, 1]        */
} ctr_her_td_t;
int ctr_her_sample_td(const ctr_her_t *her, int64_t batch_size, uint64_t seed, uint64_t counter,
                      const ctr_her_batch_t *out, const ctr_her_td_t *td, void *stream);

/* TD3: ctr_her_sample_td with the clipped double-Q target on a smoothed target action (added within
 * ABI 17: a new symbol, no entry point or struct changes).  It writes everything ctr_her_sample
 * writes for the same (her, batch_size, seed, counter), bit for bit, and in the same launch, for row
 * i of the batch,
 *     a'     = tanhf(y)                                    as ctr_her_sample_td
 *     e_k    = fminf(fmaxf(sigma * z_k, -clip), clip)      (one f32 product)
 *     a''_k  = fminf(fmaxf(a'_k + e_k, -1), 1)             (one f32 sum)
 *     q1, q2 = critic1([next_obs row, a'']), critic2([next_obs row, a''])     (ctr_critic's arithmetic)
 *     target = done != 0 ? reward : (gamma * fminf(q1, q2)) + reward          (two f32 roundings)
 * The smoothing noise z_0..z_5 is a pure function of (seed, counter, i), like the row draw (it does
 * not depend on batch_size, the lane or the workgroup): two Philox4x32-10 blocks blk = 0, 1 of
 * stream 7, counter {blk, (uint32)counter, (uint32)i, (uint32)(counter >> 32) ^ (7u << 24)}, key
 * {(uint32)seed, (uint32)(seed >> 32)}; the uniforms u0..u5 from the words w0..w3 | w4, w5 and the
 * Gaussians z from the uniforms exactly as under "Exploration noise" above (u = (float)(w >> 8) *
 * 2^-24; r = sqrtf(-2 logf(1 - u_2j)), z_2j = r cosf(t), z_2j+1 = r sinf(t), t = 6.2831855f *
 * u_2j+1; every product one f32 rounding).  sigma == 0 is a no-op: a'' = a' with its bits, and
 * nothing is drawn.  clip = INFINITY: the noise is not clipped.
 * The three blobs take turns in one LDS region beside the sampler's row staging, which is sized for
 * the largest of them, so every supported actor works with every two supported critics; critic1
 * and critic2 may be the same struct or blob.  Three launches (the sampler's two scans, then this
 * kernel); stream-ordered, nothing allocated, nothing read back.
 * Refused (CTR_EINVAL, before any HIP call, ctr_last_error names ctr_her_sample_td3): whatever
 * ctr_her_sample_td refuses, of actor, critic1 and critic2; a NULL td or td->target; a non-finite
 * gamma; a sigma that is not finite or negative; a clip that is NaN or negative.  batch_size = 0 is
 * a no-op. */
typedef struct ctr_her_td3_t {
    const ctr_actor_t  *actor;     /* target policy; its scale is not read                  */
    const ctr_critic_t *critic1;   /* target critics; they may be the same struct / blob    */
    const ctr_critic_t *critic2;
    float   gamma;                 /* finite                                                */
    float   sigma;                 /* finite, >= 0: std of the smoothing noise, in the normalised box */
    float   clip;                  /* >= 0, not NaN; INFINITY = the noise is not clipped    */
    int32_t pad;
    float  *target;                /* [B] device, required                                  */
    float  *q1_next, *q2_next;     /* [B] or NULL                                           */
    float  *next_action;           /* [B][6] or NULL: the SMOOTHED target action a''        */
} ctr_her_td3_t;
int ctr_her_sample_td3(const ctr_her_t *her, int64_t batch_size, uint64_t seed, uint64_t counter,
                       const ctr_her_batch_t *out, const ctr_her_td3_t *td, void *stream);

/* ---------------------------------------------------------------------------------------
 * The soft (Polyak) update of target networks and the refresh of their blobs, in one launch for up
 * to CTR_POLYAK_MAX_NETS networks (added within ABI 17: a new symbol, no entry point or struct
 * changes).  For every element of every target tensor, with p the online value and t the target's,
 *     tau <  0.5:  t' = t + tau * (p - t)
 *     otherwise:   t' = p - (p - t) * (1 - tau)
 * (torch.lerp's formula), every operation rounded to f32 and no fused multiply-add, so a float32
 * restatement in numpy gives the same bits.  t' is stored over t, and the net's blob is overwritten
 * with the bytes ctr_actor_pack / ctr_critic_pack would give for the new target parameters, padding
 * included: ctr_actor_load / ctr_critic_load of the updated targets, without their launches.  At
 * tau == 1 the formula gives t' = p exactly wherever p - t is finite and p is not -0 (the product
 * is then a zero, and only -0 changes when a zero is subtracted from it); at tau == 0 it likewise
 * gives t wherever p - t is finite and t is not -0.
 * The mapping is ctr_actor_load's: one thread per 16 B of a blob owns the eight weights or four
 * bias floats that item packs.  The fragment layout covers each (row, k) of a layer once, so each
 * target element is read and written by exactly one thread and the update in place needs no
 * ordering inside the launch; the online tensors are only read.  One launch on `stream`, nothing
 * read back, no allocation: it can be captured into a graph.
 * Refused (CTR_EINVAL, before any HIP call, ctr_last_error names ctr_polyak): nets NULL; n_nets
 * outside 1..CTR_POLYAK_MAX_NETS; a net with both or neither of actor / critic; a shape, scale or
 * blob that ctr_actor / ctr_critic would refuse; a NULL pointer array or a NULL layer in
 * 0..n_hidden; W[l] == W_targ[l] or b[l] == b_targ[l] (online and target are the same tensor); two
 * nets with the same blob; tau NaN or outside [0, 1]. */
#define CTR_POLYAK_MAX_NETS 4
typedef struct ctr_polyak_net_t {
    const ctr_actor_t  *actor;      /* exactly one of actor / critic is non-NULL: the   */
    const ctr_critic_t *critic;     /* TARGET network's shape and its device blob        */
    const float *const *W;          /* online parameters, device, [n_hidden + 1] layers  */
    const float *const *b;
    float *const *W_targ;           /* target parameters (the f32 masters), device,      */
    float *const *b_targ;           /* updated in place                                   */
} ctr_polyak_net_t;
int ctr_polyak(const ctr_polyak_net_t *nets, int32_t n_nets, float tau, void *stream);

/* ---------------------------------------------------------------------------------------
 * DDPG's two updates on the learner's float32 parameters (added within ABI 17: new symbols, no
 * entry point or struct changes).  The networks are the actor's and the critic's shapes ("MLP
 * actor", "MLP critic" above: only in_dim, n_hidden and width are read; scale and blob are not),
 * but here every value is float32: relu(z) = z > 0 ? z : 0 between the layers, the products on the
 * f32-in / f32-accumulate matrix instructions (chains of fmaf in a fixed order).
 *
 * ctr_ddpg_critic_step: rows [B][in_dim - 6], actions [B][6], target [B] (device).  With scale
 * (device [6]) the critic sees actions[i][j] / scale[j], one f32 division; NULL: the actions are
 * normalised already.
 *     q_i = Q([row_i, a_i]);  loss = sum_i (q_i - target_i)^2 * (1/B);  dL/dq_i = (q_i - target_i) * (2/B)
 * ctr_ddpg_actor_step: rows [B][in_dim] of the actor (device); critic_W / critic_b the critic's
 * current float32 parameters (device, [n_hidden + 1] layers), read only.
 *     a_i = (float)tanh(policy logits);  q_i = Q([row_i, a_i]);  loss = sum_i q_i * (-1/B);  dL/dq_i = -1/B
 * and backward through the critic to its six action inputs only, through 1 - a^2, through the policy
 * (actor->scale is not read).
 * Either call writes the gradient of every W[l], b[l] of its network whole to gW[l], gb[l], the
 * loss to *loss (device, or NULL), and then makes one Adam step on W, b in place with the state mW,
 * mb, vW, vb (every tensor of its parameter's shape) and pow = {beta1^t, beta2^t} (device float[2],
 * {1, 1} before the first step), every operation rounded to f32, no fused multiply-add, division
 * and sqrtf correctly rounded:
 *     pow1' = pow1 * beta1;  pow2' = pow2 * beta2
 *     m' = (beta1 * m) + ((1 - beta1) * g)
 *     v' = (beta2 * v) + (((1 - beta2) * g) * g)
 *     p' = p - lr * ((m' / (1 - pow1')) / (sqrtf(v' / (1 - pow2')) + eps))
 * so a float32 restatement in numpy of the step from the stored gradients gives the same bits.
 *
 * Two launches on `stream`: the first takes tiles of 16 rows, one workgroup per slot (at most 64
 * slots; slot s takes tiles s, s + slots, ...), keeps a tile's activations in LDS between forward
 * and backward and sums its tiles' gradients into its slot of the workspace; it also advances pow
 * into the workspace.  The second sums the slots in slot order per parameter, stores the gradient,
 * applies Adam with the advanced pow and stores that to pow.  No atomics, no workgroup waits for
 * another, the order of every sum depends on the shapes and B only: the same inputs give the same
 * bits.  (The two sums over rows whose terms cancel, the loss and the bias gradients, and the
 * policy's tanh run in f64 and are rounded to f32 once; everything else is f32.)  Nothing is allocated or read back; both
 * calls can be captured into a graph.  Every shape
 * that ctr_actor / ctr_critic accept fits (107 KB of LDS for the widest actor with the widest
 * critic).  B is 1..65 536; B = 0 is a no-op.
 * workspace: device, 16-B aligned, ctr_ddpg_workspace_bytes(actor, critic, max_B) bytes serve both
 * calls for every B <= max_B (-1 on a refused shape or max_B outside 1..65 536); the calls may
 * share it (they are stream-ordered).
 * Refused (CTR_EINVAL, before any HIP call, ctr_last_error names the function): a NULL struct; a
 * shape ctr_actor / ctr_critic refuse; actor->in_dim + 6 != critic->in_dim; a NULL pointer array,
 * pow or layer in 0..n_hidden; a gradient or state tensor (or pow) that is a parameter tensor;
 * workspace NULL, misaligned or too small for B; lr, beta1, beta2 or eps not finite; a beta
 * outside [0, 1); eps <= 0; B outside 0..65 536; a NULL batch array where B > 0. */
typedef struct ctr_ddpg_net_t {
    float *const *W;                /* parameters (the f32 masters), device, [n_hidden + 1]  */
    float *const *b;                /* layers, updated in place                              */
    float *const *gW;               /* gradients, written whole                              */
    float *const *gb;
    float *const *mW;               /* Adam's first moments                                  */
    float *const *mb;
    float *const *vW;               /* Adam's second moments                                 */
    float *const *vb;
    float *pow;                     /* device float[2]: beta1^t, beta2^t                     */
} ctr_ddpg_net_t;
typedef struct ctr_ddpg_adam_t {
    float lr, beta1, beta2, eps;
} ctr_ddpg_adam_t;
int64_t ctr_ddpg_workspace_bytes(const ctr_actor_t *actor, const ctr_critic_t *critic, int64_t max_B);
int ctr_ddpg_critic_step(const ctr_critic_t *critic, const ctr_ddpg_net_t *net, const ctr_ddpg_adam_t *adam,
                         const float *rows, const float *actions, const float *scale, const float *target, int64_t B,
                         float *loss, void *workspace, int64_t workspace_bytes, void *stream);
int ctr_ddpg_actor_step(const ctr_actor_t *actor, const ctr_ddpg_net_t *net, const ctr_ddpg_adam_t *adam,
                        const ctr_critic_t *critic, const float *const *critic_W, const float *const *critic_b,
                        const float *rows, int64_t B, float *loss, void *workspace, int64_t workspace_bytes, void *stream);

/* TD3's twin critics: ctr_ddpg_critic_step on critic[0] / net[0] and on critic[1] / net[1], on the
 * same rows, actions, scale and target and with the same Adam constants, in the two launches of one
 * such call (added within ABI 17: new symbols).  The grids get a second dimension and plane y works
 * on critic y, with ctr_ddpg_critic_step's arithmetic, tile-to-slot dealing and summation order:
 * every tensor of both nets (parameters, gradients, m, v, pow) and loss[0], loss[1] (device
 * float[2], or NULL) are what the two ctr_ddpg_critic_step calls leave, bit for bit.  The critics
 * may have different hidden shapes (one in_dim).
 * workspace: critic[0]'s region, laid out as ctr_ddpg_critic_step lays it out for this B, then
 * critic[1]'s behind it (a region is a multiple of 16 B).  ctr_td3_workspace_bytes(actor, critic1,
 * critic2, max_B) is the larger of the two regions' sum at max_B and what ctr_ddpg_actor_step
 * needs, so one workspace serves a whole TD3 learner (-1 on a refused shape or max_B outside
 * 1..65 536).
 * Refused (CTR_EINVAL, before any HIP call, ctr_last_error names the function): whatever
 * ctr_ddpg_critic_step refuses for either net; a NULL array or array entry; critics of different
 * in_dim; the two nets sharing any W, b, gradient, state or pow tensor (the planes would race). */
int64_t ctr_td3_workspace_bytes(const ctr_actor_t *actor, const ctr_critic_t *critic1,
                                const ctr_critic_t *critic2, int64_t max_B);
int ctr_td3_critic_step(const ctr_critic_t *const critic[2], const ctr_ddpg_net_t *const net[2],
                        const ctr_ddpg_adam_t *adam, const float *rows, const float *actions,
                        const float *scale, const float *target, int64_t B,
                        float *loss /* device float[2] or NULL */,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * SAC (added within ABI 17: new symbols, no entry point or struct changes): a tanh-Gaussian policy
 * on the device and the policy's update under two critics with a learned temperature.  The critics'
 * regression is ctr_td3_critic_step, the target critics are ctr_critic, the soft update ctr_polyak.
 *
 * The Gaussian policy is the "MLP actor" above -- the same ctr_actor_t, limits, blob format and
 * bf16 arithmetic -- with a 12-row output layer and no tanh on it: rows 0..5 are the mean, rows
 * 6..11 the log standard deviation before clipping.  ctr_gauss_blob_bytes / ctr_gauss_pack (host) /
 * ctr_gauss_load (device) are ctr_actor_blob_bytes / _pack / _load for W[n_hidden] [12][width] and
 * b[n_hidden] [12]; the blob has the 6-row actor's size, and equals the blob of the actor built
 * from the first six rows except in the bytes that hold rows 6..11.
 *
 * ctr_gauss_act: rows [n][in_dim] f32 (device) -> actions [n][6], unit [n][6], logp [n],
 * logits [n][12] (device; each may be NULL).  In f32, every operation rounded once, no contraction:
 *     y[0..11] = the head's f32 outputs (bias added: ctr_actor's logits of a 12-row layer)
 *     s_i      = fminf(fmaxf(y[6+i], -20), 2)
 *     eps_i    = six standard normals from two Philox4x32-10 blocks of stream 8, key = seed, counter
 *                words {blk, (u32)counter, (u32)(row_base + row), (u32)(counter >> 32) ^ (8u << 24)},
 *                blk = 0, 1: uniforms v_k = (word >> 8) * 2^-24 from words 0..3 of block 0 and 0..1
 *                of block 1; for j = 0..2: r = sqrtf(-2 * logf(1 - v_2j)),
 *                (sn, cs) = sincosf(6.2831855f * v_(2j+1)), eps_2j = r * cs, eps_(2j+1) = r * sn
 *                (ctr_her_sample_td3's draw on another stream)
 *     u_i      = fmaf(expf(s_i), eps_i, y[i]);  t_i = tanhf(u_i)
 *     unit_i   = t_i;  action_i = scale_i * t_i
 *     softplus(x) = fmaxf(x, 0) + log1pf(expf(-fabsf(x)))
 *     logp     = sum over i = 0..5, in that order, of
 *                ((-0.5f * (eps_i * eps_i) - s_i) - 0.9189385f) - 2 * ((0.6931472f - u_i) - softplus(-2 * u_i))
 * deterministic != 0: u_i = y[i] and eps_i = 0 in logp; nothing is drawn.  A row's results are a
 * pure function of the row, the weights and (seed, counter, row_base + row): they do not depend on
 * n, on the other rows or on how a batch is split into calls.  One launch, nothing read back or
 * allocated (it can be captured into a graph).  rows 0..5 of logits are ctr_actor's logits of the
 * 6-row actor built from the first six rows, bit for bit, and the deterministic action is its action.
 * Refused (CTR_EINVAL, before any HIP call): a NULL actor, a shape ctr_actor refuses, a scale that
 * is not finite, a NULL or misaligned blob, n outside 0..2^31 - 1, row_base < 0 or row_base + n
 * above 2^32, rows NULL where n > 0.
 *
 * ctr_sac_actor_step: one step of the policy (ctr_ddpg_net_t of the 12-row network) on rows
 * [B][in_dim] under the two critics' current f32 parameters critic_W[y], critic_b[y], read only.
 * The networks run in f32 as in ctr_ddpg_actor_step; eps is ctr_gauss_act's draw for (seed,
 * counter, row) with row_base 0; the head between the policy and the critics runs in f64 on the f32
 * logits and eps and is rounded to f32 where it meets the networks (the action t_i, the gradient
 * of the logits):
 *     alpha = exp(*log_alpha), read when the first launch starts
 *     s, u, t, logp as above;  q_j = Q_j([row, t])
 *     loss      = sum_r (alpha * logp_r - min(q_1r, q_2r)) * (1/B)         (a tie: critic 1)
 *     logp_mean = sum_r logp_r * (1/B)
 * backward: dL/dq = -1/B on the critic that gave the minimum and 0 on the other, through both
 * critics to their six action inputs, summed; with dt_i that sum,
 *     dL/du_i     = dt_i (1 - t_i^2) + (alpha/B) 2 t_i
 *     dL/dy[i]    = dL/du_i
 *     dL/dy[6+i]  = dL/du_i exp(s_i) eps_i - alpha/B     where -20 <= y[6+i] <= 2, else 0
 * then through the policy.  The gradients go to gW, gb, the loss to *loss, logp_mean to *logp_mean
 * (device, or NULL); the policy takes ctr_ddpg_actor_step's Adam step (tiles, slots, summation order
 * and the step's arithmetic are that call's).  The temperature: alpha_state->state is device
 * float[4] = {m, v, beta1^t, beta2^t} ({0, 0, 1, 1} before the first step); the gradient of
 * -log_alpha * (logp_mean + target_entropy), g = -(logp_mean + target_entropy) in f32, goes to
 * *alpha_state->grad (device, or NULL), and with learn != 0 *log_alpha takes the Adam step above
 * with alpha_state->lr and adam's beta1, beta2, eps; with learn == 0 log_alpha and state are not
 * written.  Two launches; the temperature's step is made by one thread of the second.
 * workspace: device, 16-B aligned; ctr_sac_workspace_bytes(actor, critic1, critic2, max_B) serves
 * this call and ctr_td3_critic_step on the same critics for every B <= max_B (-1 on a refused shape
 * or max_B outside 1..65 536).
 * LDS: a workgroup keeps one tile image of all three networks, 16 x (36 + sum (width + 4) + 20)
 * floats each.  Every trio whose blobs fit CTR_ACTOR_MAX_BYTES fits (the largest image, of hidden
 * [224, 64, 256], is 38.25 KB); a trio that did not would be refused with the byte counts in the
 * message.
 * Refused (CTR_EINVAL, before any HIP call, ctr_last_error names the function): whatever
 * ctr_ddpg_actor_step refuses for the policy's net; a NULL array, entry or layer; critics whose
 * in_dim is not actor->in_dim + 6; log_alpha, alpha_state or its state NULL; target_entropy or
 * alpha_state->lr not finite; a critic tensor that is a tensor of the policy's net or an output;
 * log_alpha, state, grad, loss, logp_mean, pow not distinct from each other, from the policy's
 * tensors and from rows; the LDS limit; B outside 0..65 536 (B = 0 is a no-op). */
typedef struct ctr_sac_alpha_t {
    float *state;                   /* device float[4]: m, v, beta1^t, beta2^t               */
    float *grad;                    /* device float, or NULL: the temperature's gradient     */
    float lr;
    int32_t learn;                  /* 0: log_alpha and state are never written              */
} ctr_sac_alpha_t;
int64_t ctr_gauss_blob_bytes(const ctr_actor_t *actor);
int ctr_gauss_pack(const ctr_actor_t *actor, const float *const *W, const float *const *b, void *blob_host);
int ctr_gauss_load(const ctr_actor_t *actor, const float *const *W, const float *const *b, void *stream);
int ctr_gauss_act(const ctr_actor_t *actor, const float *rows, int64_t n, uint64_t seed, uint64_t counter,
                  int64_t row_base, int32_t deterministic, float *actions, float *unit, float *logp,
                  float *logits, void *stream);
int64_t ctr_sac_workspace_bytes(const ctr_actor_t *actor, const ctr_critic_t *critic1,
                                const ctr_critic_t *critic2, int64_t max_B);
int ctr_sac_actor_step(const ctr_actor_t *actor, const ctr_ddpg_net_t *net, const ctr_ddpg_adam_t *adam,
                       const ctr_critic_t *const critic[2], const float *const *const critic_W[2],
                       const float *const *const critic_b[2], const float *rows, int64_t B, uint64_t seed,
                       uint64_t counter, float *log_alpha, const ctr_sac_alpha_t *alpha_state,
                       float target_entropy, float *loss, float *logp_mean, void *workspace,
                       int64_t workspace_bytes, void *stream);

/* ctr_her_sample_sac: ctr_her_sample with SAC's entropy-regularised target, as ctr_her_sample_td3
 * is with TD3's.  It writes everything ctr_her_sample writes for the same (her, batch_size, seed,
 * counter), bit for bit, and in the same launch, for row i of the batch,
 *     y[0..11]  = ctr_gauss_act's logits of the 12-row policy `actor` on the next_obs row
 *     eps       = ctr_gauss_act's draw for (seed, counter, row_base 0, row i)       (stream 8)
 *     t, logp   = ctr_gauss_act's head on y and eps, not deterministic
 *     q1, q2    = critic1([next_obs row, t]), critic2([next_obs row, t])     (ctr_critic's arithmetic)
 *     alpha     = (float)exp((double)*log_alpha)
 *     soft      = fminf(q1, q2) - alpha * logp                  (two f32 roundings, no contraction)
 *     target    = done != 0 ? reward : (gamma * soft) + reward  (two f32 roundings)
 * `actor` is the CURRENT policy (SAC has no target policy), critic1 and critic2 the target critics.
 * The noise key is the sampler's own (seed, counter): next_action and next_logp are the `unit` and
 * `logp` of the stand-alone ctr_gauss_act(actor, out->next_obs, batch_size, seed, counter, 0, 0,
 * ...), bit for bit.  A caller who keys the replay draws apart from the collection draws (as
 * HerReplayBuffer does: its draw seed is not the environments' seed) therefore needs no counter
 * offsets to keep the two from colliding.  *log_alpha is read on the device when the kernel runs,
 * never on the host: a captured graph sees the temperature of the replay.
 * The three blobs take turns in one LDS region beside the sampler's row staging, which is sized for
 * the largest of them, so every supported policy works with every two supported critics; critic1
 * and critic2 may be the same struct or blob.  Three launches (the sampler's two scans, then this
 * kernel); stream-ordered, nothing allocated, nothing read back.
 * Refused (CTR_EINVAL, before any HIP call, ctr_last_error names ctr_her_sample_sac): whatever
 * ctr_her_sample refuses (batch_size above 2^31 - 1 among it, so the row index fits the noise key's
 * 32-bit word); a NULL td, actor, critic1, critic2, log_alpha or target; a shape ctr_gauss_act or
 * ctr_critic refuses; a NULL or misaligned blob; actor->in_dim != her->obs_dim + 6; a critic's
 * in_dim != her->obs_dim + 12; a non-finite gamma.  batch_size = 0 is a no-op. */
typedef struct ctr_her_sac_t {
    const ctr_actor_t  *actor;      /* the CURRENT policy's 12-row blob (ctr_gauss_pack / _load); scale not read */
    const ctr_critic_t *critic1;    /* target critics; may be the same struct / blob */
    const ctr_critic_t *critic2;
    const float *log_alpha;         /* device, required: read by the kernel, never by the host */
    float   gamma;                  /* finite */
    int32_t pad;
    float  *target;                 /* [B] device, required */
    float  *q1_next, *q2_next;      /* [B] or NULL */
    float  *next_action;            /* [B][6] or NULL: t = tanhf(u), what the critics took (ctr_gauss_act's `unit`) */
    float  *next_logp;              /* [B] or NULL */
} ctr_her_sac_t;
int ctr_her_sample_sac(const ctr_her_t *her, int64_t batch_size, uint64_t seed, uint64_t counter,
                       const ctr_her_batch_t *out, const ctr_her_sac_t *td, void *stream);

/* ---------------------------------------------------------------------------------------
 * A run of SAC updates (added within ABI 17: a new symbol, no entry point or struct changes).
 * ctr_sac_update makes `updates` whole SAC updates on `stream`.  Update i (0-based) leaves, bit for
 * bit, in every tensor those calls write, what this sequence leaves:
 *     ctr_her_sample_sac(her, batch_size, draw_seed, draw_counter + i, batch,
 *                        {policy, critic_targ[0], critic_targ[1], log_alpha, gamma, target, q1_next, ...})
 *     ctr_td3_critic_step(critic, critic_net, critic_adam, batch->obs, batch->action, scale, target,
 *                         batch_size, critic_loss, workspace, ...)
 *     ctr_sac_actor_step(policy, policy_net, policy_adam, critic, the critics' W and b, batch->obs,
 *                        batch_size, seed, step_counter + i, log_alpha, alpha, target_entropy,
 *                        actor_loss, logp_mean, workspace, ...)
 *     ctr_gauss_load(policy, policy_net->W, policy_net->b)      (the blob the next draw's a' comes from)
 *     ctr_polyak({critic_targ[y], critic_net[y]->W, ->b, W_targ[y], b_targ[y]}, y = 0, 1; tau)
 * that is: the policy's and both critics' parameters, gradients, m, v and pow; log_alpha, its state
 * and its gradient; both target critics' float32 tensors; the three blobs; the batch and target
 * tensors (they hold the last update's draw); the four loss scalars (the last update's values).
 * Both counter sums are 64-bit and wrap, as ctr_collect_gauss's.  With history (device, [updates][5]
 * float32) row i also gets update i's critic 1 loss, critic 2 loss, actor loss, logp_mean and
 * log_alpha after its step (with alpha->learn == 0: the unchanged log_alpha).
 *
 * Launches: the sampler's two scans once per call (the call only reads the store, so the prefix
 * sums of update 0 are every update's), then five per update: the sampler's kernel, the twin
 * critics' gradient kernel and the policy's gradient kernel as the calls above launch them, and a
 * tail behind each gradient kernel.  A tail thread owns one 16-B item of a blob -- eight weights or
 * four bias floats, ctr_actor_load's and ctr_polyak's mapping, which covers every parameter once --
 * and for its elements sums the slots in slot order, stores the gradient and makes the Adam step
 * (what one thread per parameter did), then: the critics' tail (second grid dimension: the critic)
 * makes the soft update of the target with the new online value, stores it and packs the target's
 * blob item; the policy's tail packs the policy's blob item, and one of its threads makes the
 * temperature's step.  The soft update runs ahead of the policy's step: that step reads the online
 * critics, never the targets.  No allocation, no host read, no synchronisation: the call can be
 * captured into a graph (a replay repeats its draws: the counters are arguments).
 *
 * Refused (CTR_EINVAL, before any launch, ctr_last_error names ctr_sac_update): u NULL; updates < 0;
 * whatever the five calls above refuse (NULL structs, arrays and layers, shapes, the in_dim
 * relations to the store and between the networks, the LDS limit, tau NaN or outside [0, 1], a
 * non-finite gamma, rate or target_entropy, the betas and eps, the workspace NULL, misaligned or
 * smaller than ctr_sac_workspace_bytes for batch_size, batch_size outside 0..65 536); a target
 * critic whose shape differs from its online critic's; any two of these being the same pointer: a
 * parameter, gradient, state or pow tensor of the three networks, a target tensor, the three blobs,
 * log_alpha, its state and gradient, the loss outputs, the batch and target outputs, the workspace,
 * history, scale (so: every aliasing the calls above refuse, a target tensor or blob shared with an
 * online one or between the two targets); an output that starts inside history's updates * 20 bytes.
 * updates == 0 and batch_size == 0 are checked no-ops. */
typedef struct ctr_sac_update_t {
    /* the draw (ctr_her_sample_sac) */
    const ctr_her_t *her;
    int64_t  batch_size;
    uint64_t draw_seed, draw_counter;        /* update i draws under draw_counter + i                 */
    const ctr_her_batch_t *batch;
    float   *target;                         /* [B] device, required                                   */
    float   *q1_next, *q2_next;              /* [B] or NULL                                            */
    float   *next_action;                    /* [B][6] or NULL                                         */
    float   *next_logp;                      /* [B] or NULL                                            */
    float    gamma;
    float    tau;
    /* the policy: its 12-row shape and blob, its f32 masters and Adam state */
    const ctr_actor_t     *policy;
    const ctr_ddpg_net_t  *policy_net;
    const ctr_ddpg_adam_t *policy_adam;
    /* the critics (shapes; their blobs are not read), their masters and their one Adam */
    const ctr_critic_t    *critic[2];
    const ctr_ddpg_net_t  *critic_net[2];
    const ctr_ddpg_adam_t *critic_adam;
    const float *scale;                      /* device [6] or NULL, as ctr_td3_critic_step's           */
    /* the target critics: shape and blob, and their f32 tensors, [n_hidden + 1] layers each */
    const ctr_critic_t *critic_targ[2];
    float *const *W_targ[2];
    float *const *b_targ[2];
    /* the policy step's noise, the temperature */
    uint64_t seed, step_counter;             /* update i samples under step_counter + i                */
    float   *log_alpha;
    const ctr_sac_alpha_t *alpha;
    float    target_entropy;
    int32_t  pad;
    /* outputs (device): critic_loss float[2] or NULL, actor_loss and logp_mean float or NULL */
    float   *critic_loss, *actor_loss, *logp_mean;
    void    *workspace;                      /* ctr_sac_workspace_bytes(policy, critic[0], critic[1], max_B) */
    int64_t  workspace_bytes;
    float   *history;                        /* [updates][5] or NULL                                   */
} ctr_sac_update_t;
int ctr_sac_update(const ctr_sac_update_t *u, int32_t updates, void *stream);

/* ---------------------------------------------------------------------------------------
 * A run of DDPG / TD3 updates (added within ABI 17: a new symbol, no entry point or struct changes).
 * ctr_ddpg_update makes `updates` whole updates on `stream`: DDPG's with n_critics == 1, TD3's with
 * n_critics == 2.  Update i (0-based) leaves, bit for bit, in every tensor those calls write, what
 * this sequence leaves:
 *   n_critics == 1:
 *     ctr_her_sample_td(her, batch_size, draw_seed, draw_counter + i, batch,
 *                       {actor_targ, critic_targ[0], gamma, target, q1_next, next_action})
 *     ctr_ddpg_critic_step(critic[0], critic_net[0], critic_adam, batch->obs, batch->action, scale,
 *                          target, batch_size, critic_loss, workspace, ...)
 *   n_critics == 2:
 *     ctr_her_sample_td3(her, batch_size, draw_seed, draw_counter + i, batch,
 *                        {actor_targ, critic_targ[0], critic_targ[1], gamma, sigma, clip, target, q1_next, ...})
 *     ctr_td3_critic_step(critic, critic_net, critic_adam, batch->obs, batch->action, scale, target,
 *                         batch_size, critic_loss, workspace, ...)
 *   and then, only if (update_index + i + 1) % policy_delay == 0 (the policy's step):
 *     ctr_ddpg_actor_step(policy, policy_net, policy_adam, critic[0], critic_net[0]->W, ->b, batch->obs,
 *                         batch_size, actor_loss, workspace, ...)       (under critic 0's NEW parameters)
 *     ctr_polyak({actor_targ, policy_net->W, ->b, W_targ_actor, b_targ_actor},
 *                {critic_targ[y], critic_net[y]->W, ->b, W_targ[y], b_targ[y]}, y < n_critics; tau)
 *     ctr_actor_load(actor, policy_net->W, policy_net->b)               (if actor is not NULL)
 * that is: the policy's and every critic's parameters, gradients, m, v and pow; every target's
 * float32 tensors and blob; the online actor's blob; the batch and target tensors (they hold the last
 * update's draw); critic_loss (the last update's values) and actor_loss (the last policy step's).
 * The counter sum is 64-bit and wraps.  With history (device, [updates][1 + n_critics] float32) row i
 * also gets update i's critic losses and then the actor loss; the actor-loss entry of an update
 * that makes no policy step is left untouched.  critic[1], critic_net[1], critic_targ[1], W_targ[1],
 * b_targ[1], q2_next, sigma and clip are read only when n_critics == 2.
 *
 * Launches: the sampler's two scans once per call (the call only reads the store), then per update
 * with a policy step five: the sampler's kernel, the critics' gradient kernel, the critics' tail, the
 * policy's gradient kernel (k_ddpg_grad, as ctr_ddpg_actor_step launches it) and the policy's tail; per
 * update without one three: the sampler's kernel, the gradient kernel and the apply kernel of
 * ctr_ddpg_critic_step / ctr_td3_critic_step as it is (no soft update, no blob to pack).  Only when
 * the call's LAST update makes no policy step and both critic_loss and history are given, one more
 * launch of one wave copies the n_critics losses to the history row (the apply kernel has one loss
 * output).
 * A tail does for every parameter of its network what the apply kernel does (the slots' sum in slot
 * order, the gradient's store, Adam), then ctr_polyak's work with the new online value (the lerp, the
 * target's store, the target blob's 16-B item), the critics' tail with the critic as its second grid
 * dimension; the policy's tail also packs `actor`'s item.  A workgroup owns 256 consecutive items of
 * a blob (ctr_polyak's ownership: every parameter has one owner), and inside it the elements are
 * dealt so that consecutive lanes take consecutive floats of one tensor row -- 256 contiguous bytes
 * per wave where the items are four k-steps of a hidden layer's tile, 64 otherwise -- instead of
 * ctr_sac_update's one thread per item; the values a blob takes pass through LDS (8 or 16 KB) and each
 * thread packs its own item behind a barrier.  The critics' soft update runs ahead of the policy's
 * step: that step reads the online critic only.  No allocation, no host read, no synchronisation:
 * the call can be captured into a graph (a replay repeats its draws and its delay pattern: the counter
 * and update_index are arguments).
 *
 * Refused (CTR_EINVAL, before any launch, ctr_last_error names ctr_ddpg_update): u NULL; updates < 0;
 * n_critics outside 1..2; policy_delay < 1; whatever the calls above refuse (NULL structs, arrays and
 * layers, shapes, the in_dim relations to the store and between the networks, a non-finite gamma, the
 * rates, betas and eps, the workspace NULL, misaligned or smaller than ctr_ddpg_workspace_bytes (one
 * critic) / ctr_td3_workspace_bytes (two) for batch_size, batch_size outside 0..65 536); tau NaN or
 * outside [0, 1]; with two critics a sigma that is not finite or negative, a clip that is NaN or
 * negative; a target whose shape differs from its online network's; an actor whose shape differs
 * from the policy's, or whose blob is NULL or misaligned; any two of these being the same pointer: a
 * parameter, gradient, state or pow tensor of the networks, a target tensor, the targets' blobs and
 * the actor's, the loss outputs, the batch and target outputs, the workspace, history, scale; an
 * output that starts inside history's updates * (1 + n_critics) * 4 bytes.  updates == 0 and
 * batch_size == 0 are checked no-ops. */
typedef struct ctr_ddpg_update_t {
    /* the draw (ctr_her_sample_td / ctr_her_sample_td3) */
    const ctr_her_t *her;
    int64_t  batch_size;
    uint64_t draw_seed, draw_counter;        /* update i draws under draw_counter + i                  */
    const ctr_her_batch_t *batch;
    float   *target;                         /* [B] device, required                                   */
    float   *q1_next, *q2_next;              /* [B] or NULL (one critic: q1_next is q_next)            */
    float   *next_action;                    /* [B][6] or NULL                                         */
    float    gamma;
    float    tau;
    int32_t  n_critics;                      /* 1: DDPG, 2: TD3                                        */
    float    sigma, clip;                    /* TD3's target smoothing; read when n_critics == 2       */
    /* the delay */
    int32_t  policy_delay;                   /* >= 1                                                   */
    uint64_t update_index;                   /* the updates made before this call                      */
    /* the policy: its shape (scale and blob are not read), its f32 masters and Adam state */
    const ctr_actor_t     *policy;
    const ctr_ddpg_net_t  *policy_net;
    const ctr_ddpg_adam_t *policy_adam;
    /* the critics (shapes; their blobs are not read), their masters and their one Adam */
    const ctr_critic_t    *critic[2];
    const ctr_ddpg_net_t  *critic_net[2];
    const ctr_ddpg_adam_t *critic_adam;
    const float *scale;                      /* device [6] or NULL, as ctr_ddpg_critic_step's          */
    /* the targets: shape and blob, and their f32 tensors, [n_hidden + 1] layers each */
    const ctr_actor_t  *actor_targ;
    float *const *W_targ_actor;
    float *const *b_targ_actor;
    const ctr_critic_t *critic_targ[2];
    float *const *W_targ[2];
    float *const *b_targ[2];
    const ctr_actor_t  *actor;               /* the online actor's shape and blob, or NULL             */
    /* outputs (device): critic_loss float[n_critics] or NULL, actor_loss float or NULL */
    float   *critic_loss, *actor_loss;
    void    *workspace;                      /* ctr_ddpg_workspace_bytes / ctr_td3_workspace_bytes     */
    int64_t  workspace_bytes;
    float   *history;                        /* [updates][1 + n_critics] or NULL                       */
} ctr_ddpg_update_t;
int ctr_ddpg_update(const ctr_ddpg_update_t *u, int32_t updates, void *stream);

/* CtrReachEnv.reset for the environments with mask[i] != 0 (mask NULL = all).
 * goal [n][3] or NULL (sample a goal), system [n] or NULL (sample uniformly).
 * Writes the reset observation to obs [n][obs_dim]. */
int ctr_reset(const ctr_env_config_t *cfg, const ctr_batch_t *batch, const uint8_t *mask,
              const double *goal, const int32_t *system, void *obs, uint32_t *status, void *stream);

/* Precompute the resets queued in batch->refill (queued by ctr_step when a pooled reset is
 * consumed, and by ctr_reset for the P resets after the one it computes), then clear the
 * queue.  Call it every few steps; it is a no-op when the queue is empty. */
int ctr_pool_refill(const ctr_env_config_t *cfg, const ctr_batch_t *batch, void *stream);

/* Bytes of batch->carry for carry_cap resets per list (a header, then two lists of suspended
 * resets, each in 64 sub-lists); int32 counts[2][64] at byte 0 of the header give the resets each
 * sub-list holds (diagnostics).  The header's other words (the list parity, ctr_step_period's
 * claim and completion words) are zero between launches except the parity. */
int64_t ctr_refill_carry_bytes(int64_t carry_cap);

/* Queue every environment's next pool_depth resets (epoch + 1 .. epoch + P) that its pool slots
 * do not hold, e.g. after the batch state was restored from a checkpoint or the seed changed;
 * the next ctr_pool_refill computes them.  Also empties both of the refill's suspended lists
 * (batch->carry: their resets are not in the pool, so they are queued again).  A suspended reset
 * the refill finds its environment has passed (a miss sweep computed it) or its slot already
 * holding is dropped, as a queued one is. */
int ctr_pool_requeue(const ctr_env_config_t *cfg, const ctr_batch_t *batch, void *stream);

/* The tube table each environment's current episode uses (Model.current_sys_parameters,
 * model.py:13,20-28): with domain randomisation the episode's re-sampled table, else the
 * environment's system row.  sys_out [n] (derived, as the FK uses it) and raw_out [n] (the
 * re-sampled Tube inputs; U_x is in sys_out) may each be NULL.  (device) */
int ctr_domain_params(const ctr_env_config_t *cfg, const ctr_batch_t *batch, ctr_system_t *sys_out,
                      ctr_tube_raw_t *raw_out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Push all-gather of the packed step rows (BASELINE configs[3]: a single-process trainer that
 * wants every GPU's tip / reward / done; no reference counterpart -- the reference runs one env
 * per process).  Each rank pushes its [n][4] block of packed rows into every rank's receive ring
 * (IPC-mapped), then the block's sequence word into the receiver's sequence words (uncached device
 * memory).  Engines: the fused push (ctr_step_out_t.gather: k_step itself stores every env's row
 * into every rank's slot, and the next launch publishes the sequence words), ctr_gather_push (the
 * same stores as a standalone slim kernel), and ctr_copy_list, copy-engine copies (no CU at all,
 * but host-synchronous per copy in this runtime; the sequence word then comes from row n of the
 * packed rows, written by k_step: ctr_step_out_t.packed_seq).  RCCL's collective kernels, the
 * other option, cannot share a SIMD with k_step, so they hold CUs the next step needs.
 * A consumer waits for a step with ctr_gather_wait.  The host side
 * (ctr_reach_amd.distributed.PushGather) plans the destinations: receive ring
 * [depth][world][n][4] float32 (rank-major = global env id order within a slot), sequence words
 * [depth][world] uint32, release words [world] uint32.
 *
 * Ordering of the fused push (ABI 13).  Step t's rows are stored by the waves of k_step(t) with
 * system-scope stores (sc0 sc1: written through this GPU's L2) that each storing wave waits for
 * before it ends (performed at system scope), and k_step(t + 1), which the stream starts only
 * after k_step(t) has completed, publishes t's sequence words with system-scope stores.  A
 * consumer that acquires the words (system scope) therefore reads rows at least as new as step
 * t; the receive ring is uncached device memory, so the consumer's own L2 holds no stale line.
 * Flow control: slot t % depth is rewritten by step t + depth.  Consumer c releases its slot of
 * step s when it launches step s + depth - 1 (k_step's first lanes store s into every producer's
 * release word for c), so a gathered view of step s stays valid until this rank launches step
 * s + depth - 1; a producer's k_step(t) stores its rows only after every consumer has released
 * step t - depth (a bounded wait; on time-out the rows are stored anyway and err gets
 * CTR_GATHER_E_RELEASE_TIMEOUT).  ctr_gather_push and ctr_copy_list do not take part in the
 * flow control: their callers pace the ranks.
 * A time-out is also reported to the consumer it overran (ABI 14): before storing any row, the
 * producer stores the step into its poison word in the memory of every consumer that had not
 * released the slot (system scope, waited for), and every k_step with gather_wait_prev folds the
 * consumer's own poison words into its err (CTR_GATHER_E_RELEASE_TIMEOUT).  So err, read after a
 * view's readers have run (the next fused step, or PushGather.err_bits()), covers every overwrite
 * that reached the view -- no cross-rank reduction is needed to trust a local view.
 * Every bounded wait has a wall-clock budget (wait_us, s_memrealtime at 100 MHz), not a poll count.
 * ------------------------------------------------------------------------------------- */
#define CTR_IPC_HANDLE_BYTES 64
#define CTR_GATHER_MAX_RANKS 16
/* err bits of ctr_gather_wait and of the fused push (ctr_gather_push_t.err) */
#define CTR_GATHER_E_WAIT_TIMEOUT    1u   /* a consumer wait gave up after wait_us microseconds  */
#define CTR_GATHER_E_OVERWRITTEN     2u   /* a sequence word was already past the awaited step   */
#define CTR_GATHER_E_RELEASE_TIMEOUT 4u   /* a fused push stored into a slot not yet released
                                              (in the producer's err, and via the poison words in
                                              the err of the consumer it overran)                */
#define CTR_GATHER_E_PREV_TIMEOUT    8u   /* the fused consumer wait (gather_wait_prev) gave up  */

/* One rank's push of its block: the host struct of ctr_gather_push, and (in device memory) the
 * per-slot descriptor of the fused push (ctr_step_out_t.gather; src and ticket unused there). */
struct ctr_gather_push_t {
    const void *src;                          /* [n][4] float32 packed rows (16-B aligned)     */
    int64_t     n;
    int32_t     world;
    int32_t     pad;
    void       *dst[CTR_GATHER_MAX_RANKS];    /* rank p's copy of this block: its receive ring
                                                 slot + rank * n rows (IPC-mapped)           */
    uint32_t   *seqw[CTR_GATHER_MAX_RANKS];   /* this block's sequence word in rank p's memory  */
    uint32_t   *ticket;                       /* this rank's device word, zero-initialised (the
                                                 kernel leaves it zero)                      */
    /* fused push only (ABI 13): */
    uint32_t   *relw[CTR_GATHER_MAX_RANKS];   /* this rank's release word in rank p's memory   */
    const uint32_t *rel;                      /* [world] this rank's release words: rel[c] = the
                                                 last step whose slot consumer c released   */
    const uint32_t *wait_seqw;                /* [world] this rank's sequence words of the
                                                 previous slot (gather_wait_prev)           */
    uint32_t   *err;                          /* device word: CTR_GATHER_E_* bits             */
    int32_t     depth;                        /* ring slots (>= 2)                            */
    uint32_t    wait_us;                      /* wall-clock budget of every bounded wait, in
                                                 microseconds (ABI 14; was a poll count)     */
    /* ABI 14: */
    uint32_t   *poisonw[CTR_GATHER_MAX_RANKS];/* this rank's poison word in rank p's memory: on a
                                                 release time-out, step seq (1 if seq has
                                                 wrapped to 0) is stored into the words of the
                                                 consumers that had not released; a NULL entry
                                                 = not enabled for that consumer             */
    const uint32_t *poison;                   /* [world] this rank's poison words (producer p's
                                                 at [p]; zeroed, sticky): non-zero = a producer
                                                 overwrote a slot this rank had not released;
                                                 NULL = not enabled (only the producer's err
                                                 reports an overrun then)                    */
};

/* Enqueue the push kernel: the n rows to every dst[p] (p < world), then seq to every seqw[p]
 * (after all rows, release at system scope).  workgroups: grid size (e.g. 128); its waves use
 * ~20 VGPRs and no LDS, so they share SIMDs with k_step waves.  No flow control (see above). */
int ctr_gather_push(const ctr_gather_push_t *g, uint32_t seq, int32_t workgroups, void *stream);

/* Publish seq to every g_dev->seqw[p] (system scope) after the work already on
 * `stream`: the fused push's explicit publication of its last step (k_step publishes the previous
 * step itself, ctr_step_out_t.gather_prev).  g_dev: device descriptor.  One wave. */
int ctr_gather_publish(const ctr_gather_push_t *g_dev, uint32_t seq, void *stream);

/* hipIpcGetMemHandle of a device allocation (handle: CTR_IPC_HANDLE_BYTES bytes, host). */
int ctr_ipc_get_handle(const void *dev_ptr, void *handle);
/* Map another process's allocation (hipIpcOpenMemHandle, peer access enabled lazily). */
int ctr_ipc_open(const void *handle, void **dev_ptr);
int ctr_ipc_close(void *dev_ptr);

/* Uncached device memory for sequence words (zeroed; synchronous).  The only entry points that
 * allocate: the words are written by other GPUs' copy engines and polled by ctr_gather_wait,
 * so they must not sit in this GPU's L2. */
int ctr_seqw_alloc(int64_t bytes, void **dev_ptr);
int ctr_seqw_free(void *dev_ptr);

/* One copy of a copy list. */
typedef struct ctr_copy_t {
    void       *dst;
    const void *src;
    int64_t     bytes;
    int32_t     stream;      /* index into the streams of ctr_copy_list */
    int32_t     pad;
} ctr_copy_t;

/* Enqueue copy-engine copies (hipMemcpyDeviceToDeviceNoCU): every stream first waits for
 * ready_event (NULL: no wait), then runs its copies in list order, then records
 * done_events[s] (NULL array or entry: none).  Copies on one stream are ordered, so a sequence
 * word listed after its block lands after it. */
int ctr_copy_list(const ctr_copy_t *copies, int32_t n_copies, void *const *streams, int32_t n_streams,
                  void *ready_event, void *const *done_events);

/* Consumer side: enqueue on `stream` a one-wave kernel that waits until seqw[i] reaches seq for
 * every i < n (wrap-aware uint32 compare; seqw is uncached, polled at system scope), then
 * returns.  err (device, uint32) gets bit 1 if wait_us microseconds pass first (the kernel then
 * returns anyway: no unbounded wait) and bit 2 if a word is already past seq (the slot was
 * overwritten by a later step before it was consumed). */
int ctr_gather_wait(const uint32_t *seqw, int32_t n, uint32_t seq, uint32_t wait_us, uint32_t *err,
                    void *stream);

/* Batched compute_reward over leading dims: ag, dg [n][3] f64 -> reward [n] f32 in {-1, 0}. */
int ctr_compute_reward(const double *achieved, const double *desired, int64_t n, double tol,
                       float *reward, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CTR_REACH_AMD_H */
