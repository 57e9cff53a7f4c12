/* ctrlsim.h — C ABI of the MI355X-native CtRL-Sim closed-loop rollout path (libctrlsim_hip.so).
 *
 * Conventions: every pointer is a DEVICE pointer owned by the caller (in this repo: torch tensors, data_ptr()),
 * contiguous, little-endian; every function takes a hipStream_t, enqueues work on it and returns immediately
 * (0 = OK, negative errno-style code otherwise: -22 invalid argument, -5 launch failure); nothing allocates,
 * synchronises or throws.  No torch types appear here: the library links only against the HIP runtime.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference repository
 * montrealrobotics/ctrl-sim @ 2024_10_08).  The pybind11 module `nocturne_cpp` (the .cc files under nocturne/pybind11/src) and the
 * per-vehicle Python dict traffic of evaluators/policy_evaluator.py:99-159,514-542 are what a host binding calls today;
 * INTEGRATION.md shows the ctypes stub a maintainer adds to call these instead.
 *
 * Layouts (S scenarios, N <= 64 vehicles each, A context slots, T context steps, Tq = token_index+1 <= T,
 * P polylines x NP points per context, P_all polylines per scenario, Tmax rollout steps, Tmax1 = Tmax+1):
 *   hist_states [S,N,Tmax1,8] f32   x, y, vx, vy, heading, length, width, existence   (policies/policy.py:68-79)
 *   hist_tok    [S,N,Tmax]    i32   applied action token per step (default ZERO_ACTION_TOKEN = 524)
 *   hist_rtg    [S,N,Tmax,3]  i32   sampled RTG bins per step (default (0,35,35))
 *   coll        [S,N,Tmax1,2] u8    vehicle-vehicle / vehicle-road-edge collision flags
 *   phys        [S,N,20]      f32   Box2D body + FreeCar control state (see csrc/sim.hip)
 */
#ifndef CTRLSIM_H
#define CTRLSIM_H

#include <stdint.h>

/* context size classes a model batch / class-table launch may hold (csrc/common.h: MAXC) */
#define CTRLSIM_MAX_CLASSES 16

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

typedef struct ctrlsim_dims {
  int A, T, P, NP, D, H, F, V, R, C, NE, ND, MAXT;
  int variant; /* 0 CtRL-Sim (state, rtg, action tokens; cfgs/model/ctrl_sim.yaml), 1 IL (state, action; il.yaml),
                  2 Trajeglish (action tokens only; trajeglish.yaml), 3 Decision Transformer (continuous RTGs: ctx.rtg_bin
                  holds float bits; token order rtg, state, action; dt.yaml) — modules/encoder.py:27-34,116-152,
                  decoder.py:29-64; 4 (round 6) = the CtRL-Sim tokens and heads of 0 under cfg.model.attend_own_return_action
                  (cfgs/model/base.yaml:15, utils/train_utils.py:114-129: other agents' return / action tokens of EARLIER
                  timesteps are hidden; attention mask mode 5; plain 24-slot contexts, no K/V-cached entry point) */
  int flags;   /* model switches of cfgs/model/base.yaml beyond the shipped values (round 6; 0 = shipped; CtRL-Sim token layout only):
                  1 = no_actions (modules/encoder.py:129-130: action embeddings x 0 in front of embed_ln),
                  2 = use_map False (encoder.py:18,155-170: no MapEncoder — the polyline rows of the scene memory are key-padded, the weights
                      named encoder.map_encoder.* may be zeros),
                  4 = encode_initial_state False (encoder.py:84,111,135,159-166: the initial-state rows are key-padded).  2 and 4 together are
                      refused (the reference has no scene memory to build then). */
} ctrlsim_dims;

/* Agent-local context tensors of B contexts (outputs of ctrlsim_build_context, inputs of the forward). */
typedef struct ctrlsim_ctx {
  float* st12;       /* [B,Tq,A,12] x,y,vx,vy,yaw,len,wid + 5 type one-hot (-1 on padded slots) */
  float* exist;      /* [B,Tq,A]                                                                 */
  float* goal5;      /* [B,A,5]                                                                  */
  int* act_tok;      /* [B,Tq,A]                                                                 */
  int* rtg_bin;      /* [B,Tq,A,3]                                                               */
  int* tstep;        /* [B,Tq]                                                                   */
  int* slot_gid;     /* [B,A] global vehicle index per slot, -1 = padding                        */
  float* road_pts;   /* [B,P,NP,3] x,y,exist in the focal frame                                  */
  float* road_types; /* [B,P,8] one-hot, -1 rows = padding                                       */
} ctrlsim_ctx;

typedef struct ctrlsim_model ctrlsim_model;

/* ---- simulator step -------------------------------------------------------------------------------------------
 * Replaces nocturne_cpp Simulation.step(dt) + the per-vehicle setters (nocturne/pybind11/src/simulation.cc:20-38,
 * object.cc:52-54,89-92, vehicle.cc:20) i.e. Vehicle::set_acceleration/brake/set_steering/set_position,
 * PhysicsSimulation::Step -> FreeCar::Step + b2World::Step, Vehicle::Step, Scenario::UpdateCollision
 * (nocturne/cpp/src/vehicle.cc:25-135, physics/FreeCar.cpp:66-186, scenario.cc:266-328), AutoregressivePolicy.act
 * (policies/autoregressive_policy.py:256-274) and the state read-back of update_vehicle_data_dict
 * (evaluators/policy_evaluator.py:99-121).
 * contact_state: [S, ctrlsim_sim_contact_floats(N)] floats owned by the caller, initialised by ctrlsim_sim_init and carried from
 * step to step: Box2D's persistent per-pair contact manifolds with their accumulated impulses (warm starting),
 * b2World::m_inv_dt0 and the broad phase (fat AABBs, move buffer, b2DynamicTree nodes).  With it the step includes Box2D's box-box contact handling between vehicles (b2CollidePolygons,
 * islands, b2ContactSolver: third_party/box2d/src/collision/b2_collide_polygon.cpp, src/dynamics/b2_contact_solver.cpp,
 * b2_island.cpp, b2_world.cpp); NULL = contact-free integration (vehicles pass through each other; flags still exact). */
int64_t ctrlsim_sim_contact_floats(int N);
int ctrlsim_sim_init(int S, int N, int E, const float* init_pose /*[S,N,4] x,y,heading,speed*/,
                     const float* size /*[S,N,2] length,width*/, const float* edges /*[S,E,4]*/,
                     const uint8_t* exists /*[S,N]*/, float* phys, float* hist_states, uint8_t* coll, int Tmax1,
                     float* contact_state, hipStream_t stream);
/* Object.setPosition(x, y) / set_position (nocturne/pybind11/src/object.cc:52-54,87-90 -> Vehicle::set_position, vehicle.cc:75-87 ->
 * BaseCar::SetPosition = b2Body::SetTransform at the current angle, physics/BaseCar.cpp:28-32): xy [S,N,2], NaN = leave the vehicle
 * where it is.  The request is parked in `phys` and applied at the top of the next ctrlsim_sim_step, before that step's controls
 * (the reference applies it immediately; nothing observes the body in between).  The rollout's own use of it — vehicles that
 * stopped existing are parked at (-1e6, -1e6) every step, autoregressive_policy.py:260-263 — is what `exists` = 0 does. */
int ctrlsim_sim_set_position(int S, int N, const float* xy, float* phys, hipStream_t stream);
/* act_tok [S,N] (token id, or -1 = zero action) or act_f64 [S,N,2] (accel, steer); disc6 = {min_accel, max_accel,
 * min_steer, max_steer, n_accel, n_steer}; applied (nullable) [S,N,2] f64 receives the continuous actions.
 * mode 0 = FreeCar/Box2D (what eval_sim.py executes), 1 = Object::KinematicBicycleStep (object.cc:126-137). */
int ctrlsim_sim_step(int S, int N, int E, const int* act_tok, const double* act_f64, const double* disc6,
                     const float* size, const float* edges, const uint8_t* exists, float* phys, float* hist_states,
                     uint8_t* coll, double* applied, int t, int Tmax1, float dt, int mode, float* contact_state,
                     hipStream_t stream);
/* The same step (mode 0) with EXPERT-CONTROLLED objects (Object.expert_control = True, nocturne/pybind11/src/object.cc:58-59;
 * Scenario::Step, nocturne/cpp/src/scenario.cc:272-284; utils/sim.py:20-65 get_ground_truth_states): expert [S,N,4] = logged x, y,
 * heading, speed of step t + 1, x = NaN for the vehicles under policy control.  The world step moves every body; an expert vehicle is then
 * put on its logged state through Vehicle::set_position / set_heading / set_speed (vehicle.cc:75-105: two b2Body::SetTransform with proxy
 * synchronisation and the new-contact search of the next step, SetLinearVelocity) before the collision flags are taken; its history
 * row holds the logged values.  expert == NULL: ctrlsim_sim_step. */
int ctrlsim_sim_step_expert(int S, int N, int E, const int* act_tok, const double* act_f64, const double* disc6,
                            const float* size, const float* edges, const uint8_t* exists, float* phys, float* hist_states,
                            uint8_t* coll, double* applied, int t, int Tmax1, float dt, float* contact_state,
                            const float* expert, hipStream_t stream);

/* ---- log replay of partially controlled scenes -----------------------------------------------------------------
 * Replaces the per-step host work of a logged evaluation (evaluators/policy_evaluator.py:514-557): which vehicles the policy
 * drives (vehicles_to_evaluate from t >= history_steps - 1, :534-540) and the log-replay action of every other vehicle.
 * log [S,N,T1+1,6] f64 = logged x, y, heading, speed, exist, length per step, zero rows past the end of a vehicle's log (one row
 * more than the rollout has states: step t looks at row t + 1); controlled [S,N] u8 = vehicles handed to the policy;
 * exist_hist [S,N,T1] f64 = existence per step, latched.
 * ctrlsim_replay_latch — the existence bookkeeping of update_vehicle_data_dict (evaluators/policy_evaluator.py:118-121):
 * exist_hist[..,t] = log[..,t,4] (t = 0) or log[..,t,4] * (exist_hist[..,t-1] != 0), also written to hist_states[..,t,7]; call it
 * after the simulator wrote row t (ctrlsim_sim_init for t = 0) and before ctrlsim_group_build of step t, and once for row
 * T1 - 1 after the last step.  speed_hist (nullable, [S,N,T1] f32) [..,t] <- phys[..,16], the speed veh.getSpeed() returns at
 * step t (the same function's state read-back; phys may be NULL without it).
 * ctrlsim_replay_actions — after the action sampling of step t, before ctrlsim_sim_step.  A controlled vehicle from
 * t >= history_steps - 1 takes its sampled token act_now (AutoregressivePolicy.act, policies/autoregressive_policy.py:256-274;
 * undiscretize_actions, datasets/rl_waymo/dataset.py:322-338): (0, 0) for a token < 0 (no context answers for it), (0, 0) and
 * exists = 0 (parked by the simulator) once exist_hist[..,t] is 0.  Every other vehicle replays its log
 * (Evaluator.apply_gt_action, evaluators/evaluator.py:160-193): valid iff log rows t and t + 1 exist and the vehicle is not
 * latched out (t > 0 and exist_hist[..,t] == 0); then BicycleModel.backward (nocturne/bicycle_model.py:51-109, angle_sub of
 * utils/geometry.py:3-12) from the heading of hist_states row t and the speed phys[..,16] to x, y, heading, speed, length of log
 * row t + 1, steer clipped to +-0.7 and NaN -> 0; else (0, 0) and exists = 0.  Outputs: act_f64 [S,N,2] (what ctrlsim_sim_step
 * takes), exists [S,N], hist_tok[S,N,Tmax][..,t] = discretize_actions of the pair (dataset.py:365-380; np.round = round half to
 * even; the identity on a sampled token).  disc6 (host) as for ctrlsim_sim_step.  float64, the host expressions operation by
 * operation. */
int ctrlsim_replay_latch(int S, int N, int t, int T1, const double* log, const float* phys, double* exist_hist, float* hist_states,
                         float* speed_hist, hipStream_t stream);
int ctrlsim_replay_actions(int S, int N, int t, int T1, int Tmax, int history_steps, double dt, const double* log,
                           const uint8_t* controlled, const double* exist_hist, const float* hist_states, const float* phys,
                           const int* act_now, const double* disc6, double* act_f64, uint8_t* exists, int* hist_tok,
                           hipStream_t stream);
/* Policy ROLES (evaluators/planner_adversary_evaluator.py:458-546: a planner drives the ego, an adversary another vehicle, each
 * policy with its own focal groups, persisted context membership and RTG history over a common state and applied-action history).
 * A scene s has R <= CTRLSIM_MAX_ROLES policy VIEWS, rows s * R .. s * R + R - 1 of the policy-side arrays: ordinary scenarios for
 * ctrlsim_group_build, ctrlsim_build_context, the forward passes and the samplers.  role [S,N] i32: -1 = the vehicle replays its
 * log, r in [0, R) = the policy of view s * R + r drives it from step history_steps - 1 on.
 * ctrlsim_replay_latch_views = ctrlsim_replay_latch, which then copies the scene's state row t (the latched existence column
 * included) into row t of view_states [S*R,N,T1,8].
 * ctrlsim_replay_actions_views = ctrlsim_replay_actions with `role >= 0` for `controlled` and the sampled token read from the
 * vehicle's own role's view, act_now [S*R,N] at (s * R + role, v) — a role >= R answers like a token < 0; the token of the applied pair
 * also goes into column t of view_tok [S*R,N,Tmax] of every view of the scene.
 * view_states / view_tok equal to hist_states / hist_tok (or NULL) with R = 1: the scene is its own view, nothing is copied. */
#define CTRLSIM_MAX_ROLES 4
int ctrlsim_replay_latch_views(int S, int N, int R, int t, int T1, const double* log, const float* phys, double* exist_hist,
                               float* hist_states, float* speed_hist, float* view_states, hipStream_t stream);
int ctrlsim_replay_actions_views(int S, int N, int R, int t, int T1, int Tmax, int history_steps, double dt, const double* log,
                                 const int* role, const double* exist_hist, const float* hist_states, const float* phys,
                                 const int* act_now, const double* disc6, double* act_f64, uint8_t* exists, int* hist_tok,
                                 int* view_tok, hipStream_t stream);

/* ---- focal grouping + context tensors ------------------------------------------------------------------------
 * Replaces AutoregressivePolicy.get_data (policies/autoregressive_policy.py:51-165) with
 * RLWaymoDataset.select_relevant_agents / normalize_scene (datasets/rl_waymo/dataset.py:278-319,390-428).
 * ctrlsim_group_build, step t of S scenarios (one wavefront each).  hist_states [S,N,Tmax1,8] f32: positions are read from window row
 * w0 = (t < T ? 0 : t - (T - 1)), existence (column 7) from row t.  eval_order [S,N]: the evaluated vehicles in processing order, packed
 * at the front, -1 behind them, every entry unique and in [0, N) — anything else is undefined.  persist [S,N] is IN/OUT, bit v of
 * persist[s,i] = vehicle v belongs to the set vehicle i carries from step to step; 0 = "no set yet" (what the caller starts a rollout
 * with).  A focal vehicle with t == 0 or an empty set takes the A nearest vehicles (ascending distance in float64, ties to the lower
 * index) that lie strictly closer than dist_thresh; any other focal takes its set minus the vehicles at dist_thresh or beyond — a vehicle
 * that left does not come back.  Every evaluated vehicle folded into the group (the reference's list-mutated-while-iterated loop: the
 * entry behind a folded one is skipped) inherits the set.  Group g of scenario s: grp_focal / grp_ids / grp_members [s,g]; entries at
 * and beyond n_groups[s] are not written.  own_g [s,v] = first group whose ids hold v (-1: none), tilted [s,v] = v is a member of that
 * group, mem_g [s,v] = the group v is a member of (-1: none — a focal that does not exist at row t, or has_roads == 0, forms no
 * group).  Rows [s, 0..N) of own_g / mem_g / tilted / persist are always written.
 * Late vehicles: an evaluated vehicle that did not exist at step 0 and was folded into nobody's group still has persist == 0 when it
 * first exists at t > 0; it then makes the fresh nearest-A selection and carries that set on.  This is this library's rule: the
 * reference has no behaviour there (self.relevant_agent_idxs[focal_id] raises KeyError).
 * N or A outside [1, 64], T < 1, t < 0, t >= Tmax1 or a null pointer: CTRLSIM_EINVAL, nothing launched.  S <= 0: CTRLSIM_OK. */
int ctrlsim_group_build(int S, int N, int A, int T, int t, int Tmax1, double dist_thresh, const float* hist_states,
                        const int* eval_order /*[S,N] -1 padded*/, int has_roads, uint64_t* persist /*[S,N]*/,
                        int* n_groups /*[S]*/, int* grp_focal /*[S,N]*/, uint64_t* grp_ids, uint64_t* grp_members,
                        int* own_g /*[S,N]*/, int* mem_g /*[S,N]*/, uint8_t* tilted /*[S,N]*/, hipStream_t stream);
/* flag[0] |= 1 if the focal groups of scenarios [0,S) (count, focal vehicle or membership mask of any group) differ from the
 * snapshot ref_*: the device-side form of "did get_data build the same contexts as last step" that gates the K/V-cached
 * phase; the caller zeroes flag and copies it to the host together with n_groups (one asynchronous copy per step). */
int ctrlsim_groups_changed(int S, int N, const int* n_groups, const int* grp_focal, const uint64_t* grp_ids, const int* ref_n,
                           const int* ref_focal, const uint64_t* ref_ids, int* flag, hipStream_t stream);
/* Compact contexts.  Token rows of agent slots that exist nowhere in the window are identical (modules/encoder.py:127-133 multiplies
 * every embedding by the existence flag before embed_ln; the decoder puts no key padding on its targets) and remain identical
 * through all layers, so a context with n vehicles may be evaluated with any slot count Actx >= n + 1: Actx - 1 regular slots and
 * ONE representative slot standing for the dims.A - (Actx - 1) padded slots of the reference layout (its keys carry that
 * multiplicity in the attention: ctrlsim_attention_compact).  Exact in real arithmetic.  `sizes` = the ascending slot counts a
 * caller uses (nb <= CTRLSIM_MAX_CLASSES, last = dims.A; a context takes the first size >= n + 1, or dims.A).
 * ctrlsim_group_size_hist: hist[s, k] = focal groups of scenario s in size class k (with n_groups: what the host needs to cut a
 * step into model batches).  ctrlsim_ctx_index_classes: ctrlsim_ctx_index with the contexts SORTED by size class (class k =
 * contexts [sum_{j<k} count_j, ...)); ctx_row0[c] = first logits row of context c when class k emits (sizes[k] - 1, or dims.A
 * for the last class) rows per context; ctx_of_group: [S, N] scratch. */
int ctrlsim_group_size_hist(int S, int N, const int* n_groups, const uint64_t* grp_ids, int nb, const int* sizes /*host*/,
                            int* hist /*[S,nb]*/, hipStream_t stream);
int ctrlsim_ctx_index_classes(int s0, int s1, int N, int A, const int* n_groups, const uint64_t* grp_ids, const int* own_g,
                              const int* mem_g, int nb, const int* sizes /*host*/, int* ctx_scn, int* ctx_grp, int* ctx_row0,
                              int* ctx_of_group, int* own_ctx, int* own_slot, int* mem_ctx, int* mem_slot, hipStream_t stream);
int ctrlsim_ctx_index(int s0, int s1, int N, const int* n_groups, const int* grp_focal, const uint64_t* grp_ids,
                      const int* own_g, const int* mem_g, int* ctx_scn, int* ctx_grp, int* own_ctx, int* own_slot,
                      int* mem_ctx, int* mem_slot, int* ctx_base, hipStream_t stream);
int ctrlsim_build_context(int B, int N, int A, int T, int t, int Tq, int tt_first /*emit window rows [tt_first,Tq)*/,
                          int Tmax1, int Tmax, int P_all, int P, int NP,
                          const int* ctx_scn, const int* ctx_grp, const int* grp_focal, const uint64_t* grp_ids,
                          const float* hist_states, const int* hist_tok, const int* hist_rtg,
                          const double* goals /*[S,N,5]*/, const float* types /*[S,N,5]*/,
                          const float* roads /*[S,P_all,NP,3]*/, const float* road_types /*[S,P_all,8]*/,
                          const int* zero4 /*{zero action token, rtg bins x3}*/, const ctrlsim_ctx* out,
                          hipStream_t stream);
/* The same for a model batch of up to CTRLSIM_MAX_CLASSES context size classes in ONE launch (class k: B[k] contexts of A[k] slots written to
 * out[k]; the batch's context list ctx_scn / ctx_grp holds the classes back to back). */
int ctrlsim_build_context_c(int n, const int* B, const int* A, const ctrlsim_ctx* out, int N, int T, int t, int Tq, int tt_first,
                            int Tmax1, int Tmax, int P_all, int P, int NP, const int* ctx_scn, const int* ctx_grp,
                            const int* grp_focal, const uint64_t* grp_ids, const float* hist_states, const int* hist_tok,
                            const int* hist_rtg, const double* goals, const float* types, const float* roads,
                            const float* road_types, const int* zero4, hipStream_t stream);

/* ---- model ----------------------------------------------------------------------------------------------------
 * Replaces CtRLSim.load_from_checkpoint + CtRLSim.forward (models/ctrl_sim.py:19-45; modules/encoder.py,
 * map_encoder.py, decoder.py) as used by AutoregressivePolicy.predict (autoregressive_policy.py:189-210).
 * `names`/`offsets` describe the packed fp32 weight buffer (state_dict names + the "fold.*" tensors of
 * ctrlsim_amd/pack.py). */
int ctrlsim_model_create(const ctrlsim_dims* dims, const float* dev_weights, int n, const char* const* names,
                         const int64_t* offsets, ctrlsim_model** out);
void ctrlsim_model_destroy(ctrlsim_model* m);
int64_t ctrlsim_forward_workspace_bytes(const ctrlsim_dims* dims, int B, int Tq);
/* The *_a forms take a uniform batch of COMPACT contexts of Actx slots (context tensors [B,Tq,Actx,.]; Actx == dims.A: the plain
 * layout, what the forms without _a call): Actx - 1 regular slots + the representative (see ctrlsim_group_size_hist); logits
 * come back for the regular slots only, [B*(Actx-1), .] rows (Actx == dims.A: [B*A, .]). */
int64_t ctrlsim_forward_workspace_bytes_a(const ctrlsim_dims* dims, int B, int Tq, int Actx);
int ctrlsim_dt_forward_pass1_a(const ctrlsim_model* m, int B, int Tq, int Actx, const ctrlsim_ctx* ctx, void* workspace,
                               float* rtg_logits, float* dbg_seg_emb, hipStream_t stream);
int ctrlsim_dt_forward_pass2_a(const ctrlsim_model* m, int B, int Tq, int Actx, int t, int N, int Tmax, const ctrlsim_ctx* ctx,
                               const int* ctx_scn, const int* hist_rtg, void* workspace, float* act_logits, int cached,
                               hipStream_t stream);
int ctrlsim_dt_forward_pass1_cached_a(const ctrlsim_model* m, int B, int t, int Actx, const ctrlsim_ctx* ctx, void* workspace,
                                      float* rtg_logits, hipStream_t stream);
/* The *_c forms take a model BATCH of n <= CTRLSIM_MAX_CLASSES classes of compact contexts (class k: B[k] contexts of A[k] slots, context tensors
 * ctx[k]; host arrays): every row-wise kernel runs once over the rows of all classes, the attention kernel and the K/V-image
 * epilogue of the QKV projection work from a class table.  Logits rows come class after class, context after context,
 * regular slot after regular slot (ctrlsim_ctx_index_classes' ctx_row0).  ctx_scn lists the contexts in that same order. */
int64_t ctrlsim_forward_workspace_bytes_c(const ctrlsim_dims* dims, int n, const int* B, const int* A, int Tq);
int ctrlsim_dt_forward_pass1_c(const ctrlsim_model* m, int n, const int* B, const int* A, const ctrlsim_ctx* ctx, int Tq,
                               void* workspace, float* rtg_logits, float* dbg_seg_emb, hipStream_t stream);
int ctrlsim_dt_forward_pass2_c(const ctrlsim_model* m, int n, const int* B, const int* A, const ctrlsim_ctx* ctx, int Tq, int t,
                               int N, int Tmax, const int* ctx_scn, const int* hist_rtg, void* workspace, float* act_logits,
                               int cached, hipStream_t stream);
/* ctrlsim_dt_forward_pass1_c with its few-row tail (last decoder layer on the queried rows, the head) on `tail_stream`, ordered
 * behind the full-row part on `stream` by an event inside the call: the caller's next full-row work on `stream` need not wait
 * for it; rtg_logits are complete in tail_stream order. */
int ctrlsim_dt_forward_pass1_c2(const ctrlsim_model* m, int n, const int* B, const int* A, const ctrlsim_ctx* ctx, int Tq,
                                void* workspace, float* rtg_logits, hipStream_t stream, hipStream_t tail_stream);
int ctrlsim_dt_forward_pass1_cached_c(const ctrlsim_model* m, int n, const int* B, const int* A, const ctrlsim_ctx* ctx, int t,
                                      void* workspace, float* rtg_logits, hipStream_t stream);
/* pass 1: rtg_logits [B,A,R*C] of the current-timestep state tokens; caches per-layer K/V in `workspace`. */
int ctrlsim_dt_forward_pass1(const ctrlsim_model* m, int B, int Tq, const ctrlsim_ctx* ctx, void* workspace,
                             float* rtg_logits, float* dbg_seg_emb /*nullable [B,P,D]*/, hipStream_t stream);
/* The baselines of cfgs/model/{il,trajeglish,dt}.yaml (dims.variant 1 / 2 / 3) have no RTG head and one forward per step
 * (policies with predict_rtgs = False, autoregressive_policy.py:189,208-240): action logits [B,A,V] of the current step from
 * the state tokens (IL, DT) / action tokens (Trajeglish), decoder.py:55-64.  ctrlsim_dt_forward_pass1 / _pass2 / _cached refuse
 * these models and this call refuses the CtRL-Sim model. */
int ctrlsim_dt_forward_actions(const ctrlsim_model* m, int B, int Tq, const ctrlsim_ctx* ctx, void* workspace,
                               float* act_logits, hipStream_t stream);
/* Component-level entry (tests, micro-benchmarks): MapEncoder's point MLP + seed-attention pooling (modules/map_encoder.py:28-46,
 * before out_proj) of B*P polylines road_pts [B,P,NP,3] -> attn_pre [B*P,256]; pad [B,P] <- 1 for polylines without any point. */
int ctrlsim_map_pool(const ctrlsim_model* m, int B, const float* road_pts, float* attn_pre, uint8_t* pad, hipStream_t stream);
/* The reference's full return contract of CtRLSim.forward (models/ctrl_sim.py:41-45; decoder.py:52-77): teacher-forced, every
 * head on every token of the Tq window steps.  action_preds [B,Tq,A,V], rtg_preds [B,Tq,A,R*C], state_preds [B,Tq,A,2T] in
 * token-row order (the reference returns the [B,A,T,.] permutation of these).  rtg_preds / state_preds are nullable and must be
 * NULL for models without the head (predict_rtg / predict_future_states false: il, trajeglish, dt yaml).  Workspace as pass 1.
 * Training-time / debugging contract — the rollout reads one timestep and uses the pass1 / pass2 entry points. */
int ctrlsim_forward_all(const ctrlsim_model* m, int B, int Tq, const ctrlsim_ctx* ctx, void* workspace, float* action_preds,
                        float* rtg_preds, float* state_preds, hipStream_t stream);
/* Open-loop evaluation — replaces CtRLSim.compute_loss / validation_step (models/ctrl_sim.py:48-189,217-228) behind one teacher-forced
 * forward over B logged windows: cross-entropy of the action head and of the three return heads against the tokens the context itself
 * holds (ctx.act_tok, ctx.rtg_bin: teacher forcing scores its own inputs), the future-state MSE, masked by existence and (moving
 * [B,A] uint8, NULL = every agent) supervise_moving.  sums [5][2] += (sum, count) of loss_actions, loss_rtg_goal, loss_rtg_veh,
 * loss_rtg_road, loss_state over the batch — means of shards do not combine, sums and counts do: loss = sum / count
 * (x loss_action_coef for the actions), loss_state = sum / (100 * 2 * count) (:146); a term whose count is 0 is 0 / 0 = NaN in the
 * reference and here.  per_ctx [B,5,2] (nullable) the same per context; row_nll [B,Tq,A,4] (nullable) lse - logit[target] per row and
 * softmax (actions, goal, veh, road; unmasked).  By dims.variant: 0 / 4 all five terms (state only with the predict_future_states head);
 * 1 (IL) / 3 (DT) the action term, from the state tokens (decoder.py:55-64); 2 (Trajeglish) the action term with the reference's shift:
 * logits of step i against the action of step i + 1 under the existence of step i + 1 (:50-67).  local_frame_predictions: state targets
 * translated to the agent's position at step i and rotated by minus its yaw (:151-187; as there, without the moving mask).
 * fused != 0: the heads' last Linear runs with a cross-entropy epilogue (csrc/loss.hip) and no logits are written — two-fp16-plane
 * scheme; under the three-bf16-plane scheme, or with fused == 0, the generic Linear writes a chunk of rows at a time and a row kernel
 * reduces it (same results up to summation order).  The batch totals are reduced by fixed trees: identical bits from run to run.
 * Workspace: ctrlsim_forward_loss_workspace_bytes (the forward's own + 8 floats per row + the state predictions + a logits chunk). */
typedef struct ctrlsim_loss_cfg {
  int supervise_moving;          /* cfg.model.supervise_moving */
  int local_frame_predictions;   /* cfg.model.local_frame_predictions */
  int fused;                     /* 1 = cross-entropy epilogue, 0 = logits through memory */
  int pad_;
} ctrlsim_loss_cfg;
int64_t ctrlsim_forward_loss_workspace_bytes(const ctrlsim_dims* dims, int B, int Tq);
int ctrlsim_forward_loss(const ctrlsim_model* m, int B, int Tq, const ctrlsim_ctx* ctx, const uint8_t* moving,
                         const ctrlsim_loss_cfg* cfg, void* workspace, double* sums, double* per_ctx, float* row_nll,
                         hipStream_t stream);
/* ---- training, first stage: head gradients of the open-loop loss (csrc/head_grad.hip) ----------------------------------------
 * The derivative of the reference's training loss, final_loss = loss_action_coef * loss_actions + loss_rtg_goal + loss_rtg_veh +
 * loss_rtg_road + loss_state over the terms the model has (models/ctrl_sim.py:48-214), through the three MLP heads predict_action,
 * predict_rtg, predict_future_states (modules/decoder.py:23-35, utils/layers.py:6-19) down to the decoder's output rows.  X is the
 * decoder output [B*Tq*A*3, 256] in the plain layout (token type k of (b, tt, a) is row ((b*Tq + tt)*A + a)*3 + k).
 * grads: ONE flat float32 buffer holding, per head in the parameter-table order (action, returns, future states; only the heads
 * the model has), mlp.0.weight [256,256], mlp.0.bias, mlp.1.weight, mlp.1.bias (the LayerNorm), mlp.3.weight [n,256], mlp.3.bias.
 * This is scope 0 of the layout and workspace queries below.  dX (nullable) [B*Tq*A*3, 256]: the gradient at the decoder
 * output, every row written, zeros on rows no head reads.  sums / per_ctx as for ctrlsim_forward_loss; the per-row scales divide by the
 * counts found in `sums` after this call's own reduction, on the device: hand in zeroed sums for the gradient of this batch's loss.
 * A term whose count is 0 has a NaN loss and NaN gradients, as autograd gives the reference.  Arithmetic: f32-input MFMA from the
 * fp32 master weights under either operand split of the forward; sums across workgroups go through partial slabs and a second,
 * fixed-order stage, no atomics: identical bits from run to run.  Workspace: ctrlsim_train_grads_workspace_bytes(dims, B, Tq, 0) (the
 * forward-loss workspace, then Z, H, dH [B*Tq*A, 256], a logits chunk of <= 8192 rows, and the partial slabs).
 * ctrlsim_heads_loss_grad takes X from the caller and runs no forward; ctrlsim_forward_loss_grads (below) runs the teacher-forced
 * forward first, on its own X. */
int ctrlsim_heads_loss_grad(const ctrlsim_model* m, int B, int Tq, const ctrlsim_ctx* ctx, const uint8_t* moving,
                            const ctrlsim_loss_cfg* cfg, float loss_action_coef, const float* X, void* workspace, double* sums,
                            double* per_ctx, float* grads, float* dX, hipStream_t stream);
/* ---- training, second stage (a): the feed-forward block's backward (csrc/ffn_grad.hip) -------------------------------------------
 * The op.  Forward being differentiated, per row (width 256, hidden width F, LayerNorm eps 1e-5, relu'(0) = 0):
 *   Hp = U W1^T + b1,  H = relu(Hp),  S = U + H W2^T + b2,  Y = LayerNorm(S; gamma, beta)
 * — the post-LN block every encoder / decoder layer ends in (linear1, linear2, the layer's last norm).  U [rows, 256] and dY [rows, 256]
 * with leading dimensions >= 256 (floats); W1 [F,256], b1 [F], W2 [256,F], b2, gamma, beta [256]: the fp32 master tensors.
 * grads: ONE flat float32 buffer dW1 [F,256], db1 [F], dW2 [256,F], db2 [256], dgamma [256], dbeta [256] — the state-dict order
 * linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm.weight, norm.bias.  dU (nullable) [rows, 256], leading dimension
 * lddu: the gradient at the block's input.  dU MAY be dY itself with lddu == lddy (a row of dY is consumed before that row of dU is
 * written); any other overlap of dU with an input is undefined.  U and dY are not written.  rows < 1, F < 1 or a null pointer other than dU: CTRLSIM_EINVAL; any
 * F >= 1 works.  Nothing of the forward is kept: H and S are recomputed a chunk of rows at a time (ctrlsim_ffn_block_grad_chunk_rows:
 * <= 8192, fewer where F > 1024).  Arithmetic: f32-input MFMA, independent of the forward's operand split; no float atomics, sums in
 * fixed orders: identical bits from run to run, whatever the workspace held. */
int64_t ctrlsim_ffn_block_grad_workspace_bytes(int rows, int F);
int ctrlsim_ffn_block_grad_chunk_rows(int rows, int F);
int ctrlsim_ffn_block_grad(const float* U, int ldu, const float* dY, int lddy, const float* W1, const float* b1, const float* W2,
                           const float* b2, const float* gamma, const float* beta, int rows, int F, void* workspace, float* grads,
                           float* dU, int lddu, hipStream_t stream);
/* ---- training, second stage (b): the attention sublayer's backward (csrc/attn_grad.hip) -------------------------------------------
 * The op.  Forward being differentiated, per context of Lq query rows and Lk memory rows (width 256, 8 heads x 32, LayerNorm eps 1e-5):
 *   Q = X Wq^T + bq,  K = Mem Wk^T + bk,  V = Mem Wv^T + bv            (in_proj_weight [768,256] = Wq; Wk; Wv, in_proj_bias [768])
 *   O = concat_h softmax_keys(Q_h K_h^T / sqrt(32)) V_h                 (keys with key_pad = 1 excluded; every key excluded: O = 0)
 *   S = X + O Wo^T + bo,  Y = LayerNorm(S; gamma, beta)
 * — the post-LN attention sublayer of torch.nn.TransformerDecoderLayer (cross-attention: Mem = the memory) and, with X = Mem, of
 * torch.nn.TransformerEncoderLayer.  X [B*Lq, 256], Mem [B*Lk, 256], dY [B*Lq, 256] with leading dimensions >= 256 (floats);
 * key_pad [B, Lk] bytes, 1 = ignore, NULL = no key padded.  grads: ONE flat float32 buffer d in_proj_weight [768,256], d in_proj_bias
 * [768], d out_proj.weight [256,256], d out_proj.bias, dgamma, dbeta [256], back to back.  dX (nullable) [B*Lq, 256]: the gradient at X
 * (residual and query paths); it MAY be dY itself with lddx == lddy.  dMem (nullable) [B*Lk, 256]: the gradient at Mem through K and V
 * only (with X = Mem the caller adds dX); rows of padded keys are exactly 0.  Any other overlap of an output with an input is undefined.
 * B, Lq or Lk < 1, a leading dimension below 256 or a null pointer other than key_pad, dX, dMem: CTRLSIM_EINVAL, nothing launched.
 * Nothing of a forward pass is read but X, Mem and key_pad: Q, K, V, the softmax statistics, O and S are recomputed on the f32-input
 * MFMA from the fp32 masters, the query rows a chunk of whole contexts at a time (ctrlsim_attn_block_grad_chunk_contexts: <= 8192 rows
 * where a context has no more).  The gradient is that of the function evaluated this way.  No float atomics, sums in fixed orders:
 * identical bits from run to run, whatever the workspace held. */
int64_t ctrlsim_attn_block_grad_workspace_bytes(int B, int Lq, int Lk);
int ctrlsim_attn_block_grad_chunk_contexts(int B, int Lq, int Lk);
int ctrlsim_attn_block_grad(const float* X, int ldx, const float* Mem, int ldm, const uint8_t* key_pad, const float* dY, int lddy,
                            const float* in_proj_weight, const float* in_proj_bias, const float* out_proj_weight,
                            const float* out_proj_bias, const float* gamma, const float* beta, int B, int Lq, int Lk, void* workspace,
                            float* grads, float* dX, int lddx, float* dMem, int lddm, hipStream_t stream);
/* ---- training (c): the causal self-attention sublayer's backward (csrc/self_attn_grad.hip) ----------------------------------------
 * The op.  Forward being differentiated, per context of L = 3 T A token rows, token i = (t, a, k) = (i / 3A, (i / 3) % A, i % 3):
 *   Q | K | V = X Win^T + bin                                           (in_proj_weight [768,256], in_proj_bias [768])
 *   O = concat_h softmax_{visible j}(Q_h K_h^T / sqrt(32)) V_h
 *   S = X + O Wo^T + bo,  Y = LayerNorm(S; gamma, beta)
 * — the first sublayer of a decoder layer.  mask_mode 0 (dims.variant 0): visible(i, j) <=> t_j < t_i or (t_j == t_i and ((a_j == a_i
 * and k_j <= k_i) or k_j == 0)); mask_mode 1 (attend_own_return_action, dims.variant 4): the t_j < t_i term only where a_j == a_i or
 * k_j == 0.  No key-padding mask.  Masked pairs are excluded by index: their probability is exactly 0.
 * X, dY [B*L, 256] with leading dimensions >= 256 (floats).  grads: ONE flat float32 buffer d in_proj_weight [768,256], d in_proj_bias
 * [768], d out_proj.weight [256,256], d out_proj.bias, dgamma, dbeta [256], back to back.  dX (nullable) [B*L, 256] = dS + dQ Wq + dK Wk
 * + dV Wv; it MAY be dY itself with lddx == lddy.  Any other overlap of an output with an input is undefined.  Argument checks and return
 * values are ctrlsim_attn_block_grad's; any other mask_mode: CTRLSIM_EINVAL.  Nothing of a forward pass is read but X; query rows a
 * chunk of whole contexts at a time (ctrlsim_self_attn_block_grad_chunk_contexts: <= 8192 rows where a context has no more); score tiles
 * wholly beyond a query block's last timestep are never computed.  No float atomics, sums in fixed orders: identical bits from run to
 * run, whatever the workspace held. */
int64_t ctrlsim_self_attn_block_grad_workspace_bytes(int B, int T, int A);
int ctrlsim_self_attn_block_grad_chunk_contexts(int B, int T, int A);
int ctrlsim_self_attn_block_grad(const float* X, int ldx, const float* dY, int lddy, const float* in_proj_weight,
                                 const float* in_proj_bias, const float* out_proj_weight, const float* out_proj_bias, const float* gamma,
                                 const float* beta, int B, int T, int A, int mask_mode, void* workspace, float* grads, float* dX, int lddx,
                                 hipStream_t stream);
/* ---- training (d): one whole decoder layer's backward by recompute (csrc/decoder_layer_grad.hip) ---------------------------------------
 * The op.  Forward being differentiated, per context of L = 3 T A token rows and Lk memory rows: the three sublayers above in a row,
 *   X1 = the self-attention sublayer of X0 (norm1),  U = the cross-attention sublayer of X1 and Mem (norm2),  Y = the feed-forward block
 *   of U (norm3)
 * — torch.nn.TransformerDecoderLayer, post-LN, relu.  X0, dY [B*L, 256], Mem [B*Lk, 256] with leading dimensions >= 256 (floats); key_pad
 * [B, Lk] bytes or NULL; mask_mode as the self-attention op's.  tensors: a HOST array of the layer's 18 fp32 master tensors (device
 * pointers), grads: ONE flat float32 buffer of their gradients, both in the order a training scope appends them: the six feed-forward
 * tensors (linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm3.weight, norm3.bias), the six of the cross-attention
 * (multihead_attn.in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, norm2.weight, norm2.bias), the six of the self-attention
 * (self_attn.*, norm1.*), each group in state-dict order, back to back.  dX0 (nullable) [B*L, 256]: the gradient at X0; it MAY be dY
 * itself with lddx0 == lddy.  dMem (nullable) [B*Lk, 256]: the gradient at Mem; with accumulate_dmem != 0 every element's one owner
 * adds this call's value to what dMem holds (a fixed order: deterministic), otherwise it overwrites.  Rows of padded keys: exactly 0
 * without the flag, left as they are with it.  x1_out, u_out (nullable) [B*L, 256] dense: X1 and U as the backward read them.
 * Nothing of a forward pass is read but X0, Mem and key_pad: X1 and U are recomputed on the f32-input MFMA from the fp32 masters, then
 * the three ops run on (U, dY), (X1, Mem, dU) and (X0, dX1) and recompute their own sublayer's inside.  The gradient is that of the layer
 * function evaluated this way on X0 as given; the result equals, bit for bit, the three public ops called by hand on x1_out and u_out.
 * A null pointer other than key_pad, dX0, dMem, x1_out, u_out, a leading dimension below 256, B, T, A, Lk or F < 1, another mask_mode,
 * B*L*768 >= 2^31 or B*Lk*512 >= 2^31: CTRLSIM_EINVAL, nothing launched.  No float atomics, sums in fixed orders: identical bits from
 * run to run, whatever the workspace held. */
int64_t ctrlsim_decoder_layer_grad_workspace_bytes(int B, int T, int A, int Lk, int F);
int ctrlsim_decoder_layer_grad(const float* X0, int ldx, const float* Mem, int ldm, const uint8_t* key_pad, const float* dY, int lddy,
                               const float* const* tensors /* 18 fp32 masters */, int B, int T, int A, int Lk, int F, int mask_mode,
                               void* workspace, float* grads, float* dX0, int lddx0, float* dMem, int lddm, int accumulate_dmem,
                               float* x1_out, float* u_out, hipStream_t stream);
/* ---- training (e): the scene encoder's self-attention sublayer's backward (csrc/scene_attn_grad.hip) -----------------------------------
 * The op.  Forward being differentiated, per context of L rows — ONE source: the context's own rows are queries, keys and values:
 *   Q | K | V = X Win^T + bin                                           (in_proj_weight [768,256], in_proj_bias [768])
 *   O = concat_h softmax_keys(Q_h K_h^T / sqrt(32)) V_h                 (keys with key_pad = 1 excluded; every key excluded: O = 0)
 *   S = X + O Wo^T + bo,  Y = LayerNorm(S; gamma, beta)
 * — the first sublayer of torch.nn.TransformerEncoderLayer (post-LN, src_key_padding_mask).  X, dY [B*L, 256] with leading dimensions
 * >= 256 (floats); key_pad [B, L] bytes, 1 = ignore, NULL = no key padded.  grads: ONE flat float32 buffer d in_proj_weight [768,256],
 * d in_proj_bias [768], d out_proj.weight [256,256], d out_proj.bias, dgamma, dbeta [256], back to back.  dX (nullable) [B*L, 256] = dS +
 * dQ Wq + dK Wk + dV Wv; it MAY be dY itself with lddx == lddy.  Any other overlap of an output with an input is undefined.  A dX row of
 * a padded key whose dY row is zero is exactly zero.  B or L < 1, B*L*768 >= 2^31, a leading dimension below 256 or a null pointer other
 * than key_pad, dX: CTRLSIM_EINVAL, nothing launched.  The same function as ctrlsim_attn_block_grad(X, Mem = X) with dX + dMem added by
 * the caller, built as the self-attention op's chunk-local pipeline (one in_proj product, one d in_proj product, one K = 768 product for
 * dX; no K | V buffers of all contexts): nothing of a forward pass is read but X and key_pad; rows a chunk of whole contexts at a time
 * (ctrlsim_scene_attn_block_grad_chunk_contexts: <= 8192 rows where a context has no more).  f32-input MFMA from the fp32 masters; no
 * float atomics, sums in fixed orders: identical bits from run to run, whatever the workspace held. */
int64_t ctrlsim_scene_attn_block_grad_workspace_bytes(int B, int L);
int ctrlsim_scene_attn_block_grad_chunk_contexts(int B, int L);
int ctrlsim_scene_attn_block_grad(const float* X, int ldx, const uint8_t* key_pad, const float* dY, int lddy, const float* in_proj_weight,
                                  const float* in_proj_bias, const float* out_proj_weight, const float* out_proj_bias, const float* gamma,
                                  const float* beta, int B, int L, void* workspace, float* grads, float* dX, int lddx, hipStream_t stream);
/* ---- training (e): one whole scene-encoder layer's backward by recompute (csrc/encoder_layer_grad.hip) ------------------------------
 * The op.  Forward being differentiated, per context of L rows: U = the sublayer above of X0 (norm1), Y = the feed-forward block of U
 * (norm2) — torch.nn.TransformerEncoderLayer, post-LN, relu.  X0, dY [B*L, 256] with leading dimensions >= 256; key_pad [B, L] bytes or
 * NULL.  tensors: a HOST array of the layer's 12 fp32 master tensors (device pointers), grads: ONE flat float32 buffer of their
 * gradients, both in the decoder layer op's convention: the six feed-forward tensors (linear1.weight, linear1.bias, linear2.weight,
 * linear2.bias, norm2.weight, norm2.bias), then the six of the attention (self_attn.in_proj_weight, in_proj_bias, out_proj.weight,
 * out_proj.bias, norm1.weight, norm1.bias).  dX0 (nullable) [B*L, 256]: the gradient at X0; it MAY be dY itself with lddx0 == lddy.
 * u_out (nullable) [B*L, 256] dense: U as the backward read it.  U is recomputed from X0 (the attention op's own chunk forward, then the
 * out-projection + norm1), then the two ops run on (U, dY) and (X0, dU); the result equals, bit for bit, the two public ops called by
 * hand on u_out.  A null pointer other than key_pad, dX0, u_out, a leading dimension below 256, B, L or F < 1, B*L*768 >= 2^31:
 * CTRLSIM_EINVAL, nothing launched.  No float atomics, sums in fixed orders: identical bits from run to run, whatever the workspace held. */
int64_t ctrlsim_encoder_layer_grad_workspace_bytes(int B, int L, int F);
int ctrlsim_encoder_layer_grad(const float* X0, int ldx, const uint8_t* key_pad, const float* dY, int lddy,
                               const float* const* tensors /* 12 fp32 masters */, int B, int L, int F, void* workspace, float* grads,
                               float* dX0, int lddx0, float* u_out, hipStream_t stream);
/* ---- training: forward, loss, then the gradients of everything `scope` names behind the heads ---------------------------------------
 * ctrlsim_forward_loss_grads runs the teacher-forced forward on its own X, the loss (sums bit-identical to ctrlsim_forward_loss on the
 * same inputs) and the head gradients as described for ctrlsim_heads_loss_grad, then the ops above from the decoder's output back, as
 * far as `scope` says; each op's dY is the dX of the op behind it.  grads: ONE flat float32 buffer, the head tensors and then what each
 * scope appends, a narrower scope's buffer unchanged as a prefix of a wider one's:
 *   scope | tensors added to grads           | taps added       | forward, against the scope before      | models accepted   | workspace
 *   0     | the heads' tensors               | dX, x_out        | ctrlsim_forward_loss's                 | that entry's      | head-gradient carve
 *   1     | layers.{ND-1}: .linear1, .linear2| dU, u_out        | out-projection + norm2 and the feed-   | + ND >= 1, F >= 1 | + U, a dX, the
 *         | (weight, bias), .norm3           |                  | forward block as two kernels, U copied |                   | feed-forward op's
 *   2     | .multihead_attn in_proj_weight,  | dX1, dMem,       | + one row copy: X1, the norm1 output   | as scope 1        | + X1, a dU, the
 *         | in_proj_bias, out_proj, .norm2   | x1_out, mem_out  |                                        |                   | attention op's
 *   3     | .self_attn (the same), .norm1    | dX0[ND-1],       | + one row copy: X0, before the layer's | + dims.variant 0  | + X0, a dX1, the self-
 *         |                                  | x0_out[ND-1]     | first kernel                           | or 4 (mask_mode)  | attention op's
 *   4     | for l = ND-2 .. 0 the 18 tensors | dX0[l], x0_out[l]| + one row copy per earlier layer: X0_l,| + ND <= CTRLSIM_  | + ND-1 row buffers, a
 *         | of decoder layer l, in the layer | for l < ND; not  | before that layer's first kernel (the  | MAX_DECODER_LAYERS| dX0, the decoder layer
 *         | op's order                       | dU .. x1_out     | layers keep their fused forward)       |                   | op's
 *   5     | for l = NE-1 .. 0 the 12 tensors | dE0[l], e0_out[l]| + one row copy per encoder layer: E0_l,| + 0 <= NE <=      | + NE row buffers, a
 *         | of encoder layer l, in the layer | for l < NE       | before that layer's in_proj            | CTRLSIM_MAX_      | dMem, a dE0, the encoder
 *         | op's order                       |                  |                                        | ENCODER_LAYERS    | layer op's
 * Scopes 1 to 3 differentiate the LAST decoder layer (decoder.transformer_decoder.layers.{ND-1}) with the three sublayer ops.  Scope 4
 * then runs ctrlsim_decoder_layer_grad for l = ND-2 .. 0 on (X0_l, Mem, dY = dX0 of layer l + 1) with accumulate_dmem = 1; scope 5 then
 * runs ctrlsim_encoder_layer_grad for l = NE-1 .. 0 on (E0_l, the scene rows' key-padding bytes, dY), dY = dMem for the last encoder
 * layer and dE0[l + 1] otherwise.  For ND == 1 scope 4 IS scope 3, for NE == 0 scope 5 IS scope 4.
 * The gradient taps, [B*Tq*A*3, 256] each: dX at the decoder output; dU at the last layer's feed-forward block's input, its norm2 output;
 * dX1 at its norm1 output; dX0[l] at the rows that enter decoder layer l (dX0[0]: the assembled tokens).  dMem [B*M, 256], M = (P + A + 3)
 * & ~3 scene rows per context: the gradient at the scene encoder's output from every decoder layer the scope differentiates — the last
 * layer's contribution first, then descending l.  dE0[l] [B*M, 256]: the gradient at the scene rows that enter encoder layer l; dE0[0]
 * is the gradient at [polylines || initial states], rows of padded keys, the filler rows among them, exactly zero.  x_out, u_out,
 * x1_out, x0_out[l], mem_out and e0_out[l] receive the rows those gradients belong to, as the backward read them.  A non-null tap
 * outside the scopes named beside it below, a tap of a layer the scope does not differentiate (scope 3: any l but ND-1; l >= ND; l >=
 * NE), a scope outside 0 .. CTRLSIM_TRAIN_SCOPES - 1 or a model the scope does not accept: CTRLSIM_EINVAL, nothing launched.  taps ==
 * NULL: no tap.  Whatever a narrower scope returns, a wider one returns bit for bit.  The gradients are those of the function THIS call
 * evaluated: each op applied to its input rows as stored.  Rows of dX no head reads are zero; their dU is what the block's Jacobian
 * makes of a zero row.  A term with count 0 gives NaN gradients.
 * The layout query fills names[i] (state-dict names, static storage: valid until the next layout query) and offsets[i] (in floats) for
 * cap >= count entries and, if cap > count, offsets[count] = the total length; it returns the count and needs no device.  Workspace:
 * ctrlsim_train_grads_workspace_bytes(dims, B, Tq, scope); a dX / dU / dX1 / dX0 / dMem / dE0 of its own is the next op's dY where the
 * caller takes no such tap.  Scopes >= 3 also refuse B*Tq*A*3 * 768 >= 2^31. */
#define CTRLSIM_TRAIN_SCOPES 6
#define CTRLSIM_MAX_DECODER_LAYERS 8
#define CTRLSIM_MAX_ENCODER_LAYERS 8
typedef struct ctrlsim_train_taps {          /* every member nullable */
  float *dX, *x_out;                         /* scope >= 0 */
  float *dU, *u_out;                         /* scopes 1..3 */
  float *dX1, *x1_out;                       /* scopes 2..3 */
  float *dMem, *mem_out;                     /* scope >= 2 */
  float *dX0[CTRLSIM_MAX_DECODER_LAYERS], *x0_out[CTRLSIM_MAX_DECODER_LAYERS];   /* scope 3: index ND-1 only; scope >= 4: 0..ND-1 */
  float *dE0[CTRLSIM_MAX_ENCODER_LAYERS], *e0_out[CTRLSIM_MAX_ENCODER_LAYERS];   /* scope 5: 0..NE-1 */
} ctrlsim_train_taps;
int ctrlsim_train_grad_layout(const ctrlsim_dims* dims, int has_future_states, int scope, int cap, const char** names, int64_t* offsets);
int64_t ctrlsim_train_grads_workspace_bytes(const ctrlsim_dims* dims, int B, int Tq, int scope);
int ctrlsim_forward_loss_grads(const ctrlsim_model* m, int B, int Tq, const ctrlsim_ctx* ctx, const uint8_t* moving,
                               const ctrlsim_loss_cfg* cfg, float loss_action_coef, int scope, void* workspace, double* sums,
                               double* per_ctx, float* grads, const ctrlsim_train_taps* taps /* nullable */, hipStream_t stream);
/* The same sums and counts from the logits of ctrlsim_forward_all in memory (compute_loss(data, preds) in the reference's call shape):
 * action_preds [B,Tq,A,V], rtg_preds [B,Tq,A,R*C] bin-major / component-minor, state_preds [B,Tq,A,2T]; the last two nullable.
 * scratch: ctrlsim_loss_scratch_bytes. */
int64_t ctrlsim_loss_scratch_bytes(int B, int Tq, int A);
int ctrlsim_loss_from_preds(const ctrlsim_dims* dims, int B, int Tq, const ctrlsim_ctx* ctx, const uint8_t* moving,
                            const ctrlsim_loss_cfg* cfg, const float* action_preds, const float* rtg_preds, const float* state_preds,
                            void* scratch, double* sums, double* per_ctx, float* row_nll, hipStream_t stream);
/* pass 2 (same workspace, after ctrlsim_sample_rtg wrote hist_rtg[...,t,:]): act_logits [B,A,V].
 * cached = 1 pairs with ctrlsim_dt_forward_pass1_cached (workspace sized with Tq = T, ctx = last min(Tq,2) window rows). */
int ctrlsim_dt_forward_pass2(const ctrlsim_model* m, int B, int Tq, int t, int N, int Tmax, const ctrlsim_ctx* ctx,
                             const int* ctx_scn, const int* hist_rtg, void* workspace, float* act_logits, int cached,
                             hipStream_t stream);
/* pass 1 while the window still starts at step 0 (t < T) for a FIXED set of contexts: the scene side is evaluated at
 * t == 0 only and decoder K/V are cached per layer in `workspace` (ctrlsim_forward_workspace_bytes(dims, B, T), the same
 * buffer at every step); step t re-evaluates the 4A rows whose inputs changed.  ctx holds the window rows
 * [max(t-1,0), t] (ctrlsim_build_context with tt_first = max(t-1,0)). */
int ctrlsim_dt_forward_pass1_cached(const ctrlsim_model* m, int B, int t, const ctrlsim_ctx* ctx, void* workspace,
                                    float* rtg_logits, hipStream_t stream);

/* ---- sampling -------------------------------------------------------------------------------------------------
 * Replaces Policy.process_predicted_rtg (policies/policy.py:108-142) and the action-sampling block of
 * AutoregressivePolicy.predict (autoregressive_policy.py:211-240): tilt, softmax, torch.multinomial as an
 * exponential race with explicit (noise != NULL) or in-kernel counter-based Exp(1) noise.
 * tilt3 = (goal, veh_veh, veh_edge) tilts of the policy (host pointer; tilt_dict of policies/policy.py:20-25) applied to
 * every scenario, unless tilt_scn (device, [S,3]) gives one triple per scenario — a reward-tilt sweep in one batch. */
int ctrlsim_sample_rtg(const float* rtg_logits, int A, int R, const int* own_ctx, const int* own_slot,
                       const uint8_t* tilted, const double* tilt3, const double* tilt_scn /*[S,3] or NULL*/,
                       const float* noise /*[S*N,3,R] or NULL*/, uint64_t seed, const int64_t* scenario_id /*[S]*/, int t,
                       int* hist_rtg, int S, int N, int Tmax, hipStream_t stream);
/* The same with logits rows addressed through ctx_row0 (context c, slot s -> row ctx_row0[c] + s): batches of compact contexts
 * of different slot counts (ctrlsim_ctx_index_classes). */
int ctrlsim_sample_rtg_rows(const float* rtg_logits, const int* ctx_row0, int R, const int* own_ctx, const int* own_slot,
                            const uint8_t* tilted, const double* tilt3, const double* tilt_scn, const float* noise, uint64_t seed,
                            const int64_t* scenario_id, int t, int* hist_rtg, int S, int N, int Tmax, hipStream_t stream);
int ctrlsim_sample_action_rows(const float* act_logits, const int* ctx_row0, int V, const int* mem_ctx, const int* mem_slot,
                               float temperature, double top_p, const float* noise, uint64_t seed, const int64_t* scenario_id,
                               int t, int* hist_tok, int* act_now, int S, int N, int Tmax, int zero_token, hipStream_t stream);
int ctrlsim_sample_action(const float* act_logits, int A, int V, const int* mem_ctx, const int* mem_slot,
                          float temperature, double top_p /*<=0: off*/, const float* noise /*[S*N,V] or NULL*/,
                          uint64_t seed, const int64_t* scenario_id, int t, int* hist_tok, int* act_now /*[S,N]*/,
                          int S, int N, int Tmax, int zero_token, hipStream_t stream);

/* ---- real-time reward ledger (Decision-Transformer baseline) --------------------------------------------------------
 * Replaces the host bookkeeping of a policy with real_time_rewards (cfgs/policy/dt.yaml): PolicyEvaluator.update_vehicle_data_dict
 * (evaluators/policy_evaluator.py:122-147: RTG_0, RTG_t = RTG_{t-1} - dense_reward_{t-1}) + Evaluator.compute_dense_reward
 * (evaluators/evaluator.py:106-140; datasets/rl_waymo/dataset.py:187-275; utils/data.py:152-290) + the clip-normalisation of
 * AutoregressivePolicy.get_data (policies/autoregressive_policy.py:73-78).  Call once per step t, after the simulator wrote the
 * states of step t and before the contexts of step t are built: hist_rtg[S,N,Tmax,3][.., t, :] <- float bits of the normalised
 * RTG (what a variant-3 model reads); `ledger` [S,N,10] float64 carries RTG / dense reward / step-0 reward flags between calls
 * (t = 0 initialises it); init_rtg [S,N,3] float64 or NULL = (10, 90, 90) (max_return); rtg_raw [S,N,Tmax,3] float64 nullable.
 * `edges` is the simulator's road-edge segment table [S,E,4]. */
typedef struct ctrlsim_dt_reward_cfg {
  double pos_tol;        // cfg.nocturne.rew_cfg.position_target_tolerance
  double shaped_unit;    // shaped_goal_distance_scaling / reward_scaling (utils/sim.py:112-118)
  double goal_mult, shaped_min, shaped_max;     // pos_target_achieved_rew_multiplier, pos_goal_shaped_min / _max
  double veh_mult, max_veh_dist;                // veh_veh_collision_rew_multiplier, max_veh_veh_distance
  double edge_mult, edge_scale;                 // veh_edge_collision_rew_multiplier, dist_to_road_edge_scaling_factor
  double rtg_lo[3], rtg_hi[3];                  // min / max_rtg_pos, _veh, _road
  int remove_shaped_goal, remove_shaped_veh, remove_shaped_edge, pad_;
} ctrlsim_dt_reward_cfg;
int ctrlsim_dt_ledger_step(int S, int N, int E, int t, int T1, int Tmax, const float* hist_states, const uint8_t* coll,
                           const double* goals /*[S,N,5]: x, y first*/, const float* edges, const double* init_rtg,
                           const ctrlsim_dt_reward_cfg* cfg, double* ledger, double* rtg_raw, int* hist_rtg, hipStream_t stream);

/* ---- offline-RL dataset generation (csrc/dataset.hip) ---------------------------------------------------------------
 * Replaces what stands between a rolled, fully logged batch (data/generate_offline_rl_dataset.py:17-144: ctrlsim_replay_actions with
 * nothing controlled, ctrlsim_sim_step, ctrlsim_replay_latch) and the `*_physics.pkl` dictionaries of RLWaymoDatasetCtRLSim.get_data
 * (datasets/rl_waymo/dataset.py:111-275, dataset_ctrl_sim.py:54-97) with their returns-to-go.  The dataset holds T <= T1 steps: rows
 * 0 .. T-1 of hist_states [S,N,T1,8] / coll [S,N,T1,2]; exist [S,N,T] f64 is the DATASET's existence (the `exists` flag of
 * ctrlsim_replay_actions per step: logged now and at the next step, latched).  All float64, the NumPy expressions of the host forms
 * operation by operation; N <= 64.
 * ctrlsim_dataset_edge_distance — out [S,N,T] = compute_distance_to_road_edge (utils/data.py:152-290): the SIGNED distance of every
 * point to the first road-edge polyline of minimum |signed distance| (host form: rewards.signed_distance_to_road_edges).  edges
 * [S,E,4] is the simulator's segment table; poly_off [S,PE+1] i32 cuts a scene's segments into polylines in the order of its road-edge
 * polylines: polyline p = segments poly_off[s,p] .. poly_off[s,p+1]-1, poly_off[s,0] = 0, unused entries repeat the end (a one-point
 * polyline has no segment).  exist NULL = column 7 of hist_states.  A point that does not exist is written as 0 without being
 * evaluated; in a scene without segments an existing point gets +inf (callers refuse such scenes: the reference raises there).
 * ctrlsim_dataset_edge_distance_f64 — the same kernel on plain float64 tables: P query points per scene xy [S,P,2], edges [S,E,4] f64,
 * exist [S,P] (NULL = every point exists), out [S,P]: for positions and polylines that float32 does not hold (the reference's own
 * fixture values among them).
 * ctrlsim_dataset_rewards — ag_rewards [S,N,T,8] = compute_reward rows (utils/sim.py:83-141; host form metrics.compute_rewards) times
 * existence, the collision flags being those of the row's own step; veh_veh [S,N,T] = clip(nearest existing vehicle, 0, max) / max,
 * 0 when absent or alone; veh_edge [S,N,T] = -edge_dist / edge_scale * existence from ctrlsim_dataset_edge_distance's output; rtgs as
 * ctrlsim_dataset_rtgs.  goals4 [S,N,4] f64 = goal x, y, heading, speed (after initialize_goal_dict).
 * ctrlsim_dataset_rtgs — rtgs [S,N,T,5] from the dictionary's arrays (host form ingest.load_preprocessed): compute_rewards' five
 * components (goal position, heading, speed, vehicle, road edge; the remove_shaped_* switches honoured) times existence, summed from
 * the last step backwards in np.cumsum's order. */
typedef struct ctrlsim_dataset_cfg {
  double pos_tol, heading_tol, speed_tol;       // cfg.nocturne.rew_cfg.position / heading / speed_target_tolerance
  double shaped_scaling, reward_scaling;        // shaped_goal_distance_scaling, reward_scaling
  double goal_mult, shaped_min, shaped_max;     // pos_target_achieved_rew_multiplier, pos_goal_shaped_min / _max
  double veh_mult, max_veh_dist;                // veh_veh_collision_rew_multiplier, max_veh_veh_distance
  double edge_mult, edge_scale;                 // veh_edge_collision_rew_multiplier, dist_to_road_edge_scaling_factor
  int remove_shaped_goal, remove_shaped_veh, remove_shaped_edge, pad_;
} ctrlsim_dataset_cfg;
int ctrlsim_dataset_edge_distance(int S, int N, int T, int T1, int E, int PE, const float* hist_states, const double* exist,
                                  const float* edges, const int* poly_off, double* out, hipStream_t stream);
int ctrlsim_dataset_edge_distance_f64(int S, int P, int E, int PE, const double* xy, const double* exist, const double* edges,
                                      const int* poly_off, double* out, hipStream_t stream);
int ctrlsim_dataset_rewards(int S, int N, int T, int T1, const float* hist_states, const uint8_t* coll, const double* exist,
                            const double* goals4, const double* edge_dist, const ctrlsim_dataset_cfg* cfg, double* ag_rewards,
                            double* veh_veh, double* veh_edge, double* rtgs, hipStream_t stream);
int ctrlsim_dataset_rtgs(int S, int N, int T, const double* ag_rewards, const double* veh_veh, const double* veh_edge,
                         const double* exist, const ctrlsim_dataset_cfg* cfg, double* rtgs, hipStream_t stream);

/* ---- open-loop training windows (csrc/window.hip) --------------------------------------------------------------------
 * Replaces the training-mode half of RLWaymoDatasetCtRLSim.get_data (datasets/rl_waymo/dataset_ctrl_sim.py:99-160 with
 * select_relevant_agents and normalize_scene, dataset.py:278-319,390-428; host form ingest.training_window) for B windows per launch,
 * cut from a batch of S scenes of equal vehicle count N <= 64 and equal step count Td >= T that is already on the device, and written
 * straight into the context tensors ctrlsim_forward_loss reads.  Float inputs are float64 and hold the values of the `*_physics.pkl`
 * dictionary: ag_data [S,N,Td,8] (x, y, vx, vy, heading, length, width, existence), actions [S,N,Td,2], rtgs [S,N,Td,5] (the five
 * returns-to-go of ctrlsim_dataset_rtgs; components 0, 3, 4 are used), goals5 [S,N,5], types [S,N,5], road_points [S,Pmax,NP,3],
 * road_types [S,Pmax,8], n_polys [S] i32 (rows beyond n_polys[s] are never read).  Window b is (win_scn[b], win_t0[b], win_agent[b]):
 * scene, first step, and the origin agent as an index into the scene's FILTERED agents (those that exist at dataset step 0, ascending).
 * out: st12 [B,T,A,12], exist [B,T,A], goal5 [B,A,5], act_tok [B,T,A], rtg_bin [B,T,A,3] (bins, or float32 bits of the normalised
 * returns when cfg.continuous_rtg), tstep [B,T], road_pts [B,P,NP,3], road_types [B,P,8], slot_gid [B,A] = 0 .. A-1 (nullable);
 * moving [B,A] u8 (moving_agent_mask); status [B] i32.  Agents: the A nearest filtered agents at the window's first step, intersected
 * with distance < agent_dist_threshold, in ascending agent order; padded slots hold the transform of a zero state, types -1, the token
 * of the zero action and zero returns.  Roads: n_polys[s] > P keeps the P polylines of smallest max(existing point distance), nearest
 * first; otherwise all in order, the rest zeros with types -1.  Ties in either ranking go to the lower index.  Geometry is float64 in
 * the origin agent's frame (x' = c dx - s dy, y' = s dx + c dy, no FMA contraction), rounded once to float32; device sin / cos may
 * differ from libm by an ulp, integers (tokens, bins, time steps, selections away from ties) are exact.
 * A triple that cannot be served reads nothing of the dataset, leaves an all-padding window (zero states, types -1, zero-action
 * tokens, zero returns and time steps, zero polylines with types -1, nothing moving) and a non-zero status; valid windows get 0. */
enum {
  CTRLSIM_WINDOW_OK = 0,
  CTRLSIM_WINDOW_SCENE = 1,     /* win_scn outside [0, S) */
  CTRLSIM_WINDOW_STEP = 2,      /* win_t0 < 0 or win_t0 + T > Td */
  CTRLSIM_WINDOW_AGENT = 3,     /* win_agent outside the scene's filtered agents */
  CTRLSIM_WINDOW_ABSENT = 4,    /* the origin agent does not exist at the window's first step */
  CTRLSIM_WINDOW_STILL = 5      /* the origin agent is not a moving agent */
};
typedef struct ctrlsim_window_cfg {
  double agent_dist_threshold, moving_threshold;     // cfg.dataset.waymo.agent_dist_threshold, moving_threshold
  double rtg_lo[3], rtg_hi[3];                       // min / max_rtg_pos, _veh, _road
  double min_accel, max_accel, min_steer, max_steer; // discretize_actions (ctrlsim_amd/discretize.py)
  int rtg_discretization, accel_discretization, steer_discretization;
  int continuous_rtg;                                // Decision Transformer: rtg_bin holds float32 bits
} ctrlsim_window_cfg;
int ctrlsim_window_build(int B, int S, int N, int Td, int T, int A, int Pmax, int P, int NP, const double* ag_data,
                         const double* actions, const double* rtgs, const double* goals5, const double* types,
                         const double* road_points, const double* road_types, const int* n_polys, const int* win_scn,
                         const int* win_t0, const int* win_agent, const ctrlsim_window_cfg* cfg, const ctrlsim_ctx* out,
                         uint8_t* moving, int* status, hipStream_t stream);

/* ---- metrics ----------------------------------------------------------------------------------------------------
 * Replaces PolicyEvaluator.update_running_statistics (evaluators/policy_evaluator.py:162-248) with compute_reward's goal latch
 * (utils/sim.py:99-104) and compute_nearest_dist_all (evaluators/evaluator.py:87-103) for S finished rollouts: out[0 ..
 * ctrlsim_metrics_size()) += the packed accumulators — sums and counts of (goal, per-scenario collision rate, per-scenario
 * off-road rate, ADE, FDE) and the eight histograms compute_metrics builds (policy_evaluator.py:251-305), in the order of
 * ctrlsim_amd/metrics.py:MetricAccumulators.pack.  This vector is what the ranks all-reduce (the only collective of a
 * multi-GPU run).  gt [S,N,T1,5] = logged x, y, heading, speed, exist; goals4 [S,N,4] = goal x, y, heading, speed (after
 * initialize_goal_dict); eval_mask [S,N] (NULL = all vehicles evaluated); params5 (host) = position tolerance, min_accel,
 * max_accel, n_accel_bins, n_steer_bins; edges (device) = the histogram edges lin[201] ang[201] accel[21] nearest[201].  The applied
 * acceleration of a step is the centre of the sampled token's acceleration bin. */
int ctrlsim_metrics_size(void);
int ctrlsim_metrics_pack(int S, int N, int T1, int Tmax, int hist_steps, double dt, const float* hist_states, const uint8_t* coll,
                         const int* hist_tok, const double* gt, const double* goals4, const uint8_t* eval_mask,
                         const double* params5, const double* edges, double* out, hipStream_t stream);

/* ---- building blocks (exported for parity tests and profiling) ------------------------------------------------ */
int ctrlsim_gemm_nt(const float* A, int lda, const float* W, int ldw, const float* bias, const float* R, int ldr,
                    float* C, int ldc, int M, int N, int K, int relu, hipStream_t stream);
/* Same product evaluated on the bf16 MFMA with fp32-class accuracy: W3 = the weight split into three bf16 planes, slab-major
 * [K/16][3][2][n_total][8] (ctrlsim_amd/pack.py:split3_planes); rows [n0, n0+N) of it are used; A stays fp32.
 * ln_gamma/ln_beta non-NULL (N must be 256): C = [relu] LayerNorm(A W^T + bias [+ R]) * gamma + beta, eps 1e-5 — the
 * post-LN residual blocks of nn.TransformerEncoder/DecoderLayer and the Linear-LayerNorm-ReLU halves of MLPLayer
 * (modules/layers.py) as one kernel; C may alias R. */
int ctrlsim_gemm_nt_bf16x6(const float* A, int lda, const void* W3, int n_total, int n0, const float* bias, const float* R,
                           int ldr, float* C, int ldc, int M, int N, int K, int relu, const float* ln_gamma,
                           const float* ln_beta, hipStream_t stream);
/* Plain Linear 256 -> 256 (W3 rows [n0, n0 + 256), K = 256, two-fp16-plane scheme) whose result row i is written to row c_rows[i] of C
 * (device int32 list of M entries; an entry < 0 is not stored): the map encoder's last Linear (modules/map_encoder.py:53 feeding
 * modules/encoder.py:155-158's concatenation) writes the polyline rows of the scene-encoder source [b, 0..P-1] itself, no copy kernel.
 * Returns 1 — nothing launched — when the weight-stationary kernel does not apply (bf16x6 split selected, option 6 off): the caller
 * runs ctrlsim_gemm_nt_bf16x6 + a row copy instead. */
int ctrlsim_gemm256_rows(const float* A, int lda, const void* W3, int n_total, int n0, const float* bias, float* C, int ldc,
                         const int* c_rows, int M, hipStream_t stream);
/* The same Linear whose last 512 output columns [kv_col0, kv_col0 + 512) are the keys / values of 8 heads x 32 of contexts of
 * kv_L rows each: those columns leave the epilogue directly as the split K / V tile images of ctrlsim_kv_split (kv_nkt 64-key
 * tiles per context and head; the tail of the last tile must be zeroed by the caller), columns [0, kv_col0) as fp32 rows of C.
 * The in_proj of nn.MultiheadAttention (modules/decoder.py:16-20, encoder.py:42-46) fused with the attention kernel's operand
 * preparation. */
int ctrlsim_gemm_nt_kv(const float* A, int lda, const void* W3, int n_total, int n0, const float* bias, float* C, int ldc,
                       int M, int N, int K, void* kv_img, int kv_L, int kv_nkt, int kv_col0, hipStream_t stream);
/* The same operation through the row-stationary kernel (two-fp16-plane scheme only; CTRLSIM_EINVAL otherwise): Wblk = the weight as
 * 32-column operand blocks (ctrlsim_amd/pack.py:row_blocks of rows [n0, n0 + N) of the weight; N = kv_col0 + 512, a multiple of 32, at
 * most 768), bias = its N entries; K = 256.  Every activation row is read once; outputs as for ctrlsim_gemm_nt_kv.  kv_img == NULL: a
 * plain Linear (N a multiple of 32 in [64, 768]; kv_L / kv_nkt / kv_col0 ignored), all N columns as fp32 rows of C. */
int ctrlsim_gemm_kv_blocks(const float* A, int lda, const void* Wblk, const float* bias, float* C, int ldc, int M, int N,
                           void* kv_img, int kv_L, int kv_nkt, int kv_col0, hipStream_t stream);
/* The last Linear of an MLP head with a cross-entropy epilogue (csrc/loss.hip; two-fp16-plane scheme, returns 1 — nothing launched —
 * otherwise): H [M,256] hidden rows, Wce / bias_ce = ctrlsim_amd/pack.py:head_ce_image of the Linear (nsm interleaved softmaxes of n classes,
 * nsm <= 4), tgt [M,nsm] target classes; lt [M,4,2] receives (log-sum-exp, target logit) of softmax s at [row, s, :].  Nothing of size
 * n is written.  F.cross_entropy(reduction='none') of models/ctrl_sim.py:65,82,95-105 is lt[..., 0] - lt[..., 1]. */
int ctrlsim_head_ce(const float* H, int ldh, const void* Wce, const float* bias_ce, const int* tgt, int M, int n, int nsm, float* lt,
                    hipStream_t stream);
/* Post-LN feed-forward block of nn.TransformerEncoderLayer / DecoderLayer as one kernel:
 * Y = LayerNorm(X + W2 relu(W1 X + b1) + b2) * gamma + beta, rows of 256, F hidden units (multiple of 32); W1p / W2p are the
 * operand images of ctrlsim_amd/pack.py:ffn_planes; Y may alias X.  The hidden activation never touches memory. */
int ctrlsim_ffn_fused(const float* X, int ldx, const void* W1p, const float* b1, const void* W2p, const float* b2,
                      const float* gamma, const float* beta, float* Y, int ldy, int M, int F, hipStream_t stream);
/* The post-LN block in front of the feed-forward block fused into it (round 5, two-fp16-plane scheme only; CTRLSIM_EINVAL otherwise):
 * X1 = LayerNorm0(R + Wo O + bo), Y = LayerNorm(X1 + W2 relu(W1 X1 + b1) + b2) — the attention out-projection with its residual and
 * LayerNorm (nn.TransformerDecoderLayer: multihead_attn.out_proj + norm2; nn.TransformerEncoderLayer: self_attn.out_proj + norm1;
 * modules/decoder.py:16-20, encoder.py:42-46) and the feed-forward block behind it as one kernel: X1 is neither written nor re-read.
 * O = attention output rows, R = residual rows (Y may alias R or O), Wop / W1q / W2p = ctrlsim_amd/pack.py:ffn_planes_pre(Wo, W1, W2). */
int ctrlsim_ffn_fused_pre(const float* O, int ldo, const float* R, int ldr, const void* Wop, const float* bo, const float* g0,
                          const float* be0, const void* W1q, const float* b1, const void* W2p, const float* b2, const float* gamma,
                          const float* beta, float* Y, int ldy, int M, int F, hipStream_t stream);
/* X1 = LayerNorm0(R + Wo O + bo) and Q = Wq X1 + bq as one kernel (round 5, two-fp16-plane scheme only): a decoder layer's
 * self_attn.out_proj + residual + norm1 and the query third of multihead_attn.in_proj behind it (nn.TransformerDecoderLayer._sa_block /
 * _mha_block; modules/decoder.py:16-20) — the row goes in once, x1 and q come out.  X1 may alias R.  Wop / Wqp =
 * ctrlsim_amd/pack.py:outproj_q_planes(Wo, Wq). */
int ctrlsim_outproj_ln_q(const float* O, int ldo, const float* R, int ldr, const void* Wop, const float* bo, const float* g0, const float* be0,
                         const void* Wqp, const float* bq, float* X1, int ldx1, float* Q, int ldq, int M, hipStream_t stream);
int ctrlsim_layernorm256(const float* X, int ldx, const float* Radd, int ldr, const float* gamma, const float* beta,
                         float* Y, int ldy, int rows, int relu, hipStream_t stream);
/* mode 0: key padding (key_pad [B,Lk], 1 = ignore); mode 1: CtRL-Sim structured causal mask (utils/train_utils.py:81-129); modes 2 / 3 / 4
 * (split-operand kernels only): the IL / Trajeglish / Decision-Transformer masks of the same function; mode 5 (round 6): mode 1 with
 * cfg.model.attend_own_return_action (:114-129) — of the earlier timesteps a query sees the state tokens and its own agent's tokens only */
int ctrlsim_attention(int mode, const float* Q, int ldq, int64_t q_batch_stride, const float* K, const float* V,
                      int ldkv, int64_t kv_batch_stride, float* O, int ldo, int64_t o_batch_stride, const int* q_pos,
                      const uint8_t* key_pad, int B, int Lq, int Lk, int A, hipStream_t stream);
/* Split-bf16 K/V images for the bf16x6 attention (csrc/attention_bf16x6.hip): per (context, head, 64-key tile) 24 KB =
 * K planes [3][d>>3][key][d&7] then V^T planes [3][key>>2][d][key&3], bf16; img holds B * 8 * nkt tiles.
 * pos == NULL: rows [0, rows) of every context are split, keys beyond are zero-filled (rows <= 64 * nkt);
 * pos != NULL: row r of context b is written at key position pos[r] (KV-cache update; other keys untouched). */
int ctrlsim_kv_split(const float* K, const float* V, int ldkv, int64_t kv_batch_stride, const int* pos, int B, int rows,
                     int nkt, void* img, hipStream_t stream);
/* ctrlsim_attention with K/V taken from such images (staged by LDS-DMA, no in-kernel split); same modes and masks. */
int ctrlsim_attention_presplit(int mode, const float* Q, int ldq, int64_t q_batch_stride, const void* img, int nkt, float* O,
                               int ldo, int64_t o_batch_stride, const int* q_pos, const uint8_t* key_pad, int B, int Lq,
                               int Lk, int A, hipStream_t stream);

/* Causal (CtRL-Sim mask) attention over the K/V images of COMPACT contexts: Lk regular keys (slots < A) in the tiles
 * [0, ceil(Lk/64)), rep_keys representative keys (3 per window step, multiplicity rep_mult) in the tiles from ceil(rep_pos0/64)
 * on; rep_pos0 >= Lk = the regular length of the full window (K/V-cache layout).  Query positions (row index or q_pos) >=
 * rep_pos0 are the representative's own tokens.  A representative key (t, k) is visible to a query of step tq iff t < tq or
 * (t == tq and k == 0), rep_mult-fold (log2(rep_mult) is added to its score); the representative's own queries also see their
 * tokens 1..kq of step tq, once.  rep_keys = 0: ctrlsim_attention_presplit mode 1. */
int ctrlsim_attention_compact(const float* Q, int ldq, int64_t q_batch_stride, const void* img, int nkt, float* O, int ldo,
                              int64_t o_batch_stride, const int* q_pos, int B, int Lq, int Lk, int A, int rep_keys, int rep_mult,
                              int rep_pos0, hipStream_t stream);

/* Visibility-mask table of one class of causal launches over the TOKEN ROWS (query row i = position i; round 4).  The structured mask of
 * utils/train_utils.py:81-129 (get_causal_mask) — and the representative's rules above — depends on (query position, key position) of the
 * class only, so the forward evaluates it once per pass instead of per (context, head, layer, query).  Layout (csrc/attention_bf16x6.hip):
 * per query group of 32 rows and per 32-key sub-tile (2 * nkt of them: the regular tiles, then the representative's) 32 x uint64 — sixteen
 * lane masks of the visible (query, key) pairs in the kernel's accumulator order, then sixteen of the representative's count-once keys.
 * Round 6: behind the mask entries the table carries the kernel's control flow — per query group the tile schedule of its 256-query block
 * (regular / representative tiles that hold a key some query of the block sees) and per (group, 64-key tile) one 32-bit word with a 2-bit
 * code per sub-tile (0 skip, 1 every key visible, 2 apply the masks, 3 masks + count-once keys); ctrlsim_attention_mask_table_bytes covers both.
 * ctrlsim_attention_tbl = ctrlsim_attention_compact with q_pos == NULL and rep_pos0 == Lk, masks taken from the table (same results). */
int64_t ctrlsim_attention_mask_table_bytes(int Lq, int nkt);
int ctrlsim_attention_mask_table(int Lq, int Lk, int A, int rep_keys, int rep_pos0, int nkt, void* tbl, hipStream_t stream);
int ctrlsim_attention_tbl(const float* Q, int ldq, int64_t q_batch_stride, const void* img, int nkt, float* O, int ldo,
                          int64_t o_batch_stride, int B, int Lq, int Lk, int A, int rep_keys, int rep_mult, const void* mask_tbl,
                          hipStream_t stream);

/* ---- measurement hooks (bench.py): HIP-event timing of every launch of ctrlsim_prof_classes() kernel classes on its own
 * launch stream — 0 GEMM (all Linear layers incl. the fused feed-forward block), 1 attention, 2 build_context, 3 assemble_tokens,
 * 4 sim_step, 5 map_pool.  enable(1) clears and starts recording; after the caller synchronised, collect() returns per class
 * the summed milliseconds, the launch count and the algorithmic FLOPs (2*M*N*K; 128 per visible (query,key) pair and head);
 * bytes() the compulsory HBM bytes (operands read once + results written once) of the same launches.  Arrays hold
 * ctrlsim_prof_classes() entries.  Process-global and single-threaded like the options below: one host thread per GPU. */
int ctrlsim_prof_classes(void);
void ctrlsim_prof_enable(int on);
int ctrlsim_prof_collect(double* ms, int64_t* count, double* flops);
int ctrlsim_prof_bytes(double* bytes);
/* ctrlsim_prof_collect + ctrlsim_prof_bytes restricted to the launches on `stream` (on_stream != 0) or on every other stream
 * (on_stream == 0): intervals of kernels that run concurrently on different streams overlap in time. */
int ctrlsim_prof_collect_stream(hipStream_t stream, int on_stream, double* ms, int64_t* count, double* flops, double* bytes);
/* Kernel-level rows inside the two MFMA classes, same restriction by stream.  Row 2 * kind + few: kind 0 other, 1 Linear with K/V
 * image epilogue (QKV / memory K-V projections), 2 Linear + residual + LayerNorm, 3 plain Linear, 4 fused feed-forward block,
 * 5 causal self-attention, 6 key-padded (scene / cross) attention; few = 1 for the few-row launches (last decoder layer on the
 * queried rows, second pass, K/V-cached steps).  Arrays hold ctrlsim_prof_subclasses() entries. */
int ctrlsim_prof_subclasses(void);
int ctrlsim_prof_collect_sub(hipStream_t stream, int on_stream, double* ms, int64_t* count, double* flops, double* bytes);

/* Per-size-class accounting of the causal self-attention launches over the token rows (profiling runs only: one atomic per workgroup).
 * enable != 0: clear and start; enable == 0: stop and (host_out != NULL, 64 x uint64, synchronises) copy out — host_out[2 s] = shader
 * cycles of the workgroups of the classes with s context slots (kernel entry to last store, summed), host_out[2 s + 1] = workgroups. */
int ctrlsim_attn_class_prof(int enable, unsigned long long* host_out);

/* Runtime options (csrc/common.h: OPT_*).  Keys 0 / 1 = attention / GEMM path of the forward: value 0 = f32-input MFMA
 * (v_mfma_f32_32x32x2_f32), 1 = split-operand 16-bit MFMA with fp32-class accuracy (default).  Key 2 = tile shape of the tiled
 * split-operand GEMM (0 auto; tuning).  Key 3 = fused feed-forward block (default 1).  Key 4 = operand split (1 two fp16 planes,
 * 0 three bf16 planes; per engine through ctrlsim_bind).  These are the PROCESS DEFAULTS; an engine overrides them with its own table (ctrlsim_bind_options).  Key 5 = reserved (rounds 2-3: a matrix-pipe variant of the map-encoder pooling, removed).
 * Key 3 value 2 (default) = also the attention out-projection + residual + LayerNorm in front of a feed-forward block as its leading product
 * (ctrlsim_ffn_fused_pre; two-plane scheme); 3 = and a decoder layer's self-attention out-projection + LayerNorm with the cross-attention
 * query projection behind it as one kernel (ctrlsim_outproj_ln_q; measured slightly slower than 2 in the rollout, kept selectable);
 * 1 = the feed-forward block alone; 0 = separate Linear kernels.
 * Key 6 = weight-stationary kernel for the Linear(256 -> 256 G) shapes, bit mask: 1 = launches of at least two 32-row blocks per
 * compute unit, 2 = smaller launches, 4 = the in_proj Linears with K / V-image epilogue, 8 = those through the ROW-stationary kernel
 * (rows in registers, 32-column weight blocks streamed through LDS, every activation row read once; needs the block images of
 * pack.py:row_blocks in the packed weights) inside the forward, 16 = the tall plain 256 -> 256 Linears through it as well (measured
 * slower: off) (default 15; 0 = tiled kernel everywhere).
 * Key 7 = causal self-attention over the token rows takes its visibility masks from the per-class table (default 1; 0 = built per query).
 * Key 8 = the last decoder layer of a rollout pass projects keys / values of every token and queries of the queried tokens only (default 1;
 * 0 = the whole in_proj for every token, then a gather).
 * Key 9 = attention launches with at most 96 queries per context (second pass, last layer on the queried rows, K/V-cached steps) through
 * the streaming form of the kernel: one wave per (context, head, 32 queries), K / V fragments read straight from the tile images
 * (default 1; 0 = the LDS-staged 128-query form for every launch). */
int ctrlsim_set_option(int key, int value);
/* Operand split compiled into the library (csrc/split.h): 1 = two fp16 planes / three products (weights pre-scaled by 2^8), 0 = three
 * bf16 planes / six products.  ctrlsim_amd/pack.py packs weight planes and sizes the K/V images accordingly. */
int ctrlsim_split_scheme(void);
/* Guard events since the last reset.  The guard is a PAIR of device int32 words: [0] non-finite events of the model — sampling races
 * (ctrlsim_sample_rtg / _action) that no finite score won, and rows whose LayerNorm variance was not finite in any fused LayerNorm of the
 * forward (the ReLUs of the MLP heads map NaN to 0, so the logits alone do not show an overflow of the fp16 range of the two-plane operand
 * split) — and [1] simulator events: contacts of an island beyond the solver's table (ctrlsim_sim_step).  Callers check the count (>= 0;
 * synchronises the device) and fail or repeat with ctrlsim_set_option(4, 0).  reset != 0 clears it.  The library's own pair is allocated at
 * first use on the current device; it receives the events of launches made while NO caller-owned pair is bound (ctrlsim_bind below), and
 * this function always reads the library's own pair, never a bound one.  Return value: min(non-finite events, 65535) +
 * 65536 * min(simulator events, 32767) — count % 65536 and count / 65536 tell them apart, and neither kind can carry into the other
 * (the device counts them in separate words). */
int ctrlsim_nonfinite_count(int reset);
/* Per-caller state instead of the process-wide defaults: split_scheme (0 / 1; -1 = leave as is) selects the operand split the
 * caller's weight planes, K/V images and workspace were built for, guard_counter points at TWO device int32 the CALLER owns (zeroed and
 * read by the caller: the library neither allocates nor synchronises for them) that receive every guard event until the next bind —
 * [0] the non-finite events above, [1] the simulator events.  NULL = the library's own pair behind ctrlsim_nonfinite_count.  An engine
 * re-asserts its state at the top of every run, so several engines (planner and adversary policies, a second model) can take turns in one
 * process; still one host thread at a time.  Replaces nothing in the reference: its per-process analogue is nocturne's global Box2D world
 * (physics/Singletons.cpp:5-25). */
int ctrlsim_bind(int split_scheme, int* guard_counter);
/* Before the caller frees a bound pair: un-binds it if it is the bound one (no-op otherwise). */
int ctrlsim_unbind(const int* guard_counter);
/* The pair bound at the moment (NULL = the library's own): a caller that binds its own for ONE call (Simulation.step) restores this one. */
int* ctrlsim_bound_guard(void);
/* Per-engine option table (round 5): values = ctrlsim_option_count() ints in host memory (copied); an entry >= 0 overrides the process
 * default of ctrlsim_set_option for every launch until the next ctrlsim_bind_options, -1 inherits it; NULL = the process defaults.
 * Re-asserted by an engine at the top of every run like ctrlsim_bind: two engines with different kernel options take turns in one process.
 * The operand split (key 4) is the exception: it belongs to ctrlsim_bind, with the weight planes / K/V images / workspace laid out for it;
 * a table's entry for key 4 is ignored.  ctrlsim_get_option = the value launches would use now. */
int ctrlsim_option_count(void);
int ctrlsim_bind_options(const int* values);
int ctrlsim_get_option(int key);

const char* ctrlsim_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CTRLSIM_H */
