/* mepol_amd.h -- C ABI of the MI355X (gfx950) MEPOL hot path.
 *
 * The reference (RiccZamboni/mepol) is pure Python and has no FFI; these entry points are what
 * its hot path (src/algorithms/mepol.py) binds to when it is switched to this library.  Each
 * function names the reference interface it replaces.  The Python drop-in module
 * (mepol_amd/algorithms/mepol.py) calls them through ctypes (mepol_amd/_lib.py); the binding a
 * maintainer would add to the reference is shown in INTEGRATION.md.
 *
 * Conventions
 *  - All array arguments are DEVICE pointers owned by the caller (e.g. torch tensors via
 *    data_ptr()); nothing is allocated inside a call.  Scratch comes from a caller-owned
 *    workspace whose size the *_workspace_size query returns.
 *  - `stream` is a hipStream_t; every call only enqueues work on it (no host sync), so calls
 *    can be captured into a hipGraph -- with ONE exception: mepol_knn synchronises `stream`
 *    once per call to validate its input before the scan (sklearn raises on NaN / inf);
 *    mepol_knn_deferred is the same call with the validation result left on the device, and
 *    never blocks.  The per-iteration entry points (entropy, IW, head, GEMMs, optimizer)
 *    never synchronise.
 *  - Return value: 0 on success, a hipError_t value or one of the MEPOL_ERR_* codes otherwise;
 *    mepol_last_error_string() describes the last failure of the calling thread.
 *  - Stateless and re-entrant; ordering comes from the stream.
 *  - Particle indices are int32 on device (N < 2^31); the Python boundary widens them to the
 *    reference's int64 where it returns them.
 */
#ifndef MEPOL_AMD_H
#define MEPOL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on every incompatible change of the signatures below (2: mepol_rollout_mlp takes a
 * workspace; mepol_gemm_dpp removed; 3: mepol_iw_normalize_gathered takes the per-rank
 * trajectory sums).  Additions keep the number: the *_plan_info queries, mepol_critic_fit with
 * mepol_critic_fit_plan_info, mepol_rollout_deep_goal with
 * mepol_rollout_deep_goal_plan_info, the five mepol_rollout_*goal_threshold* entry points,
 * mepol_traj_cut, mepol_rollout_deep_plan_info and the box-maze entry points (mepol_maze,
 * mepol_step_maze, mepol_rollout_step_maze, mepol_rollout_maze*, mepol_rollout_deep_maze*) came
 * in at 4.  mepol_abi_version() returns the library's value. */
#define MEPOL_ABI_VERSION 4

#define MEPOL_ERR_BAD_ARG 1001
#define MEPOL_ERR_WORKSPACE 1002
#define MEPOL_ERR_UNSUPPORTED 1003

const char* mepol_last_error_string(void);
int mepol_abi_version(void);
/* Stream-ordered copy (device <-> pinned host / device); captured as a graph memcpy node. */
int mepol_memcpy_async(void* dst, const void* src, size_t bytes, void* stream);


/* ---- k-NN ---------------------------------------------------------------------------------
 * Replaces src/algorithms/mepol.py:190-192
 *     NearestNeighbors(n_neighbors=k+1, metric='euclidean', algorithm='auto', n_jobs=W)
 *         .fit(next_states).kneighbors(next_states)
 * cand [n_cand, d] f32 row-major, query [n_query, d] f32 (a shard of cand or cand itself).
 * Outputs: dist_out [n_query, kp1] f64 = sqrt(sum_f (q_f - c_f)^2) in f64 (sklearn kd_tree's
 * arithmetic), rows ascending, ties by smaller index; idx_out [n_query, kp1] int64 (nullable);
 * idx32_out [kp1, n_query] int32 TRANSPOSED (nullable; the layout the entropy kernels read).
 * n_fallback_out (nullable, device int32): number of queries answered by the exhaustive path.
 * split_hint: 0 = automatic candidate split.  Any d >= 1 and any 1 <= kp1 <= n_cand (sklearn
 * raises for kp1 > n_samples; so does this, MEPOL_ERR_BAD_ARG); n_cand < 2^31 - 64.  Plans:
 * d <= 63 and kp1 <= 60 run the f16 MFMA screen + certified f64 re-rank (queries it cannot
 * certify take the exhaustive scan); every other shape is answered by the exhaustive f64 scan
 * for every query (mepol_knn_plan_info reports *ks = 0 for such a plan).  The screen's
 * certification bound e 2^-24 (C^2 + 2 C |q|), C = max candidate norm, is relative; it holds for
 * 2^-56 <= max(C, Q) < 2^62 and Q <= 2^8 C, Q = max query norm (the self k-NN and a query shard
 * of the candidates have Q <= C).  Any other input -- a row whose f32 squared norm overflows,
 * norms so small or large that the screen's f32 scale or its values leave f32, queries more than
 * 2^5 times larger than every candidate (the test keeps 2^3 for the norms' own error) -- is
 * valid: the screen is skipped and every query takes the exhaustive f64 scan, with
 * *n_fallback_out = n_query.
 * Input validation (sklearn's check_array in fit/kneighbors): a NaN / inf coordinate in cand or
 * query returns MEPOL_ERR_BAD_ARG ("Input contains NaN or infinity").  The check synchronises
 * `stream` once per call (before the scan is launched), as the reference's kneighbors call
 * blocks. */
int mepol_knn_workspace_size(int64_t n_cand, int64_t n_query, int d, int kp1, int split_hint,
                             size_t* bytes);
/* Plan of a call: *ks = 10 * (k-steps of 16) + candidate halves (1: f16 hi only, 2: hi + lo),
 * *list = per-half selection list length, *split = candidate ranges; an exhaustive plan
 * reports *ks = 0, *split = 0 and *list = its block-select capacity. */
int mepol_knn_plan_info(int64_t n_cand, int64_t n_query, int d, int kp1, int split_hint, int* ks,
                        int* list, int* split);
int mepol_knn(const float* cand, int64_t n_cand, const float* query, int64_t n_query, int d,
              int kp1, int split_hint, double* dist_out, int64_t* idx_out, int32_t* idx32_out,
              int32_t* n_fallback_out, void* workspace, size_t workspace_bytes, void* stream);
/* mepol_knn without the host synchronisation: invalid_out (device int32 [2], required) receives
 * [rows with a NaN / inf coordinate, rows whose squared norm overflows f32] in stream order.
 * When the first is nonzero every later kernel of the call returns at once (the outputs are
 * then undefined); the caller reads invalid_out at its next synchronisation point and raises
 * as mepol_knn would (the epoch path does so once the CSR build is queued behind the k-NN).
 * The second is informational: such a call is answered by the exhaustive scan. */
int mepol_knn_deferred(const float* cand, int64_t n_cand, const float* query, int64_t n_query,
                       int d, int kp1, int split_hint, double* dist_out, int64_t* idx_out,
                       int32_t* idx32_out, int32_t* n_fallback_out, int32_t* invalid_out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Exhaustive f64 scan for every query, no validation, no workspace (an independent check of
 * mepol_knn); kp1 <= 3072 (beyond: MEPOL_ERR_UNSUPPORTED, mepol_knn takes any kp1);
 * scratch_idx is unused (nullable). */
int mepol_knn_exact(const float* cand, int64_t n_cand, const float* query, int64_t n_query, int d,
                    int kp1, double* dist_out, int64_t* idx_out, int32_t* idx32_out,
                    int32_t* scratch_idx, void* stream);

/* ---- importance weights -------------------------------------------------------------------
 * Replaces compute_importance_weights, src/algorithms/mepol.py:114-139:
 *   u[off[n]+t] = exp(cumsum_{s<=t}(logp_t - logp_b)[n, s]);  w = u / sum(u).
 * logp_t/logp_b: [num_traj, T_stride] f64 (log-probs of target / behavioral policy);
 * traj_offsets: [num_traj+1] int64 particle offsets (real trajectory lengths, mepol.py:122).
 * traj_sum_out [num_traj]; w_out/U_out nullable (skip normalisation, e.g. multi-rank). */
int mepol_iw_forward(const double* logp_t, const double* logp_b, int64_t num_traj,
                     int64_t T_stride, const int64_t* traj_offsets, int64_t n_particles,
                     double* u_out, double* traj_sum_out, double* w_out, double* U_out,
                     void* stream);
/* w = u / *U with a device scalar U (multi-rank: U all-reduced). */
int mepol_iw_normalize(const double* u, const double* U, int64_t n, double* w, void* stream);

/* ---- entropy / KL -------------------------------------------------------------------------
 * Replaces compute_entropy (mepol.py:142-154) and compute_kl (mepol.py:157-174), fused:
 *   W_i = sum_{c<k} w[I[i,c]];  V_i = D[i,k]^ns pi^(ns/2)/G;
 *   out4[0] = H  = -sum_i (W_i/k) log(W_i/(V_i+eps)+eps) + B
 *   out4[1] = KL = (1/n_w) sum_i log(k/(n_w W_i) + eps)     (before the max(0, .) clamp)
 *   out4[2], out4[3] = the two raw sums (for cross-rank reduction).
 * w [n_w] (global), idxT [kp1, n] int32, D [n, kp1] f64; W_out, g_out [n] (g = dH/dW);
 * partials: [2 * mepol_entropy_partials_size(n)] f64 scratch. */
int mepol_entropy_partials_size(int64_t n_particles);
int mepol_entropy_forward(const double* w, const int32_t* idxT, const double* D, int64_t n,
                          int64_t n_w, int k, int kp1, double ns, double G, double B, double eps,
                          double* W_out, double* g_out, double* partials, double* out4,
                          void* stream);
/* The same with out4 updated in place and vals[2] = {out4[0] on entry (the previous pass's H),
 * the new KL}: the off-policy graph iteration's two control scalars (device_loop.py). */
int mepol_entropy_forward_emit(const double* w, const int32_t* idxT, const double* D, int64_t n,
                               int64_t n_w, int k, int kp1, double ns, double G, double B,
                               double eps, double* W_out, double* g_out, double* partials,
                               double* out4, double* vals, void* stream);
/* Sharded off-policy iteration (mepol_amd/parallel.py), one launch each: the all-gathered
 * per-rank [u (n) | trajectory sums (nt)] blocks normalised into w_glob [world n] (U = the sum of
 * all world * nt trajectory sums in one fixed order, the same on every rank), and the replay's
 * control scalars from the all-gathered raw sums (at offset off of each rank's block of `stride`
 * doubles): vals = {B - sums_cur[0], sum_kl / n_global}, then sums_cur = the sums. */
int mepol_iw_normalize_gathered(const double* xu_all, int world, int64_t n, int nt,
                                double* w_glob, void* stream);
int mepol_sharded_emit(const double* x_all, int world, int64_t stride, int64_t off, double B,
                       int64_t n_global, double* sums_cur, double* vals, void* stream);

/* ---- entropy gradient (the autograd of policy_update's loss.backward(), mepol.py:278) ----
 * CSR transpose of the first k rows of idxT ([>=k, nq]) for owned ids [col_offset, +ncand):
 * csr_off [ncand+1], csr_rows [nq*k] (query rows row_offset + i, stable order). */
int mepol_csr_workspace_size(int64_t nq, int k, int64_t ncand, size_t* bytes);
int mepol_csr_build(const int32_t* idxT, int64_t nq, int k, int64_t col_offset, int64_t ncand,
                    int64_t row_offset, int32_t* csr_off, int32_t* csr_rows, void* workspace,
                    size_t workspace_bytes, void* stream);
/* gamma_j = sum_{i in CSR(j)} g_i ; partials[b] = block sums of gamma_j w_j: partials holds
 * mepol_entropy_gamma_partials_size(n_own) doubles = min(ceil(8 n_own / 256), 2048) (8 lanes
 * per particle since ABI 4, grid-stride beyond). */
int mepol_entropy_gamma_partials_size(int64_t n_own);
int mepol_entropy_gamma(const double* g, const double* w_own, const int32_t* csr_off,
                        const int32_t* csr_rows, int64_t n_own, double* gamma_out,
                        double* partials, void* stream);
/* grad_logp[n, s] = grad_H * sum_{t>=s} (gamma_{n,t} - S) w_{n,t},  S = sum(partials) or *S_ext. */
int mepol_entropy_reverse_scan(const double* gamma, const double* w, const double* partials,
                               int64_t nparts, const double* S_ext, const int64_t* traj_offsets,
                               int64_t num_traj, int64_t T_stride, const double* grad_H,
                               double* grad_logp, void* stream);

/* Whole rollout of collect_particles (mepol.py:70-111, one call for all T steps) for the
 * reference's 2-hidden-layer ReLU policy on a 2-feature env: one or ceil(h1/64) workgroups per
 * trajectory (see mepol_rollout_mlp_workspace_size).
 * env_id 0 = MountainCar (init64 [n,2] f64), 1 = GridWorld (init32 [n,2] f32, a_dim = 2).
 * W1 [h0,2], b1 [h0], W2t = W2^T [h0,h1], b2 [h1], Wm [a_dim,h1], bm, log_std [a_dim];
 * noise [T,n,a_dim] f64 (a = mean + noise * exp(log_std), policy.py:59).  Writes states_rec
 * [n,T+1,2] f32, actions_rec [n,T,a_dim] f32, visited [n,T,2] f64 (nullable: the env state after
 * each step, for the heatmap) and final_state [n,2] f64 (nullable).  h0, h1 <= 512, a_dim <= 8. */
int mepol_rollout_mlp(int env_id, const double* W1, const double* b1, int h0, const double* W2t,
                      const double* b2, int h1, const double* Wm, const double* bm,
                      const double* log_std, int a_dim, const double* init64, const float* init32,
                      const double* noise, int64_t n, int64_t T, float* states_rec,
                      float* actions_rec, double* visited, double* final_state, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Scratch for mepol_rollout_mlp's multi-workgroup form (ceil(h1/64) workgroups per trajectory,
 * each holding its 64 columns of W2^T in LDS; used when n * ceil(h1/64) fits the CUs and
 * h0 <= 306): one 8-byte mail word per (trajectory, step, part, action).  Word 0 of the
 * workspace is a device int32 error flag: 1 = the workgroups of a trajectory could not all run
 * at once (results invalid; the caller raises).  A null or short workspace selects the
 * one-workgroup-per-trajectory form. */
int mepol_rollout_mlp_workspace_size(int64_t n, int64_t T, int h0, int h1, int a_dim,
                                     size_t* bytes);
/* Which form mepol_rollout_mlp takes for this shape (given a sufficient workspace): workgroups
 * per trajectory, and k_chunks = the number of k-ranges the second layer's sum is split into
 * (1: one fma chain over all h0 rows; 4: four chains of ceil(h0/4) rows added in order), i.e.
 * the summation order of oracle/native/rollout_kordered.c the results match bit for bit. */
int mepol_rollout_mlp_plan_info(int64_t n, int h0, int h1, int a_dim, int* workgroups_per_traj,
                                int* k_chunks);

/* The same rollout for a ReLU policy with 3 <= n_hidden <= 6 hidden layers, nf = 2 ->
 * [h_1 .. h_L] -> a_dim, every width in 1 .. 512 (odd widths included), a_dim <= 8 (GridWorld: 2),
 * in one launch with one workgroup per trajectory.  widths is a HOST array of n_hidden ints.
 * W1 [h_1,2], b1 [h_1]; Wt holds W_2^T .. W_L^T back to back, layer l as [h_{l-1}][h_l]; bt holds
 * b_2 .. b_L back to back; Wm [a_dim,h_L], bm, log_std [a_dim].  init64 / init32, noise,
 * states_rec, actions_rec, visited and final_state as for mepol_rollout_mlp.  The workspace
 * (nullable) is the 256-byte error-word header, zeroed by every call; no form of this kernel
 * sets the word (its workgroups exchange nothing).  n <= 0 or T <= 0 returns 0 without a launch;
 * every other argument is validated on the host before any launch (MEPOL_ERR_BAD_ARG).
 * Summation order, the same contract as mepol_rollout_mlp's: layer 1 is
 * relu((x0 w0 + x1 w1) + b); column j of layer l >= 2 is four fma chains over the k ranges
 * [r Lc, min(r Lc + Lc, h_{l-1})), Lc = ceil(h_{l-1} / 4), each from 0.0 in k order, combined as
 * ((c0 + c1) + c2) + c3, then + b, then ReLU; the mean layer sums Wm[a][j] h_L[j] per 64 columns
 * by the xor butterfly 32 .. 1, adds those sums in order, then bm[a]. */
int mepol_rollout_deep(int env_id, int n_hidden, const int* widths, const double* W1,
                       const double* b1, const double* Wt, const double* bt, const double* Wm,
                       const double* bm, const double* log_std, int a_dim, const double* init64,
                       const float* init32, const double* noise, int64_t n, int64_t T,
                       float* states_rec, float* actions_rec, double* visited,
                       double* final_state, void* workspace, size_t workspace_bytes,
                       void* stream);
/* Workspace of mepol_rollout_deep at these sizes: 256 bytes (the error-word header). */
int mepol_rollout_deep_workspace_size(int64_t n, int64_t T, int n_hidden, const int* widths,
                                      int a_dim, size_t* bytes);
/* Workgroups (= trajectories) of mepol_rollout_deep itself the device holds at once at this
 * shape: the occupancy of the instance without a goal on this env at the launcher's block size
 * and dynamic LDS, times the number of compute units (mepol_rollout_deep_goal_plan_info reports
 * the goal instance's).  Shapes outside mepol_rollout_deep's and a null pointer are
 * MEPOL_ERR_BAD_ARG, checked before the device is asked. */
int mepol_rollout_deep_plan_info(int env_id, int n_hidden, const int* widths, int a_dim,
                                 int* resident_workgroups);

/* ---- TRPO sampling and batch processing (src/algorithms/trpo.py:86-201, 308-331) -------------
 * Every entry point below takes device pointers, only enqueues, returns 0 without a launch for
 * n <= 0, and validates every other argument on the host before any launch.
 *
 * mepol_rollout_mlp with early termination and sparse rewards: collect_sample_batch's episodes
 * (trpo.py:118-140) for CustomRewardEnv(GridWorldContinuous(), grid_goal*) (goal_rl.py:61-77).
 * env_id 1 = GridWorld; env_id 0 returns MEPOL_ERR_UNSUPPORTED.  After each env step the f32 state
 * (sx, sy) is tested against the goal in f32, every operation rounded on its own:
 *     dx = sx - goal_x, dy = sy - goal_y, nrm = sqrt(fl(fl(dx dx) + fl(dy dy))),
 *     hit <=> (double)nrm <= radius          (np.linalg.norm(s - goal) <= 1e-1 under numpy 1.x).
 * A hit at step t (0-based) gives rewards_rec[i, t] = 1, len_out[i] = t + 1, done_out[i] = 1,
 * s_{t+1} is recorded and the trajectory's workgroup(s) leave; with no hit len_out[i] = T and
 * done_out[i] = 0.  Every output is fully defined by the call: states_rec [n,T+1,2] rows past len,
 * actions_rec [n,T,2] and rewards_rec [n,T] rows from len on are written as zeros.  Policy, noise,
 * forms, summation order and workspace (error word, mail) as for mepol_rollout_mlp: up to the end
 * of each episode the recorded states and actions are the bits mepol_rollout_mlp records. */
int mepol_rollout_goal(int env_id, const double* W1, const double* b1, int h0, const double* W2t,
                       const double* b2, int h1, const double* Wm, const double* bm,
                       const double* log_std, int a_dim, const float* init32, const double* noise,
                       int64_t n, int64_t T, float goal_x, float goal_y, double radius,
                       float* states_rec, float* actions_rec, float* rewards_rec,
                       int32_t* len_out, int32_t* done_out, void* workspace,
                       size_t workspace_bytes, void* stream);
int mepol_rollout_goal_workspace_size(int env_id, int64_t n, int64_t T, int h0, int h1, int a_dim,
                                      size_t* bytes);
/* mepol_rollout_mlp_plan_info for mepol_rollout_goal (a_dim = 2): its form is chosen by the
 * goal-mode kernel's own occupancy; k_chunks is the same. */
int mepol_rollout_goal_plan_info(int64_t n, int h0, int h1, int a_dim, int* workgroups_per_traj,
                                 int* k_chunks);
/* mepol_rollout_goal for the policies of mepol_rollout_deep (3 <= n_hidden <= 6, widths a HOST
 * array, Wt / bt packed as there): the same hit test, episode results and fully defined outputs,
 * and up to the end of each episode the recorded states and actions are the bits
 * mepol_rollout_deep records.  One workgroup per trajectory, which leaves at the episode's end.
 * env_id 0 returns MEPOL_ERR_UNSUPPORTED; a_dim != 2, a NaN goal, a radius that is not >= 0, a
 * shape outside mepol_rollout_deep's and a null pointer MEPOL_ERR_BAD_ARG; n <= 0 or T <= 0
 * returns 0 without a launch.  The workspace (nullable) is mepol_rollout_deep_workspace_size's:
 * the error-word header, zeroed by every call and never set (MEPOL_ERR_WORKSPACE if smaller). */
int mepol_rollout_deep_goal(int env_id, int n_hidden, const int* widths, const double* W1,
                            const double* b1, const double* Wt, const double* bt,
                            const double* Wm, const double* bm, const double* log_std, int a_dim,
                            const float* init32, const double* noise, int64_t n, int64_t T,
                            float goal_x, float goal_y, double radius, float* states_rec,
                            float* actions_rec, float* rewards_rec, int32_t* len_out,
                            int32_t* done_out, void* workspace, size_t workspace_bytes,
                            void* stream);
/* Workgroups (= trajectories) of mepol_rollout_deep_goal the device holds at once at this shape:
 * the goal-mode kernel's occupancy at the launcher's block size and dynamic LDS, times the
 * number of compute units.  A round of at most that many trajectories runs as one wave of
 * workgroups. */
int mepol_rollout_deep_goal_plan_info(int n_hidden, const int* widths, int a_dim,
                                      int* resident_workgroups);
/* Threshold goals, on either env: mepol_rollout_goal's episodes with the hit test of every
 * non-GridWorld goal of goal_rl.py:91-107 (s[0] >= 7, s[2] >= 3, ...),
 *     hit <=> (double)state[coord] >= threshold,
 * where coord is 0 or 1 and state is the env's own state after the step: MountainCar's f64 (p, v)
 * (env_id 0, init64 [n,2] f64, a_dim = 1) or GridWorld's f32 (sx, sy) widened exactly (env_id 1,
 * init32 [n,2] f32, a_dim = 2); the other init pointer is not read.  That is what Python computes
 * for s[coord] >= threshold on the reference's state arrays; a NaN state is no hit.  The hilltop
 * of MountainCar is coord 0, threshold 0.45: the wall clips p to exactly 0.45 when it is crossed.
 * Episode results, fully defined outputs, forms, summation order and workspace as for
 * mepol_rollout_goal: up to the end of each episode the recorded states and actions are the bits
 * mepol_rollout_mlp records.  MEPOL_ERR_BAD_ARG, before any launch, for coord outside {0, 1}, a
 * NaN threshold (+-inf are legal: never / always a hit), env_id outside {0, 1}, a_dim != 1 for
 * env 0 or != 2 for env 1, the null init pointer of the chosen env, a null output, and a shape
 * outside mepol_rollout_mlp's (hidden <= 512); n <= 0 or T <= 0 returns 0 without a launch. */
int mepol_rollout_goal_threshold(int env_id, const double* W1, const double* b1, int h0,
                                 const double* W2t, const double* b2, int h1, const double* Wm,
                                 const double* bm, const double* log_std, int a_dim,
                                 const double* init64, const float* init32, const double* noise,
                                 int64_t n, int64_t T, int coord, double threshold,
                                 float* states_rec, float* actions_rec, float* rewards_rec,
                                 int32_t* len_out, int32_t* done_out, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* Workspace and form of mepol_rollout_goal_threshold: as mepol_rollout_goal_workspace_size and
 * mepol_rollout_goal_plan_info, by the occupancy of the instance that runs (env x threshold). */
int mepol_rollout_goal_threshold_workspace_size(int env_id, int64_t n, int64_t T, int h0, int h1,
                                                int a_dim, size_t* bytes);
int mepol_rollout_goal_threshold_plan_info(int env_id, int64_t n, int h0, int h1, int a_dim,
                                           int* workgroups_per_traj, int* k_chunks);
/* mepol_rollout_goal_threshold for the policies of mepol_rollout_deep (3 <= n_hidden <= 6): the
 * same hit test, episode results and argument checks (shapes: mepol_rollout_deep's), and up to
 * the end of each episode the recorded states and actions are the bits mepol_rollout_deep
 * records.  One workgroup per trajectory; the workspace (nullable) is
 * mepol_rollout_deep_workspace_size's (MEPOL_ERR_WORKSPACE if smaller). */
int mepol_rollout_deep_goal_threshold(int env_id, int n_hidden, const int* widths,
                                      const double* W1, const double* b1, const double* Wt,
                                      const double* bt, const double* Wm, const double* bm,
                                      const double* log_std, int a_dim, const double* init64,
                                      const float* init32, const double* noise, int64_t n,
                                      int64_t T, int coord, double threshold, float* states_rec,
                                      float* actions_rec, float* rewards_rec, int32_t* len_out,
                                      int32_t* done_out, void* workspace, size_t workspace_bytes,
                                      void* stream);
/* mepol_rollout_deep_goal_plan_info for the threshold instance of this env. */
int mepol_rollout_deep_goal_threshold_plan_info(int env_id, int n_hidden, const int* widths,
                                                int a_dim, int* resident_workgroups);
/* The step budget of collect_sample_batch (`steps == batch_size`, trpo.py:98-140) over a batch
 * that was rolled out in parallel: trajectories are taken in index order while the running sum of
 * len [n] is below `budget`, and the last one is cut so that the sum equals it.  len_out [n] = the
 * kept lengths (0 for unused trajectories), done_out [n] = done && len_out == len (a cut
 * trajectory is not done), offsets [n+1] int64 = exclusive prefix sum of len_out, meta [2] int64 =
 * {trajectories used, steps kept (< budget when the batch is too short)}.  A negative len counts
 * as 0; any non-zero done is done, and done_out is 0 or 1.  A trajectory of length 0 that starts
 * below the budget is used (it counts in meta[0]) and keeps its done.  One workgroup;
 * n > 65536 returns MEPOL_ERR_UNSUPPORTED. */
int mepol_traj_budget(const int32_t* len, const int32_t* done, int64_t n, int64_t budget,
                      int32_t* len_out, int32_t* done_out, int64_t* offsets, int64_t* meta,
                      void* stream);
/* The episodes inside n un-terminated rollouts of T steps: trajectory i is cut at the first step
 * whose reached state ends the episode, with the outputs of the goal-mode rollouts
 * (mepol_rollout_goal), so that later stages cannot tell the routes apart.  done_step [n,T]
 * bytes: non-zero (any value) = the state reached by step t ends the episode.  With f the
 * smallest such t, len[i] = f + 1 and done[i] = 1; without one, len[i] = T and done[i] = 0.
 * rewards [n,T] f32 (in/out) holds the per-step rewards: rewards[i, t] for t < len[i] is not
 * touched (NaN payloads and -0.0 keep their bits); rewards[i, len ..], actions_rec[i, len ..]
 * ([n,T,a_dim] f32) and states_rec[i, len + 1 ..] ([n,T+1,num_features] f32) become +0.0f.  One
 * workgroup of 256 threads per trajectory, no communication between workgroups.  n = 0 returns 0
 * without a launch; a null pointer, n < 0, T <= 0, T > INT32_MAX - 1, num_features <= 0 or
 * a_dim <= 0 is MEPOL_ERR_BAD_ARG, checked on the host before any launch. */
int mepol_traj_cut(const uint8_t* done_step, int64_t n, int64_t T, float* rewards,
                   float* states_rec, int num_features, float* actions_rec, int a_dim,
                   int32_t* len, int32_t* done, void* stream);
/* process_traj (trpo.py:175-201) over n ragged trajectories and the concatenation of :308-326.
 * rewards [n,T] f32, values [n,T+1] f64 (the critic at every recorded state), len / done / offsets
 * as mepol_traj_budget writes them, states_rec [n,T+1,num_features] f32, actions_rec [n,T,a_dim]
 * f32.  Packed outputs over n_out = offsets[n] rows, row offsets[i] + t <-> step t < len[i] of
 * trajectory i: targets, adv [n_out] f64, states_out [n_out,num_features] and actions_out
 * [n_out,a_dim] f64 (exact widenings).  All in f64, each operation rounded on its own:
 *     boot = done[i] ? 0 : values[i][len[i]]
 *     c = boot;  t = len-1 .. 0:  c = r_t + gamma c;                       targets = c
 *     A = 0;     t = len-1 .. 0:  A = ((r_t + gamma vn) - values[i][t]) + (gamma lambd) A,
 *                                 vn = t == len-1 ? boot : values[i][t+1];  adv = A
 * len and offsets are device data that the host cannot check.  A trajectory is skipped (nothing
 * is read or written for it) when its len is negative or greater than T, or when its packed rows
 * [offsets[i], offsets[i] + len[i]) do not lie inside [0, n_out); a len outside [0, T] is never
 * clamped into it, because offsets was computed for the len that was given.  len = 0 writes
 * nothing.  The other trajectories of the batch are not affected.  With n_out = 0 nothing is
 * launched and the four outputs may be null. */
int mepol_gae(const float* rewards, const double* values, const int32_t* len, const int32_t* done,
              const int64_t* offsets, int64_t n, int64_t T, int64_t n_out, double gamma,
              double lambd, const float* states_rec, int num_features, const float* actions_rec,
              int a_dim, double* targets, double* adv, double* states_out, double* actions_out,
              void* stream);
/* out = (x - mean) / sqrt(mean((x - mean)^2)) over x [n] f64 (trpo.py:331, numpy's population
 * std), the two sums through fixed-order block partials: the same bits on every call.  A zero std
 * gives non-finite values, as numpy does.  out may alias x. */
int mepol_standardize_workspace_size(int64_t n, size_t* bytes);
int mepol_standardize(const double* x, int64_t n, double* out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- policy MLP (GaussianPolicy, src/policy.py:16-51) for the large-batch passes -----------
 * Gaussian head: mean layer + log-probability with the last hidden layer's bias and ReLU folded
 * in.  z [n, hidden] is the last hidden layer's PRE-activation WITHOUT its bias bz (nullable);
 * Wm [a_dim, hidden], bm/log_std [a_dim]; act [n, a_dim].  Forward writes mu [n, a_dim] and
 * logp [n].  Backward (grad_logp [n]) writes dz [n, hidden] (nullable), dWm, dbm, dlog_std and
 * dbz [hidden] (nullable).  Limits: hidden <= 512, a_dim <= 32. */
int mepol_head_forward(const double* z, int64_t n, int hidden, const double* bz, const double* Wm,
                       const double* bm, const double* log_std, const double* act, int a_dim,
                       double* mu_out, double* logp_out, void* stream);
int mepol_head_workspace_size(int64_t n, int hidden, int a_dim, size_t* bytes);
int mepol_head_backward(const double* grad_logp, const double* z, int64_t n, int hidden,
                        const double* bz, const double* Wm, const double* log_std,
                        const double* act, const double* mu, int a_dim, double* dz, double* dWm,
                        double* dbm, double* dlog_std, double* dbz, void* workspace,
                        size_t workspace_bytes, void* stream);
/* mepol_head_backward in two launches on possibly different streams: phase 1 = the row kernel
 * (dz and the per-block records in the workspace), phase 2 = the fixed-order reduces of those
 * records into dWm, dbm, dlog_std, dbz (the caller orders phase 2 after phase 1 and keeps the
 * workspace until phase 2 ran).  Same arguments and the same bits as mepol_head_backward
 * (ABI 4; the off-policy iteration runs phase 2 beside the dW2 / dh1 GEMMs). */
int mepol_head_backward_phase(const double* grad_logp, const double* z, int64_t n, int hidden,
                              const double* bz, const double* Wm, const double* log_std,
                              const double* act, const double* mu, int a_dim, double* dz,
                              double* dWm, double* dbm, double* dlog_std, double* dbz,
                              void* workspace, size_t workspace_bytes, int phase, void* stream);
/* Input layer h = relu(x W^T + b): x [n, in] (in <= 64), W [out, in], b [out], h [n, out];
 * backward from dh = dL/dh and h: dW [out, in], db [out] (nullable). */
int mepol_layer_forward(const double* x, int64_t n, int in_features, const double* W,
                        const double* b, int out_features, double* h_out, void* stream);
int mepol_layer_workspace_size(int64_t n, int in_features, int out_features, size_t* bytes);
int mepol_layer_backward(const double* dh, const double* h, const double* x, int64_t n,
                         int in_features, int out_features, double* dW, double* db,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Fused policy forward for the large-batch passes (GaussianPolicy.get_log_p, src/policy.py:21-51,
 * net = Linear(nf,h0) ReLU Linear(h0,h1) ReLU, mean = Linear(h1,a)): h1 = relu(x W1^T + b1)
 * [n, h0], z2 = h1 W2^T [n, h1] (pre-bias, as the head kernels take it), mu [n, a] and logp [n]
 * in one kernel.  in_features <= 64, hidden1 <= 320; W2 16-byte aligned. */
int mepol_policy_forward(const double* x, int64_t n, int in_features, const double* W1,
                         const double* b1, int hidden0, const double* W2, const double* b2,
                         int hidden1, const double* Wm, const double* bm, const double* log_std,
                         const double* actions, int action_dim, double* h1_out, double* z2_out,
                         double* mu_out, double* logp_out, void* stream);

/* mepol_policy_forward plus relu'(h1) as bits: h1_mask_out [n, ceil(hidden0 / 16)] uint16,
 * bit b of word w of row r = (h1[r][16 w + b] > 0), for mepol_dh1_layer1_backward_masked. */
int mepol_policy_forward_masked(const double* x, int64_t n, int in_features, const double* W1,
                                const double* b1, int hidden0, const double* W2, const double* b2,
                                int hidden1, const double* Wm, const double* bm,
                                const double* log_std, const double* actions, int action_dim,
                                double* h1_out, double* z2_out, double* mu_out, double* logp_out,
                                uint16_t* h1_mask_out, void* stream);

/* The same forward with the row tile of its split form (even hidden0: layer 1, then the z2 GEMM
 * and head) chosen by the caller: row_tile 0 = automatic (what the two calls above do), 64, 32
 * or 16 = that many rows per workgroup of the z2 / head kernel; any other value is
 * MEPOL_ERR_BAD_ARG.  h1_mask_out may be null.  Every output is the same bits for every tile.
 * The one-kernel form (odd hidden0) has 64-row blocks only: 32 or 16 is MEPOL_ERR_UNSUPPORTED. */
int mepol_policy_forward_tiled(const double* x, int64_t n, int in_features, const double* W1,
                               const double* b1, int hidden0, const double* W2, const double* b2,
                               int hidden1, const double* Wm, const double* bm,
                               const double* log_std, const double* actions, int action_dim,
                               double* h1_out, double* z2_out, double* mu_out, double* logp_out,
                               uint16_t* h1_mask_out, int row_tile, void* stream);

/* Host only (no GPU call): *row_tile = the rows per workgroup automatic selection takes for n
 * rows: the shortest of 16 and 32 whose grid ceil(n / tile) fits the 256 CUs (16 to n = 4096,
 * 32 to n = 8192), 64 from there on (so for every n >= 16384) and for an odd hidden0.  n > 0,
 * in_features <= 64, hidden1 <= 320. */
int mepol_policy_forward_plan_info(int64_t n, int in_features, int hidden0, int hidden1,
                                   int* row_tile);

/* Backward of the first layer fused into the dh1 GEMM: dW1 [h0, in] and db1 [h0] (nullable) of
 * h1 = relu(x W1^T + b1) from dz2 [n, k] and W2t = W2^T [h0, k] (dh1 = dz2 W2 stays on chip,
 * masked by h1 > 0 from the forward's h1 [n, h0]).  k even, in_features <= 63, dz2 and W2t
 * 16-byte aligned; workspace from mepol_dh1_layer1_workspace_size.  Replaces the dh1
 * torch.mm + threshold_backward + dW1/db1 reductions of loss.backward() (mepol.py:278).
 * Precondition, for this and the two forms below: every element of x is finite.  The kernel
 * removes the rows and columns of [x | 1] that lie past n and in_features by a product with 0,
 * not a select, and those positions re-read the last row and the last column of x: an inf or
 * nan there would reach rows of dW1 and db1 it has no path to.  dz2, W2 and h1 may hold
 * non-finite values; they reach only the outputs that depend on them.  (The register-fed form
 * of the mask calls, mepol_dh1_layer1_plan_info, removes them with a select; the precondition
 * holds for the op whichever kernel runs.) */
int mepol_dh1_layer1_workspace_size(int64_t n, int hidden0, int in_features, size_t* bytes);
int mepol_dh1_layer1_backward(const double* dz2, int64_t n, int k, const double* W2t, int hidden0,
                              const double* h1, const double* x, int in_features, double* dW1,
                              double* db1, void* workspace, size_t workspace_bytes,
                              void* stream);
/* The same with relu'(h1) from the forward's bit mask (mepol_policy_forward_masked) instead of
 * the f64 h1 values: identical results, 1/64 of the epilogue's operand bytes. */
int mepol_dh1_layer1_backward_masked(const double* dz2, int64_t n, int k, const double* W2t,
                                     int hidden0, const uint16_t* h1_mask, const double* x,
                                     int in_features, double* dW1, double* db1, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* The masked form with the second Linear's weight as stored, W2 [k][hidden0] (hidden0 even,
 * 16-B aligned), instead of W2^T: the kernel transposes its k-tiles on the way into LDS (the
 * register-fed form reads rows k and k + 1 of W2 per fragment instead), so the caller needs no
 * W2^T copy per optimizer step (ABI 4).  Identical results. */
int mepol_dh1_layer1_backward_w2(const double* dz2, int64_t n, int k, const double* W2,
                                 int hidden0, const uint16_t* h1_mask, const double* x,
                                 int in_features, double* dW1, double* db1, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* The two mask forms with the kernel chosen by the caller.  w2 == 0: W is W2^T [hidden0][k];
 * w2 != 0: W is W2 as stored [k][hidden0] (hidden0 even).  form 0 = automatic (what the two calls
 * above do), 1 = the LDS kernel (8 waves of 32 rows, both operands staged through LDS), 2 = the
 * register-fed kernel (4 waves of 64 rows, both operands from L2 straight into the MFMA
 * fragments, no LDS in the K loop, two workgroups per CU); 2 needs k and hidden0 even and
 * in_features <= 31, else MEPOL_ERR_UNSUPPORTED.  Both kernels use the same tiles, grid,
 * workspace and records and give the same bits: the register-fed one feeds the LDS kernel's
 * k-steps to the same lanes and adds a row block's eight 32-row partials in the same order. */
int mepol_dh1_layer1_backward_form(const double* dz2, int64_t n, int k, const double* W,
                                   int hidden0, const uint16_t* h1_mask, const double* x,
                                   int in_features, double* dW1, double* db1, void* workspace,
                                   size_t workspace_bytes, int w2, int form, void* stream);

/* Host only (no GPU call): which kernel the four calls above launch at these sizes, its grid and
 * the layout of the workspace.  mask != 0: the bit-mask forms (_masked, _w2, _form); w2 != 0: W2
 * as stored (needs mask and hidden0 even); ask: the form argument of _form, 0 for the other
 * calls (ask = 2 where the register-fed kernel does not fit: MEPOL_ERR_UNSUPPORTED).  *form: 1 =
 * the register-fed kernel, 0 = the LDS kernel.  Automatic choice: the register-fed kernel for a
 * mask form that fits it and whose grid has more tiles than the chip has CUs (256), the LDS
 * kernel for everything else, the f64-h1 form included.  *nh = ceil((in_features + 1) / 16); the
 * grid is *row_blocks x *col_tiles workgroups (256 x 80 tiles) of *threads threads (*
 * waves_per_block waves of *rows_per_wave rows) and *lds_bytes of LDS; the workspace holds
 * *row_blocks records of *record_doubles = hidden0 (in_features + 1) doubles, then at byte
 * *group_offset the 16 group sums of the fixed-order reduction: *ws_bytes in all, as
 * mepol_dh1_layer1_workspace_size. */
int mepol_dh1_layer1_plan_info(int64_t n, int k, int hidden0, int in_features, int mask, int w2,
                               int ask, int* form, int* nh, int* row_blocks, int* col_tiles,
                               int* threads, int* lds_bytes, int* waves_per_block,
                               int* rows_per_wave, int64_t* record_doubles, size_t* group_offset,
                               size_t* ws_bytes);

/* Weight gradient of a linear layer over a tall batch: dW [out, in] = dy^T x with dy [n, out]
 * and x [n, in] row-major f64 (the policy's dW2 = dz2^T h1, K = n), split-K on the f64 matrix
 * cores and summed over the K-slices in a fixed order; workspace from
 * mepol_weight_grad_workspace_size.  Replaces the weight gradient of the second Linear in
 * loss.backward() (src/policy.py:21-26, mepol.py:278). */
int mepol_weight_grad_workspace_size(int64_t n, int out_features, int in_features, size_t* bytes);
int mepol_weight_grad(const double* dy, int64_t n, int out_features, const double* x,
                      int in_features, double* dW, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Host only (no GPU call): the launch plan mepol_weight_grad takes at these sizes.  *nob, *nib:
 * blocks of 64 output rows and of 80 input columns; *fol: 16-row fragments of the last o-block
 * (1 .. 4); *Sf, *Ss: K-slices of the full o-blocks (0 when nob == 1) and of the last one;
 * *rows_f, *rows_s: rows per slice of each kind (multiples of 4); *grid8: workgroups per XCD
 * (the grid is 8 * grid8).  fend, send, fbase, sbase [8]: workgroup b is entry j = b / 8 of XCD
 * x = b % 8; j < fend[x] is the full tile j % ((nob - 1) nib) of slice fbase[x] + j / ((nob - 1)
 * nib), fend[x] <= j < send[x] the short tile (j - fend[x]) % nib of slice sbase[x] +
 * (j - fend[x]) / nib, and j >= send[x] has no work.  The workspace holds [Sf][64 (nob - 1)][in]
 * then [Ss][out - 64 (nob - 1)][in] doubles.  n, out_features, in_features > 0. */
int mepol_weight_grad_plan_info(int64_t n, int out_features, int in_features, int* nob, int* nib,
                                int* fol, int* Sf, int* Ss, int64_t* rows_f, int64_t* rows_s,
                                int* grid8, int* fend, int* send, int* fbase, int* sbase);

/* Hidden layer on the f64 matrix cores: C = act(A B^T + bias), A [n, k] (row stride lda),
 * B [m, k] (ldb), bias [m] (nullable), C [n, m] (ldc); act = ReLU when relu != 0.  k, lda, ldb
 * even and A, B 16-byte aligned.  variant 0 = default tiling.  Replaces the torch.mm /
 * nn.Linear GEMMs of GaussianPolicy.net (src/policy.py:21-26) in the large-batch passes. */
int mepol_gemm_nt(const double* A, int64_t n, int k, int64_t lda, const double* B, int m,
                  int64_t ldb, const double* bias, int relu, double* C, int64_t ldc, int variant,
                  void* stream);

/* Backward through a hidden layer h_out = relu(h_in W^T + b) given dz_out = dL/d(pre-activation
 * of h_out) [n, out_features]: dz_in [n, in_features] = (dz_out W) * (h_in > 0), the gradient at
 * the previous layer's pre-activation (h_in [n, in_features] is that layer's ReLU output), and
 * db_in [in_features] (nullable) = the column sums of dz_in, the previous layer's bias gradient.
 * W [out_features, in_features] is the Linear weight as stored (no W^T copy).  The GEMM runs on
 * the f64 matrix cores; db_in is summed in a fixed order (the same bits on every call).
 * out_features and in_features even, dz_out and W 16-byte aligned; workspace from
 * mepol_hidden_backward_workspace_size.  Replaces the torch.mm + threshold_backward + bias sum of
 * a hidden layer in loss.backward() (src/policy.py:21-26, mepol.py:278) for policies with three
 * or more hidden layers. */
int mepol_hidden_backward_workspace_size(int64_t n, int in_features, size_t* bytes);
int mepol_hidden_backward(const double* dz_out, int64_t n, int out_features, const double* W,
                          const double* h_in, int in_features, double* dz_in, double* db_in,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- Fisher-vector product of TRPO's policy step (src/algorithms/trpo.py:369-406) ------------
 * Replaces hessian_vector_product's double backward through policy(states): at theta = theta_0
 * the Hessian of KL(theta_0 || theta) over the network parameters is (1/n) sum_i J_i^T
 * diag(1 / (exp(2 log_std) + 1e-7)) J_i with J_i = d mu_i / d theta, so one product is a tangent
 * (forward-mode) pass, the entry points below, and the backward pass of the kernels above
 * (mepol_weight_grad, mepol_hidden_backward, mepol_layer_backward) over activations kept from
 * one forward.  relu'(0) = 0 as torch.  Every entry point only enqueues; n <= 0 returns 0
 * without a launch; every other argument is validated on the host before any launch.
 *
 * Input layer: t_out [n, out] = (x dW^T + db) * (h > 0) for x [n, in] (in <= 64), the tangent
 * direction dW [out, in], db [out] and the forward's h = relu(x W^T + b) [n, out]. */
int mepol_layer_tangent(const double* x, int64_t n, int in_features, const double* dW,
                        const double* db, int out_features, const double* h, double* t_out,
                        void* stream);
/* Hidden layer h_out = relu(h_in W^T + b) on the f64 matrix cores: t_out [n, m] = (t_in W^T +
 * h_in dW^T + db) * (mask_src + mask_bias > 0) for the incoming tangent t_in [n, k], h_in [n, k],
 * W and the direction dW [m, k] as stored, db [m]; the ReLU mask is taken from mask_src [n, m]
 * plus mask_bias [m] (nullable: pass h_out with a null bias, or the pre-bias z with b).  Both
 * products accumulate in the same MFMA accumulators.  k even; t_in, h_in, W and dW 16-byte
 * aligned; `variant` = mepol_gemm_nt's tilings (0 = default, 2 = the 64-row one). */
int mepol_hidden_tangent(const double* t_in, const double* h_in, int64_t n, int k, const double* W,
                         const double* dW, const double* db, int m, const double* mask_src,
                         const double* mask_bias, double* t_out, int variant, void* stream);
/* Mean layer: c_out [n, a_dim] = scale[a] * (sum_j t[r][j] Wm[a][j] + relu(z[r][j] + bz[j])
 * dWm[a][j] + dbm[a]) for the last hidden layer's tangent t and pre-bias pre-activation z
 * [n, hidden], its bias bz (nullable), Wm and the direction dWm [a_dim, hidden], dbm [a_dim];
 * scale [a_dim] is a DEVICE vector (the caller's 1 / ((exp(2 log_std) + 1e-7) n)).
 * hidden <= 512, a_dim <= 32 (beyond: MEPOL_ERR_UNSUPPORTED). */
int mepol_mean_tangent(const double* t, const double* z, int64_t n, int hidden, const double* bz,
                       const double* Wm, const double* dWm, const double* dbm, const double* scale,
                       int a_dim, double* c_out, void* stream);
/* Mean-layer backward from a cotangent c [n, a_dim] on mu (mepol_head_backward with d mu given
 * and no dlog_std): dWm [a_dim, hidden] = c^T relu(z + bz), dbm [a_dim] = column sums of c,
 * dz [n, hidden] (nullable) = (c Wm) * (z + bz > 0), dbz [hidden] (nullable) = column sums of dz.
 * Row sums go through fixed-order partials (the same bits on every call); workspace from
 * mepol_mean_backward_workspace_size.  hidden <= 512, a_dim <= 32.  The outputs are written, not
 * accumulated, so n <= 0 is refused with MEPOL_ERR_BAD_ARG and nothing is written (as
 * mepol_head_backward and mepol_layer_backward do); mepol_mean_tangent with n <= 0 succeeds and
 * writes nothing: it has no output that is a sum over rows. */
int mepol_mean_backward_workspace_size(int64_t n, int hidden, int a_dim, size_t* bytes);
int mepol_mean_backward(const double* c, const double* z, int64_t n, int hidden, const double* bz,
                        const double* Wm, int a_dim, double* dz, double* dWm, double* dbm,
                        double* dbz, void* workspace, size_t workspace_bytes, void* stream);

/* ---- environments -------------------------------------------------------------------------
 * Replace MountainCarContinuous.step (src/envs/mountain_car_wall.py:13-45) and
 * GridWorldContinuous.step (src/envs/gridworld_continuous.py:128-154), batched. */
int mepol_step_mountaincar(double* state, const double* action, int64_t n, int64_t action_stride,
                           void* stream);
int mepol_step_gridworld(float* state, const double* action, int64_t n, void* stream);
/* One step of collect_particles (mepol.py:81-90) for n trajectories: a = mean + noise*exp(log_std),
 * record s_{t+1}/a_t as f32, advance the env. env_id 0 = MountainCar, 1 = GridWorld. */
int mepol_rollout_step(int env_id, double* env_f64, float* env_f32, const double* mean,
                       const double* noise, const double* log_std, int64_t n, int a_dim, int64_t t,
                       int64_t T, float* states_rec, float* actions_rec, double* policy_in,
                       void* stream);

/* ---- Optimizer step of policy_update (mepol.py:280, optimizer.step()) ------------------------
 * Replaces torch.optim.Adam(lr).step() (kind 0) / torch.optim.RMSprop(lr).step() (kind 1) as
 * constructed at mepol.py:308-311, over n_tensors (<= 16) f64 parameter tensors, one launch per 8 of them.
 * exp_avg (Adam only) / exp_avg_sq (Adam; RMSprop square_avg) are updated in place.
 * scalars is DEVICE memory: Adam {enable, lr/bias_correction1, sqrt(bias_correction2), beta1,
 * beta2, eps}; RMSprop {enable, lr, alpha, eps}.  enable == 0 makes the call a no-op.  A tensor
 * of size 0 is skipped; its pointers may be NULL. */
int mepol_optim_step(int kind, int n_tensors, double* const* params, const double* const* grads,
                     double* const* exp_avg, double* const* exp_avg_sq, const int64_t* sizes,
                     const double* scalars, void* stream);
/* mepol_optim_step that also writes each tensor's values from before the update into
 * params_snap / exp_avg_snap / exp_avg_sq_snap (arrays of n_tensors device pointers, each array
 * may be NULL): the device iteration's shadow of the last accepted theta and its optimizer-moment
 * snapshot (algorithms/device_loop.py, mepol.py:441-456 semantics). */
int mepol_optim_step_snapshot(int kind, int n_tensors, double* const* params,
                              const double* const* grads, double* const* exp_avg,
                              double* const* exp_avg_sq, const int64_t* sizes,
                              const double* scalars, double* const* params_snap,
                              double* const* exp_avg_snap, double* const* exp_avg_sq_snap,
                              void* stream);

/* ---- TRPO's critic fit (src/algorithms/trpo.py:441-457) -----------------------------------------
 * Replaces the Adam branch's DataLoader loop
 *     for mb_states, mb_targets in dloader:
 *         loss = mean((vfunc(mb_states) - mb_targets) ** 2); loss.backward(); optimizer.step()
 * by ONE launch of one resident workgroup that takes n_steps Adam steps of the critic
 * Linear(nf, h0) -> ReLU -> Linear(h0, h1) -> ReLU -> Linear(h1, 1), f64, with no L2 term.
 * states [n, nf], targets [n]; index [n_steps * batch] int32: step s fits rows
 * index[s * batch .. (s + 1) * batch) (the caller's shuffle; no random numbers are drawn here; an
 * index outside [0, n) reads nothing and turns that step's results into NaN).  params / exp_avg /
 * exp_avg_sq: six device pointers each, in torch's order (W1 [h0, nf], b1, W2 [h1, h0], b2,
 * W3 [1, h1], b3), updated in place; they stay on chip between steps.  scal [n_steps][2] is DEVICE
 * memory: {lr / bias_correction1, sqrt(bias_correction2)} of each step, the host-computed scalars
 * of mepol_optim_step.  loss_out [n_steps] (nullable): each step's mini-batch loss before its
 * update.  Every sum has a fixed order: the same inputs give the same bits, and a launch of k
 * steps followed by one of n - k steps (scal advanced) gives the bits of one launch of n.
 * Non-finite data in a row that IS read: the ReLUs are selects, (z > 0) ? z : 0, so a NaN
 * pre-activation is an inactive unit, not a NaN activation as in torch.  An infinite TARGET shows
 * as it does in the loop: that step's loss_out is inf and every later one NaN, and the parameters
 * come back NaN except what a unit that was off in that row shields (its row of W2, its b2).  A NaN
 * or infinite STATE coordinate does NOT show in the loss: the row's h1 is 0 (NaN) or 0 / +inf per
 * unit (inf), its value and that step's loss_out stay finite, the weight gradient puts 0 * NaN into
 * column f of W1 (f the coordinate; for inf also into W2's columns of the units driven to +inf),
 * and from the next step on every z1 is NaN, the first layer is off and every loss_out is finite
 * again.  On return exactly those columns of W1 (W2) and of their moments are NaN and everything
 * else is finite, where the loop returns a non-finite loss and every tensor NaN.  A caller that
 * watches only the loss must therefore check the parameters too (algorithms/trpo.py's _fit_critic
 * does, on the device: a fit with any non-finite parameter, moment or loss returns all of them
 * NaN).  Rows that no index reads may hold anything.  eps == 0 is allowed (an element whose
 * gradient and moments are exactly 0 then becomes NaN, as in torch).
 * 1 <= nf <= 16, 1 <= h0, h1 <= 64, 1 <= batch <= 64, n_steps >= 1, n < 2^31 (beyond:
 * MEPOL_ERR_BAD_ARG).  mepol_critic_fit_plan_info (host only, always 0): the workgroup's threads,
 * its LDS bytes, and *accepted = 1 when the shape is within those limits, else 0. */
int mepol_critic_fit_plan_info(int nf, int h0, int h1, int batch, int* threads, int* lds_bytes,
                               int* accepted);
int mepol_critic_fit(const double* states, const double* targets, int64_t n, const int32_t* index,
                     int64_t n_steps, int batch, int nf, int h0, int h1, double* const* params,
                     double* const* exp_avg, double* const* exp_avg_sq, const double* scal,
                     double beta1, double beta2, double eps, double* loss_out, void* stream);

/* ---- box mazes (mepol_amd/envs/maze.py BoxMazeContinuous) ----------------------------------------
 * A 2-D continuous maze whose bounds, step size and axis-aligned wall boxes are data: GridWorld's
 * step (src/envs/gridworld_continuous.py:128-154) with its constants made arguments, in the same
 * IEEE order.  Configured as the default GridWorld it gives the bits of the env_id 1 entry points.
 * The state is f32 [n, 2], the action count is 2.  A move is undone when its landing point lies in
 * any of the first n_walls closed boxes (x0, x1, y0, y1), then when it lies on or outside a bound.
 *
 * The maze entry points are the env_id 1 ones folded by goal kind: MEPOL_GOAL_NONE is
 * mepol_rollout_mlp / mepol_rollout_deep (visited and final_state may be given, the goal arguments
 * and rewards_rec / len_out / done_out are ignored and may be 0 / NULL); MEPOL_GOAL_BALL is
 * mepol_rollout_goal / mepol_rollout_deep_goal with (goal_x, goal_y) and goal_value = radius >= 0;
 * MEPOL_GOAL_THRESHOLD is mepol_rollout_goal_threshold / mepol_rollout_deep_goal_threshold with
 * coord 0 or 1 and goal_value = threshold (not NaN).  Outputs, workspace layout, error word and
 * summation order are those of the calls they fold; the plan and workspace queries ask the
 * occupancy of the maze instance of that goal kind.  The existing entry points keep rejecting
 * env_id 2.  MEPOL_ERR_BAD_ARG, with a message, for a NULL maze, n_walls outside
 * 0 .. MEPOL_MAZE_MAX_WALLS, a bound, max_delta or used wall number that is not finite, an
 * inverted wall box (x0 > x1 or y0 > y1), inverted bounds (lo >= hi), a_dim != 2, and whatever
 * the folded call rejects. */
#define MEPOL_MAZE_MAX_WALLS 16
typedef struct mepol_maze {
  double xlo, xhi, ylo, yhi; /* open bounds */
  double max_delta;          /* each action coordinate is clipped to +-max_delta */
  int32_t n_walls;           /* walls in use, 0 .. MEPOL_MAZE_MAX_WALLS */
  int32_t reserved;          /* 0 */
  double walls[MEPOL_MAZE_MAX_WALLS][4]; /* (x0, x1, y0, y1), closed boxes */
} mepol_maze;

#define MEPOL_GOAL_NONE 0
#define MEPOL_GOAL_BALL 1
#define MEPOL_GOAL_THRESHOLD 2

/* mepol_step_gridworld and mepol_rollout_step on a maze. */
int mepol_step_maze(const mepol_maze* maze, float* state, const double* action, int64_t n,
                    void* stream);
int mepol_rollout_step_maze(const mepol_maze* maze, float* env_f32, const double* mean,
                            const double* noise, const double* log_std, int64_t n, int a_dim,
                            int64_t t, int64_t T, float* states_rec, float* actions_rec,
                            double* policy_in, void* stream);
/* The two-layer one-launch rollout on a maze, in both of its forms. */
int mepol_rollout_maze_workspace_size(int goal_kind, int64_t n, int64_t T, int h0, int h1,
                                      int a_dim, size_t* bytes);
int mepol_rollout_maze_plan_info(int goal_kind, int64_t n, int h0, int h1, int a_dim,
                                 int* workgroups_per_traj, int* k_chunks);
int mepol_rollout_maze(const mepol_maze* maze, int goal_kind, const double* W1, const double* b1,
                       int h0, const double* W2t, const double* b2, int h1, const double* Wm,
                       const double* bm, const double* log_std, int a_dim, const float* init32,
                       const double* noise, int64_t n, int64_t T, float goal_x, float goal_y,
                       int coord, double goal_value, float* states_rec, float* actions_rec,
                       double* visited, double* final_state, float* rewards_rec, int32_t* len_out,
                       int32_t* done_out, void* workspace, size_t workspace_bytes, void* stream);
/* The 3-to-6-layer one-launch rollout on a maze. */
int mepol_rollout_deep_maze_workspace_size(int64_t n, int64_t T, int n_hidden, const int* widths,
                                           int a_dim, size_t* bytes);
int mepol_rollout_deep_maze_plan_info(int goal_kind, int n_hidden, const int* widths, int a_dim,
                                      int* resident_workgroups);
int mepol_rollout_deep_maze(const mepol_maze* maze, int goal_kind, int n_hidden, const int* widths,
                            const double* W1, const double* b1, const double* Wt, const double* bt,
                            const double* Wm, const double* bm, const double* log_std, int a_dim,
                            const float* init32, const double* noise, int64_t n, int64_t T,
                            float goal_x, float goal_y, int coord, double goal_value,
                            float* states_rec, float* actions_rec, double* visited,
                            double* final_state, float* rewards_rec, int32_t* len_out,
                            int32_t* done_out, void* workspace, size_t workspace_bytes,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MEPOL_AMD_H */
