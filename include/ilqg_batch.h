/* Batched iLQG on MI355X — public C-ABI (additive; the reference has no batch mode).
 *
 * The library is built per problem (like the reference, whose N_X/N_U are
 * compile-time macros of the generated header, iLQG_problem.tem:16-21):
 *     libilqg_<problem>_fd<FULL_DDP>_hip.so
 * It exports
 *   (1) the reference's own link-time symbols — iLQG(), back_pass(),
 *       line_search(), boxQP(), standard_parameters(), setOptParam(),
 *       makeCandidateNominal(), printParams() (include/iLQG.h, back_pass.h,
 *       line_search.h, boxQP.h) — operating on one `tOptSet`, with the hot path
 *       executed by the HIP kernels, and
 *   (2) the batch interface below: B independent trajectories of the same
 *       problem advanced in lock step on one GPU, all state resident in HBM.
 *
 * Every entry point takes plain pointers and sizes.  Host arrays are
 * trajectory-major: x is [B][n_hor+1][N_X], u is [B][n_hor][N_U], l is
 * [B][n_hor][N_U], L is [B][n_hor][N_U*N_X] (each step an N_U x N_X
 * column-major matrix, reference iLQG_func.tem:152) — for B = 1 exactly the
 * column-major x_new(n,N), u_new(m,N-1) matrices of the reference's MEX entry
 * (iLQG_mex.c:93-97,127-137).
 *
 * Functions returning int: 0 = ok, non-zero = error, text via ilqg_batch_error().
 */
#ifndef ILQG_BATCH_H
#define ILQG_BATCH_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ilqg_batch ilqg_batch_t;

/* problem facts of this build: out[0..7] = N_X, N_U, FULL_DDP, derivative
 * record size (host view), record size stored on the device, 1 if input limits
 * depend on the state, number of problem parameters, mapping (0 = one lane per
 * trajectory, 1 = one wavefront per trajectory; chosen at build time from N_X) */
void ilqg_problem_dims(int *out);
/* problem parameters, as the generated paramdesc[] declares them (iLQG_func.tem:11-18);
 * size -1 = one value per time step (n_hor+1 values) */
const char *ilqg_problem_param_name(int i);
int ilqg_problem_param_size(int i);

/* number of HIP devices visible; 0 if none */
int ilqg_device_count(void);

ilqg_batch_t *ilqg_batch_create(int device, int batch, int n_hor); /* NULL on failure (ilqg_batch_error(NULL)) */
/* The batch is advanced as `groups` independent sets of consecutive trajectories, each on its own HIP stream,
 * so that the latency-bound kernels of one set overlap with the throughput-bound ones of another.  Results do
 * not depend on it.  groups = 0 (what ilqg_batch_create passes): ILQG_GROUPS from the environment, else 4 for
 * batches >= 8192 in the one-lane-per-trajectory mapping (measured best at 65 536 trajectories), else 1.  At most 4. */
ilqg_batch_t *ilqg_batch_create_groups(int device, int batch, int n_hor, int groups);
/* Builds with one wavefront per trajectory (N_X > 8) keep the derivative records of the trajectories in flight in ONE
 * work buffer per device, shared by all batches on it, allocated by the first and released with the last: sized to hold
 * the first batch in the record form ilqg_batch_iterate uses if the device has the memory, else what is free after
 * that batch's other arrays (at least half of what is free).  ILQG_WORK_GB in the environment sets its size. */
int ilqg_batch_groups(const ilqg_batch_t *c);
void ilqg_batch_destroy(ilqg_batch_t *c);
const char *ilqg_batch_error(const ilqg_batch_t *c);

/* options: same keys, validation and messages as the reference's setOptParam
 * (iLQG.c:91-216); additionally
 *   "resweep"     0/1: repeat the reference's cost-only sweep after each accepted step
 *                 (iLQG.c:338).  Default 1 for problems with multipliers, 0 otherwise: without
 *                 multipliers that sweep returns the cost of the accepted roll-out bit for bit.
 *   "fuse_derivs" 0/1: ilqg_batch_iterate/solve evaluate the derivatives inside the backward
 *                 kernel instead of materialising the records in HBM.  Default 1, 0 for problems
 *                 with multipliers (measured faster there); same results either way.
 *   "ls_split"    default 4 (1 for builds with one wavefront per trajectory): step sizes
 *                 alpha[0..ls_split) are rolled out for every trajectory,
 *                 the remaining ones only for trajectories that found none acceptable among
 *                 them; 0 = all step sizes for every trajectory.  The accepted step size is the
 *                 same either way (first acceptable, line_search.c:37-60).
 *   "ls_keep"     default 2.  One lane per trajectory (first stages of up to 4 step sizes): every
 *                 roll-out of the line search is kept where it is rolled out and the accepted one becomes the
 *                 current trajectory by a change of its location index — no second roll-out, no copy.  One
 *                 wavefront per trajectory, generated file with the step in parts: both stages keep their
 *                 roll-outs and the accepted ones are copied (no second roll-out); else as 1.
 *                 1: the second stage runs side by side with the
 *                 roll-out that stores the accepted trajectories of the first stage, and keeps what it rolls
 *                 out, so that its own accepted trajectories are copied instead of rolled out once more;
 *                 0: second stage, then one storing roll-out for all.  Same results in all three.
 *   "bw_split"    default 0.  1: the fused backward pass runs on two wavefronts per 64 trajectories
 *                 (derivatives of step k-1 on one, Riccati update of step k on the other, hand-over in
 *                 LDS) where the problem allows it (no multipliers, constant limits).  Same results;
 *                 measured no faster.
 *   "compact"     default 0.  n > 0: ilqg_batch_solve retires finished trajectories — between iterations, once at most
 *                 half of the slots it iterates over are still active (and at least n are), the active trajectories are
 *                 gathered into a smaller context and iterated there; they return to their own slots of this batch when
 *                 they are gathered again or the solve ends, so every getter reads this batch as before.  Same results
 *                 bit for bit (a trajectory's iterations depend on nothing but its own state); a solve whose
 *                 trajectories converge at very different iterations (CarParking: 50 to 550) does not run 64-lane
 *                 wavefronts for one live lane.  Reference: the loop exits of iLQG.c:297-303, :331, :365-378.
 * Defaults = standard_parameters() (iLQG.c:57-78). */
int ilqg_batch_set_option(ilqg_batch_t *c, const char *name, const double *value, int n);
/* problem parameter by name, shared by all trajectories (iLQG_mex.c:70-84) */
int ilqg_batch_set_param(ilqg_batch_t *c, const char *name, const double *value, int n);
/* PROBLEM PARAMETERS PER TRAJECTORY: a goal per agent, a model per vehicle, a sweep over a cost weight — a batch that differs
 * in more than x0.  From the next launch on, every generated callback evaluated for trajectory b sees the batch's fixed-size
 * parameters with the NAMED ones replaced by row b of values — in every stage: the initial roll-out of ilqg_batch_init and
 * ilqg_batch_shift, calc_derivs, back_pass in all three modes, line_search, the multiplier update and the cost re-sweep,
 * iterate, solve, receding.  Like ilqg_batch_set_param the call recomputes nothing: costs and records of the current
 * trajectories stay as they are until ilqg_batch_init or ilqg_batch_shift.  PER-TIME-STEP PARAMETERS (size -1) STAY SHARED
 * HERE; they have an entry of their own, ilqg_batch_set_param_steps_batch (below).
 *
 * names, W and the row layout are those of ilqg_batch_policy_rollout_params with n_starts = 1 and shared = 0: n_names host
 * strings, each a fixed-size parameter of paramdesc[], in any order, none twice; W = the sum of their sizes; values [B][W],
 * row b belongs to trajectory b, the named parameters one behind the other in the order of names, each contiguous.  A call
 * REPLACES the whole per-trajectory set, it is not incremental.  n_names = 0 clears it (names and values are not read): the
 * batch is shared-only again and runs the very kernels of a batch that never had a table.
 *
 * ORDER WITH THE ROLL-OUT AND PLANT TABLES: THE TRAJECTORY'S ROW FIRST, THEN THE ROLL-OUT'S OR THE PLANT'S ROW.  Where those
 * entries say "the batch's parameters", read "trajectory b's": ilqg_batch_policy_rollout evaluates roll-out (b, r) under
 * trajectory b's parameters; ilqg_batch_policy_rollout_params puts its named columns on top of them (a parameter named in
 * both gets the roll-out's value); the plant of ilqg_batch_receding_plant with n_names = 0 is trajectory b's model, and with
 * named plant parameters the plant's row goes on top of it.  ilqg_batch_head, ilqg_batch_shift_param and every getter are
 * unaffected.
 * Option "compact": the rows travel with their trajectories, a compacted solve stays bit for bit the plain one.
 * ilqg_batch_solve_stream is REFUSED while a per-trajectory set exists: the rows belong to slots, the starts of a stream pass
 * through them, and a table per start is out of scope.  Option bw_split runs the one-wavefront backward pass while a set
 * exists.  (A row per START of a stream is an argument of ilqg_batch_solve_stream_rows.)
 *
 * ilqg_batch_set_params_batch takes host memory and waits once per group; ilqg_batch_set_params_batch_device takes DEVICE
 * memory under the stream contract of ilqg_batch_head_device (event in, one event per group out, no host wait, no allocation
 * in steady state) — for an estimator on the GPU that refreshes the rows every control interval.  The library copies the
 * table into a buffer of its own, which only grows: the caller's memory is free afterwards (in the device form: once its
 * stream has passed the call).
 * ilqg_batch_get_params_batch: out [B][size], what trajectory b sees of fixed-size parameter `name` — its row, or the shared
 * value repeated where the parameter is not per-trajectory.
 * ilqg_multi_set_params_batch (below): every shard gets the rows from its first trajectory on.
 *
 * REFUSED, with the argument named in the error text and before anything is launched, allocated or changed: a name that is
 * no parameter ("Parameter name '%s' is not member of parameters struct."), a per-time-step parameter, a name given twice,
 * n_names < 0, n_names > 0 with names or values NULL, in the device form values that is not device memory of the context's
 * device; ilqg_batch_set_param of a name that currently is per-trajectory (the text points at
 * ilqg_batch_set_params_batch(c, 0, NULL, NULL)); and every library of the WAVE MAPPING (one wavefront per trajectory: the
 * *_wave libraries and the problems with N_X = 10 or 16 — the text names the mapping): those kernels do not carry parameters
 * per lane.  Not supported, beside the wave, row and quad mappings: a table per start in ilqg_batch_solve_stream, the
 * drop-in iLQG().  (Per-trajectory values of per-time-step parameters: ilqg_batch_set_param_steps_batch, below; the table per
 * start that ilqg_batch_solve_stream leaves out: ilqg_batch_solve_stream_rows.) */
int ilqg_batch_set_params_batch(ilqg_batch_t *c, int n_names, const char *const *names, const double *values /* [B][W] host */);
int ilqg_batch_set_params_batch_device(ilqg_batch_t *c, int n_names, const char *const *names, const double *values /* [B][W] device */, void *stream);
int ilqg_batch_get_params_batch(ilqg_batch_t *c, const char *name, double *out /* [B][size] host */);

/* initial conditions and initial controls, then the initial roll-out
 * (forward_pass with alpha = 0, which also clamps u; iLQG_mex.c:113-120)
 * and the solver's entry state (iLQG.c:226-237) */
int ilqg_batch_set_x0(ilqg_batch_t *c, const double *x0 /* [B][N_X] */);
int ilqg_batch_set_u(ilqg_batch_t *c, const double *u /* [B][n_hor][N_U] */);
/* overwrite the whole nominal state trajectory (tests: re-synchronise with a checker) */
int ilqg_batch_set_x(ilqg_batch_t *c, const double *x /* [B][n_hor+1][N_X] */);
int ilqg_batch_init(ilqg_batch_t *c);

/* Receding horizon, on the device: what the caller of the reference's MEX entry does between two calls — it passes
 * u_nom = [u(:, s+1:end), tail] and the new x0 (iLQG_mex.c:113-120) — without the trajectories leaving the GPU.  With
 * (x, u) the current nominal trajectory of every slot, whatever its status:
 *     u'[k] = u[k + steps] for k < n_hor - steps; the last `steps` controls are u_tail [B][steps][N_U], or u[n_hor-1]
 *     repeated if u_tail is NULL;  x0' = x0_new [B][N_X], or x[steps] if x0_new is NULL;
 * then exactly what ilqg_batch_init does: the initial roll-out (clamps u, re-initialises multipliers, may set status 7)
 * and the solver entry state, so that every trajectory is active again with 0 iterations and lambda = lambdaInit.  Gains
 * and derivative records are left as ilqg_batch_init leaves them.  0 <= steps < n_hor, anything else is an error;
 * steps = 0 with both pointers NULL is ilqg_batch_init.  Only x0_new and u_tail cross to the device.
 * PROBLEM PARAMETERS ARE LEFT ALONE, those with one value per time step (size -1) included: the caller moves their
 * window with ilqg_batch_set_param before (or after) the shift. */
int ilqg_batch_shift(ilqg_batch_t *c, int steps, const double *x0_new /* [B][N_X] or NULL */,
                     const double *u_tail /* [B][steps][N_U] or NULL */);
/* `rounds` times { ilqg_batch_iterate(c, iterations); record; ilqg_batch_shift(c, steps, NULL, NULL) }: a closed loop on
 * the model itself.  "record" appends the first `steps` (x_k, u_k) of every plan and its cost to a log on the device,
 * which reaches the host once, at the end.  1 <= steps < n_hor.  A problem with a per-time-step parameter (size -1) is
 * refused: its window has to move with the horizon, which is the caller's loop over ilqg_batch_iterate,
 * ilqg_batch_set_param and ilqg_batch_shift. */
int ilqg_batch_receding(ilqg_batch_t *c, int rounds, int steps, int iterations,
                        double *x_applied /* [B][rounds*steps][N_X] */, double *u_applied /* [B][rounds*steps][N_U] */,
                        double *cost /* [B][rounds] */);   /* any output may be NULL */

/* A control interval with the caller's OWN plant (a simulator, a learned model, hardware) is
 *     ilqg_batch_iterate;  ilqg_batch_head*;  the plant's step;  ilqg_batch_shift*  (and ilqg_batch_shift_param)
 * and none of it needs a whole field on the host.
 *
 * The first `steps` steps of every CURRENT plan, wherever it lives (a kept roll-out plane of the line search included),
 * trajectory-major: x [B][steps][N_X] (x_0 .. x_{steps-1}), u [B][steps][N_U], l [B][steps][N_U],
 * L [B][steps][N_U*N_X] (each step column-major, as ilqg_batch_get_gains), cost [B].  Any pointer may be NULL.
 * 1 <= steps <= n_hor.  Changes nothing in the batch (in particular it does not move trajectories home).
 * ilqg_batch_head fills host memory and waits once per group of trajectories; it moves steps * (N_X + N_U + ...) doubles
 * per trajectory, not whole fields.  ilqg_batch_head_device fills DEVICE memory of the context's device.
 *
 * Stream contract of the two _device entries: `stream` is the caller's hipStream_t (NULL = the null stream, handled like
 * any other: by events).  Work that produces the inputs has been enqueued on it; the outputs are consumed on it.  On
 * entry the library records an event on `stream` and lets its own streams wait for it; behind the last kernel that
 * touches the caller's memory (the gather of the heads; the scatter of x0_new / u_tail, NOT the initial roll-out) it
 * records an event per group of trajectories and lets `stream` wait for it.  The host waits for nothing, copies nothing
 * and allocates nothing in steady state.  Pointers that are not device memory on the context's device are refused and
 * the batch is left untouched. */
int ilqg_batch_head(ilqg_batch_t *c, int steps, double *x, double *u, double *l, double *L, double *cost);
int ilqg_batch_head_device(ilqg_batch_t *c, int steps, double *x, double *u, double *l, double *L, double *cost, void *stream);
/* ilqg_batch_shift with x0_new / u_tail in DEVICE memory of the context's device (same layouts, same NULL meanings) */
int ilqg_batch_shift_device(ilqg_batch_t *c, int steps, const double *x0_new, const double *u_tail, void *stream);
/* CANDIDATES PER AGENT.  A batch of B = G * K slots read as G SEGMENTS of K consecutive slots: segment g is slots
 * gK .. gK + K - 1, one agent's K candidate plans.  K is one of 1, 2, 4, 8, 16, 32, 64 and B % K == 0, anything else is an
 * error.  (Groups of trajectories and the lane mapping's tiles are whole multiples of 64, so a segment never straddles a
 * group, a tile or a wavefront; the kernels rely on it and the host checks it.)
 *
 * ilqg_batch_best_of chooses each segment's winner.  score [B], or NULL = every slot's current cost (as it stands, penalty
 * terms included); otherwise the caller's own figure, e.g. a mean closed-loop cost out of ilqg_batch_policy_rollout_device.
 * A slot is ELIGIBLE iff its score is finite (NaN, +Inf and -Inf are not) and its status is not ILQG_ST_INIT_FAILED.
 * winner[g] = the batch-absolute index of the eligible slot of segment g with the smallest score; EQUAL SCORES RESOLVE TO
 * THE LOWEST INDEX, the comparison is `<` on doubles, so -0.0 and 0.0 tie; -1 if no slot is eligible.  best[g] = the
 * winner's score, NaN for -1; n_eligible[g] = the count of eligible slots; either may be NULL, winner may not.  The call
 * CHANGES NOTHING in the batch; in particular it moves no trajectory home.  One launch of k_best_of per group.
 * ilqg_batch_best_of_device: score and the outputs in DEVICE memory of the context's device, under the stream contract of
 * ilqg_batch_head_device (event in, one event per group out, no host wait, no allocation in steady state, pointers
 * checked before any launch). */
int ilqg_batch_best_of(ilqg_batch_t *c, int K, const double *score /* [B] or NULL */, int *winner /* [G] */,
                       double *best /* [G] or NULL */, int *n_eligible /* [G] or NULL */);
int ilqg_batch_best_of_device(ilqg_batch_t *c, int K, const double *score, int *winner, double *best, int *n_eligible, void *stream);
/* ilqg_batch_shift, except that every slot b of segment g takes the plan of slot w = winner[g] in place of its own.  With
 * (x, u) the winner's current trajectory wherever it lives (a kept roll-out plane included):
 *     u'_b[k] = (k + steps < n_hor ? u_w[k + steps] : (u_tail ? u_tail[g][k + steps - n_hor] : u_w[n_hor-1])) + (du ? du[b][k] : 0)
 *     x0'_b   = x0_new ? x0_new[g] : x_w[steps]
 * (the sum is one fp64 add; without du nothing is added), then exactly what ilqg_batch_shift does: the initial roll-out,
 * which clamps u', re-initialises multipliers and may set status 7, and the solver entry state.  Gains, derivative
 * records, histories, parameter rows and windows are left alone as ilqg_batch_shift leaves them.  x0_new and u_tail are
 * per SEGMENT, du per SLOT; the caller keeps the incumbent unperturbed by zeroing one slot's rows of du.
 * 0 <= steps < n_hor.  winner == NULL is refused.  winner[g] == -1: every slot of segment g is its own winner, i.e. shifts
 * its own plan.  The host form refuses a winner outside its segment.  THE DEVICE FORM CANNOT LOOK: there the kernel treats
 * a value outside segment g as -1.  With K = 1, winner[g] = g and du = NULL the result is ilqg_batch_shift's bit for bit.
 * ilqg_batch_shift_winners_device: winner, x0_new, u_tail, du in DEVICE memory of the context's device (same layouts, same
 * NULL meanings), stream contract as ilqg_batch_shift_device. */
int ilqg_batch_shift_winners(ilqg_batch_t *c, int K, const int *winner /* [G] */, int steps,
                             const double *x0_new /* [G][N_X] or NULL */, const double *u_tail /* [G][steps][N_U] or NULL */,
                             const double *du /* [B][n_hor][N_U] or NULL */);
int ilqg_batch_shift_winners_device(ilqg_batch_t *c, int K, const int *winner, int steps, const double *x0_new, const double *u_tail,
                                    const double *du, void *stream);
/* Every plan's feedback POLICY rolled out from n_starts starts per trajectory, on the device (one lane per roll-out).
 *
 * The policy of trajectory b is what ilqg_batch_head(c, n_hor, x, u, l, L, NULL) returns for it: the current trajectory,
 * read where it lives, and the gains stored with it.  A trajectory's status does not matter.  BEHIND AN ACCEPTED STEP THE
 * STORED GAINS WERE COMPUTED ABOUT THE PREVIOUS NOMINAL TRAJECTORY (the backward pass runs before the line search that
 * moves the trajectory) — this is what a caller applies today from ilqg_batch_head; right after a backward pass
 * (ilqg_batch_back_pass, or an iteration whose step was rejected) the gains are exact.
 *
 * For start s = x0[b][r] the reference's forward_pass (iLQG_func.tem:121-185) runs with o->x0 = s, the nominal = the
 * policy, the multipliers and penalty weights trajectory b has now, the per-time-step parameters as they stand, and
 *     u_k = u_nom_k  [+ alpha * l_k  if alpha != 0]  [+ L_k (x_k - x_nom_k)  if feedback]
 * then calcXVariableAux, clampU, calcXUVariableAux, ddpf, ddpL per step and calcFVariableAux, ddpF at the end:
 *     feedback = 1, alpha != 0   the reference's forward_pass(alpha)
 *     feedback = 0, alpha  = 0   the reference's forward_pass(0): open-loop replay from another start
 *     feedback = 1, alpha  = 0   the pure feedback law u_nom + L dx
 *     feedback = 0, alpha != 0   the feed-forward step alone
 * x0 [B][n_starts][N_X].  Outputs, any of them NULL: cost [B][n_starts]; ok [B][n_starts] = forward_pass's return value
 * (1, or 0 as soon as a guarded value is NaN or Inf — then cost and the trajectory of that roll-out are unspecified);
 * x_end [B][n_starts][N_X]; the whole roll-out x [B][n_starts][n_hor+1][N_X], u [B][n_starts][n_hor][N_U] (u is the
 * clamped control that was applied).  NOTHING in the batch changes.  n_starts >= 1 and x0 != NULL, else an error; all
 * outputs NULL is a no-op.
 * ilqg_batch_policy_rollout takes host memory, stages through device buffers of the context that only grow, and waits once
 * per group of trajectories.  ilqg_batch_policy_rollout_device takes DEVICE memory of the context's device under the
 * stream contract of ilqg_batch_head_device above (event in, one event per group out, no host wait); pointers are checked
 * before anything is launched. */
int ilqg_batch_policy_rollout(ilqg_batch_t *c, int n_starts, const double *x0, double alpha, int feedback, double *cost, int *ok,
                              double *x_end, double *x, double *u);
int ilqg_batch_policy_rollout_device(ilqg_batch_t *c, int n_starts, const double *x0, double alpha, int feedback, double *cost, int *ok,
                                     double *x_end, double *x, double *u, void *stream);
/* The same roll-outs, EACH UNDER PROBLEM PARAMETERS OF ITS OWN: what a plan does on a plant whose wheelbase, time step,
 * limits or cost weights differ from the model it was planned with (a Monte-Carlo estimate over model error).
 *
 * Everything is as in ilqg_batch_policy_rollout — the nominal data, the four (alpha, feedback) kinds, the clamp, the
 * multipliers and penalty weights of trajectory b, the outputs, their layouts and the per-roll-out ok, and NOTHING in the
 * batch changes, its parameters included — with one difference: roll-out (b, r) evaluates every generated callback
 * (init_running, calcXVariableAux, clampU, calcXUVariableAux, ddpf, ddpL, calcFVariableAux, ddpF) with a parameter set of
 * its own: the batch's current fixed-size parameters, in which the values of the NAMED PARAMETERS REPLACE THE BATCH'S by
 * the caller's row for that roll-out.  The policy itself stays the plan's: x, u, l, L, THE GAINS HAVING BEEN COMPUTED UNDER
 * THE BATCH'S PARAMETERS — applying a policy planned for one model to another is the purpose.  PER-TIME-STEP PARAMETERS
 * (size -1) STAY SHARED, as they stand; naming one is refused.
 *
 * names: n_names >= 1 host strings, each a fixed-size parameter of paramdesc[], in any order (not necessarily that of
 * paramdesc[]), none twice.  W = the sum of the named parameters' sizes.  values: [B][n_starts][W], or with shared != 0
 * [n_starts][W], used for every trajectory; within a row the named parameters follow each other in the order of names,
 * each contiguous.  Refused before anything is launched, with the argument and the parameter named in the error text and
 * the batch untouched: a name that is no parameter ("Parameter name '%s' is not member of parameters struct."), a
 * per-time-step parameter, a name given twice, n_names < 1, names or values NULL, n_starts < 1, x0 NULL and, in the device
 * form, x0 / values / an output that is not device memory of the context's device.  All outputs NULL is a no-op after these
 * checks.
 * ilqg_batch_policy_rollout_params takes host memory for x0 and values, stages them through the context's buffers, which
 * only grow, and waits once per group.  ilqg_batch_policy_rollout_params_device takes DEVICE memory for x0, values and the
 * outputs under the stream contract of ilqg_batch_head_device (event in, one event per group out, no host wait, no
 * allocation in steady state); names are host strings in both. */
int ilqg_batch_policy_rollout_params(ilqg_batch_t *c, int n_starts, const double *x0, int n_names, const char *const *names, const double *values,
                                     int shared, double alpha, int feedback, double *cost, int *ok, double *x_end, double *x, double *u);
int ilqg_batch_policy_rollout_params_device(ilqg_batch_t *c, int n_starts, const double *x0, int n_names, const char *const *names,
                                            const double *values, int shared, double alpha, int feedback, double *cost, int *ok, double *x_end,
                                            double *x, double *u, void *stream);
/* The same roll-outs UNDER PROCESS NOISE, each under a disturbance table of its own: the closed-loop cost of a plan over its
 * whole horizon when the state is pushed behind every step — what the feedback gains L exist for.  The superset entry: with
 * disturbance = NULL and n_names = 0 it is ilqg_batch_policy_rollout, with disturbance = NULL and n_names > 0
 * ilqg_batch_policy_rollout_params, the same kernels, launches and bits.
 *
 * For roll-out (b, r) and step k = 0 .. n_hor-1, behind the step of forward_pass (the rule of ilqg_batch_receding_plant,
 * step (2)):      x_{k+1} <- x_next + w[b][r][k]
 * disturbance: [B][n_starts][n_hor][N_X], or with disturbance_shared != 0 [n_starts][n_hor][N_X], used for every trajectory
 * (common random numbers across trajectories).  The control of step k+1 is computed at the disturbed state; row n_hor-1 moves
 * the end state, so x_end, x[n_hor] and the final cost, which is evaluated at the disturbed state.  x holds the states the
 * controls were applied at, x[0] = the start; u the clamped controls.  ok = 0 as soon as a guard fails or a disturbed state is
 * not finite, the one behind row n_hor-1 included; no other roll-out changes by a bit.
 * n_names = 0: no parameter table — names, values and shared are not read.  n_names > 0: the rules and refusals of
 * ilqg_batch_policy_rollout_params; the order stays "trajectory's row, then roll-out's row".  Refused before anything is
 * launched or changed, the argument named: what those entries refuse and, in the device form, a disturbance that is not device
 * memory of the context's device.  All outputs NULL is a no-op after the checks.  The host form stages the table behind the
 * values through the context's buffers, which only grow; the device form reads it where it lies, under the stream contract of
 * ilqg_batch_head_device. */
int ilqg_batch_policy_rollout_noise(ilqg_batch_t *c, int n_starts, const double *x0, int n_names, const char *const *names, const double *values,
                                    int shared, const double *disturbance, int disturbance_shared, double alpha, int feedback, double *cost,
                                    int *ok, double *x_end, double *x, double *u);
int ilqg_batch_policy_rollout_noise_device(ilqg_batch_t *c, int n_starts, const double *x0, int n_names, const char *const *names,
                                           const double *values, int shared, const double *disturbance, int disturbance_shared, double alpha,
                                           int feedback, double *cost, int *ok, double *x_end, double *x, double *u, void *stream);
/* THE SAME ROLL-OUTS WITH THE PROCESS NOISE DRAWN ON THE DEVICE FROM A SEED: no table, no upload, no memory proportional to
 * n_starts.  The arguments of the _noise forms with `disturbance, disturbance_shared` replaced by
 *     seed, sigma, noise_shared, first_trajectory
 * and w[b][r][k][i] = sigma[i] z[b][r][k][i], added by the rule above.  z: standard normals from the counter-based generator
 * Philox4x32-10 (Random123) under the key (seed & 0xffffffff, seed >> 32) at the counter (k, r, t, i / 4), t the GLOBAL
 * trajectory index first_trajectory + b — with noise_shared != 0 t = 0: every trajectory gets the draws of trajectory 0,
 * common random numbers —, turned into normals by Box-Muller in double precision (two words a pair; the tail ends at 6.7
 * sigma); each w is rounded to double before it is added.  A draw depends on its counter alone, so roll-out (b, r) has the
 * same bits whatever n_starts, the stream groups, the shards (ilqg_multi_* passes each shard its own first trajectory) or a
 * caller who rolls a large batch out in chunks with first_trajectory = the chunk's first trajectory.
 * ilqg_batch_noise_table writes the same draws as a table, w [B][n_starts][n_hor][N_X] or with noise_shared
 * [n_starts][n_hor][N_X]: given to the _noise forms as `disturbance` it yields what the _drawn forms yield, bit for bit in
 * every output; it is also the table for ilqg_batch_receding_plant, for inspection, or for a caller who adds a term of their own.
 * sigma: N_X doubles in HOST memory in every form.  Refused before anything is launched or changed, the argument named: sigma
 * NULL, a sigma entry negative or not finite, first_trajectory < 0, first_trajectory + B > 2^32, what the _noise forms refuse
 * of n_starts, x0 and the names, and host memory in the device forms (x0, values, the outputs, w). */
int ilqg_batch_policy_rollout_drawn(ilqg_batch_t *c, int n_starts, const double *x0, int n_names, const char *const *names, const double *values,
                                    int shared, unsigned long long seed, const double *sigma, int noise_shared, long long first_trajectory,
                                    double alpha, int feedback, double *cost, int *ok, double *x_end, double *x, double *u);
int ilqg_batch_policy_rollout_drawn_device(ilqg_batch_t *c, int n_starts, const double *x0, int n_names, const char *const *names,
                                           const double *values, int shared, unsigned long long seed, const double *sigma, int noise_shared,
                                           long long first_trajectory, double alpha, int feedback, double *cost, int *ok, double *x_end,
                                           double *x, double *u, void *stream);
int ilqg_batch_noise_table(ilqg_batch_t *c, int n_starts, unsigned long long seed, const double *sigma, int noise_shared, long long first_trajectory,
                           double *w);
int ilqg_batch_noise_table_device(ilqg_batch_t *c, int n_starts, unsigned long long seed, const double *sigma, int noise_shared,
                                  long long first_trajectory, double *w, void *stream);
/* THE CLOSED LOOP OF PLANNER AND PLANT, resident on the device for `rounds` control intervals — ilqg_batch_receding with a
 * plant that has a state of its own, may differ from the model and may be disturbed: what closed-loop cost the controllers
 * reach when the wheelbase is 5 % off and the state is pushed at every step.  Each of the `rounds` rounds is
 *   (1) ilqg_batch_iterate(c, iterations);
 *   (2) the plant of every trajectory b advances `steps` steps from ITS OWN state xp: for k = 0 .. steps-1
 *           u = u_nom_k  [+ L_k (xp - x_nom_k)  if feedback],
 *       the policy being the one ilqg_batch_head hands out (the current plan where it lives and the gains stored with it;
 *       BEHIND AN ACCEPTED STEP THE GAINS ARE THOSE ABOUT THE PREVIOUS NOMINAL TRAJECTORY, see ilqg_batch_policy_rollout;
 *       alpha = 0: l is not used), then the step of the reference's forward_pass (iLQG_func.tem:121-185: calcXVariableAux,
 *       clampU, calcXUVariableAux, ddpf, ddpL, time index k) with the multipliers and penalty weights trajectory b has,
 *       evaluated under THE PLANT'S PARAMETERS, then  xp <- x_next + disturbance[b][round*steps + k];
 *   (3) ilqg_batch_shift(c, steps, x0_new = xp, u_tail = NULL), the states never leaving the device.
 * The planner stays under the batch's parameters throughout, and they are unchanged afterwards.
 * The plant's parameters are the batch's fixed-size parameters with the named ones replaced by row b of values [B][W]:
 * names, their order, W and the refusals are those of ilqg_batch_policy_rollout_params with n_starts = 1 and shared = 0.
 * n_names = 0 (names and values are then not read): the plant is the model.  disturbance [B][rounds*steps][N_X], or NULL:
 * none (nothing is added, not even a zero).
 * x_plant [B][N_X]: the plants' states on entry and, on return, behind the last round; NULL: every plant starts from its
 * plan's x_0 and no final state is returned.
 * Logs (host memory, any of them NULL): x_applied [B][rounds*steps][N_X] the plant's state each control was applied at,
 * u_applied [B][rounds*steps][N_U] the CLAMPED control that was applied, cost_applied [B][rounds] the sum of the round's
 * running costs (ct.c of ddpL, from 0.0 in step order, under the plant's parameters, multipliers and penalty weights as
 * above), plan_cost [B][rounds] the cost of the plan the round applied (what ilqg_batch_receding logs as cost), ok [B].
 * FAILURE IS PER TRAJECTORY: a step whose guards fail (forward_pass would return 0: a guarded value is NaN or Inf) or
 * behind which the disturbed state is not finite sets ok[b] = 0 for the rest of the call.  That plant no longer advances:
 * it stays at its last finite state, the planner goes on re-planning from it, and its later log entries and cost_applied
 * are unspecified.  A start that is not finite fails at once.  No other trajectory's results change by a bit.
 * Refused with the argument named in the error text, before anything is launched, allocated or changed: rounds < 1,
 * iterations < 0, steps outside 1 .. n_hor-1, a problem with a per-time-step parameter (as ilqg_batch_receding), n_names < 0,
 * n_names > 0 with names or values NULL, a name that is no parameter, a per-time-step parameter, a name given twice.
 * All outputs NULL is NOT a no-op: the batch advances.
 * Memory: everything is host memory.  values, disturbance and x_plant go up once before the first round; the logs, ok and
 * the final states come down once behind the last; between rounds the host waits for nothing and copies nothing. */
int ilqg_batch_receding_plant(ilqg_batch_t *c, int rounds, int steps, int iterations, int feedback,
                              double *x_plant /* [B][N_X] in/out, or NULL */,
                              int n_names, const char *const *names, const double *values /* [B][W] */,
                              const double *disturbance /* [B][rounds*steps][N_X] or NULL */,
                              double *x_applied, double *u_applied /* [B][rounds*steps][N_X] / [N_U] */,
                              double *cost_applied, double *plan_cost /* [B][rounds] each */, int *ok /* [B] */);
/* The window of ONE per-time-step parameter (size -1) moves `steps` values on: p'[k] = p[k + steps], the last `steps`
 * values from tail [steps] (host), or p[n_hor] held if tail is NULL.  0 <= steps <= n_hor.  Exactly what
 * ilqg_batch_set_param(c, name, [p[steps:], tail], n_hor + 1) gives, without re-allocating or re-sending the table: the
 * values move in place on the device, and in the host copy a later ilqg_batch_set_param of another parameter re-sends.
 * (Wave-mapped problems: written as the full re-send implies, but no such problem with a per-time-step parameter is
 * built in this tree, so that path is untested.) */
int ilqg_batch_shift_param(ilqg_batch_t *c, const char *name, int steps, const double *tail /* [steps] or NULL */);
/* PER-TIME-STEP PARAMETERS PER TRAJECTORY: a reference track or speed profile per agent, a moving obstacle bound per vehicle,
 * a forecast per unit.  ilqg_batch_set_param_steps_batch(c, name, values): name is ONE parameter of size -1, values
 * [B][n_hor + 1] trajectory-major.  From the next launch on every generated callback evaluated for trajectory b reads
 * p[name][k] from row b, for the running steps and the final step k = n_hor, in every stage ilqg_batch_set_params_batch
 * covers (the initial roll-out of init and shift, calc_derivs, back_pass in all three modes, line_search, the multiplier
 * update and the cost re-sweep, iterate, solve) and in ilqg_batch_policy_rollout*: where that entry says "the per-time-step
 * parameters as they stand", read "trajectory b's".  Like ilqg_batch_set_param the call recomputes nothing.  It works PER
 * NAME: values = NULL makes that name shared again, with the window ilqg_batch_set_param last gave it; other names keep what
 * they have.  The fixed-size set of ilqg_batch_set_params_batch is independent: setting or clearing one leaves the other
 * alone.  With no per-trajectory name left and no fixed-size table the batch runs the very kernels of a batch that never had
 * one.  The library copies the rows into a buffer of its own per name, which only grows.  The _device forms take DEVICE
 * memory under the stream contract of ilqg_batch_head_device (event in, one event per group out, no host wait, no
 * allocation in steady state).
 * ilqg_batch_get_param_steps_batch: out [B][n_hor + 1], what trajectory b sees: its row, or the shared window repeated.
 * ilqg_batch_shift_param_batch: per row what ilqg_batch_shift_param does, p'[b][k] = p[b][k + steps], the last `steps` values
 * from tail [B][steps], or p[b][n_hor] held if tail is NULL; 0 <= steps <= n_hor, steps = 0 is a no-op.  The rows move in
 * place on the device; the result is bit for bit what re-sending [rows[:, steps:], tail] through the setter gives.
 * Option "compact": the rows travel with their trajectories, a compacted solve stays bit for bit the plain one.
 *
 * REFUSED, with the argument named in the error text and before anything is launched, allocated or changed: a name that is
 * no parameter ("Parameter name '%s' is not member of parameters struct."), a fixed-size name (the text points at
 * ilqg_batch_set_params_batch), out NULL (c NULL returns 1), steps out of range, ilqg_batch_shift_param_batch of a name
 * that is currently shared, in the device forms memory that is not device memory of the context's device;
 * ilqg_batch_set_param and ilqg_batch_shift_param of a name that currently is per-trajectory (the text points at the _batch
 * forms and at values = NULL); ilqg_batch_solve_stream while any name has rows; every library of the WAVE MAPPING (the text
 * names the mapping).  A per-time-step name given to ilqg_batch_set_params_batch, _policy_rollout_params or _receding_plant
 * stays refused, and ilqg_batch_receding / _receding_plant still refuse a problem that has a per-time-step parameter.
 * Not supported: the wave, row and quad mappings; the drop-in iLQG(); rows per start in ilqg_batch_solve_stream; the
 * resident closed loops receding / receding_plant for problems with per-time-step parameters (moving windows inside those
 * loops).  (A window per START of a stream is an argument of ilqg_batch_solve_stream_rows.) */
int ilqg_batch_set_param_steps_batch(ilqg_batch_t *c, const char *name, const double *values /* [B][n_hor+1] host, or NULL */);
int ilqg_batch_set_param_steps_batch_device(ilqg_batch_t *c, const char *name, const double *values /* device, or NULL */, void *stream);
int ilqg_batch_get_param_steps_batch(ilqg_batch_t *c, const char *name, double *out /* [B][n_hor+1] host */);
int ilqg_batch_shift_param_batch(ilqg_batch_t *c, const char *name, int steps, const double *tail /* [B][steps] host, or NULL */);
int ilqg_batch_shift_param_batch_device(ilqg_batch_t *c, const char *name, int steps, const double *tail /* device or NULL */, void *stream);

/* MOVING WINDOWS INSIDE THE RESIDENT LOOPS: tracking MPC that stays on the device.  ilqg_batch_receding and
 * ilqg_batch_receding_plant refuse a problem that has a per-time-step parameter (size -1), because its window has to move with
 * the horizon.  The two _windows entries below are the way round that limitation: the same loops, in which EVERY size -1
 * parameter's window moves `steps` values on each round, fed from futures that sit on the device from before round 0.  The old
 * entries keep every behaviour, their refusal included.
 *
 * window_names: n_windows host strings, each a parameter of size -1 of paramdesc[], in any order, none twice.  future[i] is HOST
 * memory holding the values of window_names[i] BEYOND its current window, for the whole call:
 *     [B][rounds*steps]  where the name currently has per-trajectory rows (ilqg_batch_set_param_steps_batch), row b for trajectory b;
 *     [rounds*steps]     where the name is shared;
 *     NULL               the window holds its last value, p[n_hor], per row.
 * Every size -1 parameter of the problem moves, named or not: one that is not named holds its last value.  n_windows = 0 is
 * allowed (window_names and future are then not read).  On a problem without a per-time-step parameter n_windows must be 0, and
 * the call is ilqg_batch_receding / ilqg_batch_receding_plant bit for bit.
 *
 * ORDER WITHIN A ROUND r.  ilqg_batch_receding_windows:
 *   (1) ilqg_batch_iterate(c, iterations);
 *   (2) record, as ilqg_batch_receding does;
 *   (3) every window moves `steps` on: p'[k] = p[k + steps], its last `steps` values columns [r*steps, (r+1)*steps) of its
 *       future (what ilqg_batch_shift_param / ilqg_batch_shift_param_batch do with that tail, for all windows in one launch
 *       per group of trajectories);
 *   (4) ilqg_batch_shift(c, steps, NULL, NULL).
 * ilqg_batch_receding_plant_windows:
 *   (1) ilqg_batch_iterate(c, iterations);
 *   (2) the plants advance `steps` steps as in ilqg_batch_receding_plant; the plant's step k reads p[name][k] of the round's
 *       NOT YET MOVED window — trajectory b's row where the name has rows.  The plant has no window of its own, and a
 *       per-time-step name among the plant's `names` stays refused;
 *   (3) the windows move, as above;
 *   (4) the plans shift onto the plants' states.
 * THE WINDOWS MOVE BEFORE THE SHIFT, because the shift's initial roll-out reads them.
 *
 * Afterwards every window has moved rounds*steps on, on the device; the host copy of a shared window has moved with it (a
 * later ilqg_batch_set_param of another parameter re-sends from that copy); ilqg_batch_get_param_steps_batch returns the moved
 * rows; a following ilqg_batch_iterate continues as the caller's own loop over iterate / shift_param* / shift would.  Every
 * other argument, the logs, the per-trajectory failure of the plant loop and its ok are those of the old entries.
 * Memory: the futures go up once, before round 0, into buffers of the context that only grow; between rounds the host copies
 * nothing and waits for nothing.  Wave-mapped libraries have no rows, so every name is shared there and takes a shared future.
 *
 * REFUSED, with the argument named in the error text and before anything is launched, allocated or changed: everything
 * ilqg_batch_receding / ilqg_batch_receding_plant refuse except the per-time-step problem itself; a name that is no parameter
 * ("Parameter name '%s' is not member of parameters struct."); a fixed-size name; a name given twice; n_windows < 0;
 * n_windows > 0 with window_names or future NULL; n_windows > 0 on a problem without per-time-step parameters.
 * Not supported: windows of the plant that differ from the planner's; futures in device memory. */
int ilqg_batch_receding_windows(ilqg_batch_t *c, int rounds, int steps, int iterations,
                                int n_windows, const char *const *window_names, const double *const *future,
                                double *x_applied, double *u_applied, double *cost);
int ilqg_batch_receding_plant_windows(ilqg_batch_t *c, int rounds, int steps, int iterations, int feedback, double *x_plant,
                                      int n_names, const char *const *names, const double *values, const double *disturbance,
                                      int n_windows, const char *const *window_names, const double *const *future,
                                      double *x_applied, double *u_applied, double *cost_applied, double *plan_cost, int *ok);

/* n lock-step iterations of { calc_derivs, back_pass (+ lambda retries),
 * line_search over all alpha, accept/reject } for every still-active trajectory */
int ilqg_batch_iterate(ilqg_batch_t *c, int n);
/* iterate until no trajectory is active (at most max_iter iterations) */
int ilqg_batch_solve(ilqg_batch_t *c);
int ilqg_batch_sync(ilqg_batch_t *c);
int ilqg_batch_active(ilqg_batch_t *c, int *n_active);
/* A STREAM of `total` starts solved through this batch's slots: finished trajectories are harvested every 8 iterations and
 * their slots given to the next starts of the stream (initialised in a staging context as ilqg_batch_init does, then moved
 * in), so that the slots stay full while starts remain.  x0 [total][N_X], u0 [total][n_hor][N_U] in; per start out: cost,
 * status (exit reason, see below), iterations, and — if not NULL — x [total][n_hor+1][N_X], u [total][n_hor][N_U].
 * Every start gets the result a plain ilqg_batch_solve of a batch holding it gives, bit for bit.  Options and parameters:
 * those of c; what c held before is overwritten.  ilqg_batch_solve_trace reports the polls (its `compactions` counts the
 * refills).  No reference counterpart (the reference solves one trajectory per call, iLQG.c:224). */
int ilqg_batch_solve_stream(ilqg_batch_t *c, int total, const double *x0, const double *u0, double *cost, int *status,
                            int *iterations, double *x, double *u);
/* The same stream with what the three notes above leave out of ilqg_batch_solve_stream: every start may bring a ROW of
 * fixed-size parameters, a WINDOW per per-time-step parameter and an iteration HISTORY of its own.  ilqg_batch_solve_stream is
 * this entry with nothing named: one loop, the same results, trace and refill rule (a refill once a sixteenth of the slots is
 * free, polls every 8 iterations).
 * The starts: start s is solved as a plain ilqg_batch_solve solves it in a batch that holds it at slot b, after
 * ilqg_batch_set_params_batch(names, ...) with row values[s] at b and ilqg_batch_set_param_steps_batch(step_names[i], ...)
 * with row step_values[i][s] at b: the plain solve's result bit for bit, in every build.  names, their order, W and the row
 * layout are those of ilqg_batch_set_params_batch, values [total][W] (n_names = 0: none, names and values are not read);
 * step_names are parameters of size -1, step_values[i] [total][n_hor+1] (n_step_names = 0: none).  A parameter not named stays
 * the batch's shared value or window.
 * The history: with hist_cap > 0 every start records its own iteration history under the one rule of
 * ilqg_batch_set_history (the staging context's init clears it, the move carries it).  hist_names are the names of
 * ilqg_batch_get_history / _get_history_int; hist_out[i] is double [total][hist_cap] for a double name, int [total][hist_cap]
 * for an int name and int [total] for "n".  Unwritten entries read as zero, and n may exceed hist_cap (dropped but counted).
 * Before and after: on entry c has no per-trajectory set, no step rows and no history; on return, success or failure, c is as
 * on entry: it has none again — ilqg_batch_get_params_batch gives the shared values, ilqg_batch_history_cap gives 0.  Its
 * trajectories are overwritten.  ilqg_batch_solve_trace reports polls and refills as for ilqg_batch_solve_stream.
 * How: the rows reach the staging context through the setters above (slots beyond the starts it initialises hold the shared
 * values, never zeros), c gets the same map and a table of the shared values once, before the first refill.  Finished starts
 * come back through a gather kernel (k_harvest): per stream group and poll one launch and one copy of exactly what was asked
 * for; a poll in which nothing finished reads the statuses and nothing else.  No context is made per poll.
 * REFUSED, with the argument (and the parameter) named in the error text, before anything is launched, allocated or changed —
 * c's trajectories are still what they were: total < 1; x0 or u0 NULL; a c that already has a set, rows or a history (the
 * text tells the caller to pass them to this call); what ilqg_batch_set_params_batch refuses of names / values; what
 * ilqg_batch_set_param_steps_batch refuses of a name (fixed-size, unknown, given twice, a NULL table); hist_cap < 0; n_hist > 0
 * with hist_cap = 0; an unknown history name; w_pen_* without multipliers; a NULL hist_out[i]; and in a library of the WAVE
 * MAPPING n_names > 0 or n_step_names > 0 (the text names the mapping) — a history alone is served there.
 * No such refusal, but a FAILURE of the call: device memory that runs out.  A history capacity the batch's device has no memory
 * for fails with c's trajectories still what they were; the staging context or its history failing to fit fails behind that,
 * with c's trajectories already overwritten (c is as on entry in every other respect).
 * Not supported: ilqg_multi_* (no stream); option "compact" inside a stream; rows in device memory; the drop-in iLQG(). */
int ilqg_batch_solve_stream_rows(ilqg_batch_t *c, int total, const double *x0, const double *u0,
                                 int n_names, const char *const *names, const double *values,
                                 int n_step_names, const char *const *step_names, const double *const *step_values,
                                 int hist_cap, int n_hist, const char *const *hist_names, void *const *hist_out,
                                 double *cost, int *status, int *iterations, double *x, double *u);
/* the last stream, counted: out[0] polls (status reads), out[1] launches of k_harvest, out[2] bytes the harvests copied to the
 * host, out[3] contexts made (the staging context: 1) */
void ilqg_batch_stream_counts(const ilqg_batch_t *c, long long *out /* [4] */);
/* the last ilqg_batch_solve, poll by poll (it polls every 4 iterations): iterations done so far, trajectories still
 * active, slots the iterations ran over (the batch, or the smaller context of option "compact"); returns the number of
 * polls (at most cap entries are written; any pointer may be NULL), *compactions = how often the active set was gathered */
int ilqg_batch_solve_trace(ilqg_batch_t *c, int *iterations, int *active, int *slots, int cap, int *compactions);

/* single stages, for tests and for callers that interleave their own work */
int ilqg_batch_calc_derivs(ilqg_batch_t *c);
/* mode 0: derivative records from HBM, with the lambda retry loop and the gradient test (iLQG.c:261-303);
 *      1: records from HBM, exactly one sweep (what the drop-in back_pass() runs);
 *      2: as 0, derivatives evaluated inside the kernel from (x,u) (what ilqg_batch_iterate uses when
 *         option "fuse_derivs" is 1) */
int ilqg_batch_back_pass(ilqg_batch_t *c, int mode);
int ilqg_batch_line_search(ilqg_batch_t *c);  /* search + selection + store the winner */
int ilqg_batch_update(ilqg_batch_t *c);

/* results (copied to host, trajectory-major) */
int ilqg_batch_get_x(ilqg_batch_t *c, double *x);
int ilqg_batch_get_u(ilqg_batch_t *c, double *u);
int ilqg_batch_get_gains(ilqg_batch_t *c, double *l, double *L);
int ilqg_batch_get_derivs(ilqg_batch_t *c, double *rec /* [B][n_hor][record] */, double *fin /* [B][N_X+sizeofQxx] */);
/* Augmented-Lagrangian multipliers of problems with hle / hli / hfe / hfi constraints (reference
 * iLQG_problem.tem:70-89, iLQG_func.tem:371-521): out[0..1] = doubles in multipliersEl_t / multipliersFin_t
 * (0, 0 for a problem without such constraints).  The arrays hold the structs member by member:
 * running [B][n_hor][out[0]], final [B][out[1]]; either pointer may be NULL.  The current penalty weights
 * are the per-trajectory scalars "w_pen_l" / "w_pen_f" of ilqg_batch_get_scalar. */
void ilqg_problem_multiplier_dims(int *out);
int ilqg_batch_get_multipliers(ilqg_batch_t *c, double *running, double *final);
int ilqg_batch_set_multipliers(ilqg_batch_t *c, const double *running, const double *final);
int ilqg_batch_set_derivs(ilqg_batch_t *c, const double *rec, const double *fin);
int ilqg_batch_set_gains(ilqg_batch_t *c, const double *l, const double *L);
/* name in: cost new_cost dcost expected lambda dlambda g_norm dV0 dV1 ([B] each),
 * alpha_cost ([B][16]) */
int ilqg_batch_get_scalar(ilqg_batch_t *c, const char *name, double *out);
int ilqg_batch_set_scalar(ilqg_batch_t *c, const char *name, const double *in);
/* name in: status iterations alpha_idx accepted bp_calls bp_rc need_derivs ([B] each), alpha_ok ([B][16]) */
int ilqg_batch_get_int(ilqg_batch_t *c, const char *name, int *out);
int ilqg_batch_set_int(ilqg_batch_t *c, const char *name, const int *in);

/* The ITERATION HISTORY: every trajectory's line searches, recorded on the device without a host round trip — what the
 * reference keeps in log_linesearch / log_z / log_cost (line_search.c:70-72) and prints per iteration (iLQG.c:314, 353).
 * ONE RULE.  With a history of capacity cap switched on, every time the batch runs the update of an iteration — inside
 * ilqg_batch_iterate, ilqg_batch_solve (compacted too: a trajectory's history moves with it and is home at the end), every
 * ilqg_batch_receding* loop, or as the stage ilqg_batch_update — it first APPENDS one entry for every trajectory that is
 * active (status 0) at that point: exactly those whose line search has just run.  A trajectory that left in this
 * iteration's backward pass (status 4, 1, 6) appends nothing, as the reference writes no log for it.  The entry holds what
 * the per-trajectory fields hold then, i.e. at the return of line_search():
 *   doubles  cost      the nominal cost the search started from
 *            new_cost  the reference's log_cost
 *            z         dcost / expected where expected > 0, else 0 (line_search.c:44-48): the reference's log_z
 *            lambda    behind the backward pass's retries, BEFORE the update moves it
 *            g_norm dV0 dV1
 *            w_pen_l w_pen_f   only in libraries of problems with multipliers; elsewhere the names are refused
 *   ints     alpha_idx   1-based, n_alpha + 1 = none accepted: the reference's log_linesearch
 *            bp_calls    backward sweeps of this iteration
 *            iterations  the reference's `iter` at that moment, the index it logs under
 * For a rejected search new_cost and z are whatever the fields hold (the reference's carried-over values).
 * The entry goes to position n[b], a count per trajectory, which then goes up by one; entries at positions >= cap are
 * DROPPED while n counts on.  ilqg_batch_set_history and ilqg_batch_init CLEAR counts and entries; ilqg_batch_shift and
 * the resident loops do NOT: receding(rounds, steps, iterations) leaves rounds * iterations entries whose `iterations`
 * field restarts at 0 every round, and from an init on position and `iterations` coincide.  Unwritten entries read as zero.
 * Recording changes no solver output; without a history nothing is launched and nothing allocated.
 * set: cap > 0 switches on (or resizes) and clears, 0 switches off and frees.  get: out [B][cap], trajectory-major.
 * get_int: name "n" gives [B] (it may exceed cap), the others [B][cap].  Refused, with the batch and its history left as
 * they were and nothing launched: cap < 0; a capacity the device has no memory for; a getter without a history; an unknown
 * name; w_pen_* without multipliers; out = NULL.  ilqg_batch_solve_stream refuses a batch with a history: it belongs to
 * slots, starts pass through them — switch it off first, ilqg_batch_set_history(c, 0).  (A history per START of a stream is
 * an argument of ilqg_batch_solve_stream_rows: hist_cap.) */
int ilqg_batch_set_history(ilqg_batch_t *c, int cap);
int ilqg_batch_get_history(ilqg_batch_t *c, const char *name, double *out /* [B][cap] */);
int ilqg_batch_get_history_int(ilqg_batch_t *c, const char *name, int *out /* "n": [B]; else [B][cap] */);
int ilqg_batch_history_cap(const ilqg_batch_t *c);

/* Per-trajectory exit reasons ("status" of ilqg_batch_get_int): 0 active; 1 gradient test passed (iLQG.c:297-303);
 * 2 accepted step with dcost < tolFun (iLQG.c:330-335); 3 max_iter iterations done (iLQG.c:372-376); 4 backward pass:
 * lambda > lambdaMax (iLQG.c:273-274); 5 rejected step: lambda > lambdaMax (iLQG.c:356-360); 6 NaN/Inf in calc_derivs
 * (iLQG.c:247-249); 7 NaN/Inf in the initial roll-out (iLQG_mex.c:116).
 * ilqg_reference_success: what the reference's iLQG() returns for that exit (1 for 1, 2, 5; 0 for 3, 4, 7; for 6 the
 * back-pass flag of the previous iteration is still set, iLQG.c:247-249 and 365-378: 1 unless no iteration was done). */
int ilqg_reference_success(int status, int iterations);

/* For a collective over device memory: a per-trajectory scalar of the whole batch ("cost", ...) copied device to
 * device into `dst_device` (batch doubles, contiguous); synchronises.  ilqg_batch_cost_device_ptr is the address
 * of the cost vector itself while the batch is ONE group (NULL otherwise); ilqg_batch_stream the HIP stream of
 * the first group. */
int ilqg_batch_scalar_to_device(ilqg_batch_t *c, const char *name, void *dst_device);
void *ilqg_batch_cost_device_ptr(ilqg_batch_t *c);
void *ilqg_batch_stream(ilqg_batch_t *c);

/* ---- several GPUs of one node, ONE process (no reference counterpart) -----------------------------
 * The batch is sharded in contiguous blocks of ceil(batch / n_devices) trajectories; device g advances its block with
 * the interface above and shares nothing with the others.  The single exchange is ilqg_multi_gather_costs: one
 * ncclGather (RCCL, xGMI) of the per-trajectory costs to the first device, delivered to the host.  devices = NULL:
 * devices 0..n_devices-1.  Host arrays are those of the batch interface for the WHOLE batch. */
#define ILQG_MULTI_MAX 16
typedef struct ilqg_multi ilqg_multi_t;
ilqg_multi_t *ilqg_multi_create(int n_devices, const int *devices, int batch, int n_hor); /* NULL: ilqg_multi_error(NULL) */
void ilqg_multi_destroy(ilqg_multi_t *m);
const char *ilqg_multi_error(const ilqg_multi_t *m);
int ilqg_multi_devices(const ilqg_multi_t *m);
/* the batch object of device g and its block of the batch (for everything not forwarded below) */
ilqg_batch_t *ilqg_multi_shard(ilqg_multi_t *m, int g, int *first, int *count);
int ilqg_multi_set_option(ilqg_multi_t *m, const char *name, const double *value, int n);
int ilqg_multi_set_param(ilqg_multi_t *m, const char *name, const double *value, int n);
int ilqg_multi_set_params_batch(ilqg_multi_t *m, int n_names, const char *const *names, const double *values);  /* [batch][W], sharded by rows */
int ilqg_multi_set_param_steps_batch(ilqg_multi_t *m, const char *name, const double *values);  /* [batch][n_hor+1], sharded by rows */
int ilqg_multi_shift_param_batch(ilqg_multi_t *m, const char *name, int steps, const double *tail);  /* [batch][steps] or NULL */
int ilqg_multi_set_x0(ilqg_multi_t *m, const double *x0);
int ilqg_multi_set_u(ilqg_multi_t *m, const double *u);
int ilqg_multi_init(ilqg_multi_t *m);
int ilqg_multi_shift(ilqg_multi_t *m, int steps, const double *x0_new, const double *u_tail);  /* ilqg_batch_shift per shard */
/* ilqg_batch_best_of / ilqg_batch_shift_winners per shard; winner[] is absolute in the WHOLE batch.  Refused, with the reason
 * in the text, when a shard's first trajectory is not a multiple of K (the shard boundary would cut a segment). */
int ilqg_multi_best_of(ilqg_multi_t *m, int K, const double *score, int *winner, double *best, int *n_eligible);
int ilqg_multi_shift_winners(ilqg_multi_t *m, int K, const int *winner, int steps, const double *x0_new, const double *u_tail, const double *du);
int ilqg_multi_head(ilqg_multi_t *m, int steps, double *x, double *u, double *l, double *L, double *cost);  /* ilqg_batch_head per shard */
int ilqg_multi_policy_rollout(ilqg_multi_t *m, int n_starts, const double *x0, double alpha, int feedback, double *cost, int *ok,
                              double *x_end, double *x, double *u);  /* ilqg_batch_policy_rollout per shard (host memory) */
/* ilqg_batch_policy_rollout_params per shard (host memory): values is offset by the shard's first trajectory unless shared */
int ilqg_multi_policy_rollout_params(ilqg_multi_t *m, int n_starts, const double *x0, int n_names, const char *const *names, const double *values,
                                     int shared, double alpha, int feedback, double *cost, int *ok, double *x_end, double *x, double *u);
/* ilqg_batch_policy_rollout_noise per shard (host memory): a full disturbance table is offset by the shard's first trajectory
 * like values, a shared one is given to every shard */
int ilqg_multi_policy_rollout_noise(ilqg_multi_t *m, int n_starts, const double *x0, int n_names, const char *const *names, const double *values,
                                    int shared, const double *disturbance, int disturbance_shared, double alpha, int feedback, double *cost,
                                    int *ok, double *x_end, double *x, double *u);
/* ilqg_batch_policy_rollout_drawn per shard (host memory): shard g draws under first_trajectory + its own first trajectory,
 * so the bits are those of the single batch */
int ilqg_multi_policy_rollout_drawn(ilqg_multi_t *m, int n_starts, const double *x0, int n_names, const char *const *names, const double *values,
                                    int shared, unsigned long long seed, const double *sigma, int noise_shared, long long first_trajectory,
                                    double alpha, int feedback, double *cost, int *ok, double *x_end, double *x, double *u);
/* ilqg_batch_receding_plant per shard, one shard after the other (host memory): every [B]... array is offset by the shard's first trajectory */
int ilqg_multi_receding_plant(ilqg_multi_t *m, int rounds, int steps, int iterations, int feedback, double *x_plant, int n_names,
                              const char *const *names, const double *values, const double *disturbance, double *x_applied, double *u_applied,
                              double *cost_applied, double *plan_cost, int *ok);
/* ilqg_batch_receding_plant_windows per shard: a future of a name that has rows is [batch][rounds*steps], sharded by rows like
 * every other [B]... array; a shared future goes to every shard as it is */
int ilqg_multi_receding_plant_windows(ilqg_multi_t *m, int rounds, int steps, int iterations, int feedback, double *x_plant, int n_names,
                                      const char *const *names, const double *values, const double *disturbance, int n_windows,
                                      const char *const *window_names, const double *const *future, double *x_applied, double *u_applied,
                                      double *cost_applied, double *plan_cost, int *ok);
int ilqg_multi_iterate(ilqg_multi_t *m, int n);   /* asynchronous on every device; the devices are served in turn */
int ilqg_multi_solve(ilqg_multi_t *m);
int ilqg_multi_sync(ilqg_multi_t *m);
int ilqg_multi_active(ilqg_multi_t *m, int *n_active);
int ilqg_multi_get_x(ilqg_multi_t *m, double *x);
int ilqg_multi_get_u(ilqg_multi_t *m, double *u);
int ilqg_multi_get_int(ilqg_multi_t *m, const char *name, int *out);
/* ilqg_batch_set_history / _get_history / _get_history_int per shard; out [batch][cap] resp. [batch], placed by rows */
int ilqg_multi_set_history(ilqg_multi_t *m, int cap);
int ilqg_multi_get_history(ilqg_multi_t *m, const char *name, double *out);
int ilqg_multi_get_history_int(ilqg_multi_t *m, const char *name, int *out);
int ilqg_multi_history_cap(const ilqg_multi_t *m);
int ilqg_multi_gather_costs(ilqg_multi_t *m, double *cost /* [batch] */);

/* The reference's MEX entry for a C caller (iLQG_mex.c:19-144):
 *     [success, x, u, cost] = iLQG<Problem>(x0, u_nom, params, opts)
 * One trajectory through the drop-in iLQG() (outer loop on the host, back_pass() / line_search() on the GPU).
 * params: every parameter of the problem by name (length checked against paramdesc[]); opts: setOptParam keys.
 * x [n_hor+1][N_X], u [n_hor][N_U], cost, iterations, seconds (wall time of iLQG() alone, iLQG_mex.c:123-126) out.
 * Returns iLQG()'s 1 / 0, or -1 with the MEX entry's message in err when an argument is refused. */
typedef struct {
    const char *name;
    const double *value;
    int n;
} ilqg_named_t;
int ilqg_solve_single(int n_hor, const double *x0, const double *u_nom, const ilqg_named_t *params, int n_params_given,
                      const ilqg_named_t *opts, int n_opts, double *x, double *u, double *cost, int *iterations,
                      double *seconds, char *err, int err_len);

/* per-kernel device time measured with HIP events on the context's stream */
int ilqg_batch_timing(ilqg_batch_t *c, int enable);
int ilqg_batch_kernel_count(void);
const char *ilqg_batch_kernel_name(int kernel);
int ilqg_batch_get_timing(ilqg_batch_t *c, int kernel, int *launches, double *total_ms);
/* ms of wall clock the kernel occupied since timing was switched on: the union of its launch intervals per group of
 * trajectories, summed over the groups (launches on a group's two streams overlap in the event clock) */
int ilqg_batch_get_busy(ilqg_batch_t *c, int kernel, double *busy_ms);

/* device box-QP on `count` independent problems of size n in {2, 8, N_U} (unit tests) */
int ilqg_boxqp_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                     const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc);

/* the same problems through the cooperative form the one-wavefront-per-trajectory mapping uses
 * (one problem per wavefront, one lane per variable); same results bit for bit */
int ilqg_boxqp_wave_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                          const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc);

/* ... and through the per-lane form that factorises every clamp pattern up front (n = 2, or N_U when N_U <= 3) */
int ilqg_boxqp_table_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                           const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc);

/* ... and through the form of the quad mapping (four problems per wavefront, one per 16-lane row; n = 2 or N_U).
 * active: one int per problem, 0 = the problem's row runs along without committing anything (x stays as given, rc 0),
 * NULL = every problem active.  Only the libraries of the one-wavefront-per-trajectory mapping carry this form; any
 * other refuses before anything is allocated, text via ilqg_batch_error(NULL) */
int ilqg_boxqp_quad_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                          const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc, const int *active);

/* device sin/cos as the generated callbacks see them, on n arguments (unit tests) */
int ilqg_sincos_batch(int device, int n, const double *x, double *s, double *c);

#ifdef __cplusplus
}
#endif
#endif
