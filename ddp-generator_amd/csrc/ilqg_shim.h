/* Thin extern-"C" boundary between the C host code (ilqg_host.c) and the HIP
 * kernels (ilqg_kernels.hip).  Plain pointers, ints and doubles only.
 *
 * Host-side data crosses this boundary in trajectory-major layout
 * [trajectory][time step][field], i.e. what a caller holding `trajEl_t`
 * arrays can produce with a memcpy per field (reference iLQG_mex.c:113-137
 * walks its trajectories the same way).  The device layouts (packed per-step
 * trajectory records, tiled arrays) are private to ilqg_kernels.hip, see
 * DESIGN.md section 2.
 */
#ifndef ILQG_SHIM_H
#define ILQG_SHIM_H

#ifdef __cplusplus
extern "C" {
#endif

#define ILQG_MAX_ALPHA 16

typedef struct ilqg_dev ilqg_dev_t;

/* solver options, same meaning as the fields of tOptSet (reference iLQG.h:37-76) */
typedef struct {
    int n_alpha;
    double alpha[ILQG_MAX_ALPHA];
    double tolFun, tolGrad, tolConstraint;
    double lambdaInit, dlambdaInit, lambdaFactor, lambdaMax, lambdaMin;
    double zMin;
    int regType;
    int max_iter;
    double w_pen_init_l, w_pen_init_f, w_pen_max_l, w_pen_max_f, w_pen_fact1, w_pen_fact2;
    int resweep; /* 1: repeat the reference's cost-only sweep after an accepted step (iLQG.c:338) */
    int ls_split; /* step sizes rolled out for every trajectory in the first line-search stage; the rest only
                   * for trajectories still without an acceptable one (0 or >= n_alpha: single stage) */
    int ls_keep; /* 2 (lane mapping; the default there): every roll-out of the line search is KEPT where it is rolled out
                  * and an accepted trajectory becomes the current one by a change of its location index (k_search,
                  * k_commit): no second roll-out of the winner, no copy;
                  * 1: the second stage keeps the trajectories it rolls out and runs side by side with the winner pass
                  * of the first stage's trajectories; 0: second stage, then one winner pass for all */
    int bw_split; /* 1: the fused backward pass runs on two wavefronts per 64 trajectories (derivatives of step k-1 on
                   * one, Riccati update of step k on the other) where the problem allows it; 0: on one */
    int fuse_derivs; /* 1: ilqg_dev_iterate evaluates derivatives inside the backward kernel (no records in HBM) */
} ilqg_dev_opts_t;

/* per-trajectory status of the lock-step solver */
enum {
    ILQG_ST_ACTIVE = 0,
    ILQG_ST_CONVERGED_GRAD = 1, /* g_norm < tolGrad && lambda < 1e-5      (iLQG.c:297-303) */
    ILQG_ST_CONVERGED_FUN = 2,  /* accepted step with dcost < tolFun      (iLQG.c:330-335) */
    ILQG_ST_MAX_ITER = 3,       /* max_iter iterations done               (iLQG.c:372-376) */
    ILQG_ST_NO_DESCENT = 4,     /* back pass: lambda > lambdaMax          (iLQG.c:273-274) */
    ILQG_ST_LAMBDA_MAX = 5,     /* rejected step: lambda > lambdaMax      (iLQG.c:356-360) */
    ILQG_ST_DERIVS_FAILED = 6,  /* NaN/Inf in calc_derivs                 (iLQG.c:247-249) */
    ILQG_ST_INIT_FAILED = 7     /* NaN/Inf in the initial roll-out        (iLQG_mex.c:116) */
};

/* double-valued device fields.  [N] = n_hor */
enum {
    ILQG_F_X = 0,    /* [N+1][N_X]   nominal states                     */
    ILQG_F_U,        /* [N][N_U]     nominal controls                   */
    ILQG_F_LG,       /* [N][N_U]     feed-forward gains l               */
    ILQG_F_KG,       /* [N][N_U*N_X] feedback gains L (column-major)    */
    ILQG_F_DER,      /* [N][host record] derivative records             */
    ILQG_F_FIN,      /* [N_X+sizeofQxx] final cx, cxx                   */
    ILQG_F_MUL,      /* [N][multipliersEl_t as doubles] running multipliers (problems with hle / hli) */
    ILQG_F_MULF,     /* [multipliersFin_t as doubles]   final multipliers (problems with hfe / hfi)   */
    ILQG_F_COST,     /* scalars per trajectory from here on             */
    ILQG_F_NEW_COST,
    ILQG_F_DCOST,
    ILQG_F_EXPECTED,
    ILQG_F_LAMBDA,
    ILQG_F_DLAMBDA,
    ILQG_F_GNORM,
    ILQG_F_DV0,
    ILQG_F_DV1,
    ILQG_F_WPEN_L,   /* current penalty weights o->w_pen_l / o->w_pen_f (iLQG.h:78) */
    ILQG_F_WPEN_F,
    ILQG_F_WPEN_L_DER, /* the weights the current derivatives were evaluated with: a rejected step may raise  */
    ILQG_F_WPEN_F_DER, /* w_pen_* (iLQG.c:345-349) while the derivatives stay those of the last accepted step */
    ILQG_F_ALPHA_COST, /* [n_alpha] cost of every step size of the last line search */
    ILQG_F_COUNT
};

/* int-valued device fields, one value per trajectory unless noted */
enum {
    ILQG_I_STATUS = 0,
    ILQG_I_ITER,        /* reference's o->iterations                     */
    ILQG_I_NEED_DERIVS,
    ILQG_I_ALPHA_IDX,   /* 1-based accepted step index, n_alpha+1 = none */
    ILQG_I_ACCEPTED,
    ILQG_I_BP_CALLS,    /* backward sweeps in the last iteration         */
    ILQG_I_BP_RC,       /* result of the last backward sweep: 0 ok, 1 failed */
    ILQG_I_RESWEEP,     /* set by the update: 2 = update multipliers + cost sweep (iLQG.c:337-338), 1 = cost
                         * sweep after a rejected step raised the penalty weights (iLQG.c:345-349), 0 = none */
    ILQG_I_LOC,         /* lane mapping, ls_keep = 2: where the CURRENT (x, u) of the trajectory lives: 0 = the arrays
                         * X / U, p > 0 = plane p - 1 of the kept roll-outs of the line search (see cur_x) */
    ILQG_I_ALPHA_OK,    /* [n_alpha] forward pass finite?                */
    ILQG_I_COUNT
};

/* kernels, for timing queries */
enum {
    ILQG_K_DERIVS = 0,
    ILQG_K_BACKWARD,
    ILQG_K_ROLLOUT_SEARCH,
    ILQG_K_SELECT,
    ILQG_K_ROLLOUT_WINNER,
    ILQG_K_UPDATE,
    ILQG_K_ROLLOUT_COST,
    ILQG_K_ROLLOUT_INIT,
    ILQG_K_TRANSPOSE,
    ILQG_K_BACKWARD_FUSED,
    ILQG_K_ROLLOUT_SEARCH2,
    ILQG_K_MULTIPLIERS,
    ILQG_K_SEARCH,   /* ls_keep = 2: k_search on all trajectories (first stage) */
    ILQG_K_SEARCH2,  /*             k_search on the pending list (second stage) */
    ILQG_K_ADOPT,    /*             k_adopt_home / k_rejected_home, k_commit */
    ILQG_K_SHIFT,    /* receding horizon: k_shift_lane / k_shift_wave (ilqg_dev_shift) */
    ILQG_K_LOG,      /*                   k_log_steps (ilqg_dev_loop_apply) */
    ILQG_K_HEAD,     /*                   k_head (ilqg_dev_head) */
    ILQG_K_SHIFT_PARAM, /*                k_shift_param_rows on the one shared row (ilqg_dev_shift_param) */
    ILQG_K_POLICY,   /* k_policy (ilqg_dev_policy_rollout) */
    ILQG_K_POLICY_PARAMS, /* k_policy<true> (ilqg_dev_policy_rollout with a table) */
    ILQG_K_PLANT,    /* k_plant (ilqg_dev_loop_apply with plants) */
    ILQG_K_SHIFT_PARAM_ROWS, /* k_shift_param_rows (ilqg_dev_shift_param_batch) */
    ILQG_K_SHIFT_WINDOWS, /* k_shift_windows (ilqg_dev_loop_shift) */
    ILQG_K_HISTORY,  /* k_history (ilqg_dev_update of a context with a history) */
    ILQG_K_COUNT
};
/* timing slots added since: a second list that continues the first, so that every index above keeps its meaning */
enum {
    ILQG_K_BEST_OF = ILQG_K_COUNT, /* candidates per agent: k_best_of (ilqg_dev_best_of) */
    ILQG_K_SHIFT_WINNERS,          /*                       k_shift_winners_lane / _wave (ilqg_dev_shift_winners) */
    ILQG_K_POLICY_DRAWN,           /* process noise drawn on the device: the drawn launch of ilqg_dev_policy_rollout_drawn — k_policy_drawn, or (N_X > 8) k_policy with `spec` */
    ILQG_K_POLICY_DRAWN_PARAMS,    /*                       the same with a table of parameter rows (k_policy_drawn<true> / k_policy<true>) */
    ILQG_K_NOISE_FILL,             /*                       k_noise_fill (ilqg_dev_noise_table) */
    ILQG_K_TOTAL
};

/* fields of an entry of the iteration history (ilqg_dev_set_history): doubles ... */
enum {
    ILQG_H_COST = 0, /* ILQG_F_COST: the nominal cost the search started from */
    ILQG_H_NEW_COST, /* ILQG_F_NEW_COST: the reference's log_cost             */
    ILQG_H_Z,        /* reduction_ratio(dcost, expected): its log_z           */
    ILQG_H_LAMBDA,   /* behind the backward pass's retries, before the update */
    ILQG_H_GNORM,
    ILQG_H_DV0,
    ILQG_H_DV1,
    ILQG_H_WPEN_L,   /* these two in libraries of problems with multipliers only */
    ILQG_H_WPEN_F,
    ILQG_H_COUNT
};
/* ... and ints; ILQG_HI_N is no field of an entry but the per-trajectory count of entries */
enum {
    ILQG_HI_N = -1,
    ILQG_HI_ALPHA_IDX = 0, /* 1-based, n_alpha + 1 = none: the reference's log_linesearch */
    ILQG_HI_BP_CALLS,
    ILQG_HI_ITER,          /* ILQG_I_ITER then: the index the reference logs under */
    ILQG_HI_COUNT
};

/* all functions return 0 on success, non-zero on error (message via ilqg_dev_error) */
const char *ilqg_dev_error(void);
int ilqg_dev_count(void);
int ilqg_dev_create(ilqg_dev_t **out, int device, int batch, int n_hor);
void ilqg_dev_destroy(ilqg_dev_t *d);

/* compile-time facts of the problem this library was built for:
 * out[0..7] = N_X, N_U, FULL_DDP, host record size, device record size, state-dependent limits, n_params,
 * mapping (0 = one lane per trajectory, 1 = one wavefront per trajectory) */
void ilqg_dev_dims(int *out);
/* out[0..1] = doubles in multipliersEl_t / multipliersFin_t (0 for a problem without such constraints) */
void ilqg_dev_multiplier_dims(int *out);

int ilqg_dev_set_params(ilqg_dev_t *d, int n_params, const int *sizes, const double *const *values);
/* Per-trajectory problem parameters (lane mapping only; the wave mapping refuses, naming itself).  From the next launch on
 * every generated callback evaluated for trajectory b sees the context's fixed-size parameters with the n_named parameters
 * named[] (indices into paramdesc[], as for ilqg_dev_policy_rollout with R = 1 and shared = 0: fixed size, none twice)
 * replaced by row b of values [batch][W].  The context keeps its own copy of the table, in a buffer that only grows.
 * on_device = 0: values is host memory, waits once; on_device != 0: device memory of the context's device, copied in the
 * order of the context's stream, no wait and (at an unchanged size) no allocation.  n_named = 0 clears the set: the kernels
 * are then those of a context that never had one; named and values are not read.  A call replaces the whole set.  Order with
 * the tables of ilqg_dev_policy_rollout and ilqg_dev_loop_begin: the trajectory's row first, then the roll-out's or plant's.
 * ilqg_dev_move carries the rows of the trajectories it moves; the destination takes the source's map.  Touches no
 * trajectory and launches no kernel.  get: the table as it is on the device, rows [batch][W] (host); waits. */
int ilqg_dev_set_params_batch(ilqg_dev_t *d, int n_named, const int *named, const double *values, int on_device);
int ilqg_dev_get_params_batch(ilqg_dev_t *d, double *rows);
/* Per-time-step parameters per trajectory (lane mapping only).  index: a parameter of size -1 in paramdesc[].  From the next
 * launch on the callbacks evaluated for trajectory b read p[index][k], k = 0 .. n_hor, from row b of values [batch][n_hor + 1]
 * (trajectory-major); values = NULL: the shared window of ilqg_dev_set_params again.  One grow-only buffer per parameter,
 * independent of the fixed-size table above and of ilqg_dev_set_params; on_device as above.  With no rows and no table left
 * the kernels are those of a context that never had either.  ilqg_dev_move carries the rows.  Launches no kernel.
 * get: the rows as they are on the device (host, [batch][n_hor + 1]); waits; an error where the parameter is shared.
 * shift: per row what ilqg_dev_shift_param does, in place (k_shift_param_rows); tail [batch][steps] or NULL (each row's
 * last value held), host memory (staged, waits once) or with on_device != 0 device memory (no wait). */
int ilqg_dev_set_param_steps_batch(ilqg_dev_t *d, int index, const double *values, int on_device);
int ilqg_dev_get_param_steps_batch(ilqg_dev_t *d, int index, double *rows);
int ilqg_dev_shift_param_batch(ilqg_dev_t *d, int index, int steps, const double *tail, int on_device);
int ilqg_dev_set_opts(ilqg_dev_t *d, const ilqg_dev_opts_t *o);

/* host <-> device, host side trajectory-major [batch][steps][width] */
int ilqg_dev_write(ilqg_dev_t *d, int field, const double *host);
int ilqg_dev_read(ilqg_dev_t *d, int field, double *host);
/* only the first `steps` time steps of a field, host [batch][steps][width] (e.g. x0 = step 0 of X) */
int ilqg_dev_write_steps(ilqg_dev_t *d, int field, const double *host, int steps);
int ilqg_dev_write_int(ilqg_dev_t *d, int field, const int *host);
int ilqg_dev_read_int(ilqg_dev_t *d, int field, int *host);
/* Deferred transfers: between begin and end the write / read calls above return without waiting (each uses its own
 * slice of a pinned staging buffer); ilqg_dev_io_end waits once for everything on the stream and only then are the
 * arrays of the read calls filled.  Kernels launched in between run in stream order with the transfers. */
int ilqg_dev_io_begin(ilqg_dev_t *d);
int ilqg_dev_io_end(ilqg_dev_t *d);
int ilqg_dev_field_width(int field);                 /* doubles per step and trajectory (host view) */
int ilqg_dev_field_steps(ilqg_dev_t *d, int field);  /* time steps stored */
/* device address of a per-trajectory scalar field (for collectives on device memory) */
void *ilqg_dev_field_ptr(ilqg_dev_t *d, int field);
void *ilqg_dev_stream(ilqg_dev_t *d);
/* a per-trajectory scalar field (batch doubles) into device memory of the caller, on the context's stream */
int ilqg_dev_copy_scalar_to(ilqg_dev_t *d, int field, void *dst_device);

/* stages (all asynchronous on the context's stream) */
int ilqg_dev_reset(ilqg_dev_t *d);            /* solver entry state (iLQG.c:226-237) */
int ilqg_dev_rollout_init(ilqg_dev_t *d);     /* forward_pass(alpha = 0) + swap (iLQG_mex.c:113-120) */
/* Receding horizon: every trajectory's current controls move `steps` time steps towards the start, u'[k] = u[k + steps],
 * the last one held over the tail; with use_plan_x0 the state the plan reaches after `steps` steps becomes x0.  Read where
 * the current trajectory lives, written to the arrays X / U (records in the wave mapping); the location indices are
 * cleared, so the ilqg_dev_rollout_init that follows copies nothing.  0 <= steps < n_hor. */
int ilqg_dev_shift(ilqg_dev_t *d, int steps, int use_plan_x0);
/* the caller's tail behind a shift: tail [batch][steps][N_U] into the last `steps` time steps of the controls.  on_device = 0:
 * the array is host memory (staged, one wait); else device memory of the context's device, used on the context's stream without
 * a wait. */
int ilqg_dev_put_u_tail(ilqg_dev_t *d, const double *tail, int steps, int on_device);
/* Candidates per agent: the context's trajectories as batch / K segments of K consecutive slots, K one of 1, 2, 4, .. 64
 * and a divisor of batch and of `first`, the batch-absolute index of the context's first trajectory (refused otherwise: the
 * kernels rely on a segment never leaving a tile of 64).  on_device = 0: the arrays are host memory (staged, one wait);
 * else device memory of the context's device, used on the context's stream without a wait.
 * best_of: per segment the eligible slot (score finite, status not ILQG_ST_INIT_FAILED) with the smallest score, equal scores
 * to the lowest index: winner [batch / K] batch-absolute or -1, best [batch / K] its score or NaN, n_eligible [batch / K];
 * score [batch] or NULL = the current cost; best / n_eligible may be NULL.  Changes nothing of the context (k_best_of).
 * shift_winners: ilqg_dev_shift with use_plan_x0 = (x0_new == NULL), except that slot b of segment g reads the plan of slot
 * winner[g] (batch-absolute) wherever that lives, takes x0_new [batch / K][N_X] / u_tail [batch / K][steps][N_U] of its
 * SEGMENT and adds du [batch][n_hor][N_U] (any of the three NULL).  winner[g] = -1, and on the device any value outside
 * segment g, makes every slot of the segment its own winner.  One kernel (k_shift_winners_lane / _wave); the location
 * indices are cleared as ilqg_dev_shift clears them. */
int ilqg_dev_best_of(ilqg_dev_t *d, int K, int first, const double *score, int *winner, double *best, int *n_eligible, int on_device);
int ilqg_dev_shift_winners(ilqg_dev_t *d, int K, int first, const int *winner, int steps, const double *x0_new, const double *u_tail, const double *du,
                           int on_device);
/* The control interval of a caller with its own plant.  head: the first `steps` steps of every CURRENT plan, read where it
 * lives (nothing moves home), trajectory-major: x [batch][steps][N_X], u / l [batch][steps][N_U], L [batch][steps][N_U*N_X],
 * cost [batch]; any pointer may be NULL; 1 <= steps <= n_hor.  on_device = 0: the arrays are host memory (staged, one wait
 * at most); else device memory of the context's device, used on the context's stream without a wait. */
int ilqg_dev_head(ilqg_dev_t *d, int steps, double *x, double *u, double *l, double *L, double *cost, int on_device);
/* Every plan's feedback policy rolled out from R starts per trajectory (k_policy.inc): forward_pass with the caller's start
 * as x0, the nominal = what ilqg_dev_head hands out (current x / u where they live, l / L of the records), the multipliers
 * and penalty weights the trajectory has, and u_k = u_nom_k [+ alpha l_k if alpha != 0] [+ L_k (x_k - x_nom_k) if feedback].
 * x0 [batch][R][N_X]; outputs, any of them NULL: cost [batch][R], ok [batch][R] (forward_pass's return value; where it is 0
 * the other outputs of that roll-out are unspecified), x_end [batch][R][N_X], x [batch][R][n_hor+1][N_X],
 * u [batch][R][n_hor][N_U] (the clamped controls applied).  Writes nothing of the solver's state.
 * n_named = 0: under the context's parameters (k_policy<false>; named, values, shared are not read).  n_named > 0: each
 * roll-out under problem parameters of its own (k_policy<true>): roll-out (b, r) evaluates every callback with the context's
 * fixed-size parameters, those of the n_named parameters named[] (indices into paramdesc[], each of fixed size, no index
 * twice — the caller has checked names; sizes and range are checked here) replaced by row (b, r) of values:
 * [batch][R][W], or with shared != 0 [R][W] for every trajectory, W = the sum of the named sizes, the named parameters one
 * behind the other in the order of named[].  The policy, multipliers, penalty weights and per-time-step parameters are the
 * context's.  on_device = 0: the arrays are host memory (staged through the context's staging buffer, which only grows, one
 * wait); else device memory of the context's device (values lives where x0 lives), used on the context's stream without a
 * wait.  R >= 1; needs ilqg_dev_set_params before it.
 * dist = NULL: no process noise — the same kernels, launches and bits as before the argument existed.  Else behind every step
 * k = 0 .. n_hor-1 the roll-out's state is pushed, x_{k+1} <- x_next + w[b][r][k] (the rule of ilqg_dev_loop_apply):
 * dist [batch][R][n_hor][N_X], or with dist_shared != 0 [R][n_hor][N_X] for every trajectory; it lives where x0 lives (the
 * host form stages it behind the values).  ok = 0 also where a disturbed state is not finite, the one behind row n_hor-1 —
 * which moves x_end, x[n_hor] and the final cost — included.  No new kernel and no new timing slot. */
int ilqg_dev_policy_rollout(ilqg_dev_t *d, int R, const double *x0, int n_named, const int *named, const double *values, int shared,
                            const double *dist, int dist_shared, double alpha, int feedback, double *cost, int *ok, double *x_end, double *x, double *u,
                            int on_device);
/* The same roll-outs with the process noise DRAWN ON THE DEVICE (k_noise.inc, k_policy_drawn): no table, no upload and no
 * memory proportional to R.  Row (b, r, k) is w[i] = sigma[i] z[i], z the standard normals of Philox4x32-10 under the key
 * (seed & 0xffffffff, seed >> 32) at the counter (k, r, first_trajectory + b, i / 4) — with noise_shared != 0 the trajectory
 * word is 0: every trajectory gets the draws of trajectory 0 —, added by the rule of `dist` above.  A draw depends on its
 * counter alone: its bits are those of any other R, stream group, shard (first_trajectory = the context's first trajectory
 * in the caller's batch) or chunk.  sigma: N_X doubles in HOST memory in every form, each finite and >= 0; first_trajectory
 * >= 0 and first_trajectory + batch <= 2^32 (the caller has checked: ilqg_host.c).  Every other argument as in
 * ilqg_dev_policy_rollout.  The launch runs under timing slots of its own, "k_policy_drawn" / "k_policy_drawn_params": in a
 * library of a problem with N_X <= 8 they time the kernels of that name; in one with N_X > 8 there is no such kernel and they
 * time k_policy launched with its third noise argument (k_policy.inc says why).
 * noise_table: the same draws as a table, w [batch][R][n_hor][N_X] or with noise_shared [R][n_hor][N_X] (k_noise_fill) — what
 * ilqg_dev_policy_rollout's `dist` of the same call is, bit for bit.  Changes nothing of the context. */
int ilqg_dev_policy_rollout_drawn(ilqg_dev_t *d, int R, const double *x0, int n_named, const int *named, const double *values, int shared,
                                  unsigned long long seed, const double *sigma, int noise_shared, long long first_trajectory, double alpha, int feedback,
                                  double *cost, int *ok, double *x_end, double *x, double *u, int on_device);
int ilqg_dev_noise_table(ilqg_dev_t *d, int R, unsigned long long seed, const double *sigma, int noise_shared, long long first_trajectory, double *w,
                         int on_device);
/* The receding-horizon loop that stays on the device: `rounds` times { ilqg_dev_iterate; ilqg_dev_loop_apply; ilqg_dev_loop_shift;
 * ilqg_dev_rollout_init; ilqg_dev_reset } between one ilqg_dev_loop_begin and one ilqg_dev_loop_read — the caller's loop;
 * nothing in it waits or copies.  What the loop is, is stated once, here: */
typedef struct {
    int rounds, steps;          /* rounds >= 1, 1 <= steps < n_hor */
    int plant;                  /* 0: the plans' own heads are recorded (k_log_steps); 1: plants advance (k_plant.inc) */
    /* read only with `plant` (HOST memory): the plants' states [batch][N_X], or NULL = every plan's x_0; the plants' parameters —
     * the context's fixed-size ones with the n_named parameters named[] replaced by row b of values [batch][W], names and W as
     * in ilqg_dev_policy_rollout with R = 1 and shared = 0; n_named = 0: the context's own —; disturbance
     * [batch][rounds*steps][N_X], added to the state behind each step, or NULL = none */
    const double *x_plant;
    int n_named;
    const int *named;
    const double *values, *disturbance;
    int windows;                /* the windows of the per-time-step parameters move `steps` on each round (k_shift_windows) */
    /* read only with `windows` (HOST memory): future[i], i an index into paramdesc[] (n_params entries; those of fixed-size
     * parameters are not read), holds the values beyond parameter i's window for the whole loop: [batch][rounds * steps] where
     * the parameter has rows in this context (ilqg_dev_set_param_steps_batch), [rounds * steps] where it is the shared window,
     * NULL: the window holds its last value, per row.  future itself may be NULL (every window holds) */
    const double *const *future;
} ilqg_dev_loop_t;
/* begin: the one place that checks the shape.  Sizes the logs — x [batch][rounds*steps][N_X], u [..][N_U], the plans' costs
 * [batch][rounds] — and with `plant` the plants' buffers, anew for every loop, and the futures' buffers, which only grow; where
 * one of them does not fit no loop is open and no log or plant is left.  With `plant` it clears the plants' failure flags and
 * the logs (what a failed plant leaves unwritten reaches the host as zeros).  Everything the caller gave goes up once; waits
 * for the stream first and once more behind what it sent.
 * apply (round `round`): without plants (x_k, u_k), k < steps, of every current plan and its cost go to the logs.  With plants
 * every plant that has not failed advances `steps` steps from its own state under the CURRENT plan's policy,
 * u = u_nom_k [+ L_k (xp - x_nom_k) if feedback], through the step of forward_pass under the plant's parameters and the
 * multipliers and penalty weights its slot has, then xp <- x_next + disturbance; the state each control was applied at, the
 * clamped control, the sum of the running costs and the plan's cost go to the logs.  A plant fails — for the rest of the loop,
 * staying at its last finite state — when a step's guards fail or its state is not finite.  Writes nothing of the solver's
 * state.  (k_plant runs on the stream of the roll-out family, between the two hand-overs with the context's stream.)
 * shift (round `round`): with `windows` every size -1 parameter's window moves `steps` on, its tail columns
 * [round * steps, (round + 1) * steps) of its future, in ONE launch on the context's stream (wave mapping: the constant record
 * entries are marked stale as ilqg_dev_shift_param marks them; a library whose problem has no such parameter launches
 * nothing); then ilqg_dev_shift(d, steps, use_plan_x0 = !plant); with plants their states then become x_0 of the plans
 * (ilqg_dev_put_x0_device).  Apply and shift are two calls: the host moves its mirror of a shared window between them.
 * read (waits once): x_plant [batch][N_X] the plants' states now, x [batch][rounds*steps][N_X], u [..][N_U],
 * cost_applied / plan_cost [batch][rounds], ok [batch] (0 = failed); any may be NULL; x_plant, cost_applied and ok need a
 * loop with plants. */
int ilqg_dev_loop_begin(ilqg_dev_t *d, const ilqg_dev_loop_t *loop);
int ilqg_dev_loop_apply(ilqg_dev_t *d, int round, int feedback);
int ilqg_dev_loop_shift(ilqg_dev_t *d, int round);
int ilqg_dev_loop_read(ilqg_dev_t *d, double *x_plant, double *x, double *u, double *cost_applied, double *plan_cost, int *ok);
/* ilqg_dev_write_steps(d, ILQG_F_X, x0, 1) with the source in DEVICE memory: no staging, no wait */
int ilqg_dev_put_x0_device(ilqg_dev_t *d, const double *x0);
/* Ordering with a stream of the caller (a hipStream_t, NULL = the null stream), by events made once per context: after
 * stream_in the context's stream runs behind everything enqueued on `stream` so far; after stream_out `stream` runs behind
 * everything enqueued on the context's stream so far.  Neither waits on the host. */
int ilqg_dev_stream_in(ilqg_dev_t *d, void *stream);
int ilqg_dev_stream_out(ilqg_dev_t *d, void *stream);
/* 0 if [ptr, ...) is device memory on the context's device, else 1 with a message that names `what` */
int ilqg_dev_check_device_ptr(ilqg_dev_t *d, const void *ptr, const char *what);
/* The window of per-time-step parameter `index` (its n_hor + 1 doubles on the device) moves `steps` values on, in place:
 * p'[k] = p[k + steps], the last `steps` from tail [steps] (host) or p[n_hor] held if tail is NULL; 0 <= steps <= n_hor.
 * Needs ilqg_dev_set_params before it.  (Wave mapping: the constant record entries are marked stale as
 * ilqg_dev_set_params marks them; no wave-mapped problem with such a parameter is built in this tree, so that path is
 * untested.) */
int ilqg_dev_shift_param(ilqg_dev_t *d, int index, int steps, const double *tail);
int ilqg_dev_derivs(ilqg_dev_t *d);           /* calc_derivs for trajectories that need it */
/* back_pass.  mode 0: records from HBM + lambda retry loop + gradient test; 1: records from HBM, one
 * sweep (drop-in back_pass()); 2: as 0 with the derivatives evaluated on the fly (no k_derivs needed) */
int ilqg_dev_backward(ilqg_dev_t *d, int mode);
int ilqg_dev_search(ilqg_dev_t *d);           /* all step sizes in parallel + first-acceptable selection */
int ilqg_dev_winner(ilqg_dev_t *d);           /* re-roll the accepted step size, storing the trajectory */
int ilqg_dev_update(ilqg_dev_t *d);           /* accept/reject bookkeeping (iLQG.c:311-361) */
int ilqg_dev_iterate(ilqg_dev_t *d, int n);   /* n lock-step iterations */
/* The iteration history: with capacity cap > 0 every ilqg_dev_update first appends, for every trajectory that is
 * ILQG_ST_ACTIVE then (its line search has just run), one entry of the ILQG_H_* / ILQG_HI_* fields at position n[b] of the
 * trajectory's own count, which goes up by one; entries at positions >= cap are dropped while n counts on (k_history, one
 * launch in front of k_update on its stream).  set: cap > 0 allocates (two buffers of the context) and clears counts and
 * entries — at an unchanged cap it clears in the order of the context's stream, without a wait or an allocation —, cap = 0
 * frees; a context without a history launches and allocates nothing.  Where the new buffers do not fit, the history stays as
 * it was.  ilqg_dev_shift and ilqg_dev_reset do not clear.  ilqg_dev_move carries the count and the min(n, cap) entries of
 * every trajectory it moves; a destination without a history gets one of the source's capacity.
 * get (waits): field ILQG_H_* into out [batch][cap]; get_int: ILQG_HI_N into out [batch], ILQG_HI_* into out [batch][cap];
 * unwritten entries are zero.  cap: the capacity, 0 = none.
 * reserve: makes the buffers of capacity cap aside and changes nothing else; the set of that cap that follows takes them and
 * cannot fail for memory (a caller with several contexts reserves on all before it sets on any).  cap <= 0 or the capacity
 * the context has: releases what was aside. */
int ilqg_dev_reserve_history(ilqg_dev_t *d, int cap);
int ilqg_dev_set_history(ilqg_dev_t *d, int cap);
int ilqg_dev_get_history(ilqg_dev_t *d, int field, double *out);
int ilqg_dev_get_history_int(ilqg_dev_t *d, int field, int *out);
int ilqg_dev_history_cap(const ilqg_dev_t *d);
int ilqg_dev_sync(ilqg_dev_t *d);
int ilqg_dev_count_active(ilqg_dev_t *d, int *n_active); /* synchronises */
/* solver state of trajectories from[0..count) of src -> trajectories to[0..count) of dst (same device and horizon): current
 * x / u (they arrive in dst's arrays X / U), records, scalars, integers, multipliers; with_records: also the stored
 * derivative records (contexts iterated with fuse_derivs = 0).  Synchronises both contexts. */
int ilqg_dev_move(ilqg_dev_t *dst, ilqg_dev_t *src, int count, const int *to, const int *from, int with_records);
/* What a stream of starts reads of its finished trajectories, without reading the batch: of trajectories from[0..count) the
 * cost, status and iteration count, with x / u != 0 the current trajectory (read where it lives, as ilqg_dev_head reads it), and
 * the n_hist history fields hist_field[i] — with hist_int[i] = 0 a double field, else an int field or ILQG_HI_N — are gathered
 * into one packed buffer of the context, which only grows, by ONE launch (k_harvest) and copied to pinned host memory by ONE
 * copy.  ilqg_dev_harvest queues all of it on the context's stream and returns (`from` is read before it does);
 * ilqg_dev_harvest_wait waits for that stream.  *records: that memory, valid until the context's next harvest; count records of *words 8-byte words each,
 * start-major: word 0 the cost, word 1 the ints { status, iterations }, from word offsets[0] x [n_hor+1][N_X], from word
 * offsets[1] u [n_hor][N_U] (-1: not asked for), from word offsets[2 + i] history field i: cap doubles, or cap ints two to a
 * word, or the count alone — min(n, cap) entries, zeros behind them.  Refused before anything is queued: an index out of range,
 * history fields of a context without a history, a field the library does not record.  Timed under ILQG_K_TRANSPOSE. */
typedef struct {
    int x, u, n_hist;
    const int *hist_int, *hist_field;
} ilqg_dev_harvest_t;
int ilqg_dev_harvest(ilqg_dev_t *d, int count, const int *from, const ilqg_dev_harvest_t *what, int *words, int *offsets);
int ilqg_dev_harvest_wait(ilqg_dev_t *d, const void **records);

/* builds with -DILQG_PROFILE_SECTIONS: cycles per section of the fused backward step, summed over wavefronts */
int ilqg_dev_section_cycles(unsigned long long *out8);
int ilqg_dev_derivs_cycles(unsigned long long *out32);
/* quad mapping with speculative retries (ILQG_QUAD_SPEC=1): the protocol's words after the last backward launch (measurement) */
int ilqg_dev_spec_words(unsigned *out, size_t max_words, size_t *count);
/* builds with -DILQG_WAVE_PLACES: where and when the wavefronts of the backward and search kernels ran (3 words per entry) */
int ilqg_dev_wave_places(unsigned long long *out, int max_entries, int *count);

/* per-kernel HIP-event timing on the context's stream */
int ilqg_dev_timing(ilqg_dev_t *d, int enable);
int ilqg_dev_get_timing(ilqg_dev_t *d, int kernel, int *launches, double *total_ms);
int ilqg_dev_get_busy(ilqg_dev_t *d, int kernel, double *busy_ms);  /* union of the kernel's launch intervals */
const char *ilqg_dev_kernel_name(int kernel);

/* unit-test entry for the device box-QP (same template the backward kernel uses):
 * `count` independent problems of size n (2 or 8), arrays [count][...] */
int ilqg_dev_boxqp_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                         const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc);

/* the same for the wave mapping's cooperative form (one problem per wavefront, one lane per variable) */
int ilqg_dev_boxqp_wave_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                              const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc);

/* ... and for the per-lane form with the factorisations of all clamp patterns made up front (n = 2 or N_U <= 3;
 * ilqg_device.hpp chol_pattern_table: measured no faster, off in the kernels, kept tested) */
int ilqg_dev_boxqp_table_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                               const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc);

/* ... and for the quad mapping's form (ilqg_quad.hpp box_qp_quad: four problems per wavefront, one per 16-lane row;
 * n = 2 or N_U).  active: one int per problem, 0 = the row computes along and commits nothing (x unchanged, rc 0);
 * NULL = all active.  Libraries of the wave mapping only; elsewhere refused, with a message, before anything is allocated */
int ilqg_dev_boxqp_quad_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                              const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc, const int *active);

/* the reference's small dense helpers on the device (one problem): op 0 addMulVec, 1 addSquareTri, 2 addMul2Tri
 * (shape 0 = (N_X,N_U), 1 = (N_X,N_X), 2 = (N_U,N_X[,1])), 3 cholesky_tri, 4 cholesky_tri_inv (shape = n).
 * flag: 1 ok, 0 Cholesky pivot <= 0, -1 size not built */
int ilqg_dev_dense(int device, int op, int shape, const double *in0, int n_in0, const double *in1, int n_in1,
                   const double *in2, int n_in2, double *out, int n_out, int *flag);

/* Several GPUs in one process: an RCCL communicator over n distinct devices (ncclCommInitAll) and the path's single
 * collective: the caller fills device g's send buffer (per doubles, e.g. with ilqg_dev_copy_scalar_to) and waits for
 * the copies; ilqg_comm_gather then moves all of them to device 0 by one ncclGather and on to the host. */
typedef struct ilqg_comm ilqg_comm_t;
int ilqg_comm_create(ilqg_comm_t **out, int n, const int *devices, int per);
void ilqg_comm_destroy(ilqg_comm_t *c);
void *ilqg_comm_send_buffer(ilqg_comm_t *c, int g);  /* device g's `per` doubles, on device g */
int ilqg_comm_gather(ilqg_comm_t *c, ilqg_dev_t *const *devs, const int *first, const int *counts, double *host);

/* unit-test entry for the device sincos that the generated callbacks' sin()/cos() are routed through */
int ilqg_dev_sincos_batch(int device, int n, const double *x, double *s, double *c);

#ifdef __cplusplus
}
#endif
#endif
