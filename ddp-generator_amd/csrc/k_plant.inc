// The plant of a closed loop on the device (ilqg_dev_plant_*, ilqg_batch_receding_plant).  Included by ilqg_kernels.hip
// inside its anonymous namespace, behind k_policy.inc (load_policy_step, policy_control); its parameter rows: ilqg_params.inc.
//
// k_plant: the plant of trajectory b advances `steps` steps from ITS OWN state xp[b] under the policy of slot b — what
// k_policy rolls out with alpha = 0: the current (x, u) where it lives (cur_x / cur_u) and the gains L of the packed
// records —
//     u_k = u_nom_k  [+ L_k (xp - x_nom_k)  if feedback, state by state in the template's order]
// then the step of the template (iLQG_func.tem:121-185): calcXVariableAux, clampU, calcXUVariableAux, ddpf, ddpL, with the
// multipliers and penalty weights slot b has now, and  xp <- x_next [+ w_k  if there is a disturbance table].  The control
// and the guarded step go through policy_control / run_step, which k_policy goes through: in the FMA-free builds a step
// here has the bits of the same step of ilqg_dev_policy_rollout from the same state.  k_plant<true> evaluates the callbacks under the PLANT's parameters: the context's fixed-size parameters with the
// mapped slots replaced by row b of `values` [B][W] (override_params with g = b; the n = 16 FMA-free builds read them from
// memory, ILQG_POLICY_PARAMS_IN_MEMORY).  k_plant<false> has no table argument and no code for one.
//
// Lanes.  One lane per trajectory.  In the lane mapping x_nom / u_nom are the tiled arrays (a wavefront reads 512 contiguous
// bytes per component) and the gains of 64 lanes sit in 64 packed records: that load scatters, one cache line or two per
// lane, as it does in k_policy with one start per trajectory.  `steps` is small, so as there the next step's nominal data
// are requested while a step computes.  In the wave mapping L is read where it is used.
//
// State that outlives the launch, all of it the context's: xp [B][NX] (trajectory-major: what the scatter of
// ilqg_dev_put_x0_device reads), failed [B] (0 until a step of the plant fails; a failed plant no longer advances — it stays
// at the last finite state it had — and its later log entries are unspecified), and the logs in the layout the host reads:
// lx [B][total][NX] the plant's state a control was applied at, lu [B][total][NU] the CLAMPED control, both at step
// at0 + k of `total`; lc [B][rounds] the sum of the round's running costs ct.c from 0.0 in step order; lp [B][rounds] the
// cost of the plan the round applied (what k_log_steps logs).  A step fails where forward_pass would return 0 (a guarded
// value NaN or Inf) or where the state behind the disturbance is not finite; a start that is not finite fails at once.
// NOTHING of the batch is written.

template <bool PLANT_PARAMS, class... Rows>
__global__ __launch_bounds__(ROLL_BLOCK) void k_plant(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int steps, int feedback,
                                                      double *__restrict__ xp, int *__restrict__ failed,
                                                      const double *__restrict__ dist, int at0, int total, int round, int rounds,
                                                      double *__restrict__ lx, double *__restrict__ lu, double *__restrict__ lc,
                                                      double *__restrict__ lp, Rows... rows) {
    // the pack: [the context's per-trajectory table, its map,] [the plants' table, its map] (RowPack)
    const int b = (int)(blockIdx.x * ROLL_BLOCK + threadIdx.x);
    if(b >= P.B) return;
    const int N = P.N;
    const bool use_K = (feedback != 0);
    lp[(size_t)b * rounds + round] = P.f[ILQG_F_COST][b];
    if(failed[b]) return;

    double xc[NX];
    bool finite = true;
#pragma unroll
    for(int i = 0; i < NX; i++) {
        xc[i] = xp[(size_t)b * NX + i];
        finite &= (__builtin_fabs(xc[i]) < __builtin_inf());
    }
    if(!finite) {
        failed[b] = 1;
        return;
    }

    ILQG_CALLBACKS(C, H);
    apply_rows<PLANT_PARAMS ? OWN_PLANT : OWN_NONE>(C_values, C_table, P, b, (size_t)b, 0, rows...);  // (the plant's row: one per trajectory)
    load_penalty_weights(C, P, b);
    el_t ct;
    multipliersEl_t mk;
    multipliersEl_t *const mp = HAS_MUL ? &mk : nullptr;
#if ILQG_DEV_EL
    ilqgdev::set_mode(ilqgdev::DISCARD);
    [[clang::always_inline]]  // (see k_rollout)
#endif
    init_running(&ct, &C.o1);

    NomPtrs q;
    q.x = cur_x(P, 0, b);
    q.u = cur_u(P, 0, b);
    q.l = nomp(P, 0, b) + NOM_L;
    q.K = nomp(P, 0, b) + NOM_K;
    const size_t xs = cur_xstride(P), us = cur_ustride(P);
    constexpr int ks = RN;
    size_t at = (size_t)b * (size_t)total + (size_t)at0;  // this plant's step in the logs and in the disturbance table

    double csum = 0.0;
    int okc = 1;
    NomStep cur = {};
    load_policy_step(cur, q, false, use_K);
    drain_memory_ops();
    for(int k = 0; k < steps; k++) {
        NomPtrs qn;
        qn.x = q.x + xs;
        qn.u = q.u + us;
        qn.l = q.l + ks;
        qn.K = q.K + ks;
        double xin[NX], uin[NU];
#pragma unroll
        for(int i = 0; i < NX; i++) xin[i] = xc[i];
        policy_control(uin, cur, q.K, xin, 0.0, false, use_K);

        // the next step's nominal data, in flight while the step computes (steps < N: step k + 1 <= N - 1 exists everywhere)
        load_policy_step(cur, qn, false, use_K);
        double w[NX];
        if(dist) {
#pragma unroll
            for(int i = 0; i < NX; i++) w[i] = dist[at * NX + i];
        }

        if(HAS_MUL) load_mul(P, k, b, mk);
        double xnext[NX];
        auto step = ILQG_FORWARD_STEP(false, ct, mp, k, N, C, xin, uin, xnext);
        const int r = run_step(H, okc, step);
        csum += ct.c;
#pragma unroll
        for(int i = 0; i < NX; i++) lx[at * NX + i] = ct.x[i];
#pragma unroll
        for(int i = 0; i < NU; i++) lu[at * NU + i] = ct.u[i];
        at++;
        if(dist) {
#pragma unroll
            for(int i = 0; i < NX; i++) xnext[i] = xnext[i] + w[i];
        }
        bool good = (okc != 0) && (r != 0) && (H.nonfinite == 0.0);
#pragma unroll
        for(int i = 0; i < NX; i++) good &= (__builtin_fabs(xnext[i]) < __builtin_inf());
        okc = good ? 1 : 0;
        if(good) {  // a failed plant stays where it is
#pragma unroll
            for(int i = 0; i < NX; i++) xc[i] = xnext[i];
        }
        q = qn;
    }
#pragma unroll
    for(int i = 0; i < NX; i++) xp[(size_t)b * NX + i] = xc[i];
    lc[(size_t)b * rounds + round] = csum;
    if(!okc) failed[b] = 1;
}
