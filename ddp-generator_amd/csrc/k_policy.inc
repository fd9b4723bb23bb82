// Roll-outs of every plan's feedback policy from starts of the caller (ilqg_dev_policy_rollout).  Included by
// ilqg_kernels.hip inside its anonymous namespace, behind k_rollout.inc (NomStep, NomPtrs, ROLL_BLOCK).
//
// k_policy: forward_pass (iLQG_func.tem:121-185) with o->x0 = the caller's start, the nominal = the POLICY of slot b —
// what k_head hands out: the current (x, u) where it lives (cur_x / cur_u: the tiled X / U, a kept roll-out plane of the
// line search, the records in the wave mapping) and the gains l, L of the packed records — the multipliers and penalty
// weights slot b has now, the per-time-step parameters as they stand, and
//     u_k = u_nom_k  [+ alpha l_k  if alpha != 0]  [+ L_k (x_k - x_nom_k)  if feedback, state by state in the template's order]
// then the step of the template: calcXVariableAux, clampU, calcXUVariableAux, ddpf, ddpL; the final step calcFVariableAux,
// ddpF.  Each is evaluated through run_step, as in k_rollout: the huge-argument second pass of sin / cos or, in builds with
// wave-uniform guards, run_guarded.  The control law is policy_control (below).  NOTHING of the batch is written: no field,
// scalar, status, location index or multiplier, and no trajectory moves home.
//
// Lanes.  One lane per roll-out, roll-out g = b * R + r with r fastest: R consecutive lanes share slot b and so every
// address of the nominal data.  A load instruction of a wavefront touches the data of at most ceil(64 / R) + 1 slots
// (lanes with equal addresses are served by one request), for R >= 64 of one or two, for R a multiple of 64 of exactly one.
// The next step's nominal data are requested while the step computes (k_rollout's scheme: loaded into the variables the
// step has just consumed); in the wave mapping L is too large to hold a step ahead and is read where it is used, as
// k_rollout does.  What alpha / feedback do not need is not loaded (l for alpha == 0; x_nom and L without feedback):
// both are kernel arguments, the branches are scalar ones.
//
// Outputs, all optional (null = not wanted): cost [B][R], ok [B][R] (forward_pass's return value: 0 as soon as a guarded
// value is NaN or Inf; the other outputs of such a roll-out are unspecified), x_end [B][R][NX], and the whole roll-out
// x [B][R][N+1][NX], u [B][R][N][NU] (u = the CLAMPED control that was applied).  x / u are trajectory-major per
// roll-out, so a lane's stores of a step are scattered 8-byte pieces, 64 cache lines per store instruction: accepted,
// because they are optional — the costs-only call does not pay for them (one wave-uniform branch per step, no store).
// A roll-out whose start is not finite ends at once with ok = 0.  All indices over B * R are size_t.
//
// Process noise (dist != null, a run-time argument as in k_plant: a null pointer is a wave-uniform branch and the call is
// the call without a table).  Behind every step k = 0 .. N-1 the roll-out's state is pushed,
//     x_{k+1} <- x_next + w[g][k]      (dist [B][R][N][NX]; with dist_shared != 0: w[r][k], dist [R][N][NX])
// the rule of k_plant: the control of step k + 1 is computed at the disturbed state, row N - 1 moves the state the final
// cost is evaluated at (x_end, x[N]).  ok = 0 as soon as a disturbed state is not finite, the one behind row N - 1
// included; such a lane stays out of the later guarded steps as one whose guard failed does.  A lane's row is NX doubles
// from its own 8-byte-aligned place, read right before the add: requested ahead of the step, as k_plant does with its
// one lane per trajectory, the row lives across the step and costs its registers (profiles/r17_policy_noise.txt).
__device__ __forceinline__ void load_policy_step(NomStep &s, const NomPtrs &q, bool use_l, bool use_K) {
#pragma unroll
    for(int i = 0; i < NU; i++) s.u[i] = q.u[i * XSI];
    if(use_l) {
#pragma unroll
        for(int i = 0; i < NU; i++) s.l[i] = q.l[i];
    }
    if(use_K) {
#pragma unroll
        for(int i = 0; i < NX; i++) s.x[i] = q.x[i * XSI];
        if(!WAVE_MAP) {
#pragma unroll
            for(int i = 0; i < NXU; i++) s.K[i] = q.K[i];
        }
    }
}

// The control law of a policy at state x (iLQG_func.tem:146-155), for k_policy and k_plant (alpha = 0, use_l = false):
//     u = u_nom  [+ alpha l  if use_l]  [+ L (x - x_nom)  if use_K, state by state in the template's order]
// K_here: L of this step where it is read in the wave mapping (too large to hold a step ahead); the lane mapping has it in
// cur.  k_rollout and the fused search keep their own form (uf, selected on `feedback`): other arithmetic, and hot.
__device__ __forceinline__ void policy_control(double (&uin)[NU], const NomStep &cur, const double *K_here, const double (&x)[NX], double alpha,
                                               bool use_l, bool use_K) {
#pragma unroll
    for(int j = 0; j < NU; j++) uin[j] = cur.u[j];
    if(use_l) {
#pragma unroll
        for(int j = 0; j < NU; j++) uin[j] = cur.u[j] + cur.l[j] * alpha;
    }
    if(use_K) {
#pragma unroll
        for(int i = 0; i < NX; i++) {
            const double dx = x[i] - cur.x[i];
            if(WAVE_MAP) {
                const double *Kk = K_here + i * NU;
#pragma unroll
                for(int j = 0; j < NU; j++) uin[j] += Kk[j] * dx;
            } else {
#pragma unroll
                for(int j = 0; j < NU; j++) uin[j] += cur.K[j + i * NU] * dx;
            }
        }
    }
}

template <bool PER_ROLLOUT_PARAMS, class... Rows>
__global__ __launch_bounds__(ROLL_BLOCK) void k_policy(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int R, const double *__restrict__ x0,
                                                       double alpha, int feedback, double *__restrict__ ocost, int *__restrict__ ook,
                                                       double *__restrict__ oxe, double *__restrict__ ox, double *__restrict__ ou,
                                                       const double *__restrict__ dist, int dist_shared, Rows... rows) {
    // the pack: [the context's per-trajectory table, its map,] [values, shared, map of the roll-outs' own rows] (RowPack)
    const size_t g = (size_t)blockIdx.x * ROLL_BLOCK + threadIdx.x;
    if(g >= (size_t)P.B * (size_t)R) return;
    const int b = (int)(g / (size_t)R);
    const int N = P.N;
    const bool use_l = (alpha != 0.0), use_K = (feedback != 0);

    double xc[NX];
    bool finite = true;
#pragma unroll
    for(int i = 0; i < NX; i++) {
        xc[i] = x0[g * NX + i];  // o->x0 (iLQG_func.tem:141-142)
        finite &= (__builtin_fabs(xc[i]) < __builtin_inf());
    }
    if(!finite) {
        if(ook) ook[g] = 0;
        if(ocost) ocost[g] = __builtin_nan("");
        return;
    }

    // this roll-out's row of the disturbance table at step k: ((dist_shared ? r : g) * N + k) * NX, moved on step by step.
    // Computed HERE, in front of the parameters: behind them the scalar registers are the parameters' (k_policy<true> of
    // synth16p, the n = 16 pair with stored tensors, has none left for dist_shared: its library then does not compile).
    size_t wat = (dist_shared ? g - (size_t)b * (size_t)R : g) * (size_t)N * NX;
    asm volatile("" : "+v"(wat));

    ILQG_CALLBACKS(C, H);
    apply_rows<PER_ROLLOUT_PARAMS ? OWN_ROLLOUT : OWN_NONE>(C_values, C_table, P, b, g, (int)(g - (size_t)b * (size_t)R), rows...);
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
    size_t xat = g * (size_t)(N + 1) * NX, uat = g * (size_t)N * NU;  // this roll-out's step in x / u

    double csum = 0.0;
    int okc = 1;
    NomStep cur = {};
    load_policy_step(cur, q, use_l, use_K);
    drain_memory_ops();
    for(int k = 0; k < N; k++) {
        NomPtrs qn;
        qn.x = q.x + xs;
        qn.u = q.u + us;
        qn.l = q.l + ks;
        qn.K = q.K + ks;
        double xin[NX], uin[NU];
#pragma unroll
        for(int i = 0; i < NX; i++) xin[i] = xc[i];
        policy_control(uin, cur, q.K, xin, alpha, use_l, use_K);

        // the next step's nominal data, in flight while the step computes (the records have a step N; the tiled U has not)
        if(k + 1 >= N) qn.u = q.u;
        load_policy_step(cur, qn, use_l, use_K);

        if(HAS_MUL) load_mul(P, k, b, mk);
        double xnext[NX];
        auto step = ILQG_FORWARD_STEP(false, ct, mp, k, N, C, xin, uin, xnext);
        const int r = run_step(H, okc, step);
        okc &= r;
        csum += ct.c;
        if(ox) {
#pragma unroll
            for(int i = 0; i < NX; i++) ox[xat + i] = ct.x[i];
            xat += NX;
        }
        if(ou) {
#pragma unroll
            for(int i = 0; i < NU; i++) ou[uat + i] = ct.u[i];
            uat += NU;
        }
        if(dist) {  // x_{k+1} <- x_next + w_k: the row is read HERE, behind the step (held across it, it costs the step's registers)
            bool good = true;
#pragma unroll
            for(int i = 0; i < NX; i++) {
                xnext[i] = xnext[i] + dist[wat + i];
                good &= (__builtin_fabs(xnext[i]) < __builtin_inf());
            }
            wat += NX;
            okc &= good ? 1 : 0;
        }
#pragma unroll
        for(int i = 0; i < NX; i++) xc[i] = xnext[i];
        q = qn;
    }
    {
        trajFin_t cf;
        multipliersFin_t mf;
        if(HAS_MUL) load_mul_fin(P, b, mf);
        init_final(&cf, &C.o);
        auto fin = [&]() {
#pragma unroll
            for(int i = 0; i < NX; i++) cf.x[i] = xc[i];
            int r = calcFVariableAux(&cf, HAS_MUL ? &mf : nullptr, &C.o);
            r &= ddpF(&cf, &C.o);
            return r;
        };
        const int r = run_step(H, okc, fin);
        okc &= r;
        csum += cf.c;
        if(ox) {
#pragma unroll
            for(int i = 0; i < NX; i++) ox[xat + i] = cf.x[i];
        }
        if(oxe) {
#pragma unroll
            for(int i = 0; i < NX; i++) oxe[g * NX + i] = cf.x[i];
        }
    }
    if(ocost) ocost[g] = csum;
    if(ook) ook[g] = (okc && H.nonfinite == 0.0) ? 1 : 0;
}
