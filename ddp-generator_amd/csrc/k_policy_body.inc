// The text of the policy roll-out kernels, ONCE (k_policy.inc includes it once per kernel; see there for what a roll-out is):
//     ILQG_POLICY_KERNEL = k_policy,       ILQG_POLICY_DRAWN = 0   no noise, or the caller's table `dist`
//     ILQG_POLICY_KERNEL = k_policy_drawn, ILQG_POLICY_DRAWN = 1   the rows drawn in registers from `spec` (k_noise.inc)
//     ILQG_POLICY_KERNEL = k_policy,       ILQG_POLICY_DRAWN = 2   either, chosen at run time: spec != null draws, else as 0
// They differ in the noise arguments, in what is prepared in front of the parameters and in the lines behind the step.
template <bool PER_ROLLOUT_PARAMS, class... Rows>
__global__ __launch_bounds__(ROLL_BLOCK) void ILQG_POLICY_KERNEL(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int R, const double *__restrict__ x0,
                                                       double alpha, int feedback, double *__restrict__ ocost, int *__restrict__ ook,
                                                       double *__restrict__ oxe, double *__restrict__ ox, double *__restrict__ ou,
#if ILQG_POLICY_DRAWN == 1
                                                       const NoiseSpec *__restrict__ spec, Rows... rows) {
#elif ILQG_POLICY_DRAWN == 2
                                                       const double *__restrict__ dist, int dist_shared, const NoiseSpec *__restrict__ spec,
                                                       Rows... rows) {
#else
                                                       const double *__restrict__ dist, int dist_shared, Rows... rows) {
#endif
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
#if ILQG_POLICY_DRAWN != 1
    size_t wat = (dist_shared ? g - (size_t)b * (size_t)R : g) * (size_t)N * NX;
    asm volatile("" : "+v"(wat));
#endif
#if ILQG_POLICY_DRAWN != 0
    // the drawn form's counter words r and t, HERE for the same reason: two vector registers across the roll-out.  The key
    // and sigma are read behind each step, through a pointer the compiler cannot see through: read in front of the loop they
    // would be 2 N_X + 2 scalar registers held across every step (NoiseSpec, k_noise.inc).
    unsigned noise_r = (unsigned)(g - (size_t)b * (size_t)R), noise_t = (ILQG_POLICY_DRAWN == 1 || spec) ? noise_trajectory(spec, b) : 0u;
    asm volatile("" : "+v"(noise_r), "+v"(noise_t));
#endif

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
#if ILQG_POLICY_DRAWN != 0
        // x_{k+1} <- x_next + w_k: the row is drawn HERE, behind the step (its normals are not live across it).  This add is compiled
        // with contraction off, the table form's below is not (it is k_policy's text as it was): if a problem's LAST operation on
        // x_next were a multiply, the table form could fuse it with its add and the two forms would differ in the last bit.  The
        // bit-for-bit identity drawn = table therefore rests on ddpf ending in an add (x + h f), as every generated pair's does;
        // tests/test_gpu_policy_drawn.py holds it on every build.
        if(ILQG_POLICY_DRAWN == 1 || spec) {
#pragma clang fp contract(off)
            const NoiseSpec *here = spec;
            asm volatile("" : "+s"(here));
            double w[NX];
            noise_row(w, here, (unsigned)k, noise_r, noise_t);
            bool good = true;
#pragma unroll
            for(int i = 0; i < NX; i++) {
                xnext[i] = xnext[i] + w[i];
                good &= (__builtin_fabs(xnext[i]) < __builtin_inf());
            }
            okc &= good ? 1 : 0;
        }
#endif
#if ILQG_POLICY_DRAWN == 2
        else
#endif
#if ILQG_POLICY_DRAWN != 1
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
#endif
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
