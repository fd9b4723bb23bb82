// forward_pass roll-outs shared by both mappings.  Included by ilqg_kernels.hip inside its anonymous namespace.

// ---------------------------------------------------------------------------
// forward_pass: one lane per (trajectory, step size)
// ---------------------------------------------------------------------------
enum { ROLL_INIT = 0, ROLL_SEARCH = 1, ROLL_WINNER = 2, ROLL_COST = 3, ROLL_SEARCH_LIST = 4, ROLL_SECOND = 5,
       ROLL_LIST_KEEP = 6 };  // (k_rollout_parts only: the second stage alone, rows = step sizes, kept in P.cand)
constexpr int CAND_W = NX + NU;  // doubles per step of a kept second-stage roll-out

// nominal data of one step (what forward_pass reads of the nominal trajectory, iLQG_func.tem:145-155)
struct NomStep {
    double x[NX], u[NU], l[NU];
    double K[WAVE_MAP ? 1 : NXU];  // wave mapping: L is too large to prefetch, it is streamed (below)
};

// pointers to the current step of one trajectory in X, U, l, L
struct NomPtrs {
    const double *x, *u, *l, *K;
};

// CS: distance between the components of x and u where they are read (1 in the records, XSI in X / U)
template <bool GAINS, int CS>
__device__ __forceinline__ void load_nominal(NomStep &s, const NomPtrs &q) {
#pragma unroll
    for(int i = 0; i < NX; i++) s.x[i] = q.x[i * CS];
#pragma unroll
    for(int i = 0; i < NU; i++) s.u[i] = q.u[i * CS];
    if(GAINS) {
#pragma unroll
        for(int i = 0; i < NU; i++) s.l[i] = q.l[i];
        if(!WAVE_MAP) {
#pragma unroll
            for(int i = 0; i < NXU; i++) s.K[i] = q.K[i];
        }
    }
}

// Three instantiations of the roll-out:
//   RK_GENERAL  u = u_nom + alpha*l + L (x - x_nom): ROLL_SEARCH, ROLL_SEARCH_LIST and ROLL_WINNER.  These differ
//               by the RUN-TIME argument `mode` only, on purpose: the search passes and the winner pass must
//               execute the same machine code so that the re-rolled winner reproduces the cost its selection
//               was based on, bit for bit.
//   RK_INIT     alpha = 0: u = u_nom, no gains read (initial roll-out, iLQG_mex.c:116), stored in place
//   RK_COST     cost of the stored trajectory (forward_pass with cost_only = 1, iLQG.c:338)
// Lanes:
//   ROLL_SEARCH       lane = (trajectory blockIdx.x*64+lane, step size a0 + blockIdx.y); only the cost is kept
//   ROLL_SEARCH_LIST  as ROLL_SEARCH for the trajectories listed in P.pending (second stage)
//   ROLL_WINNER       lane = trajectory, accepted step size, rolled out again and stored in place of the nominal
//                     trajectory: accepted = overwritten, no candidate buffer and no swap (iLQG.c:381-386)
//   ROLL_INIT / ROLL_COST  lane = trajectory
//   ROLL_SECOND       both at once, by blockIdx.y: 0 = ROLL_WINNER for the trajectories the first stage settled,
//                     1.. = ROLL_SEARCH_LIST for step size a0 + blockIdx.y - 1, each lane KEEPING its trajectory in
//                     P.cand.  The two are independent (different trajectories), and each is a latency-bound chain of
//                     N steps that leaves most of the chip idle: side by side they cost one chain instead of two, and
//                     the few trajectories the second stage settles are copied from P.cand (k_adopt) instead of a
//                     third chain.
// Keeping the candidates of the search instead of re-rolling the winner was measured and dropped: a whole-batch copy
// of X and U per step size costs more HBM write time than the winner pass, and candidates of the compacted second
// stage can only be written or copied back as scattered 8-byte pieces (DESIGN.md).
// The time step itself is straight-line code: the generated callbacks' NaN/Inf guards and the
// huge-argument case of sin/cos are hooks (see ilqg_hooks), tested once per step (run_step).
enum { RK_GENERAL = 0, RK_INIT = 1, RK_COST = 2 };

// Wavefronts per workgroup of the roll-outs.  One: in the wave mapping a roll-out wavefront fills the
// register file of its SIMD and the backward kernel's workgroup needs a whole CU, so four per workgroup (one CU
// instead of four blocked) was tried to let the roll-outs of one group of trajectories share the chip with the
// backward pass of another — 1.86 it/s (one group) and 1.92 (two groups, 8 hardware queues) against 1.98 as is:
// the backward kernel keeps the SIMDs it runs on busy, there is little idle issue time to give away.
constexpr int ROLL_WAVES = 1;
constexpr int ROLL_BLOCK = WAVE * ROLL_WAVES;
#if ILQG_DEV_EL
static_assert(ROLL_WAVES == ilqgdev::WAVES, "ilqgdev's ring is that of ONE wavefront per workgroup");
#endif

template <int KIND, class... Rows>
__global__ __launch_bounds__(ROLL_BLOCK) void k_rollout(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int mode, int a0, Rows... rows) {
    // Rows: empty — the kernel as it always was, under its old name — or the context's per-trajectory table and its map (RowPack)
    int b = blockIdx.x * ROLL_BLOCK + threadIdx.x;
    int ai = a0 + blockIdx.y;
    double *keep = nullptr;  // second stage: where this lane's trajectory is kept
    int second_row = -1;     //   and the row of the candidate buffer (its step size)
    if(mode == ROLL_SECOND) {
        if(blockIdx.y == 0) {
            mode = ROLL_WINNER;
        } else {
            mode = ROLL_SEARCH_LIST;
            ai = a0 + blockIdx.y - 1;
            second_row = blockIdx.y - 1;
        }
    }
    if(mode == ROLL_SEARCH_LIST) {
        // The list is short (the grid covers the worst case, most blocks return at once), and workgroups go to the CUs
        // round robin: with the entries in the same place of every row of the grid, the busy workgroups of ALL rows
        // landed on the same few CUs (measured, n = 16 problem, 2 676 entries: 1 / 2 / 4 / 7 rows 38 / 53 / 66 / 83 ms).
        // Each row starts its walk over the list somewhere else.
        const int nb = gridDim.x, rows = (int)gridDim.y - (second_row >= 0 ? 1 : 0);
        const int row = second_row >= 0 ? second_row : (int)blockIdx.y;
        const int first = (int)(((long long)row * nb) / rows);
        b = ((int)blockIdx.x + first) % nb * ROLL_BLOCK + threadIdx.x;
        if(b >= *P.n_pending) return;
        if(second_row >= 0) keep = P.cand + (size_t)second_row * (P.N + 1) * CAND_W * P.Bp + b;
        b = P.pending[b];
    }
    if(b >= P.B) return;
    const int N = P.N;
    double alpha = 0.0;
    if(mode == ROLL_SEARCH || mode == ROLL_SEARCH_LIST) {
        if(P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE) return;
        alpha = O.alpha[ai];
    } else if(mode == ROLL_WINNER) {
        if(P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE || !P.i[ILQG_I_ACCEPTED][b]) return;
        alpha = O.alpha[P.i[ILQG_I_ALPHA_IDX][b] - 1];
    } else if(mode == ROLL_COST) {
        if(!P.i[ILQG_I_RESWEEP][b]) return;  // set by k_update
    }
    constexpr bool cost_only = (KIND == RK_COST);
    constexpr bool gains = (KIND == RK_GENERAL);
    const bool store = (mode == ROLL_INIT || mode == ROLL_WINNER);
    const bool feedback = (alpha != 0.0);  // alpha == 0.0: u = u_nom without feedback (iLQG_func.tem:156-158)

    ILQG_CALLBACKS(C, H);
    apply_rows<OWN_NONE>(C_values, C_table, P, b, 0, 0, rows...);
    // penalty weights of this trajectory; the initial roll-out runs before the solver entry sets them, with the
    // zero-initialised option set of the MEX entry (iLQG_mex.c:23,116; iLQG.c:233-234)
    if(HAS_MUL && KIND == RK_INIT) set_penalty_weights(C, 0.0, 0.0);
    else load_penalty_weights(C, P, b);
    el_t ct;
    multipliersEl_t mk;
    multipliersEl_t *const mp = HAS_MUL ? &mk : nullptr;
#if ILQG_DEV_EL
    ilqgdev::set_mode(ilqgdev::DISCARD);  // (the constant DERIVATIVE entries init_running also assigns go nowhere)
    // (inline: its loop over n_hor = 1 elements then folds away.  Left a call, the loop's `t < end` on two pointers into this
    // lane's private memory is something the compiler has no instruction for — "Illegal instruction detected ...
    // V_CMP_NE_U32_e32 0, $src_private_base", ROCm 7.2's clang at -O3)
    [[clang::always_inline]]
#endif
    init_running(&ct, &C.o1);  // constant auxiliaries of this problem (iLQG_func.tem:312-347)

    // this trajectory's step 0 in every field; all of them advance by one step per iteration
    // The line search reads the packed records; the initial roll-out and the cost sweep read the current (x, u)
    // where every roll-out stores them (see cur_x).
    constexpr int CS = (KIND == RK_GENERAL) ? 1 : XSI;
    NomPtrs q;
    q.x = (KIND == RK_GENERAL) ? nomp(P, 0, b) + NOM_X : cur_x(P, 0, b);
    q.u = (KIND == RK_GENERAL) ? nomp(P, 0, b) + NOM_U : cur_u(P, 0, b);
    q.l = nomp(P, 0, b) + NOM_L;
    q.K = nomp(P, 0, b) + NOM_K;
    const size_t xs = (KIND == RK_GENERAL) ? (size_t)RN : cur_xstride(P), us = (KIND == RK_GENERAL) ? (size_t)RN : cur_ustride(P);
    constexpr int ks = RN;
    // a stored roll-out (initial, winner) replaces the current trajectory
    double *xo = cur_x(P, 0, b), *uo = cur_u(P, 0, b);
    const size_t xos = cur_xstride(P), uos = cur_ustride(P);
    double *ro = nomp(P, 0, b);  // initial roll-out: the record's copy as well

    double xc[NX];
#pragma unroll
    for(int i = 0; i < NX; i++) xc[i] = q.x[i * CS];  // x0 (iLQG_func.tem:141-142)
    double csum = 0.0;
    int okc = 1;
    NomStep cur;
    load_nominal<gains, CS>(cur, q);
    drain_memory_ops();
    for(int k = 0; k < N; k++) {
        NomPtrs qn;
        qn.x = q.x + xs;
        qn.u = q.u + us;
        qn.l = q.l + ks;
        qn.K = q.K + ks;
        // inputs of the step
        double xin[NX], uin[NU];
        if(cost_only) {
#pragma unroll
            for(int i = 0; i < NX; i++) xin[i] = cur.x[i];
#pragma unroll
            for(int i = 0; i < NU; i++) uin[i] = cur.u[i];
        } else {
#pragma unroll
            for(int i = 0; i < NX; i++) xin[i] = xc[i];
            if(gains) {
                // u = u_nom + alpha*l + L (x - x_nom), state by state (iLQG_func.tem:146-155)
                double uf[NU];
#pragma unroll
                for(int j = 0; j < NU; j++) uf[j] = cur.u[j] + cur.l[j] * alpha;
#pragma unroll
                for(int i = 0; i < NX; i++) {
                    const double dx = xin[i] - cur.x[i];
                    if(WAVE_MAP) {
                        const double *Kk = q.K + i * NU;
#pragma unroll
                        for(int j = 0; j < NU; j++) uf[j] += Kk[j] * dx;
                    } else {
#pragma unroll
                        for(int j = 0; j < NU; j++) uf[j] += cur.K[j + i * NU] * dx;
                    }
                }
#pragma unroll
                for(int j = 0; j < NU; j++) uin[j] = feedback ? uf[j] : cur.u[j];
            } else {
#pragma unroll
                for(int j = 0; j < NU; j++) uin[j] = cur.u[j];
            }
        }

        // The nominal data of this step have been consumed: the next step's are loaded into the same variables
        // right here and are in flight while the step computes (no second buffer, no hand-over copies).
        // (unconditionally: the records have a step N; the tiled U has not, its pointer stays on the last step)
        if(KIND != RK_GENERAL && k + 1 >= N) qn.u = q.u;
        load_nominal<gains, CS>(cur, qn);

        if(HAS_MUL) {
            if(KIND == RK_INIT) {  // init_opt -> init_multipliers (iLQG_func.tem:371-402), element by element
                C.o1.multipliers.t = &mk;
                init_multipliers_running(&C.o1);
                store_mul(P, k, b, mk);
            } else {
                load_mul(P, k, b, mk);
            }
        }
        // the step (iLQG_func.tem:160-176)
        double xnext[NX];
        auto step = ILQG_FORWARD_STEP(cost_only, ct, mp, k, N, C, xin, uin, xnext);
        const int r = run_step(H, okc, step);
        okc &= r;
        csum += ct.c;
        // The step's results are stored right away, i.e. BEHIND the prefetch of the next step in issue order: the
        // memory counter retires in issue order, so the wait for the prefetched values at the end of this
        // iteration (vmcnt = number of younger operations) leaves these stores in flight.
        if(store) {
#pragma unroll
            for(int i = 0; i < NX; i++) xo[i * XSI] = ct.x[i];
#pragma unroll
            for(int i = 0; i < NU; i++) uo[i * XSI] = ct.u[i];
            if(KIND == RK_INIT && !WAVE_MAP) {
#pragma unroll
                for(int i = 0; i < NX; i++) ro[NOM_X + i] = ct.x[i];
#pragma unroll
                for(int i = 0; i < NU; i++) ro[NOM_U + i] = ct.u[i];
            }
        } else if(KIND == RK_GENERAL && keep) {
#pragma unroll
            for(int i = 0; i < NX; i++) keep[(size_t)i * P.Bp] = ct.x[i];
#pragma unroll
            for(int i = 0; i < NU; i++) keep[(size_t)(NX + i) * P.Bp] = ct.u[i];
            keep += (size_t)CAND_W * P.Bp;
        }
        if(!cost_only) {
#pragma unroll
            for(int i = 0; i < NX; i++) xc[i] = xnext[i];
        }
        q = qn;
        xo += xos;
        uo += uos;
        ro += RN;
    }
    // final cost (iLQG_func.tem:179-182); q.x now points at step N
    {
        trajFin_t cf;
        multipliersFin_t mf;
        if(HAS_MUL) {
            if(KIND == RK_INIT) {
                init_multipliers_final(&C.o);
                mf = C.o.multipliers.f;
                store_mul_fin(P, b, mf);
            } else {
                load_mul_fin(P, b, mf);
            }
        }
        init_final(&cf, &C.o);
        double xin[NX];
#pragma unroll
        for(int i = 0; i < NX; i++) xin[i] = cost_only ? q.x[i * CS] : xc[i];
        auto fin = [&]() {
#pragma unroll
            for(int i = 0; i < NX; i++) cf.x[i] = xin[i];
            int r = calcFVariableAux(&cf, HAS_MUL ? &mf : nullptr, &C.o);
            r &= ddpF(&cf, &C.o);
            return r;
        };
        const int r = run_step(H, okc, fin);
        okc &= r;
        csum += cf.c;
        if(store) {
#pragma unroll
            for(int i = 0; i < NX; i++) xo[i * XSI] = cf.x[i];  // xo points at step N now
            if(KIND == RK_INIT && !WAVE_MAP) {
#pragma unroll
                for(int i = 0; i < NX; i++) ro[NOM_X + i] = cf.x[i];
            }
        } else if(KIND == RK_GENERAL && keep) {
#pragma unroll
            for(int i = 0; i < NX; i++) keep[(size_t)i * P.Bp] = cf.x[i];
        }
    }
    // forward_pass returns 0 as soon as a guarded value is NaN or Inf (genenerator_main.mac:193-198)
    const int ok = (okc && H.nonfinite == 0.0) ? 1 : 0;

    if(mode == ROLL_SEARCH || mode == ROLL_SEARCH_LIST) {
        P.f[ILQG_F_ALPHA_COST][tile_ix(ILQG_MAX_ALPHA, ai, b)] = csum;
        P.i[ILQG_I_ALPHA_OK][(size_t)ai * P.Bp + b] = ok;
    } else if(mode == ROLL_WINNER) {
        P.f[ILQG_F_NEW_COST][b] = csum;
    } else if(mode == ROLL_COST) {
        P.f[ILQG_F_COST][b] = csum;
    } else {
        P.f[ILQG_F_COST][b] = csum;
        if(!ok) P.i[ILQG_I_STATUS][b] = ILQG_ST_INIT_FAILED;
    }
}
