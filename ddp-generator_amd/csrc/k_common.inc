// Selection, adoption, update, multiplier and unit-test kernels of both mappings.  Included by ilqg_kernels.hip inside
// its anonymous namespace.

// line_search.c:37-75: the FIRST step size (lowest index) whose forward pass was finite and
// whose z = dcost/expected exceeds zMin wins.  The scan over the step sizes can be cut in two
// stages [0,a1) and [a1,n_alpha): a trajectory that finds no acceptable step size in the first
// stage is appended to P.pending and only those are rolled out for the remaining step sizes.
// The scan state (last cnew / dcost / expected) is carried between the stages, so the result
// is exactly that of one scan over all step sizes.
//   from_list = 0: lane = trajectory, scans [a0,a1); from_list = 1: lane = entry of P.pending
__global__ void k_select(DevPtrs P, ilqg_dev_opts_t O, int a0, int a1, int from_list) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if(from_list) {
        if(b >= *P.n_pending) return;
        b = P.pending[b];
    }
    if(b >= P.B || P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE) return;
    const size_t Bp = P.Bp;
    const double cost = P.f[ILQG_F_COST][b], dV0 = P.f[ILQG_F_DV0][b], dV1 = P.f[ILQG_F_DV1][b];
    double cnew = (a0 > 0) ? P.f[ILQG_F_NEW_COST][b] : 0.0;
    double dcost = P.f[ILQG_F_DCOST][b], expected = P.f[ILQG_F_EXPECTED][b];
    int i, ok = 0;
    for(i = a0; i < a1; i++) {
        const double a = O.alpha[i];
        ok = P.i[ILQG_I_ALPHA_OK][(size_t)i * Bp + b];
        cnew = P.f[ILQG_F_ALPHA_COST][tile_ix(ILQG_MAX_ALPHA, i, b)];
        if(!ok) continue;
        dcost = cost - cnew;
        expected = expected_reduction(a, dV0, dV1);
        if(reduction_ratio(dcost, expected) > O.zMin) break;
        ok = 0;
    }
    // To the second stage: one atomicAdd per wavefront, its trajectories in order behind each other (the entries of
    // one wavefront are trajectories of one 64-trajectory tile: what k_adopt copies for them lands in the same rows of
    // X and U).  No measurable gain over one atomicAdd per trajectory; kept for the 64x fewer atomics.
    if(!ok && a1 < O.n_alpha) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(true);  // the lanes in here
        const int rank = __builtin_popcountll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
        int base = 0;
        if(rank == 0) base = atomicAdd(P.n_pending_next, __builtin_popcountll(m));
        base = __builtin_amdgcn_readfirstlane(base);  // the first lane in here is the one of rank 0
        P.pending[base + rank] = b;
    }
    P.i[ILQG_I_ALPHA_IDX][b] = i + 1;
    P.i[ILQG_I_ACCEPTED][b] = ok;
    P.f[ILQG_F_NEW_COST][b] = cnew;
    P.f[ILQG_F_DCOST][b] = dcost;
    P.f[ILQG_F_EXPECTED][b] = expected;
}

// After the second stage's selection: the trajectory of the accepted step size, kept by the lane that rolled it out
// (ROLL_SECOND), becomes the current one.  One thread per (entry of P.pending, step).  n2 = step sizes of the stage,
// a0 = its first.
__global__ void k_adopt(DevPtrs P, int a0, int n2) {
    const size_t n = (size_t)*P.n_pending, total = n * (P.N + 1), stride = (size_t)gridDim.x * blockDim.x;
    // a fixed grid walks over (step, entry), entry fastest: consecutive threads read consecutive entries of one row
    for(size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += stride) {
        const int e = (int)(w % n), k = (int)(w / n);
        const int b = P.pending[e];
        if(P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE || !P.i[ILQG_I_ACCEPTED][b]) continue;
        const int a = P.i[ILQG_I_ALPHA_IDX][b] - 1 - a0;
        const double *src = P.cand + ((size_t)a * (P.N + 1) + k) * CAND_W * P.Bp + e;
        double *xo = cur_x(P, k, b);
#pragma unroll
        for(int i = 0; i < NX; i++) xo[i * XSI] = src[(size_t)i * P.Bp];
        if(k < P.N) {
            double *uo = cur_u(P, k, b);
#pragma unroll
            for(int i = 0; i < NU; i++) uo[i * XSI] = src[(size_t)(NX + i) * P.Bp];
        }
    }
}

// Wave mapping, ls_keep = 2: the roll-outs the first stage accepted, kept by trajectory in P.cand1, become the current
// trajectory (the records' x and u).  Replaces the winner pass: a copy at the speed of the memory system instead of
// 16 384 chains of N steps beside the second stage's.  One wavefront per (step, tile of 64 trajectories): it reads the
// step's NX + NU components lane = trajectory (512 contiguous bytes per load), turns the tile round in LDS and writes
// lane = (trajectory, component): each trajectory's x | u of the step is one run of 192 contiguous bytes in its record
// (with one thread per (step, trajectory) writing its own run: 64 cache lines per store instruction, 5.1 ms for config 5).
__global__ __launch_bounds__(256) void k_adopt_first(DevPtrs P, int s1) {
    constexpr int TW = CAND_W + 1;  // (padded rows: the lanes' stores fall on different banks)
    __shared__ double tile[4][WAVE][TW];
    __shared__ int take[4][WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tiles = P.Bp / WAVE;
    const size_t total = (size_t)(P.N + 1) * tiles, stride = (size_t)gridDim.x * 4;
    for(size_t w = (size_t)blockIdx.x * 4 + wave; w < total; w += stride) {
        const int k = (int)(w / tiles), b0 = (int)(w % tiles) * WAVE, b = b0 + lane;
        int a = -1;
        if(b < P.B && P.i[ILQG_I_STATUS][b] == ILQG_ST_ACTIVE && P.i[ILQG_I_ACCEPTED][b]) a = P.i[ILQG_I_ALPHA_IDX][b] - 1;
        if(a >= s1) a = -1;
        if(__builtin_amdgcn_ballot_w64(a >= 0) == 0ull) continue;
        take[wave][lane] = a >= 0;
        if(a >= 0) {
            const double *src = P.cand1 + ((size_t)a * (P.N + 1) + k) * CAND_W * P.Bp + b;
#pragma unroll
            for(int i = 0; i < CAND_W; i++) tile[wave][lane][i] = src[(size_t)i * P.Bp];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int W = (k < P.N) ? CAND_W : NX;  // (the last step has a state only)
        for(int e = lane; e < WAVE * CAND_W; e += WAVE) {
            const int t = e / CAND_W, c = e - t * CAND_W;
            if(c < W && take[wave][t]) (c < NX ? cur_x(P, k, b0 + t) + c * XSI : cur_u(P, k, b0 + t) + (c - NX) * XSI)[0] = tile[wave][t][c];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// iLQG.c:311-361 and the loop bookkeeping of iLQG.c:239,365-378
// commit_s1 >= 0: also what k_commit does (the search of this iteration left the change of location to this kernel);
// reset_pending: the counter of the pending list is cleared for the next search (nothing reads it any more)
__global__ void k_update(DevPtrs P, ilqg_dev_opts_t O, int commit_s1, int commit_set, int reset_pending) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if(b == 0 && reset_pending) *P.n_pending = 0;
    if(b >= P.B) return;
    if(!WAVE_MAP && commit_s1 >= 0 && P.i[ILQG_I_STATUS][b] == ILQG_ST_ACTIVE) {
        const int a = P.i[ILQG_I_ALPHA_IDX][b] - 1;
        P.i[ILQG_I_LOC][b] = (P.i[ILQG_I_ACCEPTED][b] && a < commit_s1) ? 1 + commit_set * P.plane_n + a : 0;
    }
    if(P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE) {  // finished, possibly in this iteration's backward pass
        P.i[ILQG_I_RESWEEP][b] = 0;
        return;
    }
    double lambda = P.f[ILQG_F_LAMBDA][b], dlambda = P.f[ILQG_F_DLAMBDA][b];
    int iter = P.i[ILQG_I_ITER][b];
    int status = ILQG_ST_ACTIVE;
    int resweep = 0;
    if(P.i[ILQG_I_ACCEPTED][b]) {
        lambda_down(O.lambdaFactor, O.lambdaMin, &lambda, &dlambda);
        P.f[ILQG_F_COST][b] = P.f[ILQG_F_NEW_COST][b];
        P.i[ILQG_I_NEED_DERIVS][b] = 1;
        if(P.f[ILQG_F_DCOST][b] < O.tolFun) status = ILQG_ST_CONVERGED_FUN;
        else resweep = 2;  // update_multipliers + cost-only sweep (iLQG.c:337-338)
    } else {
        if(HAS_MUL && O.w_pen_fact2 > 1.0) {  // iLQG.c:345-349, before the lambdaMax exit
            const double wl = P.f[ILQG_F_WPEN_L][b] * O.w_pen_fact2, wf = P.f[ILQG_F_WPEN_F][b] * O.w_pen_fact2;
            P.f[ILQG_F_WPEN_L][b] = (O.w_pen_max_l < wl) ? O.w_pen_max_l : wl;
            P.f[ILQG_F_WPEN_F][b] = (O.w_pen_max_f < wf) ? O.w_pen_max_f : wf;
            resweep = 1;
        }
        lambda_up(O.lambdaFactor, O.lambdaMin, &lambda, &dlambda);
        if(lambda > O.lambdaMax) status = ILQG_ST_LAMBDA_MAX;
    }
    if(status == ILQG_ST_ACTIVE) {
        iter++;
        if(iter >= O.max_iter) status = ILQG_ST_MAX_ITER;
    }
    P.f[ILQG_F_LAMBDA][b] = lambda;
    P.f[ILQG_F_DLAMBDA][b] = dlambda;
    P.i[ILQG_I_ITER][b] = iter;
    P.i[ILQG_I_STATUS][b] = status;
    // without multipliers the sweep reproduces the cost bit for bit: only where the solve goes on (option resweep)
    if(!HAS_MUL && status != ILQG_ST_ACTIVE) resweep = 0;
    P.i[ILQG_I_RESWEEP][b] = resweep;
}

// The iteration history of a context (ilqg_dev_set_history): per trajectory the count n of line searches recorded so far and
// the first `cap` entries, laid out [field][cap][Bp] behind each other — the doubles of ILQG_H_* in d, in i the counts [Bp]
// and behind them the ints of ILQG_HI_*: lane = trajectory, so every store of a wavefront is one contiguous run.
struct History {
    double *d;
    int *i;
    int cap, Bp;
    __host__ __device__ size_t at(int field, int entry, int b) const { return ((size_t)field * cap + entry) * Bp + b; }
    __host__ __device__ int *ints() const { return i + Bp; }  // (behind the counts)
};
constexpr int HIST_DOUBLES = HAS_MUL ? ILQG_H_COUNT : ILQG_H_WPEN_L;  // the penalty weights only where the problem has multipliers

// (Both history kernels are templates for one reason: a template is instantiated, and so emitted into the code object, where
// it is first USED, and the shim first uses these two (launch_history, launch_move_history) behind every kernel of the solver,
// in front of the box QP's unit-test kernels only.  A kernel emitted in the middle moves everything behind it, and with it
// the pc-relative offsets in every kernel that calls an out-of-line function such as ilqg_sincos_slow: each of those would
// read as changed in tools/kernel_resources.py --digest.)

// In front of k_update, on its stream: one entry for every trajectory whose line search has just run (ILQG_ST_ACTIVE here:
// what left in this iteration's backward pass logs nothing, as in the reference) — what the per-trajectory fields hold at the
// return of line_search(), i.e. line_search.c:70-72's log_linesearch / log_z / log_cost and the values iLQG.c:314,353 print,
// before k_update moves lambda, the cost and the iteration count.  Position n[b]; beyond cap dropped while n counts on.
template <class Hist = History>
__global__ void k_history(DevPtrs P, Hist H) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if(b >= P.B || P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE) return;
    const int n = H.i[b];
    H.i[b] = n + 1;
    if(n >= H.cap) return;
    H.d[H.at(ILQG_H_COST, n, b)] = P.f[ILQG_F_COST][b];
    H.d[H.at(ILQG_H_NEW_COST, n, b)] = P.f[ILQG_F_NEW_COST][b];
    H.d[H.at(ILQG_H_Z, n, b)] = reduction_ratio(P.f[ILQG_F_DCOST][b], P.f[ILQG_F_EXPECTED][b]);
    H.d[H.at(ILQG_H_LAMBDA, n, b)] = P.f[ILQG_F_LAMBDA][b];
    H.d[H.at(ILQG_H_GNORM, n, b)] = P.f[ILQG_F_GNORM][b];
    H.d[H.at(ILQG_H_DV0, n, b)] = P.f[ILQG_F_DV0][b];
    H.d[H.at(ILQG_H_DV1, n, b)] = P.f[ILQG_F_DV1][b];
    if(HAS_MUL) {
        H.d[H.at(ILQG_H_WPEN_L, n, b)] = P.f[ILQG_F_WPEN_L][b];
        H.d[H.at(ILQG_H_WPEN_F, n, b)] = P.f[ILQG_F_WPEN_F][b];
    }
    int *const hi = H.ints();
    hi[H.at(ILQG_HI_ALPHA_IDX, n, b)] = P.i[ILQG_I_ALPHA_IDX][b];
    hi[H.at(ILQG_HI_BP_CALLS, n, b)] = P.i[ILQG_I_BP_CALLS][b];
    hi[H.at(ILQG_HI_ITER, n, b)] = P.i[ILQG_I_ITER][b];
}

// update_multipliers (iLQG_func.tem:419-521) for the trajectories k_update flagged, or with init != 0 at the solver
// entry (iLQG.c:236) for all live ones.  The generated functions walk o->nominal->t and o->multipliers.t over
// o->n_hor elements; here they see a one-element view per time step (the constraint values they read are the
// auxiliaries of that element, recomputed from the stored (x, u) with the multipliers and weights of the roll-out
// that stored them).  What they do across steps is restated around the calls: one raise of w_pen_l after the
// walk if any step asked for it; with init != 0 the running part returns inside its loop after the first element
// (iLQG_func.tem:447), so only step 0 is visited.
#if ILQG_WAVE_MAP  // (this mapping has no per-trajectory parameters: the kernel itself)
__global__ __launch_bounds__(WAVE) void k_multipliers(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int init) {
#else
// (lane mapping: the lane's work, for k_multipliers and for k_multipliers_rows below — Rows is empty or the context's
// per-trajectory table and its map)
template <class... Rows>
__device__ __forceinline__ void multipliers_lane(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int init, Rows... rows) {
#endif
    const int b = blockIdx.x * WAVE + threadIdx.x;
    if(b >= P.B) return;
    if(init) {
        if(P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE && P.i[ILQG_I_STATUS][b] != ILQG_ST_MAX_ITER) return;
    } else if(P.i[ILQG_I_RESWEEP][b] != 2) {
        return;
    }
    const int N = P.N;
    ILQG_CALLBACKS(C, H);
#if !ILQG_WAVE_MAP
    apply_rows<OWN_NONE>(C_values, C_table, P, b, 0, 0, rows...);
#endif
    load_penalty_weights(C, P, b);
    const double wl = C.o.w_pen_l;
    eltraj_t view;
    el_t ct;
    multipliersEl_t mk;
#if ILQG_DEV_EL
    ilqgdev::set_mode(ilqgdev::DISCARD);
    [[clang::always_inline]]  // (see k_rollout)
#endif
    init_running(&ct, &C.o1);
    view.t = &ct;
    C.o.nominal = C.o1.nominal = &view;
    C.o1.multipliers.t = &mk;
    bool raise = false;
    if(ME > 0) {
        const int steps = init ? 1 : N;
        for(int k = 0; k < steps; k++) {
            const double *xs = cur_x(P, k, b), *us = cur_u(P, k, b);
            load_mul(P, k, b, mk);
            H.huge = 0.0;
            auto aux = [&]() {
#pragma unroll
                for(int i = 0; i < NX; i++) ct.x[i] = xs[i * XSI];
#pragma unroll
                for(int i = 0; i < NU; i++) ct.u[i] = us[i * XSI];
                calcXVariableAux(&ct, &mk, k, &C.o);
                calcXUVariableAux(&ct, &mk, k, &C.o);
            };
            aux();
            if(H.huge != 0.0) {
                H.slow = 1.0;
                aux();
                H.slow = 0.0;
            }
            C.o1.w_pen_l = wl;
            update_multipliers_running(&C.o1, init);
            raise |= (C.o1.w_pen_l != wl);
            store_mul(P, k, b, mk);
        }
    }
    if(MF > 0) {
        const double *xs = cur_x(P, N, b);
        load_mul_fin(P, b, C.o.multipliers.f);
        init_final(&view.f, &C.o);
        H.huge = 0.0;
        auto aux = [&]() {
#pragma unroll
            for(int i = 0; i < NX; i++) view.f.x[i] = xs[i * XSI];
            calcFVariableAux(&view.f, &C.o.multipliers.f, &C.o);
        };
        aux();
        if(H.huge != 0.0) {
            H.slow = 1.0;
            aux();
            H.slow = 0.0;
        }
        update_multipliers_final(&C.o, init);
        store_mul_fin(P, b, C.o.multipliers.f);
        P.f[ILQG_F_WPEN_F][b] = C.o.w_pen_f;
    }
    double wl_new = wl;
    if(raise) {
        const double w = wl * O.w_pen_fact1;
        wl_new = (O.w_pen_max_l < w) ? O.w_pen_max_l : w;
        P.f[ILQG_F_WPEN_L][b] = wl_new;
    }
    // the derivatives evaluated next (this trajectory was accepted, or the solve starts) see these weights
    P.f[ILQG_F_WPEN_L_DER][b] = wl_new;
    P.f[ILQG_F_WPEN_F_DER][b] = (MF > 0) ? C.o.w_pen_f : P.f[ILQG_F_WPEN_F][b];
}
#if !ILQG_WAVE_MAP
__global__ __launch_bounds__(WAVE) void k_multipliers(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int init) { multipliers_lane(P, O, A, init); }
// ... under per-trajectory parameters (k_multipliers keeps its name: it is no template)
template <class... Rows>
__global__ __launch_bounds__(WAVE) void k_multipliers_rows(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int init, Rows... rows) {
    multipliers_lane(P, O, A, init, rows...);
}
#endif

// solver entry state (iLQG.c:226-237)
__global__ void k_reset(DevPtrs P, ilqg_dev_opts_t O) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if(b >= P.Bp) return;
    const bool live = b < P.B && P.i[ILQG_I_STATUS][b] != ILQG_ST_INIT_FAILED;
    P.f[ILQG_F_LAMBDA][b] = O.lambdaInit;
    P.f[ILQG_F_DLAMBDA][b] = O.dlambdaInit;
    P.i[ILQG_I_ITER][b] = 0;
    P.i[ILQG_I_NEED_DERIVS][b] = 1;
    P.i[ILQG_I_ACCEPTED][b] = 0;
    P.i[ILQG_I_BP_CALLS][b] = 0;
    P.derivs_failed[b] = 0;
    P.i[ILQG_I_RESWEEP][b] = 0;
    P.f[ILQG_F_WPEN_L][b] = O.w_pen_init_l;
    P.f[ILQG_F_WPEN_F][b] = O.w_pen_init_f;
    P.f[ILQG_F_WPEN_L_DER][b] = O.w_pen_init_l;
    P.f[ILQG_F_WPEN_F_DER][b] = O.w_pen_init_f;
    if(live) P.i[ILQG_I_STATUS][b] = (O.max_iter > 0) ? ILQG_ST_ACTIVE : ILQG_ST_MAX_ITER;
}

// Full solves retire finished trajectories (ilqg_host.c, option "compact"): the solver state of trajectory from[j] of
// context S becomes that of trajectory to[j] of context D — everything an iteration reads of a trajectory or a getter
// reports: the current (x, u) wherever it lives (cur_x; it arrives in the arrays X / U, location index 0), the packed records
// (gains), every per-trajectory scalar and integer, the multipliers, and with `records` the stored derivative records of
// the unfused path.  A trajectory's iterations depend on nothing but this state and its lane's own arithmetic, so it
// continues in its new place bit for bit as it would have in the old one.  Lane = (step k, entry j), j fastest: the side
// whose indices are consecutive moves whole rows of the tiled arrays.
__global__ void k_move_traj(DevPtrs D, DevPtrs S, const int *to, const int *from, int count, int records) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(w >= (size_t)count * (S.N + 1)) return;
    const int j = (int)(w % count), k = (int)(w / count);
    const int bs = from[j], bd = to[j];
    const int N = S.N;
    {
        const double *rs = nomp(S, k, bs);
        double *rd = nomp(D, k, bd);
#pragma unroll
        for(int i = 0; i < RN; i++) rd[i] = rs[i];
    }
    if(!WAVE_MAP) {
        const double *xs = cur_x(S, k, bs);
        double *xo = home_x(D, k, bd);
#pragma unroll
        for(int i = 0; i < NX; i++) xo[i * XSI] = xs[i * XSI];
        if(k < N) {
            const double *us = cur_u(S, k, bs);
            double *uo = home_u(D, k, bd);
#pragma unroll
            for(int i = 0; i < NU; i++) uo[i * XSI] = us[i * XSI];
        }
        if(records && k < N) {
            const double *a = S.f[ILQG_F_DER] + ix(S, REC, N, k, 0, bs);
            double *o = D.f[ILQG_F_DER] + ix(D, REC, N, k, 0, bd);
            for(int i = 0; i < REC; i++) o[i * SI] = a[i * SI];
        }
    }
    if(ME > 0 && k < N) {
        const double *a = S.f[ILQG_F_MUL] + mul_ix(S, ME, k, bs);
        double *o = D.f[ILQG_F_MUL] + mul_ix(D, ME, k, bd);
        for(int i = 0; i < ME; i++) o[i * WAVE] = a[i * WAVE];
    }
    if(k != 0) return;
    if(MF > 0) {
        const double *a = S.f[ILQG_F_MULF] + mul_ix(S, MF, 0, bs);
        double *o = D.f[ILQG_F_MULF] + mul_ix(D, MF, 0, bd);
        for(int i = 0; i < MF; i++) o[i * WAVE] = a[i * WAVE];
    }
    if(records || WAVE_MAP) {
        const double *a = S.f[ILQG_F_FIN] + ix(S, FIN, 1, 0, 0, bs);
        double *o = D.f[ILQG_F_FIN] + ix(D, FIN, 1, 0, 0, bd);
        for(int i = 0; i < FIN; i++) o[i * SI] = a[i * SI];
    }
    for(int f = ILQG_F_COST; f < ILQG_F_ALPHA_COST; f++) D.f[f][bd] = S.f[f][bs];
    for(int i = 0; i < ILQG_MAX_ALPHA; i++) D.f[ILQG_F_ALPHA_COST][tile_ix(ILQG_MAX_ALPHA, i, bd)] = S.f[ILQG_F_ALPHA_COST][tile_ix(ILQG_MAX_ALPHA, i, bs)];
    for(int f = 0; f < ILQG_I_COUNT; f++) {
        const int wd = (f == ILQG_I_ALPHA_OK) ? ILQG_MAX_ALPHA : 1;
        for(int i = 0; i < wd; i++) D.i[f][(size_t)i * D.Bp + bd] = (f == ILQG_I_LOC) ? 0 : S.i[f][(size_t)i * S.Bp + bs];
    }
    D.derivs_failed[bd] = S.derivs_failed[bs];
}

// ... and with them their rows of the per-trajectory parameter table [B][W] (ilqg_dev_set_params_batch)
__global__ void k_move_rows(double *__restrict__ dst, const double *__restrict__ src, const int *to, const int *from, int count, int W) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(w >= (size_t)count * W) return;
    const int j = (int)(w / W), i = (int)(w % W);
    dst[(size_t)to[j] * W + i] = src[(size_t)from[j] * W + i];
}

// ... and their histories: slot to[j] of D becomes a copy of slot from[j] of S — the count as it is, the entries S holds of
// it (min(n, S.cap)) as far as D has room, zero behind them.  One thread per (entry of D, j), j fastest.
template <class Hist = History>
__global__ void k_move_history(Hist D, Hist S, const int *to, const int *from, int count) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(w >= (size_t)count * D.cap) return;
    const int j = (int)(w % count), e = (int)(w / count);
    const int bs = from[j], bd = to[j];
    const int n = S.i[bs];
    const bool held = e < n && e < S.cap;
    if(e == 0) D.i[bd] = n;
    for(int f = 0; f < HIST_DOUBLES; f++) D.d[D.at(f, e, bd)] = held ? S.d[S.at(f, e, bs)] : 0.0;
    for(int f = 0; f < ILQG_HI_COUNT; f++) D.ints()[D.at(f, e, bd)] = held ? S.ints()[S.at(f, e, bs)] : 0;
}

// The harvest of a stream of starts (ilqg_dev_harvest; ilqg_host.c stream_solve): what the caller wants of the finished
// trajectories from[0..count) leaves the solver's layouts for ONE packed buffer, a record of W 8-byte words per entry behind
// each other (start-major), so that a poll costs one launch and one copy to the host whatever it asks for.  A record:
//   word 0 the cost, word 1 the ints { status, iterations };
//   words [ox, ox + (N + 1) NX) the current x [N + 1][NX], words [ou, ou + N NU) the current u [N][NU] (each only if asked
//   for: o* < 0 = left out), read where the trajectory lives — cur_x / cur_u as in k_head and k_move_traj: the tiled X / U or a
//   kept plane by the location index in the lane mapping, the packed records in the wave mapping;
//   per requested history field i the words [off[i], off[i + 1]): a double field's cap entries, an int field's cap entries two
//   to a word, or the count n alone in a word — min(n, cap) entries as recorded, zero behind them (the rule of k_move_history).
// Thread-to-element map: a wavefront takes 64 consecutive WORDS of one record, so every store instruction of it writes 512
// contiguous bytes, whole lines.  The reads are the gather: x, u and the history are laid out along the trajectory, one
// wavefront's words of them are 64 different lines, 8 useful bytes each: a load instruction fetches 64 lines for 512 bytes.
// That price is paid as it stands (measured 0.025 ms for 4.5 MB of whole trajectories, about 180 GB/s): a transposing form needs
// LDS, for a kernel that moves a few kilobytes per finished start once every eight iterations.  (The four wavefronts of a
// workgroup take the SAME words of four consecutive entries of the ascending list, so neighbouring slots that finished in the
// same poll share lines; with CarParking's spread of iteration counts they mostly are no neighbours, and nothing relies on
// it.)  No arithmetic, no LDS, no scratch: the plan's arrays are indexed by unrolled constants only.
// A template for the reason k_history is one: it is emitted where the shim first uses it (launch_harvest).
constexpr int HARVEST_FIELDS = ILQG_H_COUNT + ILQG_HI_COUNT + 1;
enum { HARVEST_DOUBLE = 0, HARVEST_INT = 1, HARVEST_N = 2 };
struct HarvestPlan {
    int count, W, ox, ou, n_hist;
    int off[HARVEST_FIELDS + 1], kind[HARVEST_FIELDS], field[HARVEST_FIELDS];
};
constexpr int HARVEST_WAVES = 4;
template <class Hist = History>
__global__ void __launch_bounds__(WAVE * HARVEST_WAVES) k_harvest(DevPtrs P, Hist H, HarvestPlan A, const int *__restrict__ from,
                                                                  unsigned long long *__restrict__ out) {
    const int j = (int)blockIdx.x * HARVEST_WAVES + (int)(threadIdx.x >> 6);  // wave-uniform
    const int q = (int)blockIdx.y * WAVE + (int)(threadIdx.x & 63);
    if(j >= A.count || q >= A.W) return;
    const int b = from[j];
    const int NXW = (P.N + 1) * NX, NUW = P.N * NU;
    unsigned long long word = 0ull;
    auto ints = [](int lo, int hi) { return (unsigned long long)(unsigned)lo | ((unsigned long long)(unsigned)hi << 32); };
    if(q == 0) {
        word = (unsigned long long)__double_as_longlong(P.f[ILQG_F_COST][b]);
    } else if(q == 1) {
        word = ints(P.i[ILQG_I_STATUS][b], P.i[ILQG_I_ITER][b]);
    } else if(A.ox >= 0 && q >= A.ox && q < A.ox + NXW) {
        const int e = q - A.ox;
        word = (unsigned long long)__double_as_longlong(cur_x(P, e / NX, b)[(size_t)(e % NX) * XSI]);
    } else if(A.ou >= 0 && q >= A.ou && q < A.ou + NUW) {
        const int e = q - A.ou;
        word = (unsigned long long)__double_as_longlong(cur_u(P, e / NU, b)[(size_t)(e % NU) * XSI]);
    } else {
#pragma unroll
        for(int i = 0; i < HARVEST_FIELDS; i++) {
            if(i >= A.n_hist || q < A.off[i] || q >= A.off[i + 1]) continue;
            const int n = H.i[b], held = n < H.cap ? n : H.cap, e = q - A.off[i];
            if(A.kind[i] == HARVEST_N) {
                word = ints(n, 0);
            } else if(A.kind[i] == HARVEST_DOUBLE) {
                if(e < held) word = (unsigned long long)__double_as_longlong(H.d[H.at(A.field[i], e, b)]);
            } else {
                const int *hi = H.ints();
                word = ints(2 * e < held ? hi[H.at(A.field[i], 2 * e, b)] : 0, 2 * e + 1 < held ? hi[H.at(A.field[i], 2 * e + 1, b)] : 0);
            }
        }
    }
    out[(size_t)j * A.W + q] = word;
}

__global__ void k_count_active(const int *status, int B, int *out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int active = (b < B && status[b] == ILQG_ST_ACTIVE) ? 1 : 0;
    const unsigned long long m = __ballot(active);
    if((threadIdx.x & 63) == 0 && m) atomicAdd(out, __popcll(m));
}

// unit-test kernel for the shared sincos the generated callbacks are routed through
__global__ void k_sincos_test(int n, const double *x, double *s, double *c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    const ilqg_sc r = ilqg_sincos(x[i]);
    s[i] = r.s;
    c[i] = r.c;
}

// The reference's small dense helpers as callable entry points (matMult.h:11-14, cholesky.h:4-6), executed by
// the same device templates the lane-mapped kernels use.  One problem on one lane; sizes are those of this
// build's problem (matMult) resp. 1, 2, 3, 8 and N_U (Cholesky).
enum { DENSE_MULVEC = 0, DENSE_SQUARETRI = 1, DENSE_MUL2TRI = 2, DENSE_CHOL = 3, DENSE_CHOLINV = 4 };

template <int M>
__device__ void dense_chol(int op, const double *in, double *out, int *flag) {
    constexpr int T = tri(M);
    double A[T], U[T];
#pragma unroll
    for(int i = 0; i < T; i++) A[i] = in[i];
    if(op == DENSE_CHOL) {
        *flag = chol_factor<M>(A, U) ? 1 : 0;  // on failure the content of L is unspecified (as in the reference)
#pragma unroll
        for(int i = 0; i < T; i++) out[i] = U[i];
    } else {
        chol_inverse<M>(A, U);
#pragma unroll
        for(int i = 0; i < T; i++) out[i] = U[i];
    }
}

__global__ void k_dense_test(int op, int v0, int v1, int v2, const double *in0, const double *in1, const double *in2,
                             double *out, int *flag) {
    if(blockIdx.x || threadIdx.x) return;
    *flag = 1;
    if(op == DENSE_CHOL || op == DENSE_CHOLINV) {
        switch(v0) {
            case 1: dense_chol<1>(op, in0, out, flag); break;
            case 2: dense_chol<2>(op, in0, out, flag); break;
            case 3: dense_chol<3>(op, in0, out, flag); break;
            case 8: dense_chol<8>(op, in0, out, flag); break;
            default:
                if(v0 == NU) dense_chol<NU>(op, in0, out, flag); else *flag = -1;
        }
        return;
    }
#if !ILQG_WAVE_MAP
    // v0 selects the shape: 0 = (N_X, N_U), 1 = (N_X, N_X), 2 = (N_U, N_X) / (N_U, N_X, 1)
    if(op == DENSE_MULVEC) {
        if(v0 == 0) add_mul_vec<NX, NU>(out, in0, in1); else add_mul_vec<NX, NX>(out, in0, in1);
    } else if(op == DENSE_SQUARETRI) {
        if(v0 == 0) add_square_tri<NX, NU>(out, in0, in1);
        else if(v0 == 1) add_square_tri<NX, NX>(out, in0, in1);
        else add_square_tri<NU, NX>(out, in0, in1);
    } else if(op == DENSE_MUL2TRI) {
        if(v0 == 0) add_mul2_tri<NX, NX, NU>(out, in0, in1, in2); else add_mul2_tri<NU, NX, 1>(out, in0, in1, in2);
    }
#else
    *flag = -1;
#endif
}

// unit-test kernel for box_qp<M>, one problem per lane (TABLE: the pattern-table form, see chol_pattern_table)
template <int M, bool TABLE = false>
__global__ __launch_bounds__(64, 1) void k_boxqp_test(int count, const double *H, const double *g, const double *lower, const double *upper,
                             double *x, int *clamp, int *n_free, double *invH, int *rc) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= count) return;
    constexpr int T = tri(M);
    double h[T], gg[M], lo[M], up[M], xx[M], inv[T];
    int cl[M], nf;
#pragma unroll
    for(int i = 0; i < T; i++) h[i] = H[(size_t)t * T + i];
#pragma unroll
    for(int i = 0; i < M; i++) {
        gg[i] = g[(size_t)t * M + i];
        lo[i] = lower[(size_t)t * M + i];
        up[i] = upper[(size_t)t * M + i];
        xx[i] = x[(size_t)t * M + i];
    }
    rc[t] = box_qp<M, TABLE>(h, gg, lo, up, xx, cl, nf, inv);
    n_free[t] = nf;
#pragma unroll
    for(int i = 0; i < M; i++) {
        x[(size_t)t * M + i] = xx[i];
        clamp[t * M + i] = cl[i];
    }
#pragma unroll
    for(int i = 0; i < T; i++) invH[(size_t)t * T + i] = inv[i];
}

// unit-test kernel for the cooperative box QP of the wave mapping, one problem per wavefront, in the form this library's
// backward step runs: box_qp_row<M> (ilqg_row.hpp) where the step is the row mapping's, box_qp_rows<M> (ilqg_wave.hpp)
// where it is the one-output-element-per-lane one (N_X or N_U beyond 16, and the `_elem` library)
template <int M>
__global__ __launch_bounds__(64) void k_boxqp_rows_test(int count, const double *H, const double *g, const double *lower,
                                                        const double *upper, double *x, int *clamp, int *n_free, double *invH,
                                                        int *rc) {
    constexpr int T = tri(M);
    __shared__ double sH[T], sl[M], sinv[T];
    __shared__ int scl[M];
    const int t = blockIdx.x, lane = threadIdx.x;
    if(t >= count) return;
    for(int i = lane; i < T; i += 64) sH[i] = H[(size_t)t * T + i];
    if(lane < M) sl[lane] = x[(size_t)t * M + lane];
    wave_sync();
    const int me = (ROW_STEP && M <= 16) ? (lane & 15) % M : lane % M;
    int nf, r;
    if constexpr(ROW_STEP && M <= 16)
        r = box_qp_row<M>(sH, g[(size_t)t * M + me], lower[(size_t)t * M + me], upper[(size_t)t * M + me], sl, scl, sinv, nf);
    else
        r = box_qp_rows<M>(sH, g[(size_t)t * M + me], lower[(size_t)t * M + me], upper[(size_t)t * M + me], sl, scl, sinv, nf);
    wave_sync();
    if(lane == 0) {
        rc[t] = r;
        n_free[t] = nf;
    }
    if(lane < M) {
        x[(size_t)t * M + lane] = sl[lane];
        clamp[t * M + lane] = scl[lane];
    }
    for(int i = lane; i < T; i += 64) invH[(size_t)t * T + i] = sinv[i];
}

#if ILQG_WAVE_MAP
// unit-test kernel for box_qp_quad<M> (quad mapping, ilqg_quad.hpp): one wavefront per workgroup, four problems per
// wavefront — row r = lane / 16 takes problem 4 * blockIdx.x + r.  A row whose problem lies beyond `count` loads and
// stores nothing and is not active, nor is one whose entry of `active` is 0; every lane reaches the call (its ballots
// are the wavefront's).  n_free is M minus the clamp flags set (box_qp_quad does not hand it back); the inverse goes out
// in the packed full-index form of k_boxqp_test, lane `me` writing the entries (me, j), j >= me, of its row.
template <int M>
__global__ __launch_bounds__(64) void k_boxqp_quad_test(int count, const int *active, const double *H, const double *g, const double *lower,
                                                        const double *upper, double *x, int *clamp, int *n_free, double *invH,
                                                        int *rc) {
    constexpr int T = tri(M), INV = (M + 1) * M, ROW = INV + 2 * M;  // per row: the inverse's exchange, the lean build's diagonal
    __shared__ double S[4 * ROW];
    const int lane = threadIdx.x & 63, row = lane >> 4, c = lane & 15, me = c % M;
    const int t = 4 * (int)blockIdx.x + row;
    const bool in = t < count;
    double Hrow[M], gg = 0.0, lo = 0.0, up = 0.0, xx = 0.0, invrow[M];
#pragma unroll
    for(int j = 0; j < M; j++) Hrow[j] = 0.0;
    bool act = false;
    if(in) {
#pragma unroll
        for(int j = 0; j < M; j++) Hrow[j] = H[(size_t)t * T + sy(me, j)];
        gg = g[(size_t)t * M + me];
        lo = lower[(size_t)t * M + me];
        up = upper[(size_t)t * M + me];
        xx = x[(size_t)t * M + me];
        act = active[t] != 0;
    }
    const unsigned inv_at = lds_addr(S + row * ROW);
    int cl;
    const int r = box_qp_quad<M>(Hrow, gg, lo, up, xx, act, inv_at, cl, invrow, inv_at + INV * 8);
    const unsigned set = row_bits(__builtin_amdgcn_ballot_w64(cl != 0 && c < M), lane);
    if(in && c < M) {
        x[(size_t)t * M + me] = xx;
        clamp[t * M + me] = cl;
#pragma unroll
        for(int j = 0; j < M; j++)
            if(j >= me) invH[(size_t)t * T + ut(me, j)] = invrow[j];
        if(c == 0) {
            rc[t] = r;
            n_free[t] = M - __builtin_popcount(set);
        }
    }
}
#endif
