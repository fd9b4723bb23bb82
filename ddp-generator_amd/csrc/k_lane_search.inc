// Lane mapping: the line search that keeps what it rolls out.  Included by ilqg_kernels.hip (anonymous namespace)
// when !ILQG_WAVE_MAP.
// ---------------------------------------------------------------------------
// Line search that KEEPS what it rolls out (lane mapping, option ls_keep = 2)
// ---------------------------------------------------------------------------
// A wavefront takes T = 64 / n trajectories and all n step sizes of the stage, lane = a * T + t (step size a,
// trajectory t of the wavefront).  What that buys:
//  * everything the selection of line_search.c:37-75 needs is in the wavefront when the roll-outs end, so it happens
//    right there, by wavefront shuffles (no k_select launch, no per-alpha round trip through HBM);
//  * the nominal record of a step is ONE line request per trajectory, shared by its n lanes — which is what leaves
//    the memory system room for the stores: every lane keeps its roll-out (measured: the first stage with one step
//    size per ROW of the grid fetches the records once per row, 11 GB per iteration, and slows from 2.15 to 3.26 ms
//    when it also stores; in this mapping 2.80 -> 2.87 ms);
//  * with T = 16 (n = 4) the 16 lanes of a step size store 16 consecutive doubles: one whole line.
// Stage 0 (all trajectories, step sizes [0, n)): the roll-outs go to the planes of set `set` (see cur_x), in the layout
// of X / U, and the accepted one BECOMES the current trajectory when k_commit changes the trajectory's location index:
// no second roll-out of the winner (a chain of N dependent steps, 376 vector instructions per step and trajectory) and
// no copy.  Trajectories without an acceptable step size are appended to P.pending.
// Stage 1 (the entries of P.pending, step sizes [a0, a0 + n)): kept in P.cand by entry; k_adopt_home copies the
// accepted ones (few) into X / U.
// The scan state (last cnew / dcost / expected) is carried from stage to stage exactly as k_select does, so the
// accepted index and the values left behind are those of one sequential scan (line_search.c:37-75).
// DMA: the nominal records of the wavefront's T trajectories reach the lanes through LDS.  Every lane needs the whole
// record of its trajectory (x, u, l, L: 128 bytes for CarParking) in every step, and with per-lane loads the n lanes of
// a trajectory each pull it through the CU's vector-memory path: 8 KB per wavefront and step for 2 KB of data, on the
// path that also carries the stores of the kept roll-outs — measured, the stores alone cost 0.65 of the kernel's 3.07
// ms, so that path and not the arithmetic bounds the kernel.  Instead the records are fetched ONCE, by
// global_load_lds_dwordx4 straight into LDS (no staging registers): lane i of load m moves the 16-byte piece
// q = 64 m + i, and the pieces lie piece-major, q = j T + r (piece j of record r), so that the T lanes of a step size
// read T consecutive 16-byte pieces (no bank conflicts).  Two buffers: the records of step k+2 are on their way while
// step k+1's are read.  Used when a step's pieces fit DMA_LOADS loads (T * RN / 2 <= 64 DMA_LOADS).
constexpr int DMA_LOADS = 3;
template <int stage, bool DMA, class... Rows>
__global__ __launch_bounds__(WAVE, 1)  // (1: wavefronts of k_search per SIMD the register allocation must allow)
void k_search(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int a0, int n, int set, Rows... rows) {
    // Rows: empty — the kernel as it always was, under its old name — or the context's per-trajectory table and its map
    constexpr bool PER_TRAJECTORY = RowPack<OWN_NONE, Rows...>::has_trajectory_rows;
    extern __shared__ __attribute__((aligned(16))) double s_rec[];  // DMA: [2][T * RN] doubles
    const Place place(2 + stage);
    const int lane = threadIdx.x;
    const int T = WAVE / n;
    int a = lane / T;
    const int t = lane - a * T;
    const bool used = a < n;  // (64 - n * T) lanes have nothing of their own to do: they repeat the last step size
    if(!used) a = n - 1;
    const int count = stage ? *P.n_pending : P.B;
    if((int)blockIdx.x * T >= count) return;
    const int e = blockIdx.x * T + t;                   // trajectory (stage 0) or entry of the pending list
    const int ee = e < count ? e : count - 1;           // lanes beyond the end repeat the last one (results dropped)
    const int b = stage ? P.pending[ee] : ee;
    const bool live = used && e < count && P.i[ILQG_I_STATUS][b] == ILQG_ST_ACTIVE;
    if(__builtin_amdgcn_ballot_w64(live) == 0ull) return;
    const int N = P.N;
    const int ai = a0 + a;
    const double alpha = O.alpha[ai];
    const bool feedback = (alpha != 0.0);  // alpha == 0.0: u = u_nom without feedback (iLQG_func.tem:156-158)

    // (the shared kernels with the records through LDS: parameters per lane, where measured faster — load_params)
    ILQG_CALLBACKS_IN(C, H, VECTOR_PARAMS && !PER_TRAJECTORY && DMA);
    // (b = pending[ee] or ee: lanes beyond the end repeat the last entry, and read its row)
    apply_rows<OWN_NONE>(C_values, C_table, P, b, 0, 0, rows...);
    load_penalty_weights(C, P, b);
    trajEl_t ct;
    multipliersEl_t mk;
    multipliersEl_t *const mp = HAS_MUL ? &mk : nullptr;
    init_running(&ct, &C.o1);

    NomPtrs q;
    q.x = nomp(P, 0, b) + NOM_X;
    q.u = nomp(P, 0, b) + NOM_U;
    q.l = nomp(P, 0, b) + NOM_L;
    q.K = nomp(P, 0, b) + NOM_K;
    // DMA: this lane's pieces (see above) — source of load m at step 0, and whether the lane takes part in it
    constexpr int PIECES = RN / 2;
    const double *dsrc[DMA_LOADS];
    bool dact[DMA_LOADS];
    if(DMA) {
#pragma unroll
        for(int m = 0; m < DMA_LOADS; m++) {
            const int qq = m * WAVE + lane;
            const int j = qq / T, r = qq - j * T;
            dact[m] = qq < T * PIECES;
            const int br = __shfl(b, r < T ? r : 0);  // trajectory of record r: held by lane r (step size 0)
            dsrc[m] = nomp(P, 0, br) + 2 * (j < PIECES ? j : 0);
        }
    }
    auto dma_issue = [&](int buf) {  // the records of the step dsrc points at -> LDS buffer buf; dsrc moves on one step
#pragma unroll
        for(int m = 0; m < DMA_LOADS; m++) {
            if(dact[m])
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)dsrc[m],
                                                 (__attribute__((address_space(3))) void *)(s_rec + (size_t)buf * T * RN + m * WAVE * 2),
                                                 16, 0, 0);
            dsrc[m] += RN;
        }
    };
    auto dma_read = [&](NomStep &c, int buf) {  // this lane's record out of LDS buffer buf
        double rec[RN];
        const double *base = s_rec + (size_t)buf * T * RN + 2 * t;
#pragma unroll
        for(int j = 0; j < PIECES; j++) {
            rec[2 * j] = base[(size_t)j * T * 2];
            rec[2 * j + 1] = base[(size_t)j * T * 2 + 1];
        }
#pragma unroll
        for(int i = 0; i < NX; i++) c.x[i] = rec[NOM_X + i];
#pragma unroll
        for(int i = 0; i < NU; i++) c.u[i] = rec[NOM_U + i];
#pragma unroll
        for(int i = 0; i < NU; i++) c.l[i] = rec[NOM_L + i];
#pragma unroll
        for(int i = 0; i < NXU; i++) c.K[i] = rec[NOM_K + i];
    };
    // where this lane keeps its roll-out: stage 0 in plane (set, a) in the layout of X / U, stage 1 in P.cand by entry
    double *kx, *ku;
    const size_t kxs = stage ? (size_t)CAND_W * P.Bp : cur_xstride(P), kus = stage ? kxs : cur_ustride(P);  // between steps
    const size_t kcs = stage ? (size_t)P.Bp : (size_t)XSI;                                                 // between components
    if(stage) {
        kx = P.cand + (size_t)a * (N + 1) * CAND_W * P.Bp + ee;
        ku = kx + (size_t)NX * P.Bp;
    } else {
        const int plane = set * P.plane_n + a;
        kx = P.xpl + (size_t)plane * P.xplane + ix(P, NX, N + 1, 0, 0, b);
        ku = P.upl + (size_t)plane * P.uplane + ix(P, NU, N, 0, 0, b);
    }

    double xc[NX];
#pragma unroll
    for(int i = 0; i < NX; i++) xc[i] = q.x[i];  // x0 (iLQG_func.tem:141-142)
    double csum = 0.0;
    int okc = 1;
    NomStep cur;
    if(DMA) {
        dma_issue(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        dma_issue(1);  // step 1 (N >= 2)
    } else {
        load_nominal<true, 1>(cur, q);
    }
    drain_memory_ops();
    for(int k = 0; k < N; k++) {
        NomPtrs qn;
        qn.x = q.x + RN;
        qn.u = q.u + RN;
        qn.l = q.l + RN;
        qn.K = q.K + RN;
        // DMA: the record is read out of LDS HERE, where it is consumed, not a step ahead: its 32 registers are live for
        // the first few instructions of the step only, not across the sin / cos evaluations (145 -> fewer registers)
        if(DMA) dma_read(cur, k & 1);
        double xin[NX], uin[NU];
#pragma unroll
        for(int i = 0; i < NX; i++) xin[i] = xc[i];
        {   // u = u_nom + alpha*l + L (x - x_nom), state by state (iLQG_func.tem:146-155)
            double uf[NU];
#pragma unroll
            for(int j = 0; j < NU; j++) uf[j] = cur.u[j] + cur.l[j] * alpha;
#pragma unroll
            for(int i = 0; i < NX; i++) {
                const double dx = xin[i] - cur.x[i];
#pragma unroll
                for(int j = 0; j < NU; j++) uf[j] += cur.K[j + i * NU] * dx;
            }
#pragma unroll
            for(int j = 0; j < NU; j++) uin[j] = feedback ? uf[j] : cur.u[j];
        }
        if(!DMA) load_nominal<true, 1>(cur, qn);  // the next step's record is in flight while this one computes
        if(HAS_MUL) load_mul(P, k, b, mk);
        double xnext[NX];
        auto step = ILQG_FORWARD_STEP(false, ct, mp, k, N, C, xin, uin, xnext);
        const int r = run_step(H, okc, step);
        okc &= r;
        csum += ct.c;
        if(DMA) {
            // Outstanding here: the kept roll-out of step k-1 and the records of step k+1, both issued a whole step
            // ago.  The wait stands BEFORE this step's stores so that it never waits for a store just issued.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if(live) {  // (!DMA: behind the prefetch in issue order: the wait for the prefetched values leaves these in flight)
#pragma unroll
            for(int i = 0; i < NX; i++) kx[i * kcs] = ct.x[i];
#pragma unroll
            for(int i = 0; i < NU; i++) ku[i * kcs] = ct.u[i];
        }
        if(DMA && k + 2 <= N) dma_issue(k & 1);  // (that buffer held step k: read at the end of step k-1)
        kx += kxs;
        ku += kus;
#pragma unroll
        for(int i = 0; i < NX; i++) xc[i] = xnext[i];
        q = qn;
    }
    {   // final cost (iLQG_func.tem:179-182)
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
        if(live) {
#pragma unroll
            for(int i = 0; i < NX; i++) kx[i * kcs] = cf.x[i];
        }
    }
    const int ok = (okc && H.nonfinite == 0.0) ? 1 : 0;
    if(live) {
        P.f[ILQG_F_ALPHA_COST][tile_ix(ILQG_MAX_ALPHA, ai, b)] = csum;
        P.i[ILQG_I_ALPHA_OK][(size_t)ai * P.Bp + b] = ok;
    }

    // Selection, as k_select does it (line_search.c:37-75), by the lane of the trajectory's first step size; the
    // other lanes' values come by wavefront shuffles.  Every lane computes the test of its own step size.
    const double cost = P.f[ILQG_F_COST][b], dV0 = P.f[ILQG_F_DV0][b], dV1 = P.f[ILQG_F_DV1][b];
    const double my_dcost = cost - csum;
    const double my_expected = expected_reduction(alpha, dV0, dV1);
    const double my_z = reduction_ratio(my_dcost, my_expected);
    const int my_pass = (ok && my_z > O.zMin) ? 1 : 0;
    double cnew = (a0 > 0) ? P.f[ILQG_F_NEW_COST][b] : 0.0;
    double dcost = P.f[ILQG_F_DCOST][b], expected = P.f[ILQG_F_EXPECTED][b];
    int win = -1;
    for(int i = 0; i < n; i++) {
        const int src = i * T + t;
        const int ok_i = __shfl(ok, src);
        const int pass_i = __shfl(my_pass, src);
        const double cnew_i = __shfl(csum, src);
        const double dcost_i = __shfl(my_dcost, src);
        const double expected_i = __shfl(my_expected, src);
        if(win < 0) {
            cnew = cnew_i;
            if(ok_i) {
                dcost = dcost_i;
                expected = expected_i;
                if(pass_i) win = i;
            }
        }
    }
    const bool leader = live && lane < T;  // a == 0
    if(leader) {
        P.i[ILQG_I_ALPHA_IDX][b] = (win >= 0 ? a0 + win : a0 + n) + 1;
        P.i[ILQG_I_ACCEPTED][b] = win >= 0 ? 1 : 0;
        P.f[ILQG_F_NEW_COST][b] = cnew;
        P.f[ILQG_F_DCOST][b] = dcost;
        P.f[ILQG_F_EXPECTED][b] = expected;
    }
    // to the second stage: one atomicAdd per wavefront
    const bool more = leader && win < 0 && stage == 0 && a0 + n < O.n_alpha;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(more);
    if(m != 0ull) {
        int base = 0;
        const int first = __builtin_ctzll(m);
        if(lane == first) base = atomicAdd(P.n_pending_next, __builtin_popcountll(m));
        base = __shfl(base, first);
        if(more) P.pending[base + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = b;
    }
}

// After k_search: what has to be COPIED into X / U, one thread per (step, trajectory or entry).
//  * the trajectories the second stage settled, from P.cand (by entry);
//  * the trajectories that found no acceptable step size at all while their current trajectory lives in a plane: the
//    next search writes the set of planes it is in (the sets take turns), so it moves to X / U (rare: 0.5 % of the
//    trajectories of the benchmark window).
// The location indices change afterwards (k_commit), when nothing reads the old ones any more.  s1 = step sizes of
// the first stage.
__global__ void k_adopt_home(DevPtrs P, int s1) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int np = *P.n_pending, N1 = P.N + 1;
    const size_t total2 = (size_t)N1 * np;
    for(size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total2; w += stride) {
        const int e = (int)(w % np), k = (int)(w / np);
        const int b = P.pending[e];
        if(P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE) continue;
        double *xo = home_x(P, k, b);
        if(P.i[ILQG_I_ACCEPTED][b]) {
            const int a = P.i[ILQG_I_ALPHA_IDX][b] - 1 - s1;
            const double *src = P.cand + ((size_t)a * N1 + k) * CAND_W * P.Bp + e;
#pragma unroll
            for(int i = 0; i < NX; i++) xo[i * XSI] = src[(size_t)i * P.Bp];
            if(k < P.N) {
                double *uo = home_u(P, k, b);
#pragma unroll
                for(int i = 0; i < NU; i++) uo[i * XSI] = src[(size_t)(NX + i) * P.Bp];
            }
        } else if(P.i[ILQG_I_LOC][b]) {
            const double *xs = cur_x(P, k, b);
#pragma unroll
            for(int i = 0; i < NX; i++) xo[i * XSI] = xs[i * XSI];
            if(k < P.N) {
                const double *us = cur_u(P, k, b);
                double *uo = home_u(P, k, b);
#pragma unroll
                for(int i = 0; i < NU; i++) uo[i * XSI] = us[i * XSI];
            }
        }
    }
}

// ... and the same for a search without a second stage, where no list of the undecided exists: rejected trajectories
// whose current trajectory lives in a plane move to X / U.  One thread per (step, trajectory).
__global__ void k_rejected_home(DevPtrs P) {
    const size_t total = (size_t)(P.N + 1) * P.Bp, stride = (size_t)gridDim.x * blockDim.x;
    for(size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += stride) {
        const int b = (int)(w % P.Bp), k = (int)(w / P.Bp);
        if(b >= P.B || P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE || P.i[ILQG_I_ACCEPTED][b] || !P.i[ILQG_I_LOC][b]) continue;
        const double *xs = cur_x(P, k, b);
        double *xo = home_x(P, k, b);
#pragma unroll
        for(int i = 0; i < NX; i++) xo[i * XSI] = xs[i * XSI];
        if(k < P.N) {
            const double *us = cur_u(P, k, b);
            double *uo = home_u(P, k, b);
#pragma unroll
            for(int i = 0; i < NU; i++) uo[i * XSI] = us[i * XSI];
        }
    }
}

// The new location of every trajectory that took part in the search: the plane of the accepted step size of the first
// stage, else X / U (adopted from the second stage, or moved there by the kernels above, or there already).
__global__ void k_commit(DevPtrs P, int s1, int set) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if(b >= P.B || P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE) return;
    const int a = P.i[ILQG_I_ALPHA_IDX][b] - 1;
    if(P.i[ILQG_I_ACCEPTED][b])
        P.i[ILQG_I_LOC][b] = (a < s1) ? 1 + set * P.plane_n + a : 0;
    else
        P.i[ILQG_I_LOC][b] = 0;
}

// every current trajectory into X / U (before the host reads or writes them, before an initial roll-out): copy, then
// the caller clears the location indices
__global__ void k_all_home(DevPtrs P) {
    const size_t total = (size_t)(P.N + 1) * P.Bp, stride = (size_t)gridDim.x * blockDim.x;
    for(size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += stride) {
        const int b = (int)(w % P.Bp), k = (int)(w / P.Bp);
        if(b >= P.B || !P.i[ILQG_I_LOC][b]) continue;
        const double *xs = cur_x(P, k, b);
        double *xo = home_x(P, k, b);
#pragma unroll
        for(int i = 0; i < NX; i++) xo[i * XSI] = xs[i * XSI];
        if(k < P.N) {
            const double *us = cur_u(P, k, b);
            double *uo = home_u(P, k, b);
#pragma unroll
            for(int i = 0; i < NU; i++) uo[i * XSI] = us[i * XSI];
        }
    }
}
