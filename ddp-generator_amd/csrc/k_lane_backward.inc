// Lane mapping (one lane = one trajectory): calc_derivs and the backward pass.  Included by ilqg_kernels.hip inside its
// anonymous namespace when !ILQG_WAVE_MAP; not a translation unit of its own.
// ---------------------------------------------------------------------------
// The reference's calc_derivs body for one time step (iLQG_func.tem:207-211), from (x_k, u_k) in t.
// Auxiliaries are not kept in HBM: they are recomputed from (x,u) exactly as forward_pass did
// (iLQG_func.tem:160-164).  Straight-line code (see ilqg_hooks); evaluated a second time through the
// device library's sin/cos in the rare case that an argument was beyond the fast reduction.
// ---------------------------------------------------------------------------
// `overlapped` is called between the evaluation and the test for the rare second evaluation: a caller
// that has independent work in flight pins its results there, so that both share one basic block.
template <class F>
__device__ __forceinline__ int derivs_step(trajEl_t &t, multipliersEl_t *m, Callbacks &C, ilqg_hooks &H, int k, int N,
                                           F &&overlapped) {
    double x[NX], u[NU];
#pragma unroll
    for(int i = 0; i < NX; i++) x[i] = t.x[i];
#pragma unroll
    for(int i = 0; i < NU; i++) u[i] = t.u[i];
    const double nf0 = H.nonfinite;
    H.huge = 0.0;
    int ok = 1;
    auto body = [&]() {
        ok = calcXVariableAux(&t, m, k, &C.o);
        ok &= calcXUVariableAux(&t, m, k, &C.o);
        ok &= calcLAuxDeriv(&t, m, k, &C.o);
        ok &= bp_derivsL(&t, k, C.o.p);
        limitsU(&t, k, C.o.p, N);
    };
    body();
    overlapped();
    if(H.huge != 0.0) {
#pragma unroll
        for(int i = 0; i < NX; i++) t.x[i] = x[i];
#pragma unroll
        for(int i = 0; i < NU; i++) t.u[i] = u[i];
        H.nonfinite = nf0;
        H.slow = 1.0;
        body();
        H.slow = 0.0;
    }
    return ok;
}

__device__ __forceinline__ int derivs_final(trajFin_t &fin, multipliersFin_t *m, Callbacks &C, ilqg_hooks &H, int N) {
    double x[NX];
#pragma unroll
    for(int i = 0; i < NX; i++) x[i] = fin.x[i];
    const double nf0 = H.nonfinite;
    H.huge = 0.0;
    int ok = 1;
    auto body = [&]() {
        ok = calcFVariableAux(&fin, m, &C.o);
        ok &= calcFAuxDeriv(&fin, m, &C.o);
        ok &= bp_derivsF(&fin, N, C.o.p);
    };
    body();
    if(H.huge != 0.0) {
#pragma unroll
        for(int i = 0; i < NX; i++) fin.x[i] = x[i];
        H.nonfinite = nf0;
        H.slow = 1.0;
        body();
        H.slow = 0.0;
    }
    return ok;
}

// record of one step in the order of RecLayout
#define REC_COPY(OP, t)                                                                                 \
    OP(RL::CX, (t).cx, NX) OP(RL::CXX, (t).cxx, SXX) OP(RL::CU, (t).cu, NU) OP(RL::CUU, (t).cuu, SUU)  \
    OP(RL::CXU, (t).cxu, NXU) OP(RL::FX, (t).fx, NX * NX) OP(RL::FU, (t).fu, NXU)                      \
    OP(RL::LOWER, (t).lower, NU) OP(RL::UPPER, (t).upper, NU) REC_COPY_FULL(OP, t)                      \
    if(HX) {                                                                                            \
        OP(RL::LSIGN, (t).lower_sign, NU) OP(RL::USIGN, (t).upper_sign, NU)                             \
        OP(RL::LHX, (t).lower_hx, NXU) OP(RL::UHX, (t).upper_hx, NXU)                                   \
    }
#if FULL_DDP
#define REC_COPY_FULL(OP, t) OP(RL::FXX, (t).fxx, NX * SXX) OP(RL::FUU, (t).fuu, NX * SUU) OP(RL::FXU, (t).fxu, NX * NXU)
#else
#define REC_COPY_FULL(OP, t)
#endif

// The entries of a step's record that are identically 0, for the fused sweep (ilqg_device.hpp, NoZeros): the generated
// header's list ILQG_STRUCTURAL_ZERO in RecLayout's numbering.  A header without the list (Maxima-generated) and the
// FMA-free twin keep the dense products.
#if defined(ILQG_STRUCTURAL_ZERO) && !defined(ILQG_STRICT_FP)
struct RecZeros {
    static constexpr bool at(int i) {
        bool z = false;
#define ILQG_ZERO_ENTRY(member, index) z = z || (i == RL::off_##member + (index));
        ILQG_STRUCTURAL_ZERO(ILQG_ZERO_ENTRY) ILQG_STRUCTURAL_ZERO_FULL(ILQG_ZERO_ENTRY)
#undef ILQG_ZERO_ENTRY
        return z;
    }
};
#else
using RecZeros = NoZeros;
#endif

// ---------------------------------------------------------------------------
// calc_derivs: one lane per (trajectory, time step); step N is the final record
// ---------------------------------------------------------------------------
// (the lane's work, for k_derivs and for k_derivs_rows below: Rows is empty or the context's per-trajectory table and its map)
template <class... Rows>
__device__ __forceinline__ void derivs_lane(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, Rows... rows) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = (int)(tid % P.Bp);
    const int k = (int)(tid / P.Bp);
    if(k > P.N || b >= P.B) return;
    if(P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE || !P.i[ILQG_I_NEED_DERIVS][b]) return;

    ILQG_CALLBACKS(C, H);
    apply_rows<OWN_NONE>(C_values, C_table, P, b, 0, 0, rows...);
    load_penalty_weights_der(C, P, b);
    int ok = 1;
    if(k < P.N) {
        trajEl_t t;
        multipliersEl_t m;
        load_mul(P, k, b, m);
        init_running(&t, &C.o1);
        const double *xs = cur_x(P, k, b), *us = cur_u(P, k, b);
#pragma unroll
        for(int i = 0; i < NX; i++) t.x[i] = xs[i * XSI];
#pragma unroll
        for(int i = 0; i < NU; i++) t.u[i] = us[i * XSI];

        ok = derivs_step(t, HAS_MUL ? &m : nullptr, C, H, k, P.N, [] {});
        double *out = P.f[ILQG_F_DER] + ix(P, REC, P.N, k, 0, b);
#define PUT(off, arr, cnt) _Pragma("unroll") for(int i = 0; i < (cnt); i++) out[((off) + i) * SI] = (arr)[i];
        REC_COPY(PUT, t)
    } else {
        trajFin_t fin;
        multipliersFin_t mf;
        load_mul_fin(P, b, mf);
        init_final(&fin, &C.o);
        const double *xs = cur_x(P, P.N, b);
#pragma unroll
        for(int i = 0; i < NX; i++) fin.x[i] = xs[i * XSI];

        ok = derivs_final(fin, HAS_MUL ? &mf : nullptr, C, H, P.N);
        double *out = P.f[ILQG_F_FIN] + ix(P, FIN, 1, 0, 0, b);
        PUT(0, fin.cx, NX)
        PUT(NX, fin.cxx, SXX)
#undef PUT
    }
    if(!ok || H.nonfinite != 0.0) P.derivs_failed[b] = 1;
}
__global__ __launch_bounds__(256) void k_derivs(DevPtrs P, ilqg_dev_opts_t O, ParamValues A) { derivs_lane(P, O, A); }
// ... under per-trajectory parameters (k_derivs keeps its name: it is no template)
template <class... Rows>
__global__ __launch_bounds__(256) void k_derivs_rows(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, Rows... rows) {
    derivs_lane(P, O, A, rows...);
}

// ---------------------------------------------------------------------------
// back_pass: one lane per trajectory, sequential in time, next record prefetched
// ---------------------------------------------------------------------------
__device__ __forceinline__ void load_record(double *dst, double *udst, const double *src, const double *us) {
#pragma unroll
    for(int i = 0; i < REC; i++) dst[i] = src[i * SI];
#pragma unroll
    for(int i = 0; i < NU; i++) udst[i] = us[i * XSI];
}

// The gains of a step are stored right behind its arithmetic, i.e. BEHIND the prefetch of the next step's inputs
// in issue order: the memory counter retires in issue order, so the wait for the prefetched values (vmcnt = number
// of younger operations) leaves the stores in flight.  They are stored for every lane, also for one whose box QP
// has just failed (back_pass.c:168-171 returns before writing L): that lane leaves the sweep right after, and a
// retry rewrites all gains.
template <int CS = 1>
__device__ __forceinline__ void store_gains(const double *l, const double *K, double *lo, double *ko) {
#pragma unroll
    for(int i = 0; i < NU; i++) lo[i * CS] = l[i];
#pragma unroll
    for(int i = 0; i < NXU; i++) ko[i * CS] = K[i];
}

// one sweep k = N-1..0; returns 0 ok, 1 box-QP failed (back_pass.c:168-171)
__device__ __forceinline__ int backward_sweep(const DevPtrs &P, int b, double lambda, int regType, double &dV0,
                                              double &dV1, double &g_norm) {
    const int N = P.N;
    double Vx[NX], Vxx[SXX], l[NU], K[NXU];
    const double *fin = P.f[ILQG_F_FIN] + ix(P, FIN, 1, 0, 0, b);
#pragma unroll
    for(int i = 0; i < NX; i++) Vx[i] = fin[i * SI];
#pragma unroll
    for(int i = 0; i < SXX; i++) Vxx[i] = fin[(NX + i) * SI];
#pragma unroll
    for(int i = 0; i < NU; i++) l[i] = 0.0;  // warm start of the last step (back_pass.c:163-164)
    dV0 = 0.0;
    dV1 = 0.0;
    double gsum = 0.0;

    // pointers to step k of this lane's trajectory, walked backwards
    const double *rp = P.f[ILQG_F_DER] + ix(P, REC, N, N - 1, 0, b);
    // This sweep streams the stored records; its gains go to the tiled arrays l / L (512 contiguous bytes per
    // component and wavefront) and k_pack_records turns them into the line search's records afterwards.
    const double *up = cur_u(P, N - 1, b);
    double *lo = WAVE_MAP ? nomp(P, N - 1, b) + NOM_L : P.f[ILQG_F_LG] + ix(P, NU, N, N - 1, 0, b);
    double *ko = WAVE_MAP ? nomp(P, N - 1, b) + NOM_K : P.f[ILQG_F_KG] + ix(P, NXU, N, N - 1, 0, b);
    const size_t rs = step_stride(P, REC), us = cur_ustride(P);
    const size_t ls = WAVE_MAP ? (size_t)RN : step_stride(P, NU), ks = WAVE_MAP ? (size_t)RN : step_stride(P, NXU);

    double cur[REC], ucur[NU];
    load_record(cur, ucur, rp, up);
    int failed = 0;
    drain_memory_ops();
    for(int k = N - 1; k >= 0; k--) {
        double nxt[REC], unxt[NU];
        if(k > 0) load_record(nxt, unxt, rp - rs, up - us);  // in flight while this step computes
        // l still holds the solution of step k+1: the warm start (back_pass.c:165-166)
        const int rc = back_step<NX, NU, FULL, HX>(cur, ucur, Vx, Vxx, l, K, lambda, regType, dV0, dV1, gsum);
        store_gains<XSI>(l, K, lo, ko);
        if(BOXQP_FAILED(rc)) {
            failed = 1;
            break;
        }
        rp -= rs;
        up -= us;
        lo -= ls;
        ko -= ks;
#pragma unroll
        for(int i = 0; i < REC; i++) cur[i] = nxt[i];
#pragma unroll
        for(int i = 0; i < NU; i++) ucur[i] = unxt[i];
    }
    if(!failed) g_norm = gsum / ((double)(N - 1));  // N summands over N-1 (back_pass.c:254)
    return failed;
}

// The same sweep with the derivative record of each step evaluated on the fly from the stored
// (x_k, u_k) by the generated callbacks instead of being read from HBM: per step 6 doubles are
// read and 10 written, instead of 57 + 10 (and k_derivs' 61 are not moved at all).  The values
// are the ones k_derivs would have stored (same callbacks, same inputs).
// Returns 0 ok, 1 box-QP failed, 2 NaN/Inf in the derivatives (iLQG.c:247-249).
__device__ __forceinline__ int backward_sweep_fused(const DevPtrs &P, Callbacks &C, ilqg_hooks &H, int b, double lambda, int regType,
                                                    double &dV0, double &dV1, double &g_norm) {
    const int N = P.N;
    H.nonfinite = 0.0;
    const double *xp = cur_x(P, N, b);
    const double *up = cur_u(P, N - 1, b);
    double *rec_k = nomp(P, N - 1, b);  // record of step k, completed here: (x_k, u_k) as read + the gains
    const size_t xs = cur_xstride(P), us = cur_ustride(P);

    double Vx[NX], Vxx[SXX], l[NU], K[NXU];
    {
        trajFin_t fin;
        init_final(&fin, &C.o);
#pragma unroll
        for(int i = 0; i < NX; i++) fin.x[i] = xp[i * XSI];
        if(!WAVE_MAP) {
            double *recN = nomp(P, N, b);
#pragma unroll
            for(int i = 0; i < NX; i++) recN[NOM_X + i] = fin.x[i];
        }
        multipliersFin_t mf;
        load_mul_fin(P, b, mf);
        const int ok = derivs_final(fin, HAS_MUL ? &mf : nullptr, C, H, N);
        if(!ok || H.nonfinite != 0.0) return 2;
#pragma unroll
        for(int i = 0; i < NX; i++) Vx[i] = fin.cx[i];
#pragma unroll
        for(int i = 0; i < SXX; i++) Vxx[i] = fin.cxx[i];
    }
    xp -= xs;  // step N-1
#pragma unroll
    for(int i = 0; i < NU; i++) l[i] = 0.0;
    dV0 = 0.0;
    dV1 = 0.0;
    double gsum = 0.0;

    // Software pipeline: the record of step k-1 is evaluated in the same loop iteration as the Riccati
    // update of step k, behind the box QP.  The two are independent chains of dependent fp64
    // operations, so with ONE wavefront per SIMD (all that 65 536 trajectories give) the scheduler can
    // fill the latency of one with the other.
    trajEl_t t;
    init_running(&t, &C.o1);  // constant entries of the record (iLQG_func.tem:312-347)
    double xk[NX], uk[NU];    // state and control of the step whose record is in `cur`
    double cur[REC];
#define GETF(off, arr, cnt) _Pragma("unroll") for(int i = 0; i < (cnt); i++) rec[(off) + i] = (arr)[i];
    auto record_of = [&](const double *xv, const double *uv, int k, double *rec, auto &&overlapped) {
#pragma unroll
        for(int i = 0; i < NX; i++) t.x[i] = xv[i];
#pragma unroll
        for(int i = 0; i < NU; i++) t.u[i] = uv[i];
        multipliersEl_t m;
        load_mul(P, k, b, m);
        const int ok = derivs_step(t, HAS_MUL ? &m : nullptr, C, H, k, N, overlapped);
        REC_COPY(GETF, t)
        return ok;
    };
    {
#pragma unroll
        for(int i = 0; i < NX; i++) xk[i] = xp[i * XSI];
#pragma unroll
        for(int i = 0; i < NU; i++) uk[i] = up[i * XSI];
        const int ok = record_of(xk, uk, N - 1, cur, [] {});
        if(!ok || H.nonfinite != 0.0) return 2;
    }
    // (x, u) of step k-1, loaded one iteration ahead of their use (N >= 2)
    double xn[NX], un[NU];
#pragma unroll
    for(int i = 0; i < NX; i++) xn[i] = (xp - xs)[i * XSI];
#pragma unroll
    for(int i = 0; i < NU; i++) un[i] = (up - us)[i * XSI];
    int result = 0;
#ifdef ILQG_PROFILE_SECTIONS
    Prof prof;
    prof.start();
    Prof *pf = &prof;
#else
    Prof *pf = nullptr;
#endif
    drain_memory_ops();
    for(int k = N - 1; k >= 0; k--) {
        if(pf) pf->probe(7);
        // step k-2 (clamped at step 0, so that the pipeline below needs no special case at its end: the
        // last iteration evaluates the record of step 0 once more and discards it)
        double xnn[NX], unn[NU];
        const int back = (k > 1) ? 2 : k;
#pragma unroll
        for(int i = 0; i < NX; i++) xnn[i] = (xp - back * xs)[i * XSI];
#pragma unroll
        for(int i = 0; i < NU; i++) unn[i] = (up - back * us)[i * XSI];
        if(pf) pf->probe(0);
        const int rc = back_step<NX, NU, FULL, HX, RecZeros>(cur, uk, Vx, Vxx, l, K, lambda, regType, dV0, dV1, gsum, pf);
        double nxt[REC];
        // The value-function update above is only needed by the next iteration, so the optimiser would
        // sink it behind the exit tests below, into a block of its own, where it cannot overlap with
        // the derivative evaluation.  Pinning its results right behind that evaluation keeps both in
        // one block.
        const int ok = record_of(xn, un, (k > 0) ? k - 1 : 0, nxt, [&] {
#pragma unroll
            for(int i = 0; i < NX; i++) pin(Vx[i]);
#pragma unroll
            for(int i = 0; i < SXX; i++) pin(Vxx[i]);
            pin(dV0);
            pin(dV1);
            pin(gsum);
        });
        if(!ok || H.nonfinite != 0.0) {
            result = 2;
            break;
        }
        if(pf) pf->probe(6);
        // the record of step k for the line search: gains, and (lane mapping) the (x_k, u_k) they belong to
        store_gains(l, K, rec_k + NOM_L, rec_k + NOM_K);
        if(!WAVE_MAP) {
#pragma unroll
            for(int i = 0; i < NX; i++) rec_k[NOM_X + i] = xk[i];
#pragma unroll
            for(int i = 0; i < NU; i++) rec_k[NOM_U + i] = uk[i];
        }
        if(BOXQP_FAILED(rc)) {
            result = 1;
            break;
        }
#pragma unroll
        for(int i = 0; i < REC; i++) cur[i] = nxt[i];
        xp -= xs;
        up -= us;
        rec_k -= RN;
#pragma unroll
        for(int i = 0; i < NX; i++) xk[i] = xn[i];
#pragma unroll
        for(int i = 0; i < NU; i++) uk[i] = un[i];
#pragma unroll
        for(int i = 0; i < NX; i++) xn[i] = xnn[i];
#pragma unroll
        for(int i = 0; i < NU; i++) un[i] = unn[i];
    }
#undef GETF
    if(!result) g_norm = gsum / ((double)(N - 1));
#ifdef ILQG_PROFILE_SECTIONS
    if((threadIdx.x & 63) == 0)
        for(int i = 0; i < 8; i++) atomicAdd(&ilqg_prof_cycles[i], (unsigned long long)prof.acc[i]);
#endif
    return result;
}

// mode: 0 = records from HBM, lambda retry loop and gradient test (iLQG.c:261-303)
//       1 = records from HBM, ONE sweep (the drop-in back_pass(): the caller owns the retry loop)
//       2 = as 0 with the derivatives evaluated on the fly (k_derivs is not needed)
template <int mode, class... Rows>
__global__ __launch_bounds__(WAVE, 1)  // (1: wavefronts of k_backward per SIMD the register allocation must allow)
void k_backward(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, Rows... rows) {
    // Rows: empty — the kernel as it always was, under its old name — or the context's per-trajectory table and its map
    constexpr bool PER_TRAJECTORY = RowPack<OWN_NONE, Rows...>::has_trajectory_rows;
    const Place place(1);
    const int b = blockIdx.x * WAVE + threadIdx.x;
    if(b >= P.B) return;
    if(P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE) return;
    const int single_sweep = (mode == 1);
    P.i[ILQG_I_NEED_DERIVS][b] = 0;
    if(P.derivs_failed[b]) {  // iLQG.c:247-249
        P.i[ILQG_I_STATUS][b] = ILQG_ST_DERIVS_FAILED;
        return;
    }
    // (the shared fused sweep: parameters per lane, where measured faster — load_params)
    ILQG_CALLBACKS_IN(C, H, VECTOR_PARAMS && !PER_TRAJECTORY && mode == 2);
    apply_rows<OWN_NONE>(C_values, C_table, P, b, 0, 0, rows...);
    load_penalty_weights_der(C, P, b);
    double lambda = P.f[ILQG_F_LAMBDA][b], dlambda = P.f[ILQG_F_DLAMBDA][b];
    double dV0 = 0.0, dV1 = 0.0, g_norm = P.f[ILQG_F_GNORM][b];
    int calls = 0, rc;
    for(;;) {
        if(mode == 2)
            rc = backward_sweep_fused(P, C, H, b, lambda, O.regType, dV0, dV1, g_norm);
        else
            rc = backward_sweep(P, b, lambda, O.regType, dV0, dV1, g_norm);
        calls++;
        if(single_sweep || rc != 1) break;
        lambda_up(O.lambdaFactor, O.lambdaMin, &lambda, &dlambda);  // raise the regularisation and retry
        if(lambda > O.lambdaMax) break;
    }
    const int status = back_status(rc, g_norm, lambda, dlambda, single_sweep, O);
    store_result(P, b, {status, lambda, dlambda, dV0, dV1, g_norm, calls, rc});
}

// ---------------------------------------------------------------------------
// Mode 2 on TWO wavefronts per tile of 64 trajectories ("split"; problems whose header lists the entries bp_derivsL
// writes, no multipliers, constant limits).  65 536 trajectories are one wavefront per SIMD, and that wavefront's step is
// a chain of ~1 265 dependent-ish instructions: the derivative evaluation of step k-1 and the Riccati update of step k
// are independent, and the software pipeline of backward_sweep_fused only lets the scheduler interleave them.  Here the
// PRODUCER wavefront evaluates the record of step k-1 (same generated callbacks, same arithmetic) while the CONSUMER
// wavefront of the same workgroup — on another SIMD of the CU — does step k; the time-varying entries of a record
// (ILQG_TIME_VARYING: 14 of 55 doubles for CarParking), x_k, u_k and a failure flag cross over in LDS, two slots, one
// s_barrier per step.  The consumer fills the constant entries from init_running() as before, so what the optimiser
// folds stays folded.  Control flow is the consumer's: it publishes "some lane still sweeps" / "another sweep" and both
// wavefronts leave their loops together.  Results, memory effects and failure behaviour are those of mode 2.
// MEASURED: no gain — 2.73 ms alone against 2.65 ms for k_backward<2>, headline 130-133 against 135.6 it/s: what bounds
// a step is the chain of dependent operations of the Riccati update with its box QP (~5.3 us), behind which the
// derivative evaluation already hides in ONE instruction stream.  Off by default (option bw_split), kept with its test.
// ---------------------------------------------------------------------------
// (a measured negative result: compiled into the -DILQG_EXPERIMENTS libraries only, lib*_exp.so, which its test loads)
#if defined(ILQG_TIME_VARYING) && !ILQG_STATE_DEPENDENT_LIMITS && ILQG_EXPERIMENTS
#define ILQG_HAVE_SPLIT 1
#define ILQG_COUNT_ENTRY(member, index) +1
constexpr int SPLIT_VARY = 0 ILQG_TIME_VARYING(ILQG_COUNT_ENTRY) ILQG_TIME_VARYING_FULL(ILQG_COUNT_ENTRY);
constexpr int SPLIT_SLOT = SPLIT_VARY + NX + NU + 1;  // + x_k, u_k, failure flag

__global__ __launch_bounds__(2 * WAVE) void k_backward_split(DevPtrs P, ilqg_dev_opts_t O, ParamValues A) {
    __shared__ double ring[2][SPLIT_SLOT][WAVE];
    // the consumer's word: [k & 1] "some lane goes on after step k" (two cells: the producer reads the one of step k+1
    // while the consumer may already write the one of step k), [2] "some lane needs another sweep"
    __shared__ int ctl[3];
    const int role = threadIdx.x >> 6, lane = threadIdx.x & 63;  // 0 consumer, 1 producer
    const int b = blockIdx.x * WAVE + lane;
    const int N = P.N;
    const bool mine = b < P.B && P.i[ILQG_I_STATUS][b] == ILQG_ST_ACTIVE;
    if(__builtin_amdgcn_ballot_w64(mine) == 0ull) return;  // the same for both wavefronts: they hold the same trajectories
    ILQG_CALLBACKS(C, H);
    const size_t xs = cur_xstride(P), us = cur_ustride(P);

    if(role == 1) {
        // ---------------- producer: records of steps N-1, N-2, ..., 0 of every sweep ----------------
        trajEl_t t;
        init_running(&t, &C.o1);
        for(;;) {  // sweeps
            H.nonfinite = 0.0;
            const double *xp = cur_x(P, N - 1, b), *up = cur_u(P, N - 1, b);
            double xn[NX], un[NU];
#pragma unroll
            for(int i = 0; i < NX; i++) xn[i] = xp[i * XSI];
#pragma unroll
            for(int i = 0; i < NU; i++) un[i] = up[i * XSI];
            for(int k = N - 1; k >= 0; k--) {
                // (x, u) of the step after this one, in flight while this record is evaluated
                double xnn[NX], unn[NU];
                const int back = (k > 0) ? 1 : 0;
#pragma unroll
                for(int i = 0; i < NX; i++) xnn[i] = (xp - back * xs)[i * XSI];
#pragma unroll
                for(int i = 0; i < NU; i++) unn[i] = (up - back * us)[i * XSI];
#pragma unroll
                for(int i = 0; i < NX; i++) t.x[i] = xn[i];
#pragma unroll
                for(int i = 0; i < NU; i++) t.u[i] = un[i];
                const int ok = derivs_step(t, nullptr, C, H, k, N, [] {});
                double(*slot)[WAVE] = ring[k & 1];
                int j = 0;
#define ILQG_PUT_ENTRY(member, index) slot[j++][lane] = t.member[index];
                ILQG_TIME_VARYING(ILQG_PUT_ENTRY) ILQG_TIME_VARYING_FULL(ILQG_PUT_ENTRY)
#undef ILQG_PUT_ENTRY
#pragma unroll
                for(int i = 0; i < NX; i++) slot[SPLIT_VARY + i][lane] = xn[i];
#pragma unroll
                for(int i = 0; i < NU; i++) slot[SPLIT_VARY + NX + i][lane] = un[i];
                slot[SPLIT_VARY + NX + NU][lane] = (!ok || H.nonfinite != 0.0) ? 1.0 : 0.0;
                __syncthreads();  // record k is there; the consumer is done with record k+1 (whose slot is written next)
                // The consumer's word on step k+1.  If every lane left there, the consumer has matched the barrier
                // above with one of its own and is on its way to the end of the sweep.
                if(k < N - 1 && !ctl[(k + 1) & 1]) break;
                xp -= back * xs;
                up -= back * us;
#pragma unroll
                for(int i = 0; i < NX; i++) xn[i] = xnn[i];
#pragma unroll
                for(int i = 0; i < NU; i++) un[i] = unn[i];
            }
            // the consumer's last step (0, or the one every lane left at) and its decision about another sweep
            __syncthreads();
            if(!ctl[2]) break;
        }
        return;
    }

    // ---------------- consumer: back_pass + retry loop of k_backward<2>, records from the ring ----------------
    load_penalty_weights_der(C, P, b);
    if(mine) P.i[ILQG_I_NEED_DERIVS][b] = 0;
    // iLQG.c:247-249.  (The status is written at the end: the producer reads it when it starts.)
    const bool dead = mine && P.derivs_failed[b];
    bool sweeping = mine && !dead;  // this lane wants (another) sweep
    double lambda = mine ? P.f[ILQG_F_LAMBDA][b] : 1.0, dlambda = mine ? P.f[ILQG_F_DLAMBDA][b] : 1.0;
    double dV0 = 0.0, dV1 = 0.0, g_norm = mine ? P.f[ILQG_F_GNORM][b] : 0.0;
    int calls = 0, rc = 0;
    const bool took_part = sweeping;
    trajEl_t t;
    init_running(&t, &C.o1);
    for(;;) {  // sweeps of the tile: the lanes that want one take part, the others idle through it
        bool in_sweep = sweeping;
        int result = 0;
        double Vx[NX], Vxx[SXX], l[NU], K[NXU], gsum = 0.0;
        H.nonfinite = 0.0;
        if(in_sweep) {
            const double *xp = cur_x(P, N, b);
            trajFin_t fin;
            init_final(&fin, &C.o);
#pragma unroll
            for(int i = 0; i < NX; i++) fin.x[i] = xp[i * XSI];
            double *recN = nomp(P, N, b);
#pragma unroll
            for(int i = 0; i < NX; i++) recN[NOM_X + i] = fin.x[i];
            const int ok = derivs_final(fin, nullptr, C, H, N);
            if(!ok || H.nonfinite != 0.0) {
                result = 2;
                in_sweep = false;
            }
#pragma unroll
            for(int i = 0; i < NX; i++) Vx[i] = fin.cx[i];
#pragma unroll
            for(int i = 0; i < SXX; i++) Vxx[i] = fin.cxx[i];
        }
#pragma unroll
        for(int i = 0; i < NU; i++) l[i] = 0.0;
        if(sweeping) {  // (a lane that is done keeps the results of ITS last sweep)
            dV0 = 0.0;
            dV1 = 0.0;
        }
        double *rec_k = nomp(P, N - 1, b);
        // gains of the step before (k+1), stored once the record of step k is known to be good — the order of
        // backward_sweep_fused: a failed record of step k ends the sweep before the gains of step k+1 are stored
        double lp[NU], Kp[NXU], xkp[NX], ukp[NU];
        int rcp = 1;
        bool pending = false;
        auto commit = [&]() {  // what backward_sweep_fused does behind record_of(k-1) for step k
            store_gains(lp, Kp, rec_k + NOM_L, rec_k + NOM_K);
#pragma unroll
            for(int i = 0; i < NX; i++) rec_k[NOM_X + i] = xkp[i];
#pragma unroll
            for(int i = 0; i < NU; i++) rec_k[NOM_U + i] = ukp[i];
            rec_k -= RN;
            pending = false;
            if(rcp < 1) {
                result = 1;
                in_sweep = false;
            }
        };
        for(int k = N - 1; k >= 0; k--) {
            __syncthreads();  // record k is in its slot
            if(in_sweep) {
                double(*slot)[WAVE] = ring[k & 1];
                if(slot[SPLIT_VARY + NX + NU][lane] != 0.0) {  // the record of step k failed
                    result = 2;
                    in_sweep = false;
                } else {
                    if(pending) commit();  // step k+1
                    if(in_sweep) {
                        int j = 0;
#define ILQG_GET_ENTRY(member, index) t.member[index] = slot[j++][lane];
                        ILQG_TIME_VARYING(ILQG_GET_ENTRY) ILQG_TIME_VARYING_FULL(ILQG_GET_ENTRY)
#undef ILQG_GET_ENTRY
                        double xk[NX], uk[NU];
#pragma unroll
                        for(int i = 0; i < NX; i++) xk[i] = slot[SPLIT_VARY + i][lane];
#pragma unroll
                        for(int i = 0; i < NU; i++) uk[i] = slot[SPLIT_VARY + NX + i][lane];
#pragma unroll
                        for(int i = 0; i < NX; i++) t.x[i] = xk[i];
#pragma unroll
                        for(int i = 0; i < NU; i++) t.u[i] = uk[i];
                        limitsU(&t, k, C.o.p, N);  // constant limits: parameters only
                        double cur[REC];
#define GETF(off, arr, cnt) _Pragma("unroll") for(int i = 0; i < (cnt); i++) cur[(off) + i] = (arr)[i];
                        REC_COPY(GETF, t)
#undef GETF
                        rcp = back_step<NX, NU, FULL, HX>(cur, uk, Vx, Vxx, l, K, lambda, O.regType, dV0, dV1, gsum, nullptr);
#pragma unroll
                        for(int i = 0; i < NU; i++) lp[i] = l[i];
#pragma unroll
                        for(int i = 0; i < NXU; i++) Kp[i] = K[i];
#pragma unroll
                        for(int i = 0; i < NX; i++) xkp[i] = xk[i];
#pragma unroll
                        for(int i = 0; i < NU; i++) ukp[i] = uk[i];
                        pending = true;
                    }
                }
            }
            const bool more = __builtin_amdgcn_ballot_w64(in_sweep) != 0ull;
            if(lane == 0) ctl[k & 1] = more ? 1 : 0;
            if(!more) {
                if(k > 0) __syncthreads();  // the producer is on its way to this barrier with record k-1: meet it there
                break;
            }
        }
        if(in_sweep && pending) commit();  // step 0 (its record was checked when it arrived)
        if(sweeping) {
            rc = result;
            if(!result) g_norm = gsum / ((double)(N - 1));
            calls++;
            // raise the regularisation and retry
            sweeping = false;
            if(rc == 1) {
                lambda_up(O.lambdaFactor, O.lambdaMin, &lambda, &dlambda);
                sweeping = !(lambda > O.lambdaMax);
            }
        }
        const bool again = __builtin_amdgcn_ballot_w64(sweeping) != 0ull;
        if(lane == 0) ctl[2] = again ? 1 : 0;
        __syncthreads();
        if(!again) break;
    }
    if(dead) P.i[ILQG_I_STATUS][b] = ILQG_ST_DERIVS_FAILED;
    if(took_part) {
        const int status = back_status(rc, g_norm, lambda, dlambda, 0, O);
        store_result(P, b, {status, lambda, dlambda, dV0, dV1, g_norm, calls, rc});
    }
}
#else
#define ILQG_HAVE_SPLIT 0
#endif

// After a backward pass over stored records (modes 0 and 1): the line search's packed records from the tiled
// X, U, l, L.  One wavefront per (tile of 64 trajectories, time step): the tile's RN values per trajectory are read
// as coalesced rows (lane = trajectory), turned through LDS, and written as whole records (16 consecutive lanes =
// one 128-byte record for CarParking) — a lane-per-trajectory write of the records would touch 64 cache lines per
// instruction (measured 8.8 ms for 65 536 x 501 records; this form is bandwidth bound).  Step N holds x_N only.
constexpr int PACK_WAVES = 4, PACK_LD = RN + 1;  // row stride padded by one double: no LDS bank conflicts
__global__ __launch_bounds__(WAVE *PACK_WAVES) void k_pack_records(DevPtrs P) {
    __shared__ double rows[PACK_WAVES][WAVE * PACK_LD];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = blockIdx.x, k = blockIdx.y * PACK_WAVES + w;
    double *row = rows[w];
    const int b = tile * WAVE + lane;
    if(k <= P.N) {
        double v[RN];
#pragma unroll
        for(int i = 0; i < RN; i++) v[i] = 0.0;
        const double *xs = cur_x(P, k, b);
#pragma unroll
        for(int i = 0; i < NX; i++) v[NOM_X + i] = xs[i * XSI];
        if(k < P.N) {
            const double *us = cur_u(P, k, b);
            const double *ls = P.f[ILQG_F_LG] + ix(P, NU, P.N, k, 0, b), *ks = P.f[ILQG_F_KG] + ix(P, NXU, P.N, k, 0, b);
#pragma unroll
            for(int i = 0; i < NU; i++) v[NOM_U + i] = us[i * XSI];
#pragma unroll
            for(int i = 0; i < NU; i++) v[NOM_L + i] = ls[i * SI];
#pragma unroll
            for(int i = 0; i < NXU; i++) v[NOM_K + i] = ks[i * SI];
        }
#pragma unroll
        for(int i = 0; i < RN; i++) row[lane * PACK_LD + i] = v[i];
    }
    __syncthreads();
    if(k <= P.N) {
#pragma unroll
        for(int r = 0; r < RN; r++) {
            const int e = r * WAVE + lane;       // element e of the tile's WAVE x RN values, trajectory-major
            const int tt = e / RN, c = e % RN;
            if(tile * WAVE + tt < P.B) nomp(P, k, tile * WAVE + tt)[c] = row[tt * PACK_LD + c];
        }
    }
}
