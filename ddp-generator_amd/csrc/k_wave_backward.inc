// Wave mapping (one wavefront, or one 16-lane row, = one trajectory): calc_derivs and the backward pass.  Included by
// ilqg_kernels.hip inside its anonymous namespace when ILQG_WAVE_MAP; not a translation unit of its own.
// ---------------------------------------------------------------------------
// wave mapping: calc_derivs straight into the device trajEl_t records, one lane per
// (trajectory of the chunk, time step); step N is the final record
// ---------------------------------------------------------------------------
// Factored records use the head of trajEl_t (x .. fu and the NBASIS products at the start of fxx) and its tail (the
// members behind fxu: the auxiliaries) — the 38 KB of tensors in between are never touched.  Such records are laid
// down OVERLAPPING, FACT_STRIDE < sizeof(trajEl_t) apart, the head of one record inside the unused middle of an
// earlier one: the smallest distance at which no head (offsets [0, A) modulo the distance) meets a tail (offsets
// [TAIL mod distance, + T)).  4x as many trajectories per chunk of the work buffer for the n = 16 problem
// (11 992 instead of 47 944 bytes per step).  Only when init_running() stores nothing in the tensors (generator
// hint ILQG_TENSOR_INIT_WRITES).
#if ILQG_FACTORED && defined(ILQG_TENSOR_INIT_WRITES) && !ILQG_TENSOR_INIT_WRITES
constexpr size_t fact_stride() {
    const size_t A = offsetof(trajEl_t, fxx) + NBASIS * sizeof(double);
    const size_t TAIL = offsetof(trajEl_t, fxu) + sizeof(double) * NX * NXU, T = sizeof(trajEl_t) - TAIL;
    constexpr size_t AL = 128;  // whole cache lines (measured against 8: k_derivs_wave 116 -> 113 ms per iteration)
    if(T == 0) return (A + AL - 1) / AL * AL;
    for(size_t S = (A + T + AL - 1) / AL * AL; S < sizeof(trajEl_t); S += AL) {
        const size_t r = TAIL % S;
        if(r >= A && r + T <= S) return S;
    }
    return sizeof(trajEl_t);
}
constexpr size_t FACT_STRIDE = fact_stride();
#else
constexpr size_t FACT_STRIDE = sizeof(trajEl_t);
#endif
// distance between the records a derivative kernel writes for the backward kernel of the same call (the shared work buffer).
// Where whole runs of entries are written out from LDS (ILQG_DEV_EL), 512-byte pieces cut at multiples of 64 entries: records
// that start on multiples of 512 bytes make every such store four whole cache lines.
#if ILQG_DEV_EL
constexpr size_t STORED_STRIDE = (sizeof(trajEl_t) + 511) / 512 * 512;
#else
constexpr size_t STORED_STRIDE = sizeof(trajEl_t);
#endif
__device__ __forceinline__ trajEl_t *work_rec(const DevPtrs &P, int bw, int k) {
    return reinterpret_cast<trajEl_t *>(reinterpret_cast<char *>(P.work) + ((size_t)bw * P.N + k) * P.work_stride);
}

// factored: the first-order part of the record and, in place of the tensors, the products they are multiples of
// (NBASIS doubles at the start of the record's fxx member)
// (workgroups of four wavefronts: 105 against 112 ms per iteration of config 5 with one; 16: 128 registers, 165 ms)
#ifndef ILQG_DERIVS_BLOCK
#define ILQG_DERIVS_BLOCK 256
#endif
#if ILQG_DEV_EL
static_assert(ILQG_DERIVS_BLOCK == 64 * ilqgdev::WAVES, "ilqgdev's ring is that of ONE wavefront per workgroup");
#endif
constexpr size_t DERIVS_DYN_LDS = 0;
#if ILQG_STAGED_RECORDS
// runs of staged entries may cross from one member into the next (tools/gen_problem.py record_offsets(): the layout of
// iLQG_problem.tem:23-51)
static_assert(offsetof(trajEl_t, cxx) == offsetof(trajEl_t, cx) + sizeof(double) * NX && offsetof(trajEl_t, cu) == offsetof(trajEl_t, cxx) + sizeof(double) * SXX &&
                  offsetof(trajEl_t, cuu) == offsetof(trajEl_t, cu) + sizeof(double) * NU && offsetof(trajEl_t, cxu) == offsetof(trajEl_t, cuu) + sizeof(double) * SUU &&
                  offsetof(trajEl_t, fx) == offsetof(trajEl_t, cxu) + sizeof(double) * NXU && offsetof(trajEl_t, fu) == offsetof(trajEl_t, fx) + sizeof(double) * NX * NX,
              "cx, cxx, cu, cuu, cxu, fx, fu lie one behind the other");
#endif
// the general record (tensors stored): a function of its own, so that k_derivs_wave can take everything else inline
__device__ __attribute__((noinline)) static int derivs_with_tensors(el_t *t, int k, double **p) { return bp_derivsL(t, k, p); }
#if ILQG_DEV_EL
// a plain member of the private element into its place in the lanes' records, through the ring (runs cut at multiples of 64 entries)
template <int COUNT>
__device__ __forceinline__ void stage_member(int m, unsigned first, const double (&src)[COUNT]) {
    unsigned run = first;
#pragma unroll 1
    for(int i = 0; i < COUNT; i++) {
        const unsigned e = first + (unsigned)i;
        ilqgdev::slot(e) = src[i];
        if(i + 1 == COUNT || ((e + 1) & 63u) == 0u) {
            ilqgdev::flush(m, run, (int)(e + 1 - run));
            run = e + 1;
        }
    }
}
#endif

// FACT: the records the factored backward step reads (first-order part + the products).  That instantiation takes every
// generated function inline: nothing of the callbacks' surroundings (the parameter table, the parameter values, the
// hooks) has its address passed on, all of it dissolves into registers — the parameters into scalar ones.  While one
// function stayed a call (the general record's bp_derivsL, now in the other instantiation) they lived in scratch memory
// and every parameter the derivatives multiply by was a scratch load with a wait of its own in its own basic block
// (the wave-uniform guards end a block at every assignment): 20 memory round trips in front of the first 64 entries
// of fx alone, 100 000 of a wavefront's 290 000 cycles.
template <bool FACT>
__global__ __launch_bounds__(ILQG_DERIVS_BLOCK) void k_derivs_wave(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int chunk_first, int chunk_count,
                                                                  int init_consts, int limit_gradients, int final_only) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // (final_only: lane = trajectory, the final record alone — the steps' records come from k_derivs_parts)
    const int bw = final_only ? (int)tid : (int)(tid / (P.N + 1));
    const int k = final_only ? P.N : (int)(tid % (P.N + 1));
    const int b = chunk_first + bw;
    const bool inside = bw < chunk_count && b < P.B;
    // FACT: the problem's fixed-size parameters in LDS, one copy for the workgroup.  As a private copy they become scalar
    // registers once everything is inline — 45 doubles, 90 of 104 registers, for the n = 16 problem: spilled through
    // vector lanes that are spilled themselves.  A parameter read is then one LDS read of one address by all lanes.
    // (the same where the callbacks work on a private element with proxies, ILQG_DEV_EL: everything inline there as well)
    constexpr bool LDS_PARAMS = FACT || ILQG_DEV_EL;
    __shared__ double s_params[LDS_PARAMS && ILQG_PTOTAL > 0 ? ILQG_PTOTAL : 1];
    if constexpr(LDS_PARAMS) {
        for(int i = threadIdx.x; i < ILQG_PTOTAL; i += blockDim.x) s_params[i] = A.v[i];
        __syncthreads();
    }
    if(!any_lane(inside)) return;
    ILQG_CALLBACKS(C, H);
    if constexpr(LDS_PARAMS) {
        constexpr int sizes[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
        constexpr int offs[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_POFFSETS;
#pragma unroll
        for(int i = 0; i < ILQG_NP; i++)
            if(sizes[i] > 0) C_table.ptr[i] = &s_params[offs[i]];
    }
    if(!limit_gradients) H.limgrad = 0.0;  // (records only the backward pass reads: see ILQG_LIMIT_GRADIENTS_WANTED)
    tOptSet &o = C.o;
    // constant entries, once per buffer (init_opt, iLQG_func.tem:402-415) — of EVERY record of the chunk: the slot of a
    // trajectory that is finished serves another one in a later chunk
#if ILQG_DEV_EL
    // (the callbacks' assignments to derivative entries are collected in LDS and written out by the WAVEFRONT: every lane goes
    // through them, one without a record of its own as a copy of the first lane that has one — see below)
    // The element itself is `own`, for everything this lane does: what init_running() assigns to PLAIN members — auxiliaries
    // that are constants (iLQG_func.tem:316-318) — has to be there when the callbacks of the step run, so init_running() runs
    // on it at EVERY launch; its assignments to derivative entries go to the records when the buffer does not hold them yet
    // (init_consts) and nowhere otherwise.
    el_t own;
    {
        const bool has_rec = inside && k < P.N;
        const unsigned long long with_rec = __builtin_amdgcn_ballot_w64(has_rec);
        if(init_consts && with_rec != 0ull) {
            const int src = (int)__builtin_ctzll(with_rec);
            const int bw_i = has_rec ? bw : __builtin_amdgcn_readlane(bw, src), k_i = has_rec ? k : __builtin_amdgcn_readlane(k, src);
            ilqgdev::set_record(work_rec(P, bw_i, k_i));
            ilqgdev::set_mode(ilqgdev::TOGETHER);
        } else {
            ilqgdev::set_mode(ilqgdev::DISCARD);
        }
        [[clang::always_inline]] init_running(&own, &C.o1);
    }
#else
    if(init_consts && inside && k < P.N) [[clang::always_inline]] init_running(work_rec(P, bw, k), &C.o1);
#endif
    const bool live = inside && P.i[ILQG_I_STATUS][inside ? b : chunk_first] == ILQG_ST_ACTIVE;
    // The step records.  Runs of their entries are collected in LDS and written out by the whole wavefront
    // (ilqg_stage_flush): every lane goes through the callbacks — one without a step of its own (beyond the chunk, a
    // finished trajectory, the final record's lane) as a copy of the first lane that has one: the same record, the same
    // values, stored twice.
    const bool has_step = live && k < P.N;
    const unsigned long long with_step = __builtin_amdgcn_ballot_w64(has_step);
    int ok = 1;
    if(with_step != 0ull) {
        const int src = (int)__builtin_ctzll(with_step);
        const int bw_s = has_step ? bw : __builtin_amdgcn_readlane(bw, src);
        const int k_s = has_step ? k : __builtin_amdgcn_readlane(k, src);
        const int b_s = chunk_first + bw_s;
        load_penalty_weights_der(C, P, b_s);
        multipliersEl_t mk;
        load_mul(P, k_s, b_s, mk);
        multipliersEl_t *const mp = HAS_MUL ? &mk : nullptr;
        trajEl_t *const rec = work_rec(P, bw_s, k_s);
        H.record = reinterpret_cast<double *>(rec);
        // FACT (everything inline): the element the callbacks work on is a PRIVATE one — x, u, the auxiliaries are
        // registers, nothing of them is stored — and the record in HBM gets what the backward step reads: the staged runs
        // (by the callbacks themselves), the limits (staged here) and the entries assigned outside the runs.
#if ILQG_STAGED_RECORDS && defined(ILQG_REC_DIRECT)
        // (limits that depend on the state: limitsU() also stores their signs and gradients, which the row-mapped step
        // reads from the record — the callbacks then work on the record itself, as in the general instantiation)
        constexpr bool OWN = FACT && !HX;
#else
        constexpr bool OWN = false;  // (a function file without the staging macros stores into the record itself)
#endif
#if ILQG_DEV_EL
        static_assert(!FACT, "a pair with factored tensor tables carries the staging macros itself");
        el_t *const t = &own;  // x, u, the limits, the auxiliaries; the derivative members are proxies (ilqg_kernels.hip, ilqgdev)
        ilqgdev::set_record(rec);
#else
        trajEl_t own;
        trajEl_t *const t = OWN ? &own : rec;
#endif
        auto body = [&]() {
#if ILQG_DEV_EL
            ilqgdev::set_mode(H.alone != 0.0 ? ilqgdev::ALONE : ilqgdev::TOGETHER);
#endif
            ILQG_DPROBE(0);
            for(int i = 0; i < NX; i++) t->x[i] = nomp(P, k_s, b_s)[NOM_X + i];
            for(int i = 0; i < NU; i++) t->u[i] = nomp(P, k_s, b_s)[NOM_U + i];
            ILQG_DPROBE();
            ok = 1;
            [[clang::always_inline]] ok = calcXVariableAux(t, mp, k_s, &o);
            ILQG_DPROBE();
            [[clang::always_inline]] ok &= calcXUVariableAux(t, mp, k_s, &o);
            ILQG_DPROBE();
            [[clang::always_inline]] ok &= calcLAuxDeriv(t, mp, k_s, &o);
            ILQG_DPROBE();
#if ILQG_FACTORED
            if constexpr(FACT) {
                // (the two as ONE generated function, so that the products share the first derivatives' 32 sin / cos
                // evaluations, was measured twice: all shared products first, 105 -> 169 ms; statements grouped by the
                // sin / cos they use, 83 -> 141 ms)
                // (the products first: both functions begin with the sines and cosines of the auxiliaries, evaluated once
                // for the two — by the one that runs first; behind the first derivatives, the 64 values would have to
                // stay alive through their 400 assignments: 110 registers spilled)
                [[clang::always_inline]] ok &= bp_tensor_basis(t->fxx, t, k_s, o.p);
                ILQG_DPROBE();
                [[clang::always_inline]] ok &= bp_derivsL_first(t, k_s, o.p);
                ILQG_DPROBE();
            } else
#endif
#if ILQG_DEV_EL
                // (inline: x, u, the auxiliaries and the parameters are registers / LDS then.  As a call, the function reads them
                // from scratch memory in between its stores — and a load, waited for, waits for every store issued before it:
                // 550 such round trips per wavefront were 1.1 of its 1.26 ms, profiles/r6_stored_path.txt)
                [[clang::always_inline]] ok &= bp_derivsL(t, k_s, o.p);
#else
                ok &= derivs_with_tensors(t, k_s, o.p);
#endif
            // (the limits — which re-read u behind the 400 stores of the derivatives — moved in front of them, and the
            // products in front of the first derivatives: measured, no difference)
            [[clang::always_inline]] limitsU(t, k_s, o.p, P.N);
#if ILQG_DEV_EL
            {  // the limits (and, where somebody reads them, their signs and gradients) from the private element into the record
                const int m = H.alone != 0.0 ? ilqgdev::ALONE : ilqgdev::TOGETHER;
                stage_member(m, (unsigned)(offsetof(trajEl_t, lower) / sizeof(double)), own.lower);
                stage_member(m, (unsigned)(offsetof(trajEl_t, upper) / sizeof(double)), own.upper);
                if(limit_gradients) {
                    stage_member(m, (unsigned)(offsetof(trajEl_t, lower_sign) / sizeof(double)), own.lower_sign);
                    stage_member(m, (unsigned)(offsetof(trajEl_t, upper_sign) / sizeof(double)), own.upper_sign);
                    stage_member(m, (unsigned)(offsetof(trajEl_t, lower_hx) / sizeof(double)), own.lower_hx);
                    stage_member(m, (unsigned)(offsetof(trajEl_t, upper_hx) / sizeof(double)), own.upper_hx);
                }
            }
#endif
#if ILQG_STAGED_RECORDS && defined(ILQG_REC_DIRECT)
            if constexpr(OWN) {
                static_assert(offsetof(trajEl_t, upper) == offsetof(trajEl_t, lower) + NU * sizeof(double) && NU <= 32, "lower and upper limits: one run");
                double **const p = o.p;
#pragma unroll
                for(int i = 0; i < NU; i++) {
                    ILQG_REC(lower, i) = t->lower[i];
                    ILQG_REC(upper, i) = t->upper[i];
                }
                ILQG_REC_DONE(lower, 0, 2 * NU)
#define ILQG_COPY_ENTRY(member, index) rec->member[index] = t->member[index];
                ILQG_REC_DIRECT(ILQG_COPY_ENTRY)
#undef ILQG_COPY_ENTRY
            }
#endif
            ILQG_DPROBE();
        };
#if ILQG_UNIFORM_GUARDS
        ok = run_guarded([&]() { body(); return ok; }, &H.alone);
        H.alone = 0.0;
#else
        body();
        if(H.huge != 0.0) {  // an argument beyond the fast sin/cos reduction: once more through the library
            H.nonfinite = 0.0;
            H.slow = 1.0;
            H.alone = 1.0;  // (some lanes only: each writes its own staged entries)
            body();
            H.slow = 0.0;
            H.alone = 0.0;
        }
#endif
        if(!has_step) {  // a copy's verdict is its original's
            ok = 1;
            H.nonfinite = 0.0;
        }
    }
    if(live && k == P.N) {
        load_penalty_weights_der(C, P, b);
        H.huge = 0.0;
        trajFin_t fin;
        multipliersFin_t mfin;
        load_mul_fin(P, b, mfin);
        multipliersFin_t *const mfp = HAS_MUL ? &mfin : nullptr;
        [[clang::always_inline]] init_final(&fin, &o);
        auto body = [&]() {
            for(int i = 0; i < NX; i++) fin.x[i] = nomp(P, P.N, b)[NOM_X + i];
            [[clang::always_inline]] ok = calcFVariableAux(&fin, mfp, &o);
            [[clang::always_inline]] ok &= calcFAuxDeriv(&fin, mfp, &o);
            [[clang::always_inline]] ok &= bp_derivsF(&fin, P.N, o.p);
        };
#if ILQG_UNIFORM_GUARDS
        ok = run_guarded([&]() { body(); return ok; });
#else
        body();
        if(H.huge != 0.0) {
            H.nonfinite = 0.0;
            H.slow = 1.0;
            body();
        }
#endif
        double *out = P.f[ILQG_F_FIN] + (size_t)b * FIN;
        for(int i = 0; i < NX; i++) out[i] = fin.cx[i];
        for(int i = 0; i < SXX; i++) out[NX + i] = fin.cxx[i];
    }
    if(live && (!ok || H.nonfinite != 0.0)) P.derivs_failed[b] = 1;
}

// ---------------------------------------------------------------------------
// The time-varying part of the factored derivative records, assembled ON CHIP and written as whole cache lines (round 4).
// k_derivs_wave runs the generated scalar code on a struct per lane in HBM: every store instruction touches 64 records,
// the kernel spends most of its time waiting for stores (SQ_WAIT_ANY / SQ_WAVE_CYCLES 0.55, 116 GB written for 72 GB of
// payload) and evaluates the 64 sin / cos of a step twice (bp_derivsL_first, bp_tensor_basis).  Here a lane still owns a
// (trajectory, step), but the generated file offers the record's entries in PARTS of 16 outputs (tools/gen_problem.py
// _emit_deriv_parts: the expressions of bp_derivsL_first, bp_tensor_basis and limitsU as the same printer prints them;
// ilqg_deriv_prepare evaluates the auxiliaries, every sin / cos ONCE and the products made of them): a part's outputs go into a tile in LDS,
// [lane][16], and come out of it turned round — 16 consecutive lanes store the 16 outputs of ONE record: a whole line
// wherever the outputs are neighbours in the record (fx and fu column by column, cx, cu, the products, the limits).
// The constant entries of the records are written once per buffer by k_derivs_wave as before, the final record too.
//
// MEASURED (round 4, config 5): 51.3 ms per iteration against 43.8 for k_derivs_wave — a negative result so far, and why:
// the parts' arithmetic is a few thousand 64-bit literals.  As ONE block (parts unrolled) they are all materialised ahead
// (788 scalar registers spilled through vector lanes, 447 vector registers spilled); as a loop over a switch the
// optimiser first flattens the cheap side-effect-free cases into selects, then — with a statement at the head of every
// case that stops that — hoists the loop-invariant arithmetic of all 30 parts in front of the loop, then — with the inputs
// laundered in every trip — still holds ilqg_deriv_prepare's 32 auxiliaries + 64 sin / cos values + 64 products at
// once whatever order the generator prints them in: 360 vector registers spilled, 1.5 KB of scratch per lane, whose
// traffic is what the coalesced record stores had saved.  Called instead of inlined, a part's inputs and outputs travel
// through the caller's frame (68 ms).  What it would take: the auxiliaries and their products in a kernel of their own
// (lane = (step, auxiliary pair)) handing 64 + 32 doubles per step over in HBM or LDS.  The kernel is kept, tested
// (test_derivative_records_in_parts_equal_the_per_lane_ones) and off by default (ILQG_DERIV_PARTS=1 turns it on).
// ---------------------------------------------------------------------------
// (compiled into the -DILQG_EXPERIMENTS libraries only, lib*_exp.so, which its test loads)
#if ILQG_FACTORED && defined(ILQG_DERIV_PARTS) && ILQG_EXPERIMENTS
#define ILQG_HAVE_DERIV_PARTS 1
constexpr int DP_OUT = ILQG_DERIV_PART_OUT, DP_PARTS = ILQG_DERIV_PARTS, DP_NOUT = ILQG_DERIV_NOUT, DP_NPROD = ILQG_DERIV_NPROD;
static_assert(DP_OUT == 16, "a part's outputs are stored by the 16 lanes of a DPP row");
#define ILQG_OUT_OFFSET(member, index) (unsigned)(offsetof(trajEl_t, member) + (index) * sizeof(double)),
__device__ const unsigned deriv_out_offset[DP_PARTS * DP_OUT] = {ILQG_DERIV_OUTPUTS(ILQG_OUT_OFFSET)};
#undef ILQG_OUT_OFFSET
constexpr int DP_WAVES = 4;

__global__ __launch_bounds__(64 * DP_WAVES) void k_derivs_parts(DevPtrs P, ilqg_dev_opts_t O, ParamValues A, int chunk_first, int chunk_count) {
    __shared__ double tile[DP_WAVES][WAVE][DP_OUT + 1];  // (+1: the lanes' rows start on different banks)
    __shared__ unsigned long long recs[DP_WAVES][WAVE];  // the records of the wavefront's lanes (0: not to be written)
    __shared__ unsigned offs[DP_PARTS * DP_OUT];         // byte offset of every output in a record
    for(int i = threadIdx.x; i < DP_PARTS * DP_OUT; i += 64 * DP_WAVES) offs[i] = deriv_out_offset[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int bw = (int)(tid / P.N), k = (int)(tid % P.N);
    const int b = chunk_first + bw;
    const bool live = bw < chunk_count && b < P.B && P.i[ILQG_I_STATUS][(b < P.B) ? b : 0] == ILQG_ST_ACTIVE;
    if(__builtin_amdgcn_ballot_w64(live) == 0ull) return;
    ILQG_CALLBACKS(C, H);
    const double *nom = nomp(P, k, live ? b : chunk_first);
    double x[NX], u[NU];
#pragma unroll
    for(int i = 0; i < NX; i++) x[i] = nom[NOM_X + i];
#pragma unroll
    for(int i = 0; i < NU; i++) u[i] = nom[NOM_U + i];
    ilqg_deriv_aux_t aux;
    double prod[DP_NPROD], basis[NBASIS];
    int bad = 0;
    H.huge = 0.0;
    ilqg_deriv_prepare(&aux, prod, basis, &bad, x, u, k, C.o.p, P.N);
    if(H.huge != 0.0) {  // an argument beyond the fast sin / cos reduction: once more through the library
        H.slow = 1.0;
        bad = 0;
        ilqg_deriv_prepare(&aux, prod, basis, &bad, x, u, k, C.o.p, P.N);
        H.slow = 0.0;
    }
    recs[wave][lane] = live ? (unsigned long long)work_rec(P, bw, k) : 0ull;
    const int pr0 = lane >> 4, j = lane & 15;
    // (a LOOP over the parts, not unrolled: the parts' hundreds of 64-bit literals stay with their case of the switch; laid out
    // as one block they are all materialised ahead — 788 scalar registers spilled through vector lanes)
    const int nparts = DP_PARTS;
#pragma unroll 1
    for(int q = 0; q < nparts; q++) {
        // (every part's arithmetic is loop invariant — it depends on the step, not on q — and would be hoisted in front of
        // the loop, all 472 outputs at once; its inputs pass through a statement the optimiser cannot see through)
#pragma unroll
        for(int i = 0; i < NX; i++) asm volatile("" : "+v"(x[i]));
#pragma unroll
        for(int i = 0; i < NU; i++) asm volatile("" : "+v"(u[i]));
#pragma unroll
        for(int i = 0; i < DP_NPROD; i++) asm volatile("" : "+v"(prod[i]));
#pragma unroll
        for(int i = 0; i < NBASIS; i++) asm volatile("" : "+v"(basis[i]));
        double out[DP_OUT];
#pragma unroll
        for(int i = 0; i < DP_OUT; i++) out[i] = 0.0;
        ilqg_deriv_part(q, out, &bad, &aux, prod, basis, x, u, k, C.o.p, P.N);

#pragma unroll
        for(int i = 0; i < DP_OUT; i++) tile[wave][lane][i] = out[i];
        wave_sync();
        if(q * DP_OUT + j < DP_NOUT) {
            const unsigned off = offs[q * DP_OUT + j];
#pragma unroll
            for(int i = 0; i < WAVE / 4; i++) {
                const int pr = 4 * i + pr0;
                const unsigned long long base = recs[wave][pr];
                if(base) *reinterpret_cast<double *>(base + off) = tile[wave][pr][j];
            }
        }
        wave_sync();
    }
    if(live && bad) P.derivs_failed[b] = 1;
}
#else
#define ILQG_HAVE_DERIV_PARTS 0
#endif

using StepLds = std::conditional_t<ROW_STEP, RowLds<(ROW_STEP ? NX : 1), (ROW_STEP ? NU : 1)>, WaveLds<NX, NU>>;

// byte offsets of the members of a step's record (trajEl_t) the row-mapped backward step reads
struct RecOffsets {
    static constexpr unsigned cx = offsetof(trajEl_t, cx), cxx = offsetof(trajEl_t, cxx), cu = offsetof(trajEl_t, cu),
                              cuu = offsetof(trajEl_t, cuu), cxu = offsetof(trajEl_t, cxu), fx = offsetof(trajEl_t, fx),
                              fu = offsetof(trajEl_t, fu), lower = offsetof(trajEl_t, lower), upper = offsetof(trajEl_t, upper),
                              lower_sign = offsetof(trajEl_t, lower_sign), upper_sign = offsetof(trajEl_t, upper_sign),
                              lower_hx = offsetof(trajEl_t, lower_hx), upper_hx = offsetof(trajEl_t, upper_hx);
#if FULL_DDP
    static constexpr unsigned fxx = offsetof(trajEl_t, fxx), fuu = offsetof(trajEl_t, fuu), fxu = offsetof(trajEl_t, fxu);
#endif
};

#if ILQG_FACTORED
// The step's record with the tensors multiplied out on the fly: coefficient tables (an LDS copy of the generated
// ilqg_tensor_coef_*, shared by the workgroup) times the products bp_tensor_basis left in the record.  The LDS copy
// is slice-major, [slice][xx | uu | xu], so that what a lane reads of a slice sits within a few hundred bytes: ONE
// address register (table + 8 * lane) serves the whole contraction, the rest is immediate offsets.  A lane beyond
// the end of an array reads its neighbour's (or the next slice's) numbers; those sums are never used.
constexpr int FACT_SLICE = SXX + SUU + NXU;  // doubles per slice
struct FactoredSource : RecordSource<NX, NU, true, RecOffsets> {
    unsigned table;  // LDS address of the coefficient tables
    unsigned basis;  // LDS address of 64 doubles of this wavefront: the step's products, for all lanes to read
    double product;  // lane i: product i of this step (bp_tensor_basis)
    ILQG_DEV void contract(const double vxl, double (&dxx)[NTX], double (&duu)[NTU], double (&dxu)[NTC], const int lane) const {
        constexpr int PER = NTX + NTU + NTC;
        // The products every lane multiplies by are wave-uniform numbers held one per lane.  Through LDS (one store,
        // then reads of one address by all lanes) they cost no vector instruction; two v_readlane each otherwise.
        lds_base(basis + lane * 8)[0] = product;
        wave_sync();
        const LdsBase p = lds_base(table + lane * 8), pg = lds_base(basis);
        // what this lane multiplies of slice i: its entries of xx, uu, xu and the three products
        auto fetch = [&](auto ic, double (&t)[PER], double (&g)[3]) {
            constexpr int i = decltype(ic)::value;
#pragma unroll
            for(int q = 0; q < NTX; q++) t[q] = p.fetch(i * FACT_SLICE + 64 * q);
#pragma unroll
            for(int q = 0; q < NTU; q++) t[NTX + q] = p.fetch(i * FACT_SLICE + SXX + 64 * q);
#pragma unroll
            for(int q = 0; q < NTC; q++) t[NTX + NTU + q] = p.fetch(i * FACT_SLICE + SXX + SUU + 64 * q);
            // (entries of constant tables: folded when the loop is unrolled, as are the comparisons below)
            const int sxx = ilqg_tensor_slice_xx[i], suu = ilqg_tensor_slice_uu[i], sxu = ilqg_tensor_slice_xu[i];
            g[0] = pg.fetch(sxx);
            g[1] = (suu == sxx) ? g[0] : pg.fetch(suu);
            g[2] = (sxu == sxx) ? g[0] : ((sxu == suu) ? g[1] : pg.fetch(sxu));
        };
        double cur[PER], nxt[PER], gc[3], gn[3];
        fetch(std::integral_constant<int, 0>{}, cur, gc);
        static_for<0, NX>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if constexpr(i + 1 < NX) fetch(std::integral_constant<int, i + 1>{}, nxt, gn);  // (in flight during this slice's arithmetic)
            // d += Vx[i] * (coefficient * product), Vx[i] broadcast from lane i of the row
#pragma unroll
            for(int q = 0; q < NTC; q++) row_fma<i>(dxu[q], vxl, cur[NTX + NTU + q] * gc[2]);
#pragma unroll
            for(int q = 0; q < NTU; q++) row_fma<i>(duu[q], vxl, cur[NTX + q] * gc[1]);
#pragma unroll
            for(int q = 0; q < NTX; q++) row_fma<i>(dxx[q], vxl, cur[q] * gc[0]);
#pragma unroll
            for(int q = 0; q < PER; q++) cur[q] = nxt[q];
#pragma unroll
            for(int q = 0; q < 3; q++) gc[q] = gn[q];
        });
    }
};
constexpr int TABLE_DOUBLES = NX * FACT_SLICE;
#else
constexpr int TABLE_DOUBLES = 0;
#endif
constexpr int WAVE_LDS_DOUBLES = (int)((sizeof(StepLds) + 7) / 8);  // LDS of one wavefront

// one backward step in the form that goes with the LDS block (a template, so that only that form is instantiated)
template <bool FACT, class Lds>
__device__ __forceinline__ int step_of_wave(Lds &S, const double *tables, double product, const trajEl_t *t, const double *u_nom,
                                            const StepFields<NX, NU> &F, double *lout,
                                            double *Kout, double lambda, int regType, double &dV0, double &dV1, double &gsum,
                                            Prof *pf) {
    if constexpr(std::is_same<Lds, WaveLds<NX, NU>>::value) {
        return back_step_wave<NX, NU, FULL, HX>(S, F, lout, Kout, lambda, regType, dV0, dV1, gsum, pf);
    } else if constexpr(FACT) {
#if ILQG_FACTORED
        FactoredSource D;
        D.rec = reinterpret_cast<const char *>(t);
        D.table = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr(tables));
        D.basis = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr(S.basis));
        D.product = product;
        return back_step_row<NX, NU, FULL, HX>(S, D, u_nom, lout, Kout, lambda, regType, dV0, dV1, gsum, pf);
#else
        return 0;
#endif
    } else {
        const RecordSource<NX, NU, FULL, RecOffsets> D{reinterpret_cast<const char *>(t)};
        return back_step_row<NX, NU, FULL, HX>(S, D, u_nom, lout, Kout, lambda, regType, dV0, dV1, gsum, pf);
    }
}

// the value function behind the last step (Vx, packed Vxx of the final cost) into the LDS block, in the block's form
template <int A, int B>
__device__ __forceinline__ void set_final_value(RowLds<A, B> &S, const double *vx, const double *vxx, int lane) { S.set_value(vx, vxx, lane); }
template <int A, int B>
__device__ __forceinline__ void set_final_value(WaveLds<A, B> &S, const double *vx, const double *vxx, int lane) {
    for(int i = lane; i < A; i += 64) S.Vx[i] = vx[i];
    for(int i = lane; i < tri(A); i += 64) S.Vxx[i] = vxx[i];
}

// one sweep of one trajectory on one wave; returns 0 ok, 1 box-QP failed (wave-uniform)
template <bool FACT>
__device__ __forceinline__ int backward_sweep_wave(StepLds &S, const double *tables, const DevPtrs &P, int b, int bw, double lambda,
                                                   int regType, double &dV0, double &dV1, double &g_norm) {
    const int lane = threadIdx.x & 63;
    const int N = P.N;
    const double *fin = P.f[ILQG_F_FIN] + (size_t)b * FIN;
    set_final_value(S, fin, fin + NX, lane);
    for(int i = lane; i < NU; i += 64) S.l[i] = 0.0;
    wave_sync();
    dV0 = 0.0;
    dV1 = 0.0;
    double gsum = 0.0;
#ifdef ILQG_PROFILE_SECTIONS
    Prof prof;
    prof.start();
    Prof *pf = &prof;
#else
    Prof *pf = nullptr;
#endif
    auto fields = [&](int k) {
        const trajEl_t *t = work_rec(P, bw, k);
        StepFields<NX, NU> F;
        F.cx = t->cx; F.cxx = t->cxx; F.cu = t->cu; F.cuu = t->cuu; F.cxu = t->cxu;
        F.fx = t->fx; F.fu = t->fu; F.lower = t->lower; F.upper = t->upper;
#if FULL_DDP
        F.fxx = t->fxx; F.fuu = t->fuu; F.fxu = t->fxu;
#else
        F.fxx = F.fuu = F.fxu = nullptr;
#endif
        F.lower_sign = t->lower_sign; F.upper_sign = t->upper_sign;
        F.lower_hx = t->lower_hx; F.upper_hx = t->upper_hx;
        F.u = nomp(P, k, b) + NOM_U;
        return F;
    };
    // factored records: lane i holds product i of the step (the one of step k-1 is requested at the start of step k)
    const int bl = (lane < NBASIS) ? lane : 0;
    double product = 0.0;
    if(FACT) product = fields(N - 1).fxx[bl];
    int failed = 0;
    for(int k = N - 1; k >= 0; k--) {
        if(pf) pf->probe(0);
        const StepFields<NX, NU> F = fields(k);
        double next_product = 0.0;
        if(FACT && k > 0) next_product = fields(k - 1).fxx[bl];
        const int rc = step_of_wave<FACT>(S, tables, product, work_rec(P, bw, k), nomp(P, k, b) + NOM_U, F, nomp(P, k, b) + NOM_L,
                                         nomp(P, k, b) + NOM_K, lambda, regType, dV0, dV1, gsum, pf);
#ifdef ILQG_PROFILE_SECTIONS
        prof.acc[7]++;  // steps executed (sweeps that are abandoned half way count with the steps they ran)
#endif
        if(BOXQP_FAILED(rc)) {
            failed = 1;
            break;
        }
        product = next_product;
    }
#ifdef ILQG_PROFILE_SECTIONS
    if(lane == 0)
        for(int i = 0; i < 8; i++) atomicAdd(&ilqg_prof_cycles[i], (unsigned long long)prof.acc[i]);
#endif
    if(failed) return 1;
    g_norm = gsum / ((double)(N - 1));
    return 0;
}

// back_pass + retry loop, one wavefront (= one block) per trajectory of the chunk.  single_sweep: 1 = the
// drop-in back_pass() (caller owns the retry loop)
// FACT: factored records (see FactoredSource); ILQG_FACT_WAVES wavefronts per workgroup share the coefficient tables
// back_pass + retry loop of ONE trajectory (b; slot bw of the chunk's records) on the calling wavefront
template <bool FACT>
__device__ __forceinline__ void backward_of_trajectory(StepLds &S, const double *tables, const DevPtrs &P, const ilqg_dev_opts_t &O,
                                                       int single_sweep, int b, int bw) {
    const int lane = threadIdx.x & 63;
    if(P.i[ILQG_I_STATUS][b] != ILQG_ST_ACTIVE) return;
    if(P.derivs_failed[b]) {
        if(lane == 0) {
            P.i[ILQG_I_NEED_DERIVS][b] = 0;
            P.i[ILQG_I_STATUS][b] = ILQG_ST_DERIVS_FAILED;
        }
        return;
    }
    double lambda = P.f[ILQG_F_LAMBDA][b], dlambda = P.f[ILQG_F_DLAMBDA][b];
    double dV0 = 0.0, dV1 = 0.0, g_norm = P.f[ILQG_F_GNORM][b];
    int calls = 0, rc;
    for(;;) {
        rc = backward_sweep_wave<FACT>(S, tables, P, b, bw, lambda, O.regType, dV0, dV1, g_norm);
        calls++;
        if(single_sweep || rc != 1) break;
        lambda_up(O.lambdaFactor, O.lambdaMin, &lambda, &dlambda);
        if(lambda > O.lambdaMax) break;
        wave_sync();
    }
    const int status = back_status(rc, g_norm, lambda, dlambda, single_sweep, O);
    if(lane == 0) {
        P.i[ILQG_I_NEED_DERIVS][b] = 0;
        store_result(P, b, {status, lambda, dlambda, dV0, dV1, g_norm, calls, rc});
    }
}

// The trajectories of a chunk need very different numbers of sweeps (lambda retries: 1 to 4 and more), so wavefronts
// are not tied to trajectories: each takes the next one of the chunk from a counter (P.queue, zeroed before the
// launch) until the chunk is used up — the grid is at most what the chip holds at once, and a wavefront whose
// trajectory was quick does not wait for the slow ones of its workgroup.  Every wavefront leaves the loop: the counter
// only grows.
template <bool FACT>
__global__ __launch_bounds__(64 * (FACT ? ILQG_FACT_WAVES : 1), 1)
void k_backward_wave(DevPtrs P, ilqg_dev_opts_t O, int single_sweep, int chunk_first, int chunk_count) {
    extern __shared__ double wave_lds[];  // [coefficient tables][per wavefront: step block, products]
    constexpr int WAVES = FACT ? ILQG_FACT_WAVES : 1;
#if ILQG_FACTORED
    if(FACT) {
        for(int i = threadIdx.x; i < NX * SXX; i += 64 * WAVES) wave_lds[i / SXX * FACT_SLICE + i % SXX] = ilqg_tensor_coef_xx[i];
        for(int i = threadIdx.x; i < NX * SUU; i += 64 * WAVES) wave_lds[i / SUU * FACT_SLICE + SXX + i % SUU] = ilqg_tensor_coef_uu[i];
        for(int i = threadIdx.x; i < NX * NXU; i += 64 * WAVES) wave_lds[i / NXU * FACT_SLICE + SXX + SUU + i % NXU] = ilqg_tensor_coef_xu[i];
        __syncthreads();  // the only meeting of the workgroup's wavefronts
    }
#endif
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    StepLds &S = *reinterpret_cast<StepLds *>(wave_lds + (FACT ? TABLE_DOUBLES : 0) + wave * WAVE_LDS_DOUBLES);
#ifdef ILQG_LDS_POISON  // debugging: whatever reads LDS it has not written gets this (a NaN, or any other pattern)
    {
        double *w = wave_lds + (FACT ? TABLE_DOUBLES : 0) + wave * WAVE_LDS_DOUBLES;
        for(int i = lane; i < WAVE_LDS_DOUBLES; i += 64) w[i] = __longlong_as_double(ILQG_LDS_POISON);
        wave_sync();
    }
#endif
    for(;;) {
        int bw = 0;
        if(lane == 0) bw = atomicAdd(P.queue, 1);
        bw = __builtin_amdgcn_readfirstlane(bw);
        if(bw >= chunk_count || chunk_first + bw >= P.B) break;
        backward_of_trajectory<FACT>(S, wave_lds, P, O, single_sweep, chunk_first + bw, bw);
        wave_sync();  // the LDS block goes to the next trajectory
    }
}
// ---------------------------------------------------------------------------
// Quad mapping (ilqg_quad.hpp): 16 lanes per trajectory, four trajectories per wavefront, each 16-lane row a worker of its
// own — it takes the next trajectory of the piece from the queue, walks its sweeps (lambda retries included) at its own
// pace and goes back to the queue.  Nothing in a step depends on the other rows of the wavefront but the instruction
// stream, so there is no hand-over and no waiting between trajectories; a row without work computes along on a valid
// record and commits nothing.  Used where the limits do not depend on the state and regType is 1 — with factored tensors,
// without tensors and (round 6) with STORED tensors, whose 38 KB per step a row reads as 16-byte pieces a few slices ahead
// of its multiply-adds (ilqg_quad.hpp); the row mapping above takes the rest.
// ---------------------------------------------------------------------------
constexpr bool QUAD_STEP = ROW_STEP && !HX && NU <= NX;
#ifndef ILQG_QUAD_WAVES  // wavefronts per workgroup (one workgroup per CU: the coefficient tables are shared)
#if ILQG_QUAD_LEAN == 63
#define ILQG_QUAD_WAVES 8  // two per SIMD: at most 256 registers each (round 5; ilqg_quad.hpp ILQG_QUAD_LEAN)
#else
#define ILQG_QUAD_WAVES 4
#endif
#endif
constexpr int QUAD_WAVES = ILQG_QUAD_WAVES;
using QRow = QuadRow<(QUAD_STEP ? NX : 1), (QUAD_STEP ? NU : 1)>;
struct QuadTab {
    static constexpr int NBASIS = ::NBASIS > 0 ? ::NBASIS : 1;
#if ILQG_FACTORED
    static constexpr int SLICE = FACT_SLICE;
    static __device__ __forceinline__ int slice_xx(int i) { return ilqg_tensor_slice_xx[i]; }
    static __device__ __forceinline__ int slice_uu(int i) { return ilqg_tensor_slice_uu[i]; }
    static __device__ __forceinline__ int slice_xu(int i) { return ilqg_tensor_slice_xu[i]; }
#else
    static constexpr int SLICE = 1;
    static __device__ __forceinline__ int slice_xx(int) { return 0; }
    static __device__ __forceinline__ int slice_uu(int) { return 0; }
    static __device__ __forceinline__ int slice_xu(int) { return 0; }
#endif
};

// SPEC — speculative retries (the default where the batch is one piece and the retry loop runs on the device; ILQG_QUAD_SPEC=0:
// off).  The kernel is bound by the chains of its longest trajectories — a failed sweep stops after 600-900 of 1 000 steps, a
// trajectory with five sweeps is 3 800 steps however idle the chip is (profiles/r5_quad_lean.txt, r5_quad_spec.txt).  But the
// sweeps of a trajectory are independent of each other given lambda_j, and lambda_j follows from the trajectory's (lambda,
// dlambda) by replaying iLQG.c:271-274 j times: a row whose queue is used up JOINS a trajectory that fewer than
// ILQG_SPEC_MAXRUN rows are working on and runs its next attempt beside them.
// Protocol (per trajectory, all through L2 atomics; no row ever waits for another):
//  * spec_word hands out attempt numbers and counts the rows at work on the trajectory; a row that is ALONE when it takes
//    an attempt writes its gains into the trajectory's records as always ("direct": every earlier attempt has ended, so
//    nothing can overtake it), any other into the gains buffer of its ROW;
//  * an attempt ends FAILED, or with a RESULT (success, or the failure of the last attempt the lambda schedule allows);
//    the row leaves the result's scalars in spec_res, publishes how the attempt ended in spec_out, and whoever then sees
//    "attempt j* has a result and all before it failed" takes spec_done by compare-and-swap and writes the trajectory —
//    copying the gains out of the winner's buffer unless they are in place;
//  * a row whose attempt failed takes the next free attempt; a row whose result has to wait — for an earlier attempt, or
//    for another row that is copying it — retires (its buffers stay as they are); rows on attempts that can be overtaken
//    poll spec_best / spec_done every 8 steps;
//  * two rows that end at the same time each publish with a RETURNING atomic before they look at the other's word, so at
//    least one of them sees both publications (the store-buffering case).
// What is written for a trajectory is what the sequential loop writes: same sweeps, same lambda sequence, bit for bit
// (tests/test_gpu_parity.py::test_speculative_retries_equal_the_sequential_sweeps).  Measured: 101-110 -> 93-102 ms.
constexpr int SPEC_ATTEMPTS = 16;  // (lambdaFactor^(j(j+1)/2) passes lambdaMax / lambdaMin = 1e16 at j = 13 for the default 1.6)
constexpr int SPEC_GW = NU + NXU;
#ifndef ILQG_SPEC_MAXRUN  // rows at work on one trajectory at most (its owner and the rows that joined)
#define ILQG_SPEC_MAXRUN 3
#endif
#ifndef ILQG_SPEC_PROBES  // looks into the row table (16 rows each) before an idle row gives up
#define ILQG_SPEC_PROBES 8
#endif
constexpr unsigned SPEC_FAILED = 1u, SPEC_RESULT = 2u;
template <bool FACT, bool SPEC = false>
__global__ __launch_bounds__(64 * QUAD_WAVES) void k_backward_quad(DevPtrs P, ilqg_dev_opts_t O, int single_sweep, int chunk_first, int chunk_count) {
    extern __shared__ double quad_lds[];  // [coefficient tables][per wavefront: four QuadRow blocks]
    if constexpr(QUAD_STEP) {
#if ILQG_FACTORED
        if(FACT) {
            for(int i = threadIdx.x; i < NX * SXX; i += 64 * QUAD_WAVES) quad_lds[i / SXX * FACT_SLICE + i % SXX] = ilqg_tensor_coef_xx[i];
            for(int i = threadIdx.x; i < NX * SUU; i += 64 * QUAD_WAVES) quad_lds[i / SUU * FACT_SLICE + SXX + i % SUU] = ilqg_tensor_coef_uu[i];
            for(int i = threadIdx.x; i < NX * NXU; i += 64 * QUAD_WAVES) quad_lds[i / NXU * FACT_SLICE + SXX + SUU + i % NXU] = ilqg_tensor_coef_xu[i];
            __syncthreads();  // the only meeting of the workgroup's wavefronts
        }
#endif
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
        const int cx_ = (c < NX) ? c : 0;
        const int N = P.N;
        const unsigned table = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr(quad_lds));
        const unsigned rb = (unsigned)lds_addr(quad_lds + (FACT ? TABLE_DOUBLES : 0) + (wave * 4 + g) * QRow::SIZE);
        // state of this row's trajectory (the same in its 16 lanes)
        bool busy = false, start = false, drained = false;
        int b = 0, bw = 0, k = 0, calls = 0;
#ifdef ILQG_COUNT_STEPS  // measurement builds (tools/experiments/steps_hist.py): bp_rc reports the steps the trajectory's sweeps walked
        int walked = 0;
#endif
        double lambda = 1.0, dlambda = 1.0, dV0 = 0.0, dV1 = 0.0, gsum = 0.0, g_norm = 0.0;
        double vx = 0.0, vxx[NX], lcur = 0.0;
#pragma unroll
        for(int r = 0; r < NX; r++) vxx[r] = 0.0;
        // SPEC: the attempt this row runs, whether its gains go to the trajectory's records, probes left for a trajectory to join
        int attempt = 0, probes = 0;
        bool direct = true, queue_empty = false;
        const int rowid = ((int)blockIdx.x * QUAD_WAVES + wave) * 4 + g;
        double *const my_gains = SPEC ? P.spec_gains + (size_t)rowid * N * SPEC_GW : nullptr;
        const int lead = lane & 48;  // the row's first lane: the one that talks to memory for the row
        auto ld = [&](const unsigned *q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        // the row leaves its trajectory (busy -> false): one runner less
        auto leave = [&](bool mine) {
            if(mine && c == 0) {
                atomicSub(&P.spec_word[b], 0x10000u);
                P.spec_row_b[rowid] = -1;
            }
        };
        // "attempt j* has a result and all before it failed": write the trajectory (once).  Returns 2 if this row wrote it, 1 if it
        // is (being) written by another row, 0 if an earlier attempt is still running.  The gains of a winner that did not
        // write the records are copied by the whole wavefront: its rows step together, so the others would stand by anyway.
        auto settle = [&](bool mine) -> int {
            int winner = -1;
            unsigned wo = 0;
            // Whatever this row has published (spec_out, spec_best: atomics at L2) is performed before it looks at the other
            // rows' words: of two rows that end at the same time at least one then sees both publications (store buffering
            // needs the fence BETWEEN a row's store and its loads; a relaxed atomic whose result is unused may not wait).
            __atomic_thread_fence(__ATOMIC_SEQ_CST);
            if(mine) {
                for(int i = 0; i < SPEC_ATTEMPTS; i++) {
                    const unsigned o = atomicOr(&P.spec_out[(size_t)b * SPEC_ATTEMPTS + i], 0u);
                    if((o & 3u) == SPEC_FAILED) continue;
                    if((o & 3u) == SPEC_RESULT) {
                        winner = i;
                        wo = o;
                    }
                    break;
                }
            }
            bool got = false;
            if(mine && winner >= 0 && c == 0) got = atomicCAS(&P.spec_done[b], 0u, 1u) == 0u;
            got = __shfl((int)got, lead) != 0;
            got = got && mine;
            if(any_lane(got)) {
                __threadfence();
                for(int r = 0; r < 4; r++) {  // one row's trajectory at a time, all 64 lanes
                    const int rg = __shfl((int)got, r * 16), rwo = __shfl((int)wo, r * 16), rb_ = __shfl(b, r * 16);
                    // (the result of a sweep that FAILED at the end of the lambda schedule — exit "no descent" — has gains for the
                    // steps above its failure only, and nothing reads the gains of a trajectory that has left the iteration: the
                    // records keep what the trajectory's own direct sweeps wrote, the row's buffer is not copied)
                    const bool no_descent = rg && P.spec_res[(size_t)((unsigned)rwo >> 3) * SPEC_SLOTS + SPEC_STATUS] == ILQG_ST_NO_DESCENT;
                    if(rg && !(((unsigned)rwo >> 2) & 1u) && !no_descent) {
                        const double2 *src = reinterpret_cast<const double2 *>(P.spec_gains + (size_t)((unsigned)rwo >> 3) * N * SPEC_GW);
                        constexpr int PAIRS = SPEC_GW / 2;
                        static_assert(SPEC_GW % 2 == 0 && NOM_L % 2 == 0 && RN % 2 == 0, "gains are copied as 16-byte pieces");
                        const int total = N * PAIRS;
                        auto put = [&](int i, const double2 &v) {
                            if(i < total) {
                                const int kk = i / PAIRS, e = i - kk * PAIRS;
                                reinterpret_cast<double2 *>(nomp(P, kk, rb_) + NOM_L)[e] = v;
                            }
                        };
                        for(int i0 = lane; i0 < total; i0 += 64 * 8) {  // eight loads in flight per lane, then their stores
                            const int i1 = i0 + 64, i2 = i0 + 128, i3 = i0 + 192, i4 = i0 + 256, i5 = i0 + 320, i6 = i0 + 384, i7 = i0 + 448;
                            const double2 v0 = src[i0], v1 = src[i1 < total ? i1 : i0], v2 = src[i2 < total ? i2 : i0], v3 = src[i3 < total ? i3 : i0];
                            const double2 v4 = src[i4 < total ? i4 : i0], v5 = src[i5 < total ? i5 : i0], v6 = src[i6 < total ? i6 : i0], v7 = src[i7 < total ? i7 : i0];
                            put(i0, v0);
                            put(i1, v1);
                            put(i2, v2);
                            put(i3, v3);
                            put(i4, v4);
                            put(i5, v5);
                            put(i6, v6);
                            put(i7, v7);
                        }
                    }
                }
                if(got && c == 0) {
                    P.i[ILQG_I_NEED_DERIVS][b] = 0;
                    store_result(P, b, spec_get(P.spec_res + (size_t)(wo >> 3) * SPEC_SLOTS));
                }
                __threadfence();
            }
            return got ? 2 : (mine && winner >= 0) ? 1 : 0;
        };

#ifdef ILQG_PROFILE_SECTIONS
        Prof prof;
        prof.start();
        Prof *pf = &prof;
#else
        Prof *pf = nullptr;
#endif
        for(;;) {
            if(pf) pf->probe(7);
            // ---- rows without a trajectory take the next ones of the piece: one atomic per wavefront and round
            while(any_lane(!busy && !drained)) {
                const bool want = !busy && !drained && !(SPEC && queue_empty);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(want && c == 0);
                if(m != 0ull) {
                    const int first = __builtin_ctzll(m);
                    int base = 0;
                    if(lane == first) base = atomicAdd(P.queue, __builtin_popcountll(m));
                    base = __shfl(base, first);
                    int mine = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));  // (the row's first lane)
                    mine = __shfl(mine, lane & 48);
                    if(want) {
                        if(mine >= chunk_count || chunk_first + mine >= P.B) {
                            if(SPEC) queue_empty = true;
                            else drained = true;
                        } else {
                            bw = mine;
                            b = chunk_first + mine;
                            if(P.i[ILQG_I_STATUS][b] == ILQG_ST_ACTIVE) {
                                if(P.derivs_failed[b]) {
                                    if(c == 0) {
                                        P.i[ILQG_I_NEED_DERIVS][b] = 0;
                                        P.i[ILQG_I_STATUS][b] = ILQG_ST_DERIVS_FAILED;
                                    }
                                } else {
                                    lambda = P.f[ILQG_F_LAMBDA][b];
                                    dlambda = P.f[ILQG_F_DLAMBDA][b];
                                    g_norm = P.f[ILQG_F_GNORM][b];
                                    dV0 = dV1 = 0.0;
                                    calls = 0;
#ifdef ILQG_COUNT_STEPS
                                    walked = 0;
#endif
                                    busy = start = true;
                                    if constexpr(SPEC) {  // attempt 0, alone: its gains go to the trajectory's records
                                        attempt = 0;
                                        direct = true;
                                        if(c == 0) {
                                            atomicAdd(&P.spec_word[b], 0x10001u);
                                            P.spec_row_b[rowid] = b;
                                        }
                                    }
                                }
                            }
                        }
                    }
                }
                if constexpr(SPEC) {
                    // ---- the queue is used up: join a trajectory that ONE row is working on, with its next attempt
                    const bool seek = !busy && !drained && queue_empty;
                    if(any_lane(seek)) {
                        const unsigned h = ((unsigned)rowid * 2654435761u + (unsigned)probes * 2246822519u) >> 7;
                        const int e = (int)(h % (unsigned)(P.spec_rows / 16)) * 16 + c;  // 16 rows of the table per probe, one per lane
                        int cand = -1;
                        unsigned w = 0;
                        bool ok = false;
                        if(seek && e != rowid) cand = (int)ld(reinterpret_cast<const unsigned *>(&P.spec_row_b[e]));
                        if(cand >= 0) {
                            w = ld(&P.spec_word[cand]);
                            ok = (w >> 16) >= 1u && (w >> 16) < (unsigned)ILQG_SPEC_MAXRUN && (w & 0xffffu) < (unsigned)(SPEC_ATTEMPTS - 1) && ld(&P.spec_done[cand]) == 0u;
                        }
                        const unsigned mk = (unsigned)((__builtin_amdgcn_ballot_w64(ok) >> lead) & 0xffffull);
                        const int src = lead + (mk ? __builtin_ctz(mk) : 0);
                        const int tb = __shfl(cand, src);
                        const unsigned tw = (unsigned)__shfl((int)w, src);
                        bool joined = false;
                        if(seek && mk != 0u && c == 0) joined = atomicCAS(&P.spec_word[tb], tw, tw + 0x10001u) == tw;
                        joined = __shfl((int)joined, lead) != 0;
                        if(seek) {
                            probes++;
                            if(joined) {
                                b = tb;
                                bw = tb - chunk_first;
                                attempt = (int)(tw & 0xffffu);
                                direct = false;
                                lambda = P.f[ILQG_F_LAMBDA][b];
                                dlambda = P.f[ILQG_F_DLAMBDA][b];
                                g_norm = P.f[ILQG_F_GNORM][b];
                                bool gone = false;
                                for(int i = 0; i < attempt; i++) {
                                    lambda_up(O.lambdaFactor, O.lambdaMin, &lambda, &dlambda);
                                    gone = gone || lambda > O.lambdaMax;
                                }
                                gone = gone || ld(&P.spec_done[b]) != 0u;
                                if(gone) {
                                    if(c == 0) atomicSub(&P.spec_word[b], 0x10000u);
                                } else {
                                    if(c == 0) P.spec_row_b[rowid] = b;
                                    dV0 = dV1 = 0.0;
                                    calls = attempt;
#ifdef ILQG_COUNT_STEPS
                                    walked = 0;
#endif
                                    busy = start = true;
                                    probes = 0;
                                }
                            }
                            if(!busy && probes >= ILQG_SPEC_PROBES) drained = true;
                        }
                    }
                }
            }
            if(!any_lane(busy)) break;  // every row is out of work and the queue is used up
#ifdef ILQG_PROFILE_SECTIONS
            prof.wave_steps++;
#endif
            // ---- a sweep begins: the value function behind the last step (the final cost's), back_pass.c:60-67
            if(any_lane(start)) {
                if(start) {
                    const double *fin = P.f[ILQG_F_FIN] + (size_t)b * FIN;
                    vx = fin[cx_];
#pragma unroll
                    for(int r = 0; r < NX; r++) vxx[r] = fin[NX + ((r <= cx_) ? ut(r, cx_) : ut(cx_, r))];
                    lcur = 0.0;  // warm start of the last step (back_pass.c:163-164)
                    dV0 = dV1 = gsum = 0.0;
                    k = N - 1;
                    start = false;
                }
            }
            // ---- one step of every busy row
            const int kk = busy ? k : 0, bb = busy ? b : ((chunk_first < P.B) ? chunk_first : 0), ww = busy ? bw : 0;
            const char *rec = reinterpret_cast<const char *>(work_rec(P, ww, kk));
            double *nom = nomp(P, kk, bb);
            double *gl = nom + NOM_L;  // where the step's gains go (l, then L)
            if constexpr(SPEC) {
                if(busy && !direct) gl = my_gains + (size_t)kk * SPEC_GW;
            }
            const int rc = back_step_quad<NX, NU, FULL, FACT, RecOffsets, QuadTab>(rb, table, rec, nom + NOM_U, gl, gl + NU, busy, vx, vxx,
                                                                                  lcur, lambda, dV0, dV1, gsum, pf);
#ifdef ILQG_PROFILE_SECTIONS
            prof.acc[7] = 0;  // (queue, sweep starts, row transitions: not charged to a section)
#endif
            // ---- what the row does next
            if constexpr(SPEC) {
                const bool failed = busy && BOXQP_FAILED(rc), finished = busy && BOXQP_OK(rc) && k == 0;
                bool overtaken = false;
#ifdef ILQG_COUNT_STEPS
                if(busy) walked++;
#endif
                if(busy && !failed && !finished) {
                    k--;
                    // an attempt that can be overtaken looks every 8 steps whether it has been
                    overtaken = !direct && (k & 7) == 0 && (ld(&P.spec_best[b]) < (unsigned)attempt || ld(&P.spec_done[b]) != 0u);
                }
                if(any_lane(overtaken)) {  // (rare) no row leaves a trajectory without a look at whether it can be written
                    (void)settle(overtaken);
                    if(overtaken) {
                        leave(true);
                        busy = false;
                    }
                }
                if(any_lane(failed || finished)) {
                    const bool ended = failed || finished;
                    bool result = false, retire = false;
                    int bp_rc = 0;
                    if(failed) {  // back_pass.c:168-171; the next lambda decides whether there is another attempt (iLQG.c:267-275)
                        double l2 = lambda, d2 = dlambda;
                        lambda_up(O.lambdaFactor, O.lambdaMin, &l2, &d2);
                        if(l2 > O.lambdaMax) {
                            lambda = l2;
                            dlambda = d2;
                            result = true;
                            bp_rc = 1;
                        }
                    }
                    if(finished) {
                        g_norm = gsum / ((double)(N - 1));  // N summands over N-1 (back_pass.c:254)
                        result = true;
                    }
                    // (never single_sweep here: the shim speculates only where the retry loop runs on the device)
                    const int status = result ? back_status(bp_rc, g_norm, lambda, dlambda, 0, O) : ILQG_ST_ACTIVE;
#ifdef ILQG_COUNT_STEPS
                    bp_rc = walked;
#endif
                    if(ended && result && c == 0)
                        spec_put(P.spec_res + (size_t)rowid * SPEC_SLOTS, {status, lambda, dlambda, dV0, dV1, g_norm, attempt + 1, bp_rc});
                    __threadfence();  // the attempt's gains and scalars are out before it is said to have ended
                    if(ended && c == 0) {
                        if(result) atomicMin(&P.spec_best[b], (unsigned)attempt);
                        atomicExch(&P.spec_out[(size_t)b * SPEC_ATTEMPTS + attempt],
                                   (result ? SPEC_RESULT : SPEC_FAILED) | (direct ? 4u : 0u) | ((unsigned)rowid << 3));
                    }
                    const int written = settle(ended);
                    if(ended) {
                        if(written || result) {
                            // the trajectory is written — or this row's result waits: for an earlier attempt, or for another row
                            // to copy it; then the row retires, so that its buffers stay as they are
                            leave(true);
                            busy = false;
                            if(result && written != 2) drained = true;
                        } else if(ld(&P.spec_done[b]) != 0u) {
                            leave(true);
                            busy = false;
                        } else {  // the next free attempt
                            unsigned old = 0;
                            if(c == 0) old = atomicAdd(&P.spec_word[b], 1u);
                            old = (unsigned)__shfl((int)old, lead);
                            const int na = (int)(old & 0xffffu);
                            bool gone = na >= SPEC_ATTEMPTS;
                            for(int i = attempt; i < na; i++) {
                                lambda_up(O.lambdaFactor, O.lambdaMin, &lambda, &dlambda);
                                gone = gone || lambda > O.lambdaMax;
                            }
                            if(gone) {
                                retire = true;
                            } else {
                                attempt = na;
                                direct = (old >> 16) == 1u;
                                start = true;
                            }
                        }
                    }
                    // a row that found no further attempt inside the lambda schedule: the attempt that ends the schedule is
                    // another row's and has a result, or will have — one more look, then the row leaves
                    if(any_lane(retire)) {
                        (void)settle(retire);
                        if(retire) {
                            leave(true);
                            busy = false;
                        }
                    }
                }
            } else {
            if(busy) {
                bool done = false;
                int bp_rc = 0;
#ifdef ILQG_COUNT_STEPS
                walked++;
#endif
                if(BOXQP_FAILED(rc)) {  // the sweep is abandoned (back_pass.c:168-171): raise lambda and sweep again (iLQG.c:267-275)
                    calls++;
                    bp_rc = 1;
                    done = true;
                    if(!single_sweep) {
                        lambda_up(O.lambdaFactor, O.lambdaMin, &lambda, &dlambda);
                        if(!(lambda > O.lambdaMax)) {
                            done = false;
                            start = true;
                        }
                    }
                } else if(k == 0) {
                    calls++;
                    g_norm = gsum / ((double)(N - 1));  // N summands over N-1 (back_pass.c:254)
                    done = true;
                } else {
                    k--;
                }
                if(done) {
                    const int status = back_status(bp_rc, g_norm, lambda, dlambda, single_sweep, O);
#ifdef ILQG_COUNT_STEPS
                    bp_rc = walked;
#endif
                    if(c == 0) {
                        P.i[ILQG_I_NEED_DERIVS][b] = 0;
                        store_result(P, b, {status, lambda, dlambda, dV0, dV1, g_norm, calls, bp_rc});
                    }
                    busy = false;
                }
            }
            }
        }
#ifdef ILQG_PROFILE_SECTIONS
        if(lane == 0) {
            for(int i = 0; i < 7; i++) atomicAdd(&ilqg_prof_cycles[i], (unsigned long long)prof.acc[i]);
            atomicAdd(&ilqg_prof_cycles[7], (unsigned long long)prof.wave_steps);  // steps of the wavefront (1 to 4 rows busy)
        }
#endif
    }
}
