// The problem parameters as the kernels see them: the lane's private copy and the callback context built on it, the
// parameter rows a kernel's pack `Rows...` may hold, and the one statement that applies them (apply_rows).  Included by
// ilqg_kernels.hip inside its anonymous namespace, in front of every k_*.inc.

// Per-lane snapshot of the problem parameters.  The generated callbacks read parameters as
// p[i][j] through a `double **`; read from global memory, every such value would have to be
// re-loaded after each store of the kernel (the compiler cannot prove that the parameter
// arrays do not alias the output arrays), which costs two dependent memory round trips per
// use.  Fixed-size parameters are therefore passed BY VALUE as a kernel argument (ParamValues)
// and copied into a private array: after SROA every p[i][j] is a wave-uniform value that was
// loaded once from the kernel-argument segment by a scalar load, i.e. it lives in an SGPR and
// costs no vector register.  Per-time-step parameters (size -1) stay in global memory.
struct ParamValues {
    double v[ILQG_PTOTAL];
};
struct ParamTable {
    double *ptr[ILQG_NP + ILQG_HOOK_SLOTS];  // the problem's parameters, then the hooks (see ilqg_hooks)
};
//
// VECTOR = true: the copies are made lane values (an empty asm statement the optimiser cannot look through), i.e. they
// live in vector registers as the rows of a per-trajectory table do (apply_rows).  The shared lane-mapped sweep and
// searches hold more wave-uniform values than there are scalar registers; what does not fit travels through
// v_writelane / v_readlane — vector instructions with wait states, inside the step loops — while vector registers are
// to spare there.  Per kernel, where that kernel's launch time gained by it (profiles/r14_vector_params.txt), and only for
// a problem with few parameter doubles: each costs two vector registers.  The kernels that do: k_backward<2>, k_search<0, true>, k_search<1, true>.
constexpr int VECTOR_PARAMS_MAX = 24;  // parameter doubles up to which a kernel may hold them per lane (CarParking: 20)
constexpr bool VECTOR_PARAMS = !ILQG_WAVE_MAP && ILQG_PTOTAL <= VECTOR_PARAMS_MAX;
template <bool VECTOR = false>
__device__ __forceinline__ void load_params(ParamValues &V, ParamTable &T, ilqg_hooks &H, const ParamValues &A,
                                            double **p) {
    constexpr int sizes[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
    constexpr int offs[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_POFFSETS;
#pragma unroll
    for(int i = 0; i < ILQG_NP; i++) {
        if(sizes[i] > 0) {
#pragma unroll
            for(int j = 0; j < sizes[i]; j++) {
                double v = A.v[offs[i] + j];
                if(VECTOR) asm volatile("" : "+v"(v));
                V.v[offs[i] + j] = v;
            }
            T.ptr[i] = &V.v[offs[i]];
        } else {
            T.ptr[i] = p[i];
        }
    }
    H.nonfinite = 0.0;
    H.huge = 0.0;
    H.slow = 0.0;
    H.limgrad = 1.0;
    T.ptr[ILQG_HOOK_NONFINITE] = &H.nonfinite;
    T.ptr[ILQG_HOOK_HUGE] = &H.huge;
    T.ptr[ILQG_HOOK_SLOW] = &H.slow;
    T.ptr[ILQG_HOOK_LIMGRAD] = &H.limgrad;
    H.alone = 0.0;
    T.ptr[ILQG_HOOK_ALONE] = &H.alone;
    H.record = nullptr;
    T.ptr[ILQG_HOOK_RECORD] = reinterpret_cast<double *>(&H.record);
}

// What a kernel needs to call the generated callbacks.  Four separate private objects, each pointing
// only at the next (o -> table -> values, hooks): the optimiser dissolves them one level at a time into
// registers; a single struct holding pointers into itself would stay in scratch memory.
struct Callbacks {
    tOptSet o;   // what the callbacks see as `o` (p, n_hor, penalty weights)
    tOptSet o1;  // the same with n_hor = 1: init_running loops over n_hor elements
};
template <bool VECTOR = false>
__device__ __forceinline__ void make_callbacks(Callbacks &C, ParamTable &T, ParamValues &V, ilqg_hooks &H,
                                               const DevPtrs &P, const ilqg_dev_opts_t &O, const ParamValues &A) {
    load_params<VECTOR>(V, T, H, A, P.p);
    tOptSet &o = C.o;
    o.p = T.ptr;
    o.n_hor = P.N;
    o.w_pen_l = O.w_pen_init_l;
    o.w_pen_f = O.w_pen_init_f;
    o.tolConstraint = O.tolConstraint;
    o.w_pen_fact1 = O.w_pen_fact1;
    o.w_pen_fact2 = O.w_pen_fact2;
    o.w_pen_max_l = O.w_pen_max_l;
    o.w_pen_max_f = O.w_pen_max_f;
    C.o1 = o;
    C.o1.n_hor = 1;
}
// problems with multipliers: the penalty weights are per trajectory (they grow with the constraint violation)
__device__ __forceinline__ void set_penalty_weights(Callbacks &C, double w_l, double w_f) {
    C.o.w_pen_l = C.o1.w_pen_l = w_l;
    C.o.w_pen_f = C.o1.w_pen_f = w_f;
}
__device__ __forceinline__ void load_penalty_weights(Callbacks &C, const DevPtrs &P, int b) {
    if(HAS_MUL) set_penalty_weights(C, P.f[ILQG_F_WPEN_L][b], P.f[ILQG_F_WPEN_F][b]);
}
// for the derivatives: the weights of the last accepted step.  A rejected step may raise the current ones
// (iLQG.c:345-349) while the reference sweeps again over the derivatives it has; kernels that re-evaluate
// derivatives instead of keeping them (fused backward pass, wave mapping) reproduce those with these weights.
__device__ __forceinline__ void load_penalty_weights_der(Callbacks &C, const DevPtrs &P, int b) {
    if(HAS_MUL) set_penalty_weights(C, P.f[ILQG_F_WPEN_L_DER][b], P.f[ILQG_F_WPEN_F_DER][b]);
}
// declares the callback context C and the lane's hooks H of a kernel with arguments (P, O, A)
#define ILQG_CALLBACKS(C, H) ILQG_CALLBACKS_IN(C, H, false)
// the same with the fixed-size parameters in vector registers where VECTOR_ holds (see load_params)
#define ILQG_CALLBACKS_IN(C, H, VECTOR_) \
    ParamValues C##_values;              \
    ParamTable C##_table;                \
    ilqg_hooks H;                        \
    Callbacks C;                         \
    make_callbacks<(VECTOR_)>(C, C##_table, C##_values, H, P, O, A)

// Per-roll-out problem parameters (ilqg_batch_policy_rollout_params).  k_policy<true> is the same roll-out with three more
// arguments — the caller's table `values`, [B][R][W] or with `shared` [R][W], and a by-value map of the ParamValues slots:
// src[j] = the column of a row that replaces slot j, or -1 for a slot that keeps the batch's value.  Behind ILQG_CALLBACKS
// every lane overrides the mapped slots of its PRIVATE ParamValues with row (shared ? r : g) of the table; the callbacks
// then read them through the same ParamTable as ever.  The map is a kernel argument, so the test of a slot is a scalar
// branch; an overridden slot lives in two vector registers instead of two scalar ones.  The policy (x, u, l, L of slot b),
// the multipliers, the penalty weights and the per-time-step parameters are the batch's.  k_policy<false> has no further
// argument (the pack is empty) and not one statement more than before.
// Per-time-step parameters per trajectory (ilqg_batch_set_param_steps_batch) ride in the same map: for the s-th parameter of
// size -1 in paramdesc[] order, rows[s] = its table [B][n_hor + 1], trajectory-major, or null while that parameter is the
// shared window.  The member exists only in libraries whose problem has such a parameter (N_STEP_PARAMS, from ILQG_PSIZES):
// everywhere else the map, and with it every kernel that takes one, is what it was.
constexpr int n_step_params() {
    constexpr int sizes[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
    int n = 0;
    for(int i = 0; i < ILQG_NP; i++) n += sizes[i] == -1 ? 1 : 0;
    return n;
}
constexpr int N_STEP_PARAMS = n_step_params();
template <int n>
struct StepRows {
    const double *rows[n] = {};
};
template <>
struct StepRows<0> {};
struct PolicyParamMap : StepRows<N_STEP_PARAMS> {
    short src[ILQG_PTOTAL];
    int W;
};
// Register-resident overrides cost two vector registers per parameter double, 90 for the n = 16 problem.  Its FMA-free
// builds (tests only) have none to give — their k_policy<false> already takes 448 of 512 — and would pay in scratch memory;
// there the callbacks read EVERY fixed-size parameter from global memory instead: a named one in the lane's row of the
// caller's table, the others in the context's own parameter buffers (P.p, which hold the fixed-size parameters too).  No
// private copy, no register, and a reload behind every store the compiler cannot tell apart.
#ifndef ILQG_POLICY_PARAMS_IN_MEMORY
#if defined(ILQG_STRICT_FP)
#define ILQG_POLICY_PARAMS_IN_MEMORY (2 * ILQG_PTOTAL > 64)
#else
#define ILQG_POLICY_PARAMS_IN_MEMORY 0
#endif
#endif
// behind: a second override of the same lane (below); in the pointer form a slot it does not name keeps what the first one left
__device__ __forceinline__ void override_params(ParamValues &V, ParamTable &T, const DevPtrs &P, size_t g, int r, const double *__restrict__ values,
                                                int shared, const PolicyParamMap &map, bool behind = false) {
    const double *row = values + (shared ? (size_t)r : g) * (size_t)map.W;
    if(ILQG_POLICY_PARAMS_IN_MEMORY) {
        constexpr int sizes[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
        constexpr int offs[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_POFFSETS;
#pragma unroll
        for(int i = 0; i < ILQG_NP; i++)
            if(sizes[i] > 0) T.ptr[i] = map.src[offs[i]] >= 0 ? const_cast<double *>(row + map.src[offs[i]]) : (behind ? T.ptr[i] : P.p[i]);
    } else {
#pragma unroll
        for(int j = 0; j < ILQG_PTOTAL; j++)
            if(map.src[j] >= 0) V.v[j] = row[map.src[j]];
    }
}

// The trajectory's windows of the per-time-step parameters.  load_params left T.ptr[i] = the shared array, which the
// generated callbacks index as p[i][k], k = 0 .. n_hor: that indexing is fixed, so a window per trajectory is a POINTER PER
// LANE, row b of the table (two vector registers per such parameter, and a vector load per use where the shared window takes
// a scalar one; eight consecutive steps of a lane share a 64-byte line).  A null table (a scalar test: the map is a kernel
// argument) leaves the shared window.  Index arithmetic over B (n_hor + 1) in size_t.
template <class Map>
__device__ __forceinline__ void trajectory_step_params(ParamTable &T, const DevPtrs &P, int b, const Map &map) {
    constexpr int sizes[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
    int s = 0;
#pragma unroll
    for(int i = 0; i < ILQG_NP; i++)
        if(sizes[i] == -1) {
            if(map.rows[s]) T.ptr[i] = const_cast<double *>(map.rows[s]) + (size_t)b * (size_t)(P.N + 1);
            s++;
        }
}

// Per-trajectory problem parameters (ilqg_batch_set_params_batch): the context's table [B][W] with its map, the first two of
// a kernel's pack `rows` (a kernel with an EMPTY pack is the kernel of before, under its old name; the two kernels that were no
// templates, k_derivs and k_multipliers, stay so and have the twins k_derivs_rows / k_multipliers_rows).  Right behind ILQG_CALLBACKS a lane overrides the mapped slots of its private ParamValues with row b
// of the table — b = the trajectory the lane works for, whatever its lane index means — ONCE per launch, never inside a step
// loop: from there on the values are the lane's registers, where the shared ones are the wavefront's.  This is the one place
// that states it, for k_rollout, k_derivs, k_backward, k_search, k_multipliers, k_policy and k_plant (and, with the plant's
// table, for the plant's own row).  The same statement points the lane at its rows of the per-time-step parameters
// (trajectory_step_params); with step rows only, the table's map is empty (every src -1, W = 0) and `values` is not read.  ORDER: the trajectory's row first, then the roll-out's or the plant's row — whatever the pack
// holds behind the first two: a slot named in both gets the latter.
//
// The grammar of a pack, [table, map,] [own...]: what a kernel's own rows are is the kernel's to say (OwnRows); whether the
// trajectory's table stands in front of them follows from the pack's length.
enum OwnRows {
    OWN_NONE,     // k_rollout, k_derivs_rows, k_backward, k_search, k_multipliers_rows, k_policy<false>, k_plant<false>
    OWN_ROLLOUT,  // k_policy<true>: values, shared, map — row (shared ? r : g)
    OWN_PLANT     // k_plant<true>: values, map — row g (= b)
};
template <OwnRows OWN, class... Rows>
struct RowPack {
    using Own = std::conditional_t<OWN == OWN_ROLLOUT, std::tuple<const double *, int, PolicyParamMap>,
                                   std::conditional_t<OWN == OWN_PLANT, std::tuple<const double *, PolicyParamMap>, std::tuple<>>>;
    using WithTrajectory = decltype(std::tuple_cat(std::declval<std::tuple<const double *, PolicyParamMap>>(), std::declval<Own>()));
    static constexpr bool has_trajectory_rows = sizeof...(Rows) > std::tuple_size<Own>::value;
    static_assert(std::is_same<std::tuple<Rows...>, std::conditional_t<has_trajectory_rows, WithTrajectory, Own>>::value,
                  "a kernel's pack of parameter rows is [table, map,] [own...]: table, map = const double *, PolicyParamMap (the context's "
                  "per-trajectory rows); own... = nothing, or values, shared, map = const double *, int, PolicyParamMap for k_policy<true>, "
                  "or values, map = const double *, PolicyParamMap for k_plant<true>");
};
// The statement behind ILQG_CALLBACKS (V, T = C_values, C_table): the lane's rows over its private parameters, for the
// trajectory b it works for and, of the kernel's own rows, row g resp. r.  An empty pack: no statement at all.
template <OwnRows OWN, class... Rows>
__device__ __forceinline__ void apply_rows(ParamValues &V, ParamTable &T, const DevPtrs &P, int b, size_t g, int r, const Rows &...rows) {
    constexpr bool TRAJECTORY = RowPack<OWN, Rows...>::has_trajectory_rows;
    constexpr int own = TRAJECTORY ? 2 : 0;  // where the own rows start
    const auto row = std::forward_as_tuple(rows...);
    if constexpr(TRAJECTORY) {
        override_params(V, T, P, (size_t)b, 0, std::get<0>(row), 0, std::get<1>(row));
        if constexpr(N_STEP_PARAMS > 0) trajectory_step_params(T, P, b, std::get<1>(row));
    }
    if constexpr(OWN == OWN_ROLLOUT) override_params(V, T, P, g, r, std::get<own>(row), std::get<own + 1>(row), std::get<own + 2>(row), TRAJECTORY);
    if constexpr(OWN == OWN_PLANT) override_params(V, T, P, g, 0, std::get<own>(row), 0, std::get<own + 1>(row), TRAJECTORY);
}
