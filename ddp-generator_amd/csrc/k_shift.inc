// Receding horizon (ilqg_dev_shift, ilqg_dev_log_*): the plan of every trajectory moves `steps` time steps towards the
// start WHERE IT IS, on the device — u'[k] = u[k + steps], the last control held over the tail, x0' = x[steps] — and the
// first steps of a plan are appended to a log that reaches the host once.  What the reference's caller does between two
// calls of the MEX entry (u_nom = [u(:, s+1:end), tail], a new x0: iLQG_mex.c:113-120).  No arithmetic: the initial
// roll-out that follows is the existing k_rollout<RK_INIT>.
//
// IN PLACE.  Every kernel that moves a row where it is (here, k_best.inc, k_mpc_io.inc) goes through one of the three bodies
// below, and all three move in ascending blocks: all loads of a block, ONE barrier, then its stores.  A block reads entries
// [k0 + steps, k0 + block + steps) and writes [k0, k0 + block): what it reads and writes overlaps only within the block,
// which the barrier separates; the blocks before it wrote nothing beyond k0, and the blocks behind it read nothing below
// k0 + block.  The last entry, which a tail that is not given repeats, is written by the last block alone, behind that
// block's reads.  That is the argument for ONE workgroup on a row; what each kernel adds is why no other workgroup
// touches the entries its workgroup moves.

// The row form: p [n] doubles, the last `steps` values from tl [steps] or, with tl null, p[n - 1] held.  A block is the
// workgroup's size; the caller's condition to be here is uniform over the workgroup (nobody is left at the barrier).
constexpr int PARAM_BLOCK = 256;
__device__ __forceinline__ void shift_row(double *__restrict__ p, int n, int steps, const double *__restrict__ tl) {
    const int t = (int)threadIdx.x;
    for(int k0 = 0; k0 < n; k0 += PARAM_BLOCK) {
        const int k = k0 + t, from = k + steps;
        double v = 0.0;
        if(k < n) v = (from < n || !tl) ? p[from < n ? from : n - 1] : tl[from - n];  // (as the two bodies below spell it)
        __syncthreads();
        if(k < n) p[k] = v;
    }
}

#if !ILQG_WAVE_MAP
// Lane mapping.  X / U are [step][tile of 64][component][trajectory in tile]: one step of U is NU * Bp contiguous doubles,
// and a lane owns ONE of them — element e = (tile, component, trajectory in tile) — which it walks upwards in k, so a
// wavefront moves 512 contiguous bytes per step.  The controls are read where the source's plan currently is (cur_u: X / U
// or a kept roll-out plane of the line search, ILQG_I_LOC) and written `steps` earlier into the array U of the lane's own
// trajectory.  A workgroup is SHIFT_WAVES wavefronts on the SAME 64 elements; a block is a round of SHIFT_WAVES *
// SHIFT_UNROLL steps, read by all of them (each its own SHIFT_UNROLL steps), a barrier, then written.  The tail steps take
// the source's tail where it has one, and every step its addend (one fp64 add), in the same pass.  x0' — the source's, or
// x[steps] of the plan — goes to step 0 of X.  The caller clears ILQG_I_LOC behind the kernel (every lane of a trajectory
// reads it).
// (One wavefront per 64 elements walking all N steps alone: 0.41 ms per group of 16 384 CarParking trajectories, which is
// only 512 such wavefronts; this form 0.35 ms, the four groups' launches side by side — profiles/r7_receding.txt.)
constexpr int SHIFT_UNROLL = 8;  // steps a lane has in flight: all their loads, then their stores
constexpr int SHIFT_WAVES = 8;   // wavefronts of the workgroup: each takes SHIFT_UNROLL of the round's steps
// What the plans' own shift and the shift to a segment's winner (k_best.inc) differ in, as a type the lane body below is
// instantiated with.  Here: every trajectory from its own plan, x0' = x[steps] if wanted, no tail and nothing to add — all
// of it known to the compiler, none of it a run-time flag.  from(b): the slot whose plan b takes; x0(b, c): the caller's x0'
// or null; tail(b, steps, c): the caller's tail, [steps] NU apart, or null; add(b, N, c): the addend, [N] NU apart, or null.
struct OwnPlan {
    int plan_x0;
    __device__ __forceinline__ bool live(const DevPtrs &P, int b, int steps) const { return b < P.B && (steps > 0 || P.i[ILQG_I_LOC][b]); }
    __device__ __forceinline__ bool sets_x0() const { return plan_x0 != 0; }
    __device__ __forceinline__ int from(int b) const { return b; }
    __device__ __forceinline__ const double *x0(int, int) const { return nullptr; }
    __device__ __forceinline__ const double *tail(int, int, int) const { return nullptr; }
    __device__ __forceinline__ const double *add(int, int, int) const { return nullptr; }
};
template <class Src>
__device__ __forceinline__ void shift_lane(const DevPtrs &P, int steps, const Src &S) {
    const int t = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6), N = P.N;
    const size_t e = (size_t)blockIdx.x * WAVE + t;
    if(S.sets_x0() && w == 0 && e < (size_t)NX * P.Bp) {
        const int b = (int)(e / (NX * WAVE)) * WAVE + t, c = (int)((e / WAVE) % NX);
        if(S.live(P, b, steps)) {
            const double *x0 = S.x0(b, c);
            home_x(P, 0, b)[(size_t)c * XSI] = x0 ? *x0 : cur_x(P, steps, S.from(b))[(size_t)c * XSI];
        }
    }
    if((size_t)blockIdx.x * WAVE >= (size_t)NU * P.Bp) return;  // (the whole workgroup)
    const int b = (int)(e / (NU * WAVE)) * WAVE + t, c = (int)((e / WAVE) % NU);
    const bool live = S.live(P, b, steps);
    const double *src = live ? cur_u(P, 0, S.from(b)) + (size_t)c * XSI : nullptr;
    const double *tail = live ? S.tail(b, steps, c) : nullptr;
    const double *add = live ? S.add(b, N, c) : nullptr;
    double *dst = home_u(P, 0, b) + (size_t)c * XSI;
    const size_t us = cur_ustride(P);
    for(int r0 = 0; r0 < N; r0 += SHIFT_WAVES * SHIFT_UNROLL) {
        const int k0 = r0 + w * SHIFT_UNROLL;
        double v[SHIFT_UNROLL];
        if(live) {
#pragma unroll
            for(int j = 0; j < SHIFT_UNROLL; j++) {
                const int k = k0 + j, from = k + steps;
                if(from < N || !tail) v[j] = src[(size_t)(from < N ? from : N - 1) * us];  // the tail holds u[N-1]
                else v[j] = k < N ? tail[(size_t)(from - N) * NU] : 0.0;
                if(add && k < N) v[j] += add[(size_t)k * NU];
            }
        }
        __syncthreads();
        if(live) {
#pragma unroll
            for(int j = 0; j < SHIFT_UNROLL; j++)
                if(k0 + j < N) dst[(size_t)(k0 + j) * us] = v[j];
        }
    }
}
// the plans' own shift: a workgroup's 64 elements are nobody else's
__global__ void __launch_bounds__(WAVE * SHIFT_WAVES) k_shift_lane(DevPtrs P, int steps, int plan_x0) { shift_lane(P, steps, OwnPlan{plan_x0}); }
constexpr auto k_shift = k_shift_lane;  // (what the shim launches: this mapping's kernel and workgroup size)
constexpr int SHIFT_THREADS = WAVE * SHIFT_WAVES;
#else
// Wave mapping (row, quad and element builds alike: x and u live in the packed records nom[trajectory][step][RN] only).
// One pass of a workgroup over the NOM_U entries of slot `from_b`: per block of SHIFT_BLOCK / NU steps, one lane per
// component of a step, the loads (the tail steps from tail(from - N) where has_tail), the barrier, then store(k, c, v) — the
// kernel's own: where the block goes.
constexpr int SHIFT_BLOCK = 256;
static_assert(NU <= SHIFT_BLOCK && NX <= SHIFT_BLOCK, "k_shift_wave: one lane per component of a step");
template <class Tail, class Store>
__device__ __forceinline__ void shift_wave(const DevPtrs &P, int steps, int from_b, bool has_tail, Tail &&tail, Store &&store) {
    constexpr int PER = SHIFT_BLOCK / NU;  // steps per block
    const int t = threadIdx.x, kk = t / NU, c = t % NU, N = P.N;
    for(int k0 = 0; k0 < N; k0 += PER) {
        const int k = k0 + kk;
        const bool mine = kk < PER && k < N;
        double v = 0.0;
        if(mine) {
            const int from = k + steps;
            if(from < N || !has_tail) v = nomp(P, from < N ? from : N - 1, from_b)[NOM_U + c];  // the tail holds u[N-1]
            else v = tail(from - N, c);
        }
        __syncthreads();
        if(mine) store(k, c, v);
    }
}
// the plans' own shift: one workgroup per trajectory, whose records are nobody else's
__global__ void __launch_bounds__(SHIFT_BLOCK) k_shift_wave(DevPtrs P, int steps, int plan_x0) {
    const int b = blockIdx.x, t = threadIdx.x;
    if(b >= P.B) return;  // (the whole workgroup)
    if(plan_x0 && steps > 0 && t < NX) nomp(P, 0, b)[NOM_X + t] = nomp(P, steps, b)[NOM_X + t];
    if(steps == 0) return;
    shift_wave(P, steps, b, false, [](int, int) { return 0.0; }, [&](int k, int c, double v) { nomp(P, k, b)[NOM_U + c] = v; });
}
constexpr auto k_shift = k_shift_wave;  // (what the shim launches: this mapping's kernel and workgroup size)
constexpr int SHIFT_THREADS = SHIFT_BLOCK;
#endif

// the caller's tail: host [trajectory][steps][NU] into steps k0 .. k0 + steps - 1 of the controls (the records, and the
// array U of the lane mapping: what ilqg_dev_write does for the whole field)
__global__ void k_put_u_steps(DevPtrs P, const double *__restrict__ host, int k0, int steps) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= (size_t)P.B * steps * NU) return;
    const int c = (int)(i % NU), k = k0 + (int)((i / NU) % steps), b = (int)(i / ((size_t)NU * steps));
    const double v = host[i];
    nomp(P, k, b)[NOM_U + c] = v;
    if(!WAVE_MAP) home_u(P, k, b)[(size_t)c * XSI] = v;
}

// The applied steps of round `round`: (x_k, u_k), k < steps, of every current plan (cur_x: wherever it lives) and its cost
// into the log, which is laid out as the host reads it: x [trajectory][rounds * steps][NX], u [..][NU], cost [trajectory][rounds].
__global__ void k_log_steps(DevPtrs P, double *__restrict__ lx, double *__restrict__ lu, double *__restrict__ lc, int round,
                            int rounds, int steps) {
    constexpr int W = NX + NU;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= (size_t)P.B * steps * W) return;
    // trajectory fastest: the lane mapping's tiled arrays are read row by row
    const int b = (int)(i % P.B), c = (int)((i / P.B) % W), k = (int)(i / ((size_t)P.B * W));
    const size_t at = (size_t)b * rounds * steps + (size_t)round * steps + k;
    if(c < NX) lx[at * NX + c] = cur_x(P, k, b)[(size_t)c * XSI];
    else lu[at * NU + (c - NX)] = cur_u(P, k, b)[(size_t)(c - NX) * XSI];
    if(k == 0 && c == 0) lc[(size_t)b * rounds + round] = P.f[ILQG_F_COST][b];
}
