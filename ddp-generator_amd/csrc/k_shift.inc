// Receding horizon (ilqg_dev_shift, ilqg_dev_log_*): the plan of every trajectory moves `steps` time steps towards the
// start WHERE IT IS, on the device — u'[k] = u[k + steps], the last control held over the tail, x0' = x[steps] — and the
// first steps of a plan are appended to a log that reaches the host once.  What the reference's caller does between two
// calls of the MEX entry (u_nom = [u(:, s+1:end), tail], a new x0: iLQG_mex.c:113-120).  No arithmetic: the initial
// roll-out that follows is the existing k_rollout<RK_INIT>.

constexpr int SHIFT_UNROLL = 8;  // steps a lane of k_shift_lane has in flight: all their loads, then their stores
constexpr int SHIFT_WAVES = 8;   // wavefronts of its workgroup: each takes SHIFT_UNROLL of the round's steps

#if !ILQG_WAVE_MAP
// Lane mapping.  X / U are [step][tile of 64][component][trajectory in tile]: one step of U is NU * Bp contiguous doubles,
// and a lane owns ONE of them — element e = (tile, component, trajectory in tile) — which it walks upwards in k, so a
// wavefront moves 512 contiguous bytes per step.  The controls are read where they currently are (cur_u: X / U or a kept
// roll-out plane of the line search, ILQG_I_LOC) and written `steps` earlier into the array U.  A workgroup is
// SHIFT_WAVES wavefronts on the SAME 64 elements: a round of SHIFT_WAVES * SHIFT_UNROLL steps is read by all of them (each
// its own SHIFT_UNROLL steps), a barrier, then written.  In place (location 0) that is safe: a round reads steps
// [r0 + steps, r0 + round + steps) and writes [r0, r0 + round), the rounds before it wrote nothing beyond r0, and no other
// workgroup touches these columns; u[N-1], which the tail repeats, is written by the last round alone, behind its reads.
// (One wavefront per 64 elements walking all N steps alone: 0.41 ms per group of 16 384 CarParking trajectories, which is
// only 512 such wavefronts; this form 0.35 ms, the four groups' launches side by side — profiles/r7_receding.txt.)  x[steps] goes to step 0 of X.  The caller clears ILQG_I_LOC behind the
// kernel (every lane of a trajectory reads it).
__global__ void __launch_bounds__(WAVE * SHIFT_WAVES) k_shift_lane(DevPtrs P, int steps, int plan_x0) {
    const int t = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6), N = P.N;
    const size_t e = (size_t)blockIdx.x * WAVE + t;
    if(plan_x0 && w == 0 && e < (size_t)NX * P.Bp) {
        const int b = (int)(e / (NX * WAVE)) * WAVE + t, c = (int)((e / WAVE) % NX);
        if(b < P.B && (steps > 0 || P.i[ILQG_I_LOC][b])) home_x(P, 0, b)[(size_t)c * XSI] = cur_x(P, steps, b)[(size_t)c * XSI];
    }
    if((size_t)blockIdx.x * WAVE >= (size_t)NU * P.Bp) return;  // (the whole workgroup)
    const int b = (int)(e / (NU * WAVE)) * WAVE + t, c = (int)((e / WAVE) % NU);
    const bool live = b < P.B && (steps > 0 || P.i[ILQG_I_LOC][b]);
    const double *src = live ? cur_u(P, 0, b) + (size_t)c * XSI : nullptr;
    double *dst = home_u(P, 0, b) + (size_t)c * XSI;
    const size_t us = cur_ustride(P);
    for(int r0 = 0; r0 < N; r0 += SHIFT_WAVES * SHIFT_UNROLL) {
        const int k0 = r0 + w * SHIFT_UNROLL;
        double v[SHIFT_UNROLL];
        if(live) {
#pragma unroll
            for(int j = 0; j < SHIFT_UNROLL; j++) {
                const int from = k0 + j + steps;
                v[j] = src[(size_t)(from < N ? from : N - 1) * us];  // the tail holds u[N-1]
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
#else
// Wave mapping (row, quad and element builds alike: x and u live in the packed records nom[trajectory][step][RN] only).
// One workgroup per trajectory moves u within the trajectory's records in ascending blocks of SHIFT_BLOCK / NU steps: all
// reads of a block, a barrier, its writes.  A block reads steps [k0 + steps, k0 + block + steps) and writes [k0, k0 + block);
// the blocks before it wrote nothing beyond k0, so one barrier per block is enough.  (u[N-1], which the tail repeats, is
// written by the last block alone, behind that block's reads.)
constexpr int SHIFT_BLOCK = 256;
static_assert(NU <= SHIFT_BLOCK && NX <= SHIFT_BLOCK, "k_shift_wave: one lane per component of a step");
__global__ void __launch_bounds__(SHIFT_BLOCK) k_shift_wave(DevPtrs P, int steps, int plan_x0) {
    const int b = blockIdx.x, t = threadIdx.x, N = P.N;
    if(b >= P.B) return;  // (the whole workgroup)
    constexpr int PER = SHIFT_BLOCK / NU;  // steps per block
    const int kk = t / NU, c = t % NU;
    if(plan_x0 && steps > 0 && t < NX) nomp(P, 0, b)[NOM_X + t] = nomp(P, steps, b)[NOM_X + t];
    if(steps == 0) return;
    for(int k0 = 0; k0 < N; k0 += PER) {
        const int k = k0 + kk;
        const bool mine = kk < PER && k < N;
        double v = 0.0;
        if(mine) {
            const int from = k + steps;
            v = nomp(P, from < N ? from : N - 1, b)[NOM_U + c];
        }
        __syncthreads();
        if(mine) nomp(P, k, b)[NOM_U + c] = v;
    }
}
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
