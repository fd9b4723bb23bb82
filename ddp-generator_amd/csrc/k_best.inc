// Candidates per agent (ilqg_dev_best_of, ilqg_dev_shift_winners): a batch of B = G * K slots read as G segments of K
// consecutive slots, one agent's candidate plans.  k_best_of picks each segment's winner, k_shift_winners_* is k_shift_* with
// one change of source: every slot of a segment takes the WINNER's plan in place of its own.  K is a power of two <= 64 and
// divides the group's size; groups and tiles are whole multiples of 64 trajectories, so a segment never straddles a group, a
// tile or a wavefront (the shim refuses anything else before a launch).

// One lane per slot.  A slot is eligible iff its score is finite and its status is not ILQG_ST_INIT_FAILED; the winner of a
// segment is its eligible slot with the smallest score, equal scores (`<` on doubles: -0.0 and 0.0 tie) to the lowest index.
// The pair (score, batch-absolute index) goes through log2 K exchange steps inside the wavefront; an ineligible lane carries
// the index NO_SLOT and loses against every eligible one, whatever its score.  After the exchange every lane of a segment holds
// the winner's own pair (so best[] is the winner's score bit for bit) and the count; lane 0 of the segment writes.  score ==
// nullptr: the slot's current cost.  Lanes >= B of a group's tail wavefront are ineligible and take part in the exchange.
constexpr int NO_SLOT = 0x7fffffff;  // the index an ineligible lane carries
__global__ void __launch_bounds__(WAVE) k_best_of(DevPtrs P, int K, int first, const double *__restrict__ score, int *__restrict__ winner,
                                                  double *__restrict__ best, int *__restrict__ n_eligible) {
    const int b = (int)(blockIdx.x * WAVE + threadIdx.x);
    const bool in = b < P.B;
    double v = in ? (score ? score[b] : P.f[ILQG_F_COST][b]) : 0.0;
    const int status = in ? P.i[ILQG_I_STATUS][b] : (int)ILQG_ST_INIT_FAILED;
    const bool finite = ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
    const bool ok = in && finite && status != ILQG_ST_INIT_FAILED;
    int at = ok ? first + b : NO_SLOT, n = ok ? 1 : 0;
    for(int m = 1; m < K; m <<= 1) {
        const double ov = __shfl_xor(v, m);
        const int oa = __shfl_xor(at, m);
        n += __shfl_xor(n, m);
        if(oa != NO_SLOT && (at == NO_SLOT || ov < v || (ov == v && oa < at))) {
            v = ov;
            at = oa;
        }
    }
    if(in && b % K == 0) {
        const int g = b / K;
        winner[g] = n ? at : -1;
        if(best) best[g] = n ? v : __longlong_as_double(0x7ff8000000000000ll);
        if(n_eligible) n_eligible[g] = n;
    }
}

// the slot (of this group) whose plan slot b takes: its segment's winner, which arrives batch-absolute (the group starts at
// `first`), or b itself where the segment has none: -1, or any value outside the segment — the device form cannot look
__device__ __forceinline__ int winner_slot(const int *__restrict__ winner, int K, int first, int b) {
    const int g = b / K, lo = first + g * K, w = winner[g];
    return (w >= lo && w < lo + K) ? w - first : b;
}

#if !ILQG_WAVE_MAP
// Lane mapping: k_shift_lane's scheme (k_shift.inc) — a workgroup of SHIFT_WAVES wavefronts owns 64 elements (tile, component,
// trajectory in tile) over all steps, reads a round of SHIFT_WAVES * SHIFT_UNROLL steps, passes a barrier, writes — with the
// source cur_u of the WINNER's slot (ILQG_I_LOC of the winner: X / U or a kept roll-out plane) and the destination the lane's
// own home_u.  All K members of a segment sit in the same 64 lanes of the same workgroup (same tile, same component), so the
// in-place argument carries over: a round reads steps [r0 + steps, r0 + round + steps) of winners and writes [r0, r0 + round)
// of everybody behind the barrier, the rounds before it wrote nothing beyond r0, and no other workgroup touches these
// columns; u_w[N-1], which the tail repeats, is written by the last round alone, behind its reads.  The tail steps take
// u_tail [segment][steps][NU] where given, and every step du [slot][N][NU] (one fp64 add, none without du), in the same pass.
// x0' = x0_new [segment][NX] or x_w[steps] goes to step 0 of X.  The caller clears ILQG_I_LOC behind the kernel.
__global__ void __launch_bounds__(WAVE * SHIFT_WAVES) k_shift_winners_lane(DevPtrs P, int K, int first, const int *__restrict__ winner, int steps,
                                                                           const double *__restrict__ x0_new, const double *__restrict__ u_tail,
                                                                           const double *__restrict__ du) {
    const int t = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6), N = P.N;
    const size_t e = (size_t)blockIdx.x * WAVE + t;
    if(w == 0 && e < (size_t)NX * P.Bp) {
        const int b = (int)(e / (NX * WAVE)) * WAVE + t, c = (int)((e / WAVE) % NX);
        if(b < P.B)
            home_x(P, 0, b)[(size_t)c * XSI] = x0_new ? x0_new[(size_t)(b / K) * NX + c] : cur_x(P, steps, winner_slot(winner, K, first, b))[(size_t)c * XSI];
    }
    if((size_t)blockIdx.x * WAVE >= (size_t)NU * P.Bp) return;  // (the whole workgroup)
    const int b = (int)(e / (NU * WAVE)) * WAVE + t, c = (int)((e / WAVE) % NU);
    const bool live = b < P.B;
    const double *src = live ? cur_u(P, 0, winner_slot(winner, K, first, b)) + (size_t)c * XSI : nullptr;
    const double *tail = (live && u_tail) ? u_tail + (size_t)(b / K) * steps * NU + c : nullptr;
    const double *add = (live && du) ? du + (size_t)b * N * NU + c : nullptr;
    double *dst = home_u(P, 0, b) + (size_t)c * XSI;
    const size_t us = cur_ustride(P);
    for(int r0 = 0; r0 < N; r0 += SHIFT_WAVES * SHIFT_UNROLL) {
        const int k0 = r0 + w * SHIFT_UNROLL;
        double v[SHIFT_UNROLL];
        if(live) {
#pragma unroll
            for(int j = 0; j < SHIFT_UNROLL; j++) {
                const int k = k0 + j, from = k + steps;
                if(from < N) v[j] = src[(size_t)from * us];
                else if(!tail) v[j] = src[(size_t)(N - 1) * us];  // the tail holds u_w[N-1]
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
#else
// Wave mapping: k_shift_wave gives a workgroup to a trajectory, this one to a SEGMENT.  It reads a block of SHIFT_BLOCK / NU
// steps of the winner's NOM_U entries (or of u_tail), passes a barrier, then writes the block into all K members' records
// (+ du), in k_shift_wave's ascending order of blocks: a block reads steps [k0 + steps, k0 + block + steps) of the winner and
// writes [k0, k0 + block) of the members, the winner among them; the blocks before it wrote nothing beyond k0, and u_w[N-1],
// which the tail repeats, is written by the last block alone, behind that block's reads.  No other workgroup touches the
// segment's records.  A segment without a winner (uniform in the workgroup) moves member by member, each from itself.
__global__ void __launch_bounds__(SHIFT_BLOCK) k_shift_winners_wave(DevPtrs P, int K, int first, const int *__restrict__ winner, int steps,
                                                                    const double *__restrict__ x0_new, const double *__restrict__ u_tail,
                                                                    const double *__restrict__ du) {
    const int g = blockIdx.x, t = threadIdx.x, N = P.N, b0 = g * K;
    if(b0 + K > P.B) return;  // (the whole workgroup)
    constexpr int PER = SHIFT_BLOCK / NU;  // steps per block
    const int kk = t / NU, c = t % NU;
    const int w = winner_slot(winner, K, first, b0);
    const bool own = w == b0 && winner[g] != first + b0;  // no winner: every member is its own
    if(t < NX)
        for(int m = 0; m < K; m++) nomp(P, 0, b0 + m)[NOM_X + t] = x0_new ? x0_new[(size_t)g * NX + t] : nomp(P, steps, own ? b0 + m : w)[NOM_X + t];
    for(int p = 0; p < (own ? K : 1); p++) {
        const int from_b = own ? b0 + p : w;
        for(int k0 = 0; k0 < N; k0 += PER) {
            const int k = k0 + kk;
            const bool mine = kk < PER && k < N;
            double v = 0.0;
            if(mine) {
                const int from = k + steps;
                if(from < N) v = nomp(P, from, from_b)[NOM_U + c];
                else v = u_tail ? u_tail[((size_t)g * steps + (from - N)) * NU + c] : nomp(P, N - 1, from_b)[NOM_U + c];
            }
            __syncthreads();
            if(mine)
                for(int m = own ? p : 0; m < (own ? p + 1 : K); m++) {
                    const int b = b0 + m;
                    nomp(P, k, b)[NOM_U + c] = du ? v + du[((size_t)b * N + k) * NU + c] : v;
                }
        }
    }
}
#endif
