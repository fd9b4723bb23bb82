// Candidates per agent (ilqg_dev_best_of, ilqg_dev_shift_winners): a batch of B = G * K slots read as G segments of K
// consecutive slots, one agent's candidate plans.  k_best_of picks each segment's winner, k_shift_winners_* is k_shift_* (the
// bodies of k_shift.inc) with another source: every slot of a segment takes the WINNER's plan in place of its own.  K is a
// power of two <= 64 and divides the group's size; groups and tiles are whole multiples of 64 trajectories, so a segment
// never straddles a group, a tile or a wavefront (the shim refuses anything else before a launch).

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
// The source of k_shift.inc's lane body (OwnPlan there): every slot is live and takes its segment's winner; x0' = x0_new
// [segment][NX] or x_w[steps]; the tail steps from u_tail [segment][steps][NU] where given, else u_w[N-1] held; du
// [slot][N][NU] added where given.
struct WinnersPlan {
    int K, first;
    const int *__restrict__ winner;
    const double *__restrict__ x0_new, *__restrict__ u_tail, *__restrict__ du;
    __device__ __forceinline__ bool live(const DevPtrs &P, int b, int) const { return b < P.B; }
    __device__ __forceinline__ bool sets_x0() const { return true; }
    __device__ __forceinline__ int from(int b) const { return winner_slot(winner, K, first, b); }
    __device__ __forceinline__ const double *x0(int b, int c) const { return x0_new ? x0_new + (size_t)(b / K) * NX + c : nullptr; }
    __device__ __forceinline__ const double *tail(int b, int steps, int c) const { return u_tail ? u_tail + (size_t)(b / K) * steps * NU + c : nullptr; }
    __device__ __forceinline__ const double *add(int b, int N, int c) const { return du ? du + (size_t)b * N * NU + c : nullptr; }
};

// Lane mapping.  All K members of a segment sit in the same 64 lanes of the same workgroup (same tile, same component), so the
// winner's column, which the members' lanes read, is moved by this workgroup and no other.
__global__ void __launch_bounds__(WAVE * SHIFT_WAVES) k_shift_winners_lane(DevPtrs P, int K, int first, const int *__restrict__ winner, int steps,
                                                                           const double *__restrict__ x0_new, const double *__restrict__ u_tail,
                                                                           const double *__restrict__ du) {
    shift_lane(P, steps, WinnersPlan{K, first, winner, x0_new, u_tail, du});
}
constexpr auto k_shift_winners = k_shift_winners_lane;
#else
// Wave mapping: k_shift_wave gives a workgroup to a trajectory, this one to a SEGMENT, so the winner's records, which are
// read for all K members, are moved by this workgroup and no other: one pass from the winner into all members, the winner
// among them.  A segment without a winner (uniform in the workgroup) moves member by member, each from itself.
__global__ void __launch_bounds__(SHIFT_BLOCK) k_shift_winners_wave(DevPtrs P, int K, int first, const int *__restrict__ winner, int steps,
                                                                    const double *__restrict__ x0_new, const double *__restrict__ u_tail,
                                                                    const double *__restrict__ du) {
    const int g = blockIdx.x, t = threadIdx.x, b0 = g * K;
    if(b0 + K > P.B) return;  // (the whole workgroup)
    const int w = winner_slot(winner, K, first, b0);
    const bool own = w == b0 && winner[g] != first + b0;  // no winner: every member is its own
    if(t < NX)
        for(int m = 0; m < K; m++) nomp(P, 0, b0 + m)[NOM_X + t] = x0_new ? x0_new[(size_t)g * NX + t] : nomp(P, steps, own ? b0 + m : w)[NOM_X + t];
    const int N = P.N;
    for(int p = 0; p < (own ? K : 1); p++)
        shift_wave(
            P, steps, own ? b0 + p : w, u_tail != nullptr, [&](int j, int c) { return u_tail[((size_t)g * steps + j) * NU + c]; },
            [&](int k, int c, double v) {
                for(int m = own ? p : 0; m < (own ? p + 1 : K); m++) {
                    const int b = b0 + m;
                    nomp(P, k, b)[NOM_U + c] = du ? v + du[((size_t)b * N + k) * NU + c] : v;
                }
            });
}
constexpr auto k_shift_winners = k_shift_winners_wave;
#endif
