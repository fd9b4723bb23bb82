// Process noise drawn on the device from a seed: the ONE text of the draw, for k_policy_drawn (k_policy.inc: every lane draws
// the rows of its roll-out in registers) and k_noise_fill (below: the same draws written out as a table).  Included by
// ilqg_kernels.hip inside its anonymous namespace, in front of k_policy.inc.
//
// Generator.  Philox4x32-10 as Random123 defines it (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2,
// 3", SC11): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.  It has no state: a
// draw is a function of its counter and the key alone, so its bits do not depend on R, on the stream groups, on the shard
// or on what was drawn before — there is no table, no LDS and nothing kept between calls.
//     key      (seed & 0xffffffff, seed >> 32) of the caller's 64-bit seed
//     counter  (c0, c1, c2, c3) = (k, r, t, j):  k the step 0 .. N-1, r the roll-out within its trajectory, t the GLOBAL
//              trajectory index first_trajectory + b (with shared noise 0: every trajectory gets the draws of trajectory 0,
//              common random numbers), j the block of four state components 4j .. 4j+3
// Normals.  From the output words o0 .. o3, in fp64: ua = (o0 + 0.5) 2^-32, ub = (o1 + 0.5) 2^-32 (both exact, in (0, 1)),
//     rho = sqrt(-2 ln ua),   z[4j] = rho cos(2 pi ub),   z[4j+1] = rho sin(2 pi ub)
// (Box-Muller; sincospi of the exact argument 2 ub), o2 / o3 give z[4j+2], z[4j+3] the same way.  The smallest ua is 2^-33:
// THE TAIL ENDS AT 6.7 SIGMA (rho <= sqrt(66 ln 2) = 6.76).  Components >= NX are dropped.
// Disturbance.  w[i] = sigma[i] z[i], rounded to fp64 BEFORE it is added: draw, product and the add x_next + w are compiled
// with contraction off (the Makefile's -ffp-contract=fast-honor-pragmas honours the pragma), so a draw has the same bits in
// every kernel and every build that inlines it.
//
// What a launch needs of the caller lives in one small block in device memory (NoiseSpec, written by the shim in the order
// of the context's stream): a kernel takes ONE pointer, two scalar registers, and reads sigma and the key where it uses them.
struct NoiseSpec {
    unsigned key0, key1;  // seed & 0xffffffff, seed >> 32
    unsigned first;       // the global index of the context's trajectory 0 (first + B <= 2^32: checked by the shim)
    int shared;           // != 0: t = 0 for every trajectory
    double sigma[NX];     // the standard deviation of every state component (>= 0, finite: checked by the shim)
};

// ten rounds on the counter c under the key (k0, k1); c becomes the output
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for(int round = 0; round < 10; round++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (unsigned)p1;
        c[2] = n2;
        c[3] = (unsigned)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// the four standard normals of counter block (k, r, t, j)
__device__ __forceinline__ void noise_normals(double (&z)[4], unsigned key0, unsigned key1, unsigned k, unsigned r, unsigned t, unsigned j) {
#pragma clang fp contract(off)
    unsigned c[4] = {k, r, t, j};
    philox4x32_10(c, key0, key1);
#pragma unroll
    for(int h = 0; h < 2; h++) {
        const double ua = ((double)c[2 * h] + 0.5) * 0x1p-32, ub = ((double)c[2 * h + 1] + 0.5) * 0x1p-32;
        const double rho = sqrt(-2.0 * log(ua));
        double sn, cs;
        sincospi(2.0 * ub, &sn, &cs);
        z[2 * h] = rho * cs;
        z[2 * h + 1] = rho * sn;
    }
}

// row (k, r, t) of the disturbance: w[i] = sigma[i] z[i], i = 0 .. NX-1, block by block
__device__ __forceinline__ void noise_row(double (&w)[NX], const NoiseSpec *__restrict__ spec, unsigned k, unsigned r, unsigned t) {
#pragma clang fp contract(off)
    const unsigned key0 = spec->key0, key1 = spec->key1;
#pragma unroll
    for(int j = 0; j < (NX + 3) / 4; j++) {
        double z[4];
        noise_normals(z, key0, key1, k, r, t, (unsigned)j);
#pragma unroll
        for(int i = 4 * j; i < 4 * j + 4 && i < NX; i++) w[i] = spec->sigma[i] * z[i - 4 * j];
    }
}
// the trajectory word of the counter for the context's trajectory b
__device__ __forceinline__ unsigned noise_trajectory(const NoiseSpec *__restrict__ spec, int b) { return spec->shared ? 0u : spec->first + (unsigned)b; }

// The same draws as a table (ilqg_dev_noise_table): one lane per (b, r, k) writes w[b][r][k][0 .. NX), with shared noise one
// lane per (r, k) writes w[r][k] — rows = (shared ? 1 : B) * R * N, a size_t.  What ties the inline form to something a CPU
// can check, and a table for the plant loop or for a caller who adds a term of their own.
__global__ __launch_bounds__(256) void k_noise_fill(const NoiseSpec *__restrict__ spec, size_t rows, int R, int N, double *__restrict__ w) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if(g >= rows) return;
    const size_t br = g / (size_t)N;
    const int k = (int)(g - br * (size_t)N), b = (int)(br / (size_t)R), r = (int)(br - (size_t)b * (size_t)R);
    double row[NX];
    noise_row(row, spec, (unsigned)k, (unsigned)r, noise_trajectory(spec, b));
#pragma unroll
    for(int i = 0; i < NX; i++) w[g * NX + i] = row[i];
}
