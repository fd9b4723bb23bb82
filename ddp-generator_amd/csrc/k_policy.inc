// Roll-outs of every plan's feedback policy from starts of the caller (ilqg_dev_policy_rollout).  Included by
// ilqg_kernels.hip inside its anonymous namespace, behind k_rollout.inc (NomStep, NomPtrs, ROLL_BLOCK).
//
// k_policy: forward_pass (iLQG_func.tem:121-185) with o->x0 = the caller's start, the nominal = the POLICY of slot b —
// what k_head hands out: the current (x, u) where it lives (cur_x / cur_u: the tiled X / U, a kept roll-out plane of the
// line search, the records in the wave mapping) and the gains l, L of the packed records — the multipliers and penalty
// weights slot b has now, the per-time-step parameters as they stand, and
//     u_k = u_nom_k  [+ alpha l_k  if alpha != 0]  [+ L_k (x_k - x_nom_k)  if feedback, state by state in the template's order]
// then the step of the template: calcXVariableAux, clampU, calcXUVariableAux, ddpf, ddpL; the final step calcFVariableAux,
// ddpF.  Each is evaluated through run_step, as in k_rollout: the huge-argument second pass of sin / cos or, in builds with
// wave-uniform guards, run_guarded.  The control law is policy_control (below).  NOTHING of the batch is written: no field,
// scalar, status, location index or multiplier, and no trajectory moves home.
//
// Lanes.  One lane per roll-out, roll-out g = b * R + r with r fastest: R consecutive lanes share slot b and so every
// address of the nominal data.  A load instruction of a wavefront touches the data of at most ceil(64 / R) + 1 slots
// (lanes with equal addresses are served by one request), for R >= 64 of one or two, for R a multiple of 64 of exactly one.
// The next step's nominal data are requested while the step computes (k_rollout's scheme: loaded into the variables the
// step has just consumed); in the wave mapping L is too large to hold a step ahead and is read where it is used, as
// k_rollout does.  What alpha / feedback do not need is not loaded (l for alpha == 0; x_nom and L without feedback):
// both are kernel arguments, the branches are scalar ones.
//
// Outputs, all optional (null = not wanted): cost [B][R], ok [B][R] (forward_pass's return value: 0 as soon as a guarded
// value is NaN or Inf; the other outputs of such a roll-out are unspecified), x_end [B][R][NX], and the whole roll-out
// x [B][R][N+1][NX], u [B][R][N][NU] (u = the CLAMPED control that was applied).  x / u are trajectory-major per
// roll-out, so a lane's stores of a step are scattered 8-byte pieces, 64 cache lines per store instruction: accepted,
// because they are optional — the costs-only call does not pay for them (one wave-uniform branch per step, no store).
// A roll-out whose start is not finite ends at once with ok = 0.  All indices over B * R are size_t.
//
// Process noise (dist != null, a run-time argument as in k_plant: a null pointer is a wave-uniform branch and the call is
// the call without a table).  Behind every step k = 0 .. N-1 the roll-out's state is pushed,
//     x_{k+1} <- x_next + w[g][k]      (dist [B][R][N][NX]; with dist_shared != 0: w[r][k], dist [R][N][NX])
// the rule of k_plant: the control of step k + 1 is computed at the disturbed state, row N - 1 moves the state the final
// cost is evaluated at (x_end, x[N]).  ok = 0 as soon as a disturbed state is not finite, the one behind row N - 1
// included; such a lane stays out of the later guarded steps as one whose guard failed does.  A lane's row is NX doubles
// from its own 8-byte-aligned place, read right before the add: requested ahead of the step, as k_plant does with its
// one lane per trajectory, the row lives across the step and costs its registers (profiles/r17_policy_noise.txt).
// k_policy_drawn is the same roll-out with the row DRAWN in registers behind the step instead of read (below, k_noise.inc).
__device__ __forceinline__ void load_policy_step(NomStep &s, const NomPtrs &q, bool use_l, bool use_K) {
#pragma unroll
    for(int i = 0; i < NU; i++) s.u[i] = q.u[i * XSI];
    if(use_l) {
#pragma unroll
        for(int i = 0; i < NU; i++) s.l[i] = q.l[i];
    }
    if(use_K) {
#pragma unroll
        for(int i = 0; i < NX; i++) s.x[i] = q.x[i * XSI];
        if(!WAVE_MAP) {
#pragma unroll
            for(int i = 0; i < NXU; i++) s.K[i] = q.K[i];
        }
    }
}

// The control law of a policy at state x (iLQG_func.tem:146-155), for k_policy and k_plant (alpha = 0, use_l = false):
//     u = u_nom  [+ alpha l  if use_l]  [+ L (x - x_nom)  if use_K, state by state in the template's order]
// K_here: L of this step where it is read in the wave mapping (too large to hold a step ahead); the lane mapping has it in
// cur.  k_rollout and the fused search keep their own form (uf, selected on `feedback`): other arithmetic, and hot.
__device__ __forceinline__ void policy_control(double (&uin)[NU], const NomStep &cur, const double *K_here, const double (&x)[NX], double alpha,
                                               bool use_l, bool use_K) {
#pragma unroll
    for(int j = 0; j < NU; j++) uin[j] = cur.u[j];
    if(use_l) {
#pragma unroll
        for(int j = 0; j < NU; j++) uin[j] = cur.u[j] + cur.l[j] * alpha;
    }
    if(use_K) {
#pragma unroll
        for(int i = 0; i < NX; i++) {
            const double dx = x[i] - cur.x[i];
            if(WAVE_MAP) {
                const double *Kk = K_here + i * NU;
#pragma unroll
                for(int j = 0; j < NU; j++) uin[j] += Kk[j] * dx;
            } else {
#pragma unroll
                for(int j = 0; j < NU; j++) uin[j] += cur.K[j + i * NU] * dx;
            }
        }
    }
}

// One text for the policy roll-out kernels (k_policy_body.inc), included once per kernel and no forceinline body: a kernel's
// name is its timing slot and its resources, and with the roll-out in a function of its own the inliner treats the callbacks
// differently (see ILQG_FORWARD_STEP in ilqg_kernels.hip) — measured, k_policy<false> went from 1 293 to 1 221 instructions in
// CarParking's library and from 4 794 to 9 290 with 1 329 spilled registers in the n = 16 pair's.
//
// Process noise drawn on the device (spec: NoiseSpec in device memory, k_noise.inc).  Behind step k the lane draws the
// ceil(NX / 4) counter blocks (k, r, t, j) of its row and adds them where the table's row is added — the same rule, and with
// the table k_noise_fill writes for the same NoiseSpec the same bits in every output.  No table, no memory proportional to R.
//   N_X <= 8   a kernel of its own, k_policy_drawn: every k_policy instantiation is the code it was before there was a second
//              form (profiles/r23_policy_drawn.txt), and neither kernel uses scratch memory.
//   N_X > 8    (the problems whose roll-outs keep their trajEl_t in scratch memory, 3 472 to 48 432 bytes per lane) ONE
//              kernel, k_policy, with `spec` as a third run-time noise argument beside `dist` — null: the call as it was, a
//              wave-uniform branch per step.  A second kernel name would be a second kernel with scratch memory, which
//              tests/test_kernel_budget.py allows the names of tests/golden/kernel_scratch_parent.json only (the reason
//              `dist` is a run-time argument too).  The drawn launch still has its own timing slot: the slot is the shim's.
#if N_X > 8
#define ILQG_POLICY_ONE_KERNEL 1
#define ILQG_POLICY_KERNEL k_policy
#define ILQG_POLICY_DRAWN 2
#include "k_policy_body.inc"
#undef ILQG_POLICY_KERNEL
#undef ILQG_POLICY_DRAWN
#else
#define ILQG_POLICY_ONE_KERNEL 0
#define ILQG_POLICY_KERNEL k_policy
#define ILQG_POLICY_DRAWN 0
#include "k_policy_body.inc"
#undef ILQG_POLICY_KERNEL
#undef ILQG_POLICY_DRAWN

#define ILQG_POLICY_KERNEL k_policy_drawn
#define ILQG_POLICY_DRAWN 1
#include "k_policy_body.inc"
#undef ILQG_POLICY_KERNEL
#undef ILQG_POLICY_DRAWN
#endif
