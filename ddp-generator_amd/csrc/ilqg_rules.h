/* The reference's per-trajectory rules of the outer iteration and of the box QP, stated once for the host
 * (ilqg_host.c, C) and for the device and the shim (ilqg_kernels.hip, HIP, through ilqg_device.hpp).  Every comparison
 * is written the way the reference writes it (max / min: include/iLQG.h), so host and device round the same way.  What
 * a caller does with lambda > lambdaMax stays at the caller: for a NaN lambda, !(lambda > lambdaMax) and
 * lambda <= lambdaMax are not the same test. */
#ifndef ILQG_RULES_H
#define ILQG_RULES_H

#include <math.h>

#ifdef __HIPCC__
#define ILQG_RULE __host__ __device__ __forceinline__
#else
#define ILQG_RULE static inline
#endif

/* raise the regularisation: iLQG.c:272-273 (failed backward pass), 342-343 (rejected step) */
ILQG_RULE void lambda_up(double lambdaFactor, double lambdaMin, double *lambda, double *dlambda) {
    const double t1 = *dlambda * lambdaFactor;
    *dlambda = (t1 > lambdaFactor) ? t1 : lambdaFactor;
    const double t2 = *lambda * *dlambda;
    *lambda = (t2 > lambdaMin) ? t2 : lambdaMin;
}

/* lower it: iLQG.c:298-299 (gradient exit), 317-318 (accepted step) */
ILQG_RULE void lambda_down(double lambdaFactor, double lambdaMin, double *lambda, double *dlambda) {
    const double t1 = *dlambda / lambdaFactor, t2 = 1.0 / lambdaFactor;
    *dlambda = (t1 < t2) ? t1 : t2;
    *lambda = *lambda * *dlambda * (*lambda > lambdaMin);
}

/* the gradient exit behind a successful backward pass: iLQG.c:297 */
ILQG_RULE int grad_converged(double g_norm, double tolGrad, double lambda) { return g_norm < tolGrad && lambda < 1e-5; }

/* expected reduction of step size alpha: line_search.c:43 */
ILQG_RULE double expected_reduction(double alpha, double dV0, double dV1) { return -alpha * (dV0 + alpha * dV1); }

/* the acceptance ratio, tested against zMin: line_search.c:44-48 */
ILQG_RULE double reduction_ratio(double dcost, double expected) { return (expected > 0) ? dcost / expected : 0.0; }

/* The box QP's constants (boxQP.c:52-57), exits and line-search rules.  The device's box QPs (box_qp, box_qp_row,
 * box_qp_quad, box_qp_rows) differ in how their lanes share the work, not in these. */
#define BOXQP_MAX_ITER 100
#define BOXQP_MIN_GRAD 1e-8
#define BOXQP_MIN_REL_IMPROVE 1e-8
#define BOXQP_STEP_DEC 0.6
#define BOXQP_MIN_STEP 1e-22
#define BOXQP_ARMIJO 0.1

/* return codes */
enum {
    BOXQP_ITER_LIMIT = 1,    /* maxIter iterations: boxQP.c:237 */
    BOXQP_STEP_LIMIT = 2,    /* the Armijo step fell below minStep: boxQP.c:223-224 */
    BOXQP_STALLED = 4,       /* relative improvement below minRelImprove: boxQP.c:85-86 */
    BOXQP_SMALL_GRAD = 5,    /* free gradient below minGrad: boxQP.c:149-150 */
    BOXQP_ALL_CLAMPED = 6,   /* boxQP.c:125-126 */
    BOXQP_NOT_PD = -1,       /* the free block's Cholesky factorisation failed: boxQP.c:141-142 */
    BOXQP_NO_DESCENT = -2    /* boxQP.c:193-195 */
};

/* The tests are macros, not ILQG_RULE functions, so that each box QP compiles to the instructions it had when it wrote
 * them out: a function's result is known to be defined, which lets the optimiser rewrite `rc == 0 && test` and the
 * branches around it differently, and the register allocation of the box QPs changes with it. */

/* the QP failed and the backward pass abandons the sweep (back_pass.c:167: qpRes < 1), or it succeeded */
#define BOXQP_FAILED(rc) ((rc) < 1)
#define BOXQP_OK(rc) ((rc) >= 1)

/* x (an lvalue) into the box, upper limit first: boxQP.c:63-64, 206-207 (a block, not do { } while(0), which would
 * change the compiled code) */
#define BOXQP_CLIP(x, lower, upper) \
    { \
        if((x) > (upper)) (x) = (upper); \
        if((x) < (lower)) (x) = (lower); \
    }

/* clamp classification, boxQP.c:105-110: at the lower limit -> 1, else at the upper limit -> 2, else free -> 0 */
#define BOXQP_AT_LOWER(x, lower, grad) ((x) <= (lower) && (grad) > 0)
#define BOXQP_AT_UPPER(x, upper, grad) ((x) >= (upper) && (grad) < 0)

/* the last iteration improved the value too little: boxQP.c:85 */
#define BOXQP_STALL(oldvalue, value) (((oldvalue) - (value)) < BOXQP_MIN_REL_IMPROVE * fabs(oldvalue))

/* gnorm2, the squared norm of the free gradient, is small enough: boxQP.c:112, 149 */
#define BOXQP_GRAD_SMALL(gnorm2) ((gnorm2) < BOXQP_MIN_GRAD * BOXQP_MIN_GRAD)

/* the Armijo test of the candidate value vc at step size step: boxQP.c:219 */
#define BOXQP_ARMIJO_OK(vc, oldvalue, step, sdotg) ((((vc) - (oldvalue)) / ((step) * (sdotg))) >= BOXQP_ARMIJO)

#endif /* ILQG_RULES_H */
