/* The reference's per-trajectory rules of the outer iteration, stated once for the host (ilqg_host.c, C) and for
 * the device and the shim (ilqg_kernels.hip, HIP).  Every comparison is written the way the reference's max / min
 * (include/iLQG.h) write it, so host and device round the same way.  What a caller does with lambda > lambdaMax stays
 * at the caller: for a NaN lambda, !(lambda > lambdaMax) and lambda <= lambdaMax are not the same test. */
#ifndef ILQG_RULES_H
#define ILQG_RULES_H

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

#endif /* ILQG_RULES_H */
