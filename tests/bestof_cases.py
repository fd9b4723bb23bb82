"""Candidates per agent, stated in numpy: what ilqg_batch_best_of chooses and what ilqg_batch_shift_winners hands the initial
roll-out (include/ilqg_batch.h).  A batch of B = G * K slots is G segments of K consecutive slots.  Plain loops, so that every
rule can be read off: eligibility, `<` on doubles, ties to the lowest index; the winner's plan as every slot's source, the tail,
the one fp64 add of du."""
import numpy as np

INIT_FAILED = 7    # ILQG_ST_INIT_FAILED
DERIVS_FAILED = 6  # ILQG_ST_DERIVS_FAILED: a status like any other here
SEGMENT_SIZES = (1, 2, 4, 8, 16, 32, 64)


def best_of_rule(score, status, K):
    """(winner [G] int32 batch-absolute or -1, best [G] — NaN for -1 —, n_eligible [G] int32)"""
    score, status = np.asarray(score, dtype=np.float64), np.asarray(status)
    B = score.shape[0]
    assert K in SEGMENT_SIZES and B % K == 0 and status.shape == (B,)
    G = B // K
    winner, best, n = np.full(G, -1, dtype=np.int32), np.full(G, np.nan), np.zeros(G, dtype=np.int32)
    for g in range(G):
        for b in range(g * K, g * K + K):
            if not np.isfinite(score[b]) or status[b] == INIT_FAILED:
                continue
            n[g] += 1
            if winner[g] < 0 or score[b] < best[g]:  # (ascending b and a strict `<`: ties stay with the lowest index)
                winner[g], best[g] = b, score[b]
    return winner, best, n


def shift_winners_rule(x, u, K, winner, steps, x0_new=None, u_tail=None, du=None):
    """(x0' [B, nx], u' [B, N, nu]) that init() receives: x [B, N+1, nx] and u [B, N, nu] are the current trajectories,
    winner [G] (-1: every slot of the segment is its own winner), x0_new [G, nx], u_tail [G, steps, nu], du [B, N, nu]"""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    B, N = u.shape[0], u.shape[1]
    assert K in SEGMENT_SIZES and B % K == 0 and 0 <= steps < N
    x0, un = np.empty_like(x[:, 0]), np.empty_like(u)
    for b in range(B):
        g = b // K
        w = int(winner[g])
        assert w == -1 or g * K <= w < g * K + K
        if w == -1:
            w = b
        un[b, :N - steps] = u[w, steps:]                                      # k + steps < N: u_w[k + steps]
        un[b, N - steps:] = u_tail[g] if u_tail is not None else u[w, N - 1]  # else u_tail[g][k + steps - N], or u_w[N-1] held
        if du is not None:
            un[b] = un[b] + du[b]  # the one fp64 add; without du nothing is added (-0.0 stays -0.0)
        x0[b] = x0_new[g] if x0_new is not None else x[w, steps]
    return x0, un
