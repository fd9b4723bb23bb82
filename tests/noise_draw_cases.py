"""The process noise the device draws (ddp-generator_amd/csrc/k_noise.inc), restated in numpy: what BatchSolver.noise_table
returns and policy_rollout(noise=(seed, sigma)) adds, for tests/test_noise_draw_recipe.py (which pins this file to
Random123's known answers and to N(0, 1)) and tests/test_gpu_policy_drawn.py (which holds the device to it).

    generator  Philox4x32-10 (Random123): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85
    key        (seed & 0xffffffff, seed >> 32)
    counter    (k, r, t, j): step, roll-out, GLOBAL trajectory first + b (shared: 0), block of the components 4j .. 4j+3
    normals    ua = (o0 + 0.5) 2^-32, ub = (o1 + 0.5) 2^-32, rho = sqrt(-2 ln ua), z[4j] = rho cos(2 pi ub),
               z[4j+1] = rho sin(2 pi ub); o2, o3 give z[4j+2], z[4j+3]; components >= nx are dropped
    table      w[b, r, k, i] = sigma[i] z[b, r, k, i], [B, R, N, nx], shared [R, N, nx]

`mutant` names one deliberate mistake (MUTANTS): a restatement that cannot tell them apart from the recipe pins nothing."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
MUTANTS = ("nine rounds", "swapped multipliers", "k and r exchanged", "b local", "o0 and o1 exchanged", "0.5 dropped", "sigma after the add")


def philox4x32_10(counter, key, rounds=10, multipliers=(M0, M1)):
    """counter [..., 4] and key [..., 2] (or (k0, k1)) of 32-bit words -> the output words [..., 4] as uint32"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & MASK for i in range(4)]
    key = np.asarray(key)
    k0, k1 = (key[..., i].astype(np.uint64) & MASK for i in range(2))
    m0, m1 = np.uint64(multipliers[0]), np.uint64(multipliers[1])
    for _ in range(rounds):
        p0, p1 = m0 * c[0], m1 * c[2]  # (32 x 32 bits: exact in 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def normals(o, half=0.5, exchanged=False):
    """output words [..., 4] -> the four standard normals [..., 4] of the block"""
    o = np.asarray(o).astype(np.float64)
    z = np.empty(o.shape)
    for h in (0, 1):
        a, b = o[..., 2 * h], o[..., 2 * h + 1]
        if exchanged:
            a, b = b, a
        ua, ub = (a + half) * 2.0 ** -32, (b + half) * 2.0 ** -32
        with np.errstate(divide="ignore"):
            rho = np.sqrt(-2.0 * np.log(ua))
        z[..., 2 * h], z[..., 2 * h + 1] = rho * np.cos(2.0 * np.pi * ub), rho * np.sin(2.0 * np.pi * ub)
    return z


def table(B, R, N, nx, seed, sigma, shared=False, first=0, mutant=None):
    """the table noise_table(R, seed, sigma, shared, first) returns for a batch of B trajectories and a horizon of N steps"""
    assert mutant is None or mutant in MUTANTS
    nb, blocks = (1 if shared else B), (nx + 3) // 4
    b, r, k, j = np.meshgrid(np.arange(nb, dtype=np.uint64), np.arange(R, dtype=np.uint64), np.arange(N, dtype=np.uint64),
                             np.arange(blocks, dtype=np.uint64), indexing="ij")
    t = b * np.uint64(0) if shared else b + np.uint64(0 if mutant == "b local" else first)
    assert int(t.max()) < 2 ** 32
    if mutant == "k and r exchanged":
        k, r = r, k
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    o = philox4x32_10(np.stack([k, r, t, j], axis=-1), np.array(key, dtype=np.uint64), rounds=9 if mutant == "nine rounds" else 10,
                      multipliers=(M1, M0) if mutant == "swapped multipliers" else (M0, M1))
    z = normals(o, half=0.0 if mutant == "0.5 dropped" else 0.5, exchanged=mutant == "o0 and o1 exchanged")
    z = z.reshape(nb, R, N, 4 * blocks)[..., :nx]
    sigma = np.asarray(sigma, dtype=np.float64)
    if mutant == "sigma after the add":
        # x' = sigma (x_next + z) where the rule is x' = x_next + sigma z: as a table, the push x' - x_next it amounts to at
        # the nominal state x_next = 1.  (At sigma = 1 the two rules are one rule, and nothing can tell them apart.)
        w = sigma * (1.0 + z) - 1.0
    else:
        w = sigma * z
    return w[0] if shared else w
