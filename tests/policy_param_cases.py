"""TEST INFRASTRUCTURE — the parameter draws of BatchSolver.policy_rollout(params=...) and what a roll-out under them is
compared against: policy_cases.reference_rollout (the reference's forward_pass through the oracle driver) called with THAT
roll-out's parameter dict.  Beside tests/policy_cases.py; used by tests/test_policy_rollout_params_recipe.py (no GPU: every
reference roll-out under these draws is finite) and tests/test_gpu_policy_rollout_params.py.

Named parameters per build, deliberately NOT in paramdesc[] order.  A draw is value = nominal * (1 + SCALE * N(0, 1)),
element by element, fixed seed; row r = 0 of every trajectory is the nominal values bit for bit.  SCALE = 5 % is a choice
(a plant that differs visibly from the model, limits that keep their order), not a measurement."""
import numpy as np

R = 5
NAMED = {
    "carparking": ("limA", "d", "cf", "cx"),       # clamp, dynamics, final cost, running cost: W = 9
    "carparking_wave": ("limA", "d", "cf", "cx"),
    "hxtest": ("lim", "cf"),                       # limits that depend on the state
    "synth16x8": ("qf", "c", "lim"),               # W = 19: a row longer than a cache line
    "synth10hx": ("ru", "lim", "h"),
    "almix": ("tgt", "lim"),
}
PER_STEP = {"almix": "vref"}  # size -1: refused
SCALE = {name: 0.05 for name in NAMED}
SEED = 53


def width(params, names):
    return sum(np.size(params[n]) for n in names)


def draws(params, names, B, R=R, seed=SEED, scale=0.05):
    """{name: [B, R, size]} for the named parameters of the nominal dict `params`"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in names:
        nominal = np.asarray(params[n], dtype=np.float64).reshape(-1)
        t = nominal * (1.0 + scale * rng.standard_normal((B, R, nominal.size)))
        t[:, 0] = nominal
        out[n] = np.ascontiguousarray(t)
    return out


def nominal_table(params, names, B, R=R):
    """{name: [B, R, size]} with the batch's own value in every row"""
    return {n: np.ascontiguousarray(np.broadcast_to(np.asarray(params[n], dtype=np.float64).reshape(-1), (B, R, np.size(params[n])))) for n in names}


def params_of(params, table, b, r):
    """the parameter dict of roll-out (b, r): the nominal one with the named parameters replaced by the table's row"""
    return dict(params, **{n: t[b, r].copy() for n, t in table.items()})


def limits_ordered(table):
    """perturbed two-sided limits keep lower < upper (limA, limW, lim of size 2; hxtest's and synth10hx's lim are coefficients)"""
    return all(np.all(t[..., 0] < t[..., 1]) for n, t in table.items() if n.startswith("lim") and t.shape[-1] == 2)


def reference_ok_under(lib, n_hor, params, changed, opts, start, policy, alpha, feedback, cost=0.0, w_pen=(0.0, 0.0), multipliers=None):
    """forward_pass's return value (and cost) about `policy` from `start` under the nominal `params` with the entries of
    `changed` replaced — policy_cases.reference_rollout for parameters under which the driver's own initial roll-out need
    not be finite (a NaN time step): the driver starts under the nominal parameters and is given the others before the pass"""
    from oracle.harness import Driver
    x, u, l, L = (np.asarray(a, dtype=np.float64) for a in policy)
    if x.shape[0] == n_hor:
        x = np.concatenate([x, x[-1:]])
    d = Driver(lib, n_hor, params, opts)
    try:
        assert d.init(start, u) == 1
        d.set_state(x, u, cost, 1.0, w_pen)
        if multipliers is not None:
            d.set_multipliers(*multipliers)
        for n, v in changed.items():
            d.set_param(n, np.asarray(v, dtype=np.float64))
        if alpha == 0.0 and not feedback:
            return d.forward_pass(0.0)
        d.set_gains(l if alpha != 0.0 else np.zeros_like(l), L if feedback else np.zeros_like(L))
        return d.forward_pass(alpha if alpha != 0.0 else 1.0)
    finally:
        d.close()
