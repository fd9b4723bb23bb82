"""TEST INFRASTRUCTURE — the plants, starts and disturbances of BatchSolver.receding_plant's tests, and the cases in which its
logs are held against policy_cases.reference_plant (the reference's forward_pass, one step at a time, under the PLANT's
parameter dict).  Used by tests/test_plant_reference_recipe.py (no GPU: the chain is the reference's own roll-out, and a wrong
reference would miss the GPU tests' bar by a wide margin), tests/test_gpu_receding_plant.py and tests/test_gpu_params_batch.py.

Builds, inputs, B = 70 and SLOTS are those of tests/test_gpu_policy_rollout.py; a plant's parameters are row 1 of the 5 % draws
of tests/policy_param_cases.py, its start x_0 + 0.1 N(0, I), its disturbance 0.01 N(0, I)."""
import numpy as np

import test_gpu_receding as base
from conftest import load_package
from oracle.harness import CAR_PARAMS
from params_batch_cases import dict_of, rows
from policy_cases import perturbed_starts
from policy_param_cases import NAMED, SCALE, draws, limits_ordered, params_of
from test_gpu_policy_rollout import B, SLOTS  # noqa: F401

ROUNDS = 3
# what a plant names, per build: tests/policy_param_cases.py's names, and for hxtest the weights of its running cost as well —
# `lim` and `cf` reach a step's cost only through the state and the clamp, which leaves the applied cost of some compared
# slots within 1e-6 of the cost under the model's parameters (tests/test_plant_reference_recipe.py asks for more)
PLANT_NAMED = dict(NAMED, hxtest=NAMED["hxtest"] + ("cx",))
SHORT_N = 6  # the short horizon: steps = SHORT_N - 1 is the largest step count the entry accepts
# the seed of the short horizon's plant rows.  Under the seed of tests/policy_param_cases.py the two draws of cx nearly cancel
# in slot 69's first step (its cost moves by 1.7e-8, the reference's own numbers); 54 is the next seed, and every compared
# slot's one-step cost then moves by 2.3e-5 or more
SHORT_SEED = 54


def plant_rows(c, names=None, batch=B, seed=None):
    """(table [batch, 2, size] per name, rows [batch, size] per name): 5 % draws; row 1 of a draw, row 0 being the nominal values.
    seed None: the case's own (`plant_seed`, the short horizon's), else that of tests/policy_param_cases.py"""
    seed = getattr(c, "plant_seed", None) if seed is None else seed
    kw = {} if seed is None else dict(seed=seed)
    t = draws(c.params, names or PLANT_NAMED[c.name], batch, 2, scale=SCALE[c.name], **kw)
    assert limits_ordered(t)
    return t, {n: np.ascontiguousarray(a[:, 1]) for n, a in t.items()}


def plant_starts(c, seed=17):
    return np.ascontiguousarray(perturbed_starts(c.x0, 2, seed=seed)[:, 1])


def noise(c, steps, rounds=ROUNDS, last_only=False, batch=B, seed=3, sigma=0.01):
    w = sigma * np.random.default_rng(seed).standard_normal((batch, rounds * steps, c.nx))
    if last_only:
        keep = np.zeros(rounds * steps, dtype=bool)
        keep[steps - 1::steps] = True
        w[:, ~keep] = 0.0
    return w


def short_car(batch=B):
    """(n_hor, params, x0, u0): CarParking with a horizon of SHORT_N steps"""
    x0, u0 = load_package().synth.car_batch(batch, SHORT_N)
    return SHORT_N, CAR_PARAMS, x0, u0


def both_and_other(name, declared):
    """the two parameters a plant names on top of a per-trajectory batch (tests/test_gpu_params_batch.py, test 7): one that the
    trajectories' rows name too and the first fixed-size one, in the order the problem declares them, that they do not"""
    return BOTH[name], next(n for n, size in declared if size > 0 and n not in NAMED[name])


# the parameter named by the trajectory's row AND by the plant's: one that the first plant steps of every compared slot read
# with effect, so that the order of the two overrides shows — a weight of the running cost, a coefficient of the dynamics
# (lim[3] of hxtest).  CarParking's limA, the first of its names, reaches a result only where the clamp is active.
BOTH = {"carparking": "cx", "hxtest": "lim"}


def plant_over_rows(name, params, declared, batch=B):
    """(table, mine, plant_table, plant_rows): the trajectories' rows of tests/params_batch_cases.py and, drawn apart from them,
    the plants' rows for both_and_other's two names"""
    table, mine = rows(name, params, batch=batch)
    plant_table = draws(params, both_and_other(name, declared), batch, 2, seed=71, scale=SCALE[name])
    assert limits_ordered(plant_table)
    return table, mine, plant_table, {n: np.ascontiguousarray(a[:, 1]) for n, a in plant_table.items()}


class CpuCase:
    """one build's inputs with the attributes plant_rows, plant_starts and noise read from the GPU tests' Case"""

    def __init__(self, name, n_hor=None):
        self.name = name
        if n_hor is None:
            self.problem, self.fd, _, self.N, self.params, self.opts, self.x0, self.u0 = base.setup(name, B)
        else:
            assert name == "carparking" and n_hor == SHORT_N
            self.problem, self.fd, self.opts = "carparking", 0, {}
            self.N, self.params, self.x0, self.u0 = short_car()
            self.plant_seed = SHORT_SEED
        self.nx = self.x0.shape[1]


def model_and_plant(c, kind, declared=None):
    """(model(s), plant(s), swapped(s) or None, rows): the parameter dicts slot s plans and its plant runs under.
    kind "shared": the batch's parameters and the plant's row over them.  kind "rows": the trajectory's row, the plant's row
    on top of it, and — the wrong order — the trajectory's row on top of the plant's for the parameter both name."""
    if kind == "shared":
        table, prow = plant_rows(c)
        return (lambda s: c.params), (lambda s: params_of(c.params, table, s, 1)), None, prow
    table, _, plant_table, prow = plant_over_rows(c.name, c.params, declared)
    both = BOTH[c.name]
    assert both in table and both in plant_table

    def swapped(s):
        return dict(params_of(dict_of(c.params, table, s), plant_table, s, 1), **{both: table[both][s, 1].copy()})

    return (lambda s: dict_of(c.params, table, s)), (lambda s: params_of(dict_of(c.params, table, s), plant_table, s, 1)), swapped, prow
