"""ctypes view of the batched iLQG C-ABI (include/ilqg_batch.h).

This module holds no numerics: every method forwards to the shared library
built from ddp-generator_amd/csrc (C host + HIP kernels).  If that library is
missing the import of a solver FAILS LOUDLY — there is no Python or CPU
fallback for the hot path.

Naming follows the reference's MEX entry
`[success, x, u, cost] = iLQG<Problem>(x0, u_nom, params, opts)`
(iLQG_mex.c:19-52): parameters by name, options by name, same option keys and
error messages (iLQG.c:91-216).
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.environ.get("ILQG_LIBDIR", os.path.join(HERE, "lib"))  # override: experiments with other builds

_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")

STATUS = {0: "active", 1: "converged_grad", 2: "converged_fun", 3: "max_iter", 4: "no_descent",
          5: "lambda_max", 6: "derivs_failed", 7: "init_failed"}
# the reference's iLQG() return value for each exit (1 = "success", iLQG.c:365-378 and SURVEY Appendix B-11).
# Exit 6 (calc_derivs failed) is not in the table: iLQG() leaves its loop with the back-pass flag of the PREVIOUS
# iteration (iLQG.c:247-249, 367), i.e. returns 1 unless it happened in the very first iteration — see success().
REFERENCE_SUCCESS = {1: 1, 2: 1, 5: 1, 3: 0, 4: 0, 7: 0}

MAX_ALPHA = 16


class IlqgError(RuntimeError):
    pass


_extra_libdirs = []


def add_library_dir(path):
    """another directory problem libraries are looked up in (a `make ... LIBDIR=<dir>` of the caller: a problem built
    from its own <problem>_gen_files/)"""
    path = os.path.abspath(path)
    if path not in _extra_libdirs:
        _extra_libdirs.append(path)


def library_path(problem="carparking", full_ddp=0, strict=False):
    """strict=True: the -ffp-contract=off build (bit-for-bit CPU parity of the backward pass; tests only);
    strict="wave": the build of a small problem forced into the one-wavefront-per-trajectory mapping;
    strict="elem": the n = 16 problem built with the one-output-element-per-lane backward step (FMA-free);
    strict="lean": the n = 16 problem's product build with the quad step laid out for two wavefronts per SIMD;
    strict="exp" / "exp_strict": the -DILQG_EXPERIMENTS builds (measured negative results kept tested: the backward pass
    on two wavefronts, the derivative record in parts, the box QP's pattern tables), product / FMA-free;
    strict="direct": the hint-free n = 16 pair with its callbacks on the record itself (-DILQG_DEV_ELEMENT=0: comparison)"""
    suffix = "_" + strict if strict in ("wave", "elem", "lean", "exp", "exp_strict", "direct") else ("_strict" if strict else "")
    name = "libilqg_%s_fd%d_hip%s.so" % (problem, int(full_ddp), suffix)
    for d in [LIBDIR] + _extra_libdirs:
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return os.path.join(LIBDIR, name)


_libs = {}


class _Named(C.Structure):
    """ilqg_named_t of include/ilqg_batch.h"""
    _fields_ = [("name", C.c_char_p), ("value", C.POINTER(C.c_double)), ("n", C.c_int)]


def _named_list(items):
    keep = []  # the arrays must outlive the call
    arr = (_Named * max(1, len(items)))()
    for i, (k, v) in enumerate(items.items()):
        a = np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64)
        keep.append(a)
        arr[i] = _Named(k.encode(), a.ctypes.data_as(C.POINTER(C.c_double)), a.size)
    return arr, len(items), keep


def _optional(a, shape):
    """an optional array argument: None, or the C-contiguous doubles of that shape"""
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


def _address(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _is_cuda(a):
    """a torch tensor in GPU memory (asked of the object: torch is not imported for the question)"""
    return bool(getattr(a, "is_cuda", False))


def _cuda_address(a, shape, device, what):
    """the device address of an optional CUDA tensor argument, which must be what the library reads as it is: float64,
    contiguous, of the documented shape, on the solver's device.  Checked here, before any library call."""
    if a is None:
        return None
    if "float64" not in str(a.dtype):
        raise IlqgError("%s: a tensor on the device must be float64, not %s" % (what, a.dtype))
    if tuple(a.shape) != tuple(shape):
        raise IlqgError("%s: shape %s, expected %s" % (what, tuple(a.shape), tuple(shape)))
    if not a.is_contiguous():
        raise IlqgError("%s: a tensor on the device must be contiguous" % what)
    if a.device.index != device:
        raise IlqgError("%s: on %s, the solver is on GPU %d" % (what, a.device, device))
    return C.c_void_p(a.data_ptr() or None)


def _cuda_int_address(a, shape, device, what):
    """_cuda_address for an int32 tensor (the winners of best_of / shift_winners)"""
    if "int32" not in str(a.dtype):
        raise IlqgError("%s: a tensor on the device must be int32, not %s" % (what, a.dtype))
    if tuple(a.shape) != tuple(shape):
        raise IlqgError("%s: shape %s, expected %s" % (what, tuple(a.shape), tuple(shape)))
    if not a.is_contiguous():
        raise IlqgError("%s: a tensor on the device must be contiguous" % what)
    if a.device.index != device:
        raise IlqgError("%s: on %s, the solver is on GPU %d" % (what, a.device, device))
    return C.c_void_p(a.data_ptr() or None)


SEGMENT_SIZES = (1, 2, 4, 8, 16, 32, 64)


def _segments(who, B, K):
    """the number of segments of K consecutive slots in a batch of B (include/ilqg_batch.h, candidates per agent)"""
    try:
        ok = int(K) == K and int(K) in SEGMENT_SIZES
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise IlqgError("%s: K = %r, must be one of 1, 2, 4, 8, 16, 32, 64" % (who, K))
    if B % int(K):
        raise IlqgError("%s: K = %d does not divide the batch of %d trajectories (B %% K must be 0)" % (who, int(K), B))
    return B // int(K)


def _host_shaped(who, what, a, shape, dtype=np.float64):
    """an optional host array argument of exactly that shape (no broadcasting, no reshaping of another size)"""
    if a is None:
        return None
    if _is_cuda(a):
        raise IlqgError("%s: %s is a tensor on the device and another argument is in host memory: pass all of them the same way" % (who, what))
    a = np.asarray(a)
    if a.shape != tuple(shape):
        raise IlqgError("%s: %s has shape %s, expected %s" % (who, what, a.shape, tuple(shape)))
    return np.ascontiguousarray(a, dtype=dtype)


def _best_of(solver, prefix, K, score, device):
    """BatchSolver.best_of / MultiSolver.best_of"""
    who = "best_of"
    G = _segments(who, solver.B, K)
    if not device:
        entry = _receding_entry(solver.lib, prefix + "best_of")
        if _is_cuda(score):
            raise IlqgError("best_of: score is a tensor on the device: pass device=True")
        score = _host_shaped(who, "score", score, (solver.B,))
        winner, best, n = np.full(G, -1, dtype=np.int32), np.zeros(G), np.zeros(G, dtype=np.int32)
        solver._ck(entry(solver.h, int(K), _address(score), _address(winner), _address(best), _address(n)))
        return winner, best, n
    entry = _receding_entry(solver.lib, prefix + "best_of_device")
    if score is not None and not _is_cuda(score):
        raise IlqgError("best_of: score is in host memory: with device=True it is a float64 torch tensor on the solver's GPU")
    ps = _cuda_address(score, (solver.B,), solver.device, "best_of: score")
    torch, dev, stream = _torch_stream(solver.device)
    winner = torch.empty(G, dtype=torch.int32, device=dev)
    best = torch.empty(G, dtype=torch.float64, device=dev)
    n = torch.empty(G, dtype=torch.int32, device=dev)
    solver._ck(entry(solver.h, int(K), ps, *[C.c_void_p(t.data_ptr() or None) for t in (winner, best, n)], stream))
    return winner, best, n


def _shift_winners(solver, prefix, K, winner, steps, x0, u_tail, du, may_be_device):
    """BatchSolver.shift_winners / MultiSolver.shift_winners"""
    who = "shift_winners"
    G = _segments(who, solver.B, K)
    nx, nu, n = solver.problem.nx, solver.problem.nu, max(int(steps), 0)
    if winner is None:
        raise IlqgError("shift_winners: winner is None (one slot index per segment, [B / K]; -1 for a segment whose slots keep their own plans)")
    args = (("winner", winner, (G,)), ("x0", x0, (G, nx)), ("u_tail", u_tail, (G, n, nu)), ("du", du, (solver.B, solver.N, nu)))
    if any(_is_cuda(a) for _, a, _ in args):
        if not may_be_device:
            raise IlqgError("shift_winners: MultiSolver takes host arrays only")
        entry = _receding_entry(solver.lib, prefix + "shift_winners_device")
        for what, a, _ in args:
            if a is not None and not _is_cuda(a):
                raise IlqgError("shift_winners: %s is in host memory and another argument on the device: pass all of them the same way" % what)
        pw = _cuda_int_address(winner, (G,), solver.device, "shift_winners: winner")
        ptr = [_cuda_address(a, shape, solver.device, "shift_winners: " + what) for what, a, shape in args[1:]]
        solver._ck(entry(solver.h, int(K), pw, int(steps), *ptr, _torch_stream(solver.device)[2]))
        return
    entry = _receding_entry(solver.lib, prefix + "shift_winners")
    w = np.asarray(winner)
    if w.shape != (G,) or not np.issubdtype(w.dtype, np.integer):
        raise IlqgError("shift_winners: winner must be %d integers (one per segment, [B / K]), not %s of shape %s" % (G, w.dtype, w.shape))
    w = np.ascontiguousarray(w, dtype=np.int32)
    host = [_host_shaped(who, what, a, shape) for what, a, shape in args[1:]]
    solver._ck(entry(solver.h, int(K), _address(w), int(steps), *[_address(a) for a in host]))


def _outputs(shapes, order, torch=None, dev=None):
    """(the outputs of one library call, their addresses in the entry's order — None for one left out): numpy arrays, or
    with torch tensors on `dev`; float64 but for `ok`"""
    if torch is None:
        out = {k: np.zeros(shape, dtype=np.int32 if k == "ok" else np.float64) for k, shape in shapes.items()}
        return out, [_address(out.get(k)) for k in order]
    out = {k: torch.empty(shape, dtype=torch.int32 if k == "ok" else torch.float64, device=dev) for k, shape in shapes.items()}
    return out, [C.c_void_p(out[k].data_ptr() or None) if k in out else None for k in order]


def _head_outputs(solver, steps, gains, torch=None, dev=None):
    """the outputs of head(): see _outputs"""
    B, n, nx, nu = solver.B, max(int(steps), 0), solver.problem.nx, solver.problem.nu
    shapes = dict(x=(B, n, nx), u=(B, n, nu), cost=(B,))
    if gains:
        shapes.update(l=(B, n, nu), L=(B, n, nu * nx))
    return _outputs(shapes, ("x", "u", "l", "L", "cost"), torch, dev)


def _rollout_outputs(solver, R, trajectories, torch=None, dev=None):
    """the outputs of policy_rollout(): see _outputs"""
    B, N, nx, nu = solver.B, solver.N, solver.problem.nx, solver.problem.nu
    shapes = dict(cost=(B, R), ok=(B, R), x_end=(B, R, nx))
    if trajectories:
        shapes.update(x=(B, R, N + 1, nx), u=(B, R, N, nu))
    return _outputs(shapes, ("cost", "ok", "x_end", "x", "u"), torch, dev)


def _policy_starts(x0, B, nx):
    """the starts of policy_rollout as [B, R, nx] C-contiguous doubles: given so, or as [R, nx] for every trajectory"""
    a = np.asarray(x0, dtype=np.float64)
    if a.ndim == 2 and a.shape[1] == nx:
        a = np.broadcast_to(a, (B,) + a.shape)
    if a.ndim != 3 or a.shape[0] != B or a.shape[2] != nx or a.shape[1] < 1:
        raise IlqgError("policy_rollout: x0 has shape %s, expected (%d, R, %d) or (R, %d) with n_starts = R >= 1" % (tuple(a.shape), B, nx, nx))
    return np.ascontiguousarray(a)


def _param_size(problem, who, what, name):
    """the size of the problem's parameter `name` (-1: one value per time step); refused here as the library refuses it: a
    name that is no parameter"""
    known = dict(problem.params)
    if name not in known:
        raise IlqgError("%s: %s: Parameter name '%s' is not member of parameters struct." % (who, what, name))
    return known[name]


def _named_sizes(who, problem, params, shared_by):
    """the sizes of the fixed-size parameters the dict `params` names, in dict order; refused here as the library refuses
    them: a name that is no parameter, and one with a value per time step (those stay shared by `shared_by`)"""
    sizes = [_param_size(problem, who, "params", name) for name in params]
    for name, size in zip(params, sizes):
        if size < 1:
            raise IlqgError("%s: params: '%s' has one value per time step; per-time-step parameters stay shared by %s" % (who, name, shared_by))
    return sizes


def _host_numbers(who, what, a):
    """a host array argument as doubles, whatever its dtype and strides; refused: a tensor on the device"""
    if _is_cuda(a):
        raise IlqgError("%s: %s is a tensor on the device: pass device=True" % (who, what))
    return np.asarray(a, dtype=np.float64)


def _plant_numbers(who, what, a):
    """a host array argument of receding_plant, which has no device form; refused too: a dtype that is no real number"""
    if _is_cuda(a):
        raise IlqgError("%s: %s is a tensor on the device: the loop takes host memory (numpy arrays)" % (who, what))
    a = np.asarray(a)
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise IlqgError("%s: %s has dtype %s, expected real numbers (float64)" % (who, what, a.dtype))
    return a.astype(np.float64, copy=False)


def _plant_array(a, shape, what):
    """a host array argument of receding_plant as C-contiguous doubles of that shape"""
    a = _plant_numbers("receding_plant", what, a)
    if tuple(a.shape) != tuple(shape):
        raise IlqgError("receding_plant: %s has shape %s, expected %s" % (what, tuple(a.shape), tuple(shape)))
    return np.ascontiguousarray(a)


def _param_names(params):
    return (C.c_char_p * len(params))(*[name.encode() for name in params])


def _named_rows(who, problem, params, leads, shared_by, hint, column):
    """The table of rows a call gives by name, params = {name: array}: (names, [(array, its shape in the table)], form).
    `leads` are the admissible leading shapes — (B, R) or (R,) for roll-outs, (B,) for the planner's and the plant's tables —
    and every array is leads[form] + (size,), all in ONE form; the last axis may be left out for size 1.  column(who, what,
    a) makes of an argument what has a shape, or refuses it.  The named parameters stand one behind the other in dict order."""
    cols, forms = [], []
    for (name, a), size in zip(params.items(), _named_sizes(who, problem, params, shared_by)):
        what = "params['%s']" % name
        a = column(who, what, a)
        shape = tuple(int(n) for n in a.shape)
        full, short = [lead + (size,) for lead in leads], list(leads) if size == 1 else []
        if shape not in full + short:
            raise IlqgError("%s: %s has shape %s, expected %s%s" % (who, what, shape, " or ".join(str(f) for f in full + short), hint))
        forms.append((full + short).index(shape) % len(leads))
        cols.append((a, full[forms[-1]]))
    if len(set(forms)) != 1:
        raise IlqgError("%s: params mixes %s: every array in one form"
                        % (who, " with ".join("[%s] (%s)" % (", ".join([str(n) for n in leads[f]] + ["size"]), ", ".join(n for n, g in zip(params, forms) if g == f))
                                              for f in sorted(set(forms), reverse=True))))
    return _param_names(params), cols, forms[0]


def _pack_arrays(who, problem, params, leads, shared_by, hint="", column=_host_numbers):
    """_named_rows of host arrays: (names, the table [leads[form] + (W,)] as C-contiguous doubles, form)"""
    names, cols, form = _named_rows(who, problem, params, leads, shared_by, hint, column)
    return names, np.ascontiguousarray(np.concatenate([a.reshape(shape) for a, shape in cols], axis=-1)), form


def _pack_tensors(who, problem, params, leads, shared_by, device, hint=""):
    """_named_rows of contiguous float64 torch tensors on the solver's GPU, checked and not yet packed (_tensor_table)"""
    def column(who, what, a):
        if not _is_cuda(a):
            raise IlqgError("%s: %s is in host memory and device=True: pass a float64 torch tensor on the solver's GPU" % (who, what))
        _cuda_address(a, a.shape, device, "%s: %s" % (who, what))
        return a
    return _named_rows(who, problem, params, leads, shared_by, hint, column)


def _tensor_table(torch, dev, cols):
    """the address of the table of _pack_tensors, packed with torch.cat on torch's current stream; a single tensor is the
    table as it lies ([B] and [B, 1] are the same memory).  (address, what must outlive the call)"""
    with torch.cuda.device(dev):
        values = cols[0][0] if len(cols) == 1 else torch.cat([a.reshape(shape) for a, shape in cols], dim=-1)
    return C.c_void_p(values.data_ptr() or None), values


def _rollout_params(solver, params, R, device=None):
    """(names, table or tensor columns, shared) of policy_rollout(params=...)"""
    who, B = "policy_rollout", solver.B
    if not isinstance(params, dict) or not params:
        raise IlqgError("policy_rollout: params must be a non-empty dict of parameter name -> array ([B, R, size], or [R, size] for every trajectory)")
    args = (who, solver.problem, params, ((B, R), (R,)), "all roll-outs")
    hint = ", with R = %d as in x0" % R
    return _pack_arrays(*args, hint=hint) if device is None else _pack_tensors(*args, device, hint=hint)


def _param_steps_name(problem, who, name):
    """the name of a per-time-step parameter for set_param_steps_batch / shift_param_batch; refused here as the library refuses it"""
    size = _param_size(problem, who, "name", name)
    if size != -1:
        raise IlqgError("%s: name: '%s' has a fixed size of %d, not one value per time step: fixed-size parameters per trajectory "
                        "are set by set_params_batch" % (who, name, size))
    return name.encode()


def _param_steps_rows(who, what, a, shape, device, gpu):
    """the rows [B, n_hor+1] (or a tail [B, steps]) of a per-time-step parameter as the library reads them: (address, keep).
    Host arrays are copied as C-contiguous doubles whatever their dtype and strides; with device=True a contiguous float64
    torch tensor on the solver's GPU is read where it is."""
    if not device:
        a = _host_numbers(who, what, a)
        if tuple(a.shape) != tuple(shape):
            raise IlqgError("%s: %s has shape %s, expected %s" % (who, what, tuple(a.shape), tuple(shape)))
        a = np.ascontiguousarray(a)
        return _address(a), a
    if not _is_cuda(a):
        raise IlqgError("%s: %s is in host memory and device=True: pass a float64 torch tensor on the solver's GPU" % (who, what))
    return _cuda_address(a, shape, gpu, "%s: %s" % (who, what)), a


def _windows(solver, who, windows, rounds, steps):
    """the windows of receding(windows=...) / receding_plant(windows=...): (n_windows, the array of names, the array of
    pointers to the futures, what must outlive the call).  windows = {name: array or None}: every name a per-time-step
    parameter, its future [B, rounds*steps] where the name currently has rows (set_param_steps_batch), [rounds*steps] where it
    is shared, None: the window holds its last value.  Checked here, before any library call."""
    if not isinstance(windows, dict):
        raise IlqgError("%s: windows must be a dict of per-time-step parameter name -> future array (or None: hold the last value); "
                        "{} moves every window holding its last value, windows=None calls the loop without windows" % who)
    n = max(int(rounds), 0) * max(int(steps), 0)
    rows = getattr(solver, "_step_rows", ())
    names, keep = [], []
    for name, a in windows.items():
        names.append(_param_steps_name(solver.problem, who, name))
        if a is None:
            keep.append(None)
            continue
        what = "windows['%s']" % name
        a = _plant_numbers(who, what, a)
        shape = (solver.B, n) if name in rows else (n,)
        if tuple(a.shape) != shape:
            raise IlqgError("%s: %s has shape %s, expected %s = %s: the name %s" % (
                who, what, tuple(a.shape), shape, "(B, rounds*steps)" if name in rows else "(rounds*steps,)",
                "currently has rows per trajectory (set_param_steps_batch)" if name in rows else "is currently shared by all trajectories"))
        keep.append(np.ascontiguousarray(a))
    if not names:
        return 0, None, None, keep
    return (len(names), (C.c_char_p * len(names))(*names), (C.c_void_p * len(names))(*[None if a is None else a.ctypes.data for a in keep]), keep)


def _note_step_rows(solver, name, on):
    """the solver remembers which per-time-step names have rows per trajectory (the shape of a window's future depends on it)"""
    rows = set(getattr(solver, "_step_rows", ()))
    (rows.add if on else rows.discard)(name)
    solver._step_rows = rows


def _receding_plant(solver, entry, rounds, steps, iterations, feedback, x_plant, params, disturbance, windows=None):
    """BatchSolver.receding_plant / MultiSolver.receding_plant: the checks, the arrays and the one library call"""
    B, nx, nu = solver.B, solver.problem.nx, solver.problem.nu
    for what, v in (("rounds", rounds), ("steps", steps), ("iterations", iterations)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise IlqgError("receding_plant: %s must be an integer, not %r" % (what, v))
    r, n = max(int(rounds), 0), max(int(rounds), 0) * max(int(steps), 0)
    xp = None if x_plant is None else _plant_array(x_plant, (B, nx), "x_plant").copy()
    dist = None if disturbance is None else _plant_array(disturbance, (B, n, nx), "disturbance")
    if params is not None and (not isinstance(params, dict) or not params):
        raise IlqgError("receding_plant: params must be a non-empty dict of parameter name -> array [B, size], or None for a plant that is the model")
    names, values, _ = (None, None, 0) if params is None else _pack_arrays("receding_plant", solver.problem, params, ((B,),), "planner and plant",
                                                                           column=_plant_numbers)
    moving = ()
    if windows is not None:
        n_windows, window_names, futures, keep = _windows(solver, "receding_plant", windows, rounds, steps)
        entry, moving = entry + "_windows", (n_windows, window_names, futures)
    out = dict(x=np.zeros((B, n, nx)), u=np.zeros((B, n, nu)), cost=np.zeros((B, r)), plan_cost=np.zeros((B, r)), ok=np.zeros(B, dtype=np.int32),
               x_plant=xp)
    solver._ck(_receding_entry(solver.lib, entry)(solver.h, int(rounds), int(steps), int(iterations), 1 if feedback else 0, _address(xp),
                                                  0 if names is None else len(names), names, _address(values), _address(dist), *moving,
                                                  *[_address(out[k]) for k in ("x", "u", "cost", "plan_cost", "ok")]))
    return out


def _rollout_disturbance(solver, disturbance, R, device=None):
    """(address, disturbance_shared, what must outlive the call) of policy_rollout(disturbance=...): [B, R, N, nx], or
    [R, N, nx] for every trajectory; a host array of real numbers, or with `device` a contiguous float64 torch tensor on that
    GPU, read where it is.  Checked here, before any library call."""
    who, what = "policy_rollout", "disturbance"
    full, short = (solver.B, R, solver.N, solver.problem.nx), (R, solver.N, solver.problem.nx)
    if device is None:
        a = _host_numbers(who, what, disturbance) if _is_cuda(disturbance) else _plant_numbers(who, what, disturbance)  # (the first refuses)
    else:
        if not _is_cuda(disturbance):
            raise IlqgError("%s: %s is in host memory and device=True: pass a float64 torch tensor on the solver's GPU" % (who, what))
        a = disturbance
    shape = tuple(int(n) for n in a.shape)
    if shape not in (full, short):
        raise IlqgError("%s: %s has shape %s, expected %s = (B, R, n_hor, nx) or %s for every trajectory, with R = %d as in x0" % (
            who, what, shape, full, short, R))
    shared = 1 if shape == short and shape != full else 0
    if device is None:
        a = np.ascontiguousarray(a)
        return _address(a), shared, a
    return _cuda_address(a, shape, device, "%s: %s" % (who, what)), shared, a


def _drawn_noise(solver, who, noise, shared, first_trajectory, disturbance=None):
    """(seed, sigma as N_X C doubles, shared, first_trajectory), the arguments of the _drawn entries and of noise_table, from
    noise = (seed, sigma): a seed in 0 .. 2^64-1 and sigma [nx], the standard deviation of every state component (a scalar:
    the same for all), finite and not negative.  Checked here, before any library call."""
    nx, B = solver.problem.nx, solver.B
    if disturbance is not None:
        raise IlqgError("%s: noise and disturbance are both given: the noise is either drawn on the device (noise) or the caller's table "
                        "(disturbance); noise_table(...) gives the drawn noise as a table to add a term to" % who)
    if not isinstance(noise, (tuple, list)) or len(noise) != 2:
        raise IlqgError("%s: noise must be a pair (seed, sigma), not %r" % (who, noise))
    seed, sigma = noise
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise IlqgError("%s: noise: the seed must be an integer in 0 .. 2^64-1, not %r" % (who, seed))
    if _is_cuda(sigma):
        raise IlqgError("%s: noise: sigma is a tensor on the device: sigma is host memory in every form (%d numbers)" % (who, nx))
    try:
        a = np.asarray(sigma, dtype=np.float64)
    except (TypeError, ValueError):
        raise IlqgError("%s: noise: sigma must be %d real numbers, not %r" % (who, nx, sigma))
    if a.ndim == 0:
        a = np.full(nx, float(a))
    if a.shape != (nx,):
        raise IlqgError("%s: noise: sigma has shape %s, expected (%d,) = (nx,), or a scalar for every component" % (who, tuple(a.shape), nx))
    if not np.all(np.isfinite(a) & (a >= 0.0)):
        raise IlqgError("%s: noise: sigma must be finite and not negative, not %s" % (who, a.tolist()))
    first = first_trajectory
    if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or int(first) < 0 or int(first) + B > 2 ** 32:
        raise IlqgError("%s: first_trajectory must be an integer with 0 <= first_trajectory and first_trajectory + B <= 2^32 (B = %d), not %r"
                        % (who, B, first))
    return int(seed), (C.c_double * nx)(*a.tolist()), 1 if shared else 0, int(first)


def _policy_rollout(solver, entry, x0, alpha, feedback, trajectories, params, disturbance=None, noise=None, noise_shared=False, first_trajectory=0):
    """BatchSolver.policy_rollout / MultiSolver.policy_rollout in host memory: the checks, the arrays and the one library call.
    Without a disturbance and without noise the entries that have always been there are called with the arguments they have
    always had; with a disturbance the superset entry `entry`_noise, with noise `entry`_drawn (n_names = 0: no parameter table)."""
    x0 = _policy_starts(x0, solver.B, solver.problem.nx)
    R, named = x0.shape[1], ()
    out, ptr = _rollout_outputs(solver, R, trajectories)
    if noise is not None:
        drawn = _drawn_noise(solver, "policy_rollout", noise, noise_shared, first_trajectory, disturbance)
        named = (0, None, None, 0)
    if disturbance is not None:
        dist, dist_shared, keep = _rollout_disturbance(solver, disturbance, R)
        named = (0, None, None, 0)
    if params is not None:
        names, values, shared = _rollout_params(solver, params, R)
        named = (len(names), names, _address(values), shared)
    if noise is not None:
        entry, named = entry + "_drawn", named + drawn
    elif disturbance is not None:
        entry, named = entry + "_noise", named + (dist, dist_shared)
    elif params is not None:
        entry += "_params"
    solver._ck(_receding_entry(solver.lib, entry)(solver.h, R, _address(x0), *named, float(alpha), 1 if feedback else 0, *ptr))
    return out


HISTORY_DOUBLES = ("cost", "new_cost", "z", "lambda", "g_norm", "dV0", "dV1")
HISTORY_PENALTIES = ("w_pen_l", "w_pen_f")  # in libraries of problems with multipliers only
HISTORY_INTS = ("alpha_idx", "bp_calls", "iterations")


def _set_history(solver, prefix, cap):
    """BatchSolver.set_history / MultiSolver.set_history: the checks and the one library call"""
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)):
        raise IlqgError("set_history: cap must be an integer, not %r" % (cap,))
    if cap < 0:
        raise IlqgError("set_history: cap = %d, must not be negative (cap > 0: that many entries per trajectory, 0: no history)" % cap)
    solver._ck(_receding_entry(solver.lib, prefix + "set_history")(solver.h, int(cap)))


def _history(solver, prefix, names):
    """BatchSolver.history / MultiSolver.history: one library call per name"""
    get, get_int = _receding_entry(solver.lib, prefix + "get_history"), _receding_entry(solver.lib, prefix + "get_history_int")
    cap = int(_receding_entry(solver.lib, prefix + "history_cap")(solver.h))
    if cap < 1:
        raise IlqgError("history: the solver has no iteration history: set_history(cap > 0) switches one on")
    me, mf = solver.multiplier_dims()
    known = HISTORY_DOUBLES + (HISTORY_PENALTIES if me + mf else ()) + HISTORY_INTS + ("n",)
    if names is None:
        names = known
    if isinstance(names, str):
        names = (names,)
    for name in names:
        if name in HISTORY_PENALTIES and name not in known:
            raise IlqgError("history: '%s' is recorded in libraries of problems with multipliers only; this problem has none" % name)
        if name not in known:
            raise IlqgError("history: no such history field %r (%s)" % (name, " ".join(known)))
    out = {}
    for name in names:
        if name == "n":
            out[name] = np.zeros(solver.B, dtype=np.int32)
        else:
            out[name] = np.zeros((solver.B, cap), dtype=np.int32 if name in HISTORY_INTS else np.float64)
        solver._ck((get_int if out[name].dtype == np.int32 else get)(solver.h, name.encode(), _address(out[name])))
    return out


def _receding_entry(lib, name):
    """ilqg_batch_shift / ilqg_batch_receding / ilqg_multi_shift, ilqg_batch_head / _head_device / _shift_device /
    _shift_param / ilqg_multi_head, ilqg_batch_policy_rollout / _policy_rollout_device / ilqg_multi_policy_rollout and their
    _params forms, ilqg_batch_receding_plant / ilqg_multi_receding_plant, of a problem library; one built before they existed (a pair compiled out of tree and
    not rebuilt since) still loads and solves, and says so when they are asked for"""
    if not hasattr(lib, name):
        raise IlqgError("this problem library was built before %s existed: rebuild it (make -C ddp-generator_amd/csrc)" % name)
    return getattr(lib, name)


def _share_hip_runtime():
    """Device tensors of torch and the solver's memory and streams must belong to ONE HIP runtime, and a torch wheel may
    bring a copy of its own beside the one the problem libraries are linked with: two runtimes in one process know nothing
    of each other's allocations and streams.  Where torch has NOT been imported yet, the runtime the first problem library
    brought is made visible to everything loaded later (its scope is widened, nothing else is loaded), so a torch
    imported afterwards — BatchSolver.head(device=True) and shift() with a CUDA tensor import it themselves — runs on the
    same runtime as the solver.  Where torch was imported first nothing is touched: the loader then serves the problem
    library with the runtime torch brought where the two carry the same soname (seen with torch 2.10+rocm7.0 beside ROCm
    7.2), and where it does not, the device entries refuse torch's pointers with a message instead of reading them."""
    if "torch" in sys.modules:
        return
    try:
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    except OSError:
        return
    for p in paths:
        try:
            C.CDLL(p, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def _torch_stream(device):
    """(torch, the solver's GPU as torch names it, torch's current stream there as the library takes it) for the device
    forms: torch is imported here and nowhere else"""
    import torch
    if not torch.cuda.is_available():
        raise IlqgError("torch sees no GPU in this process: torch and the solver must share one HIP runtime, which they do "
                        "when torch is first imported after the first solver has been made (see ilqg._share_hip_runtime)")
    dev = torch.device("cuda", device)
    return torch, dev, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)


def load_library(problem="carparking", full_ddp=0, strict=False):
    path = library_path(problem, full_ddp, strict)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise IlqgError("HIP library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(make -C ddp-generator_amd/csrc). There is no CPU fallback." % path)
    lib = C.CDLL(path)
    if not _libs:
        _share_hip_runtime()
    v = C.c_void_p
    lib.ilqg_problem_dims.argtypes = [_ip]
    lib.ilqg_problem_param_name.restype = C.c_char_p
    lib.ilqg_problem_param_name.argtypes = [C.c_int]
    lib.ilqg_problem_param_size.argtypes = [C.c_int]
    lib.ilqg_reference_success.argtypes = [C.c_int, C.c_int]
    lib.ilqg_batch_create.restype = v
    lib.ilqg_batch_create.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.ilqg_batch_create_groups.restype = v
    lib.ilqg_batch_create_groups.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ilqg_batch_groups.argtypes = [v]
    lib.ilqg_batch_scalar_to_device.argtypes = [v, C.c_char_p, v]
    lib.ilqg_batch_destroy.argtypes = [v]
    lib.ilqg_batch_error.restype = C.c_char_p
    lib.ilqg_batch_error.argtypes = [v]
    lib.ilqg_batch_set_option.argtypes = [v, C.c_char_p, _dp, C.c_int]
    lib.ilqg_batch_set_param.argtypes = [v, C.c_char_p, _dp, C.c_int]
    lib.ilqg_batch_set_x0.argtypes = [v, _dp]
    lib.ilqg_batch_set_u.argtypes = [v, _dp]
    lib.ilqg_batch_set_x.argtypes = [v, _dp]
    for f in ("init", "solve", "sync", "calc_derivs", "line_search", "update"):
        getattr(lib, "ilqg_batch_" + f).argtypes = [v]
    lib.ilqg_batch_iterate.argtypes = [v, C.c_int]
    if hasattr(lib, "ilqg_batch_shift"):  # (a library built before the receding-horizon entries: see _receding_entry)
        lib.ilqg_batch_shift.argtypes = [v, C.c_int, v, v]
        lib.ilqg_batch_receding.argtypes = [v, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp]
        lib.ilqg_multi_shift.argtypes = [v, C.c_int, v, v]
    if hasattr(lib, "ilqg_batch_head"):  # (the same for the entries of a caller with its own plant)
        lib.ilqg_batch_head.argtypes = [v, C.c_int, v, v, v, v, v]
        lib.ilqg_batch_head_device.argtypes = [v, C.c_int, v, v, v, v, v, v]
        lib.ilqg_batch_shift_device.argtypes = [v, C.c_int, v, v, v]
        lib.ilqg_batch_shift_param.argtypes = [v, C.c_char_p, C.c_int, v]
        lib.ilqg_multi_head.argtypes = [v, C.c_int, v, v, v, v, v]
    if hasattr(lib, "ilqg_batch_policy_rollout"):  # (and for the roll-outs of the policy)
        lib.ilqg_batch_policy_rollout.argtypes = [v, C.c_int, v, C.c_double, C.c_int, v, v, v, v, v]
        lib.ilqg_batch_policy_rollout_device.argtypes = [v, C.c_int, v, C.c_double, C.c_int, v, v, v, v, v, v]
        lib.ilqg_multi_policy_rollout.argtypes = [v, C.c_int, v, C.c_double, C.c_int, v, v, v, v, v]
    if hasattr(lib, "ilqg_batch_policy_rollout_params"):  # (and under parameters per roll-out)
        named = [v, C.c_int, v, C.c_int, C.POINTER(C.c_char_p), v, C.c_int, C.c_double, C.c_int, v, v, v, v, v]
        lib.ilqg_batch_policy_rollout_params.argtypes = named
        lib.ilqg_batch_policy_rollout_params_device.argtypes = named + [v]
        lib.ilqg_multi_policy_rollout_params.argtypes = named
    if hasattr(lib, "ilqg_batch_policy_rollout_noise"):  # (and under a disturbance table per roll-out)
        noise = [v, C.c_int, v, C.c_int, C.POINTER(C.c_char_p), v, C.c_int, v, C.c_int, C.c_double, C.c_int, v, v, v, v, v]
        lib.ilqg_batch_policy_rollout_noise.argtypes = noise
        lib.ilqg_batch_policy_rollout_noise_device.argtypes = noise + [v]
        lib.ilqg_multi_policy_rollout_noise.argtypes = noise
    if hasattr(lib, "ilqg_batch_policy_rollout_drawn"):  # (and under process noise drawn on the device from a seed)
        drawn = [v, C.c_int, v, C.c_int, C.POINTER(C.c_char_p), v, C.c_int, C.c_ulonglong, v, C.c_int, C.c_longlong, C.c_double, C.c_int, v, v, v, v, v]
        lib.ilqg_batch_policy_rollout_drawn.argtypes = drawn
        lib.ilqg_batch_policy_rollout_drawn_device.argtypes = drawn + [v]
        lib.ilqg_multi_policy_rollout_drawn.argtypes = drawn
        lib.ilqg_batch_noise_table.argtypes = [v, C.c_int, C.c_ulonglong, v, C.c_int, C.c_longlong, v]
        lib.ilqg_batch_noise_table_device.argtypes = [v, C.c_int, C.c_ulonglong, v, C.c_int, C.c_longlong, v, v]
    if hasattr(lib, "ilqg_batch_set_params_batch"):  # (and for problem parameters per trajectory)
        lib.ilqg_batch_set_params_batch.argtypes = [v, C.c_int, C.POINTER(C.c_char_p), v]
        lib.ilqg_batch_set_params_batch_device.argtypes = [v, C.c_int, C.POINTER(C.c_char_p), v, v]
        lib.ilqg_batch_get_params_batch.argtypes = [v, C.c_char_p, v]
        lib.ilqg_multi_set_params_batch.argtypes = [v, C.c_int, C.POINTER(C.c_char_p), v]
    if hasattr(lib, "ilqg_batch_set_param_steps_batch"):  # (and for per-time-step parameters per trajectory)
        lib.ilqg_batch_set_param_steps_batch.argtypes = [v, C.c_char_p, v]
        lib.ilqg_batch_set_param_steps_batch_device.argtypes = [v, C.c_char_p, v, v]
        lib.ilqg_batch_get_param_steps_batch.argtypes = [v, C.c_char_p, v]
        lib.ilqg_batch_shift_param_batch.argtypes = [v, C.c_char_p, C.c_int, v]
        lib.ilqg_batch_shift_param_batch_device.argtypes = [v, C.c_char_p, C.c_int, v, v]
        lib.ilqg_multi_set_param_steps_batch.argtypes = [v, C.c_char_p, v]
        lib.ilqg_multi_shift_param_batch.argtypes = [v, C.c_char_p, C.c_int, v]
    if hasattr(lib, "ilqg_batch_receding_plant"):  # (and for the closed loop of planner and plant)
        lib.ilqg_batch_receding_plant.argtypes = [v, C.c_int, C.c_int, C.c_int, C.c_int, v, C.c_int, C.POINTER(C.c_char_p), v, v, v, v, v, v, v]
        lib.ilqg_multi_receding_plant.argtypes = lib.ilqg_batch_receding_plant.argtypes
    if hasattr(lib, "ilqg_batch_receding_windows"):  # (and for the windows that move inside the resident loops)
        lib.ilqg_batch_receding_windows.argtypes = [v, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(v), v, v, v]
        lib.ilqg_batch_receding_plant_windows.argtypes = [v, C.c_int, C.c_int, C.c_int, C.c_int, v, C.c_int, C.POINTER(C.c_char_p), v, v,
                                                          C.c_int, C.POINTER(C.c_char_p), C.POINTER(v), v, v, v, v, v]
        lib.ilqg_multi_receding_plant_windows.argtypes = lib.ilqg_batch_receding_plant_windows.argtypes
    if hasattr(lib, "ilqg_batch_set_history"):  # (and for the iteration history)
        lib.ilqg_batch_set_history.argtypes = [v, C.c_int]
        lib.ilqg_batch_get_history.argtypes = [v, C.c_char_p, v]
        lib.ilqg_batch_get_history_int.argtypes = [v, C.c_char_p, v]
        lib.ilqg_batch_history_cap.argtypes = [v]
        lib.ilqg_multi_set_history.argtypes = [v, C.c_int]
        lib.ilqg_multi_get_history.argtypes = [v, C.c_char_p, v]
        lib.ilqg_multi_get_history_int.argtypes = [v, C.c_char_p, v]
        lib.ilqg_multi_history_cap.argtypes = [v]
    if hasattr(lib, "ilqg_batch_best_of"):  # (and for the candidates per agent)
        lib.ilqg_batch_best_of.argtypes = [v, C.c_int, v, v, v, v]
        lib.ilqg_batch_best_of_device.argtypes = [v, C.c_int, v, v, v, v, v]
        lib.ilqg_batch_shift_winners.argtypes = [v, C.c_int, v, C.c_int, v, v, v]
        lib.ilqg_batch_shift_winners_device.argtypes = [v, C.c_int, v, C.c_int, v, v, v, v]
        lib.ilqg_multi_best_of.argtypes = [v, C.c_int, v, v, v, v]
        lib.ilqg_multi_shift_winners.argtypes = [v, C.c_int, v, C.c_int, v, v, v]
    if hasattr(lib, "ilqg_batch_solve_stream_rows"):  # (and for a stream whose starts bring rows, windows and a history)
        names = C.POINTER(C.c_char_p)
        lib.ilqg_batch_solve_stream_rows.argtypes = [v, C.c_int, v, v, C.c_int, names, v, C.c_int, names, C.POINTER(v),
                                                     C.c_int, C.c_int, names, C.POINTER(v), v, v, v, v, v]
        lib.ilqg_batch_stream_counts.argtypes = [v, C.POINTER(C.c_longlong)]
        lib.ilqg_batch_stream_counts.restype = None
    lib.ilqg_batch_back_pass.argtypes = [v, C.c_int]
    lib.ilqg_batch_active.argtypes = [v, _ip]
    lib.ilqg_batch_get_x.argtypes = [v, _dp]
    lib.ilqg_batch_get_u.argtypes = [v, _dp]
    lib.ilqg_batch_get_gains.argtypes = [v, _dp, _dp]
    lib.ilqg_batch_set_gains.argtypes = [v, _dp, _dp]
    lib.ilqg_batch_get_derivs.argtypes = [v, _dp, _dp]
    lib.ilqg_problem_multiplier_dims.argtypes = [_ip]
    lib.ilqg_batch_get_multipliers.argtypes = [v, _dp, _dp]
    lib.ilqg_batch_set_multipliers.argtypes = [v, _dp, _dp]
    lib.ilqg_batch_set_derivs.argtypes = [v, _dp, _dp]
    lib.ilqg_batch_get_scalar.argtypes = [v, C.c_char_p, _dp]
    lib.ilqg_batch_set_scalar.argtypes = [v, C.c_char_p, _dp]
    lib.ilqg_batch_get_int.argtypes = [v, C.c_char_p, _ip]
    lib.ilqg_batch_set_int.argtypes = [v, C.c_char_p, _ip]
    lib.ilqg_batch_cost_device_ptr.restype = v
    lib.ilqg_batch_cost_device_ptr.argtypes = [v]
    lib.ilqg_batch_stream.restype = v
    lib.ilqg_batch_stream.argtypes = [v]
    lib.ilqg_batch_timing.argtypes = [v, C.c_int]
    lib.ilqg_batch_kernel_name.restype = C.c_char_p
    lib.ilqg_batch_kernel_name.argtypes = [C.c_int]
    lib.ilqg_batch_get_timing.argtypes = [v, C.c_int, _ip, _dp]
    lib.ilqg_batch_get_busy.argtypes = [v, C.c_int, _dp]
    lib.ilqg_boxqp_batch.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _ip]
    lib.ilqg_boxqp_wave_batch.argtypes = lib.ilqg_boxqp_batch.argtypes
    lib.ilqg_boxqp_table_batch.argtypes = lib.ilqg_boxqp_batch.argtypes
    if hasattr(lib, "ilqg_boxqp_quad_batch"):  # (a unit-test entry: a library built before it existed still loads and solves)
        lib.ilqg_boxqp_quad_batch.argtypes = lib.ilqg_boxqp_batch.argtypes + [C.c_void_p]
    lib.ilqg_sincos_batch.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp]
    lib.ilqg_multi_create.restype = v
    lib.ilqg_multi_create.argtypes = [C.c_int, _ip, C.c_int, C.c_int]
    lib.ilqg_multi_destroy.argtypes = [v]
    lib.ilqg_multi_error.restype = C.c_char_p
    lib.ilqg_multi_error.argtypes = [v]
    lib.ilqg_multi_devices.argtypes = [v]
    lib.ilqg_multi_set_option.argtypes = [v, C.c_char_p, _dp, C.c_int]
    lib.ilqg_multi_set_param.argtypes = [v, C.c_char_p, _dp, C.c_int]
    for f in ("set_x0", "set_u", "get_x", "get_u", "gather_costs"):
        getattr(lib, "ilqg_multi_" + f).argtypes = [v, _dp]
    for f in ("init", "solve", "sync"):
        getattr(lib, "ilqg_multi_" + f).argtypes = [v]
    lib.ilqg_multi_iterate.argtypes = [v, C.c_int]
    lib.ilqg_multi_active.argtypes = [v, _ip]
    lib.ilqg_multi_get_int.argtypes = [v, C.c_char_p, _ip]
    lib.ilqg_solve_single.argtypes = [C.c_int, _dp, _dp, C.POINTER(_Named), C.c_int, C.POINTER(_Named), C.c_int, _dp, _dp,
                                      _dp, _ip, _dp, C.c_char_p, C.c_int]
    _libs[path] = lib
    return lib


class Problem:
    """compile-time facts of one problem library"""

    def __init__(self, problem="carparking", full_ddp=0, strict=False):
        self.name, self.full_ddp = problem, int(full_ddp)
        self.lib = load_library(problem, full_ddp, strict)
        d = np.zeros(8, dtype=np.int32)
        self.lib.ilqg_problem_dims(d)
        self.nx, self.nu, _, self.rec_host, self.rec_dev, self.state_dep_limits, self.n_params = [int(x) for x in d[:7]]
        self.wave_mapping = bool(d[7])
        self.sxx = self.nx * (self.nx + 1) // 2
        self.suu = self.nu * (self.nu + 1) // 2
        self.params = [(self.lib.ilqg_problem_param_name(i).decode(), self.lib.ilqg_problem_param_size(i))
                       for i in range(self.n_params)]

    def device_count(self):
        return self.lib.ilqg_device_count()


class BatchSolver:
    """B trajectories of one problem advanced in lock step on one GPU."""

    def __init__(self, problem="carparking", full_ddp=0, batch=1, n_hor=500, device=0, params=None, opts=None,
                 strict=False, groups=0):
        """groups: the batch advances as that many independent sets of trajectories on separate HIP streams
        (0 = the library's choice, see ilqg_batch_create_groups)"""
        self.problem = Problem(problem, full_ddp, strict)
        self.lib = self.problem.lib
        self.B, self.N, self.device = int(batch), int(n_hor), int(device)
        self.h = self.lib.ilqg_batch_create_groups(int(device), self.B, self.N, int(groups))
        if not self.h:
            raise IlqgError(self.lib.ilqg_batch_error(None).decode())
        for k, val in (params or {}).items():
            self.set_param(k, val)
        for k, val in (opts or {}).items():
            self.set_option(k, val)

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.ilqg_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise IlqgError(self.lib.ilqg_batch_error(self.h).decode())

    # -- configuration -----------------------------------------------------
    def set_option(self, name, value):
        v = np.ascontiguousarray(np.atleast_1d(value), dtype=np.float64)
        self._ck(self.lib.ilqg_batch_set_option(self.h, name.encode(), v, v.size))

    def set_param(self, name, value):
        v = np.ascontiguousarray(np.atleast_1d(value), dtype=np.float64)
        self._ck(self.lib.ilqg_batch_set_param(self.h, name.encode(), v, v.size))

    def set_params_batch(self, params, device=False):
        """problem parameters PER TRAJECTORY (ilqg_batch_set_params_batch): params = {name: array [B,size]} (the last axis
        may be left out for size 1) — from the next launch on trajectory b plans, is rolled out and has its plant advance
        under the batch's fixed-size parameters with every named one replaced by array[b].  Packed in dict order; a call
        replaces the whole set; {} or None clears it (the batch is shared-only again).  Nothing is recomputed: costs and
        records stay as they are until init() or shift().  Order with policy_rollout(params=...) and
        receding_plant(params=...): the trajectory's row first, then the roll-out's or the plant's.  Per-time-step
        parameters stay shared and cannot be named; set_param of a name that is per-trajectory is refused; lane-mapped
        libraries only.  With device=True contiguous float64 torch tensors on the solver's GPU, packed with torch.cat on
        torch's current stream (a single tensor is read where it is) and copied by the library in that stream's order
        without a host wait (ilqg_batch_set_params_batch_device)."""
        if params is not None and not isinstance(params, dict):
            raise IlqgError("set_params_batch: params must be a dict of parameter name -> array [B, size]; {} or None clears the set")
        if not params:
            self._ck(_receding_entry(self.lib, "ilqg_batch_set_params_batch")(self.h, 0, None, None))
            return
        args = ("set_params_batch", self.problem, params, ((self.B,),), "all trajectories")
        if not device:
            names, values, _ = _pack_arrays(*args)
            self._ck(_receding_entry(self.lib, "ilqg_batch_set_params_batch")(self.h, len(names), names, _address(values)))
            return
        names, cols, _ = _pack_tensors(*args, self.device)
        entry = _receding_entry(self.lib, "ilqg_batch_set_params_batch_device")
        torch, dev, stream = _torch_stream(self.device)
        ptr, keep = _tensor_table(torch, dev, cols)
        self._ck(entry(self.h, len(names), names, ptr, stream))

    def params_batch(self, name):
        """[B,size]: what trajectory b sees of fixed-size parameter `name` (ilqg_batch_get_params_batch) — its row of
        set_params_batch, or the shared value repeated"""
        size = dict(self.problem.params).get(name, 0)
        out = np.zeros((self.B, max(size, 1)))
        self._ck(_receding_entry(self.lib, "ilqg_batch_get_params_batch")(self.h, name.encode(), _address(out)))
        return out

    def set_param_steps_batch(self, name, values, device=False):
        """ONE per-time-step parameter PER TRAJECTORY (ilqg_batch_set_param_steps_batch): values [B, n_hor+1] — a reference
        track per agent.  From the next launch on trajectory b reads p[name][k] from values[b], running steps and the final
        step, in every stage set_params_batch covers and in policy_rollout.  Per name: None makes the name shared again,
        with the window set_param last gave it.  Independent of set_params_batch.  Nothing is recomputed.  set_param and
        shift_param of a name that has rows are refused (use this and shift_param_batch); lane-mapped libraries only.  With
        device=True a contiguous float64 torch tensor on the solver's GPU, copied by the library in the order of torch's
        current stream without a host wait (ilqg_batch_set_param_steps_batch_device)."""
        who = "set_param_steps_batch"
        cname = _param_steps_name(self.problem, who, name)
        if values is None:
            self._ck(_receding_entry(self.lib, "ilqg_batch_set_param_steps_batch")(self.h, cname, None))
            _note_step_rows(self, name, False)
            return
        ptr, keep = _param_steps_rows(who, "values", values, (self.B, self.N + 1), device, self.device)
        if not device:
            self._ck(_receding_entry(self.lib, "ilqg_batch_set_param_steps_batch")(self.h, cname, ptr))
            _note_step_rows(self, name, True)
            return
        entry = _receding_entry(self.lib, "ilqg_batch_set_param_steps_batch_device")
        self._ck(entry(self.h, cname, ptr, _torch_stream(self.device)[2]))
        _note_step_rows(self, name, True)

    def param_steps_batch(self, name):
        """[B, n_hor+1]: what trajectory b sees of per-time-step parameter `name` (ilqg_batch_get_param_steps_batch) — its
        row of set_param_steps_batch, or the shared window repeated"""
        cname = _param_steps_name(self.problem, "param_steps_batch", name)
        out = np.zeros((self.B, self.N + 1))
        self._ck(_receding_entry(self.lib, "ilqg_batch_get_param_steps_batch")(self.h, cname, _address(out)))
        return out

    def shift_param_batch(self, name, steps, tail=None, device=False):
        """the windows of set_param_steps_batch move `steps` values on, each row in place on the device
        (ilqg_batch_shift_param_batch): p'[b][k] = p[b][k+steps], the last `steps` values from tail [B, steps], or each row's
        last value held; bit for bit what set_param_steps_batch(name, [rows[:, steps:], tail]) gives.  With device=True tail
        is a contiguous float64 torch tensor on the solver's GPU (ilqg_batch_shift_param_batch_device, torch's current
        stream, no host wait)."""
        who = "shift_param_batch"
        cname = _param_steps_name(self.problem, who, name)
        if tail is None:
            self._ck(_receding_entry(self.lib, "ilqg_batch_shift_param_batch")(self.h, cname, int(steps), None))
            return
        ptr, keep = _param_steps_rows(who, "tail", tail, (self.B, max(int(steps), 0)), device, self.device)
        if not device:
            self._ck(_receding_entry(self.lib, "ilqg_batch_shift_param_batch")(self.h, cname, int(steps), ptr))
            return
        entry = _receding_entry(self.lib, "ilqg_batch_shift_param_batch_device")
        self._ck(entry(self.h, cname, int(steps), ptr, _torch_stream(self.device)[2]))

    def init(self, x0, u0):
        """x0 [B,nx], u0 [B,N,nu]: initial roll-out (clamps u) and solver entry state"""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(self.B, self.problem.nx)
        u0 = np.ascontiguousarray(u0, dtype=np.float64).reshape(self.B, self.N, self.problem.nu)
        self._ck(self.lib.ilqg_batch_set_x0(self.h, x0))
        self._ck(self.lib.ilqg_batch_set_u(self.h, u0))
        self._ck(self.lib.ilqg_batch_init(self.h))

    # -- solver ------------------------------------------------------------
    def iterate(self, n=1):
        self._ck(self.lib.ilqg_batch_iterate(self.h, int(n)))

    def solve(self):
        self._ck(self.lib.ilqg_batch_solve(self.h))

    def shift(self, steps, x0=None, u_tail=None):
        """receding horizon on the device (ilqg_batch_shift): u'[k] = u[k+steps], tail = u_tail [B,steps,nu] or the last
        control held, x0' = x0 [B,nx] or the plan's x[steps]; then what init() does.  Problem parameters are left alone
        (shift_param moves the window of one with a value per time step).
        x0 / u_tail as CUDA torch tensors (float64, contiguous, on the solver's GPU) are read where they are, in the order
        of torch's current stream, without a host copy or a host wait (ilqg_batch_shift_device); both or neither."""
        nx, nu, n = self.problem.nx, self.problem.nu, max(int(steps), 0)
        if _is_cuda(x0) or _is_cuda(u_tail):
            for what, a in (("x0", x0), ("u_tail", u_tail)):
                if a is not None and not _is_cuda(a):
                    raise IlqgError("shift: %s is in host memory and the other argument on the device: pass both the same way" % what)
            px, pt = _cuda_address(x0, (self.B, nx), self.device, "x0"), _cuda_address(u_tail, (self.B, n, nu), self.device, "u_tail")
            entry = _receding_entry(self.lib, "ilqg_batch_shift_device")
            self._ck(entry(self.h, int(steps), px, pt, _torch_stream(self.device)[2]))
            return
        x0, u_tail = _optional(x0, (self.B, nx)), _optional(u_tail, (self.B, n, nu))
        self._ck(_receding_entry(self.lib, "ilqg_batch_shift")(self.h, int(steps), _address(x0), _address(u_tail)))

    def best_of(self, K, score=None, device=False):
        """candidates per agent: the batch read as G = B / K segments of K consecutive slots (K one of 1, 2, 4, .. 64, B % K == 0),
        and per segment the eligible slot with the smallest score (ilqg_batch_best_of).  score [B], or None = every slot's
        current cost.  A slot is eligible iff its score is finite and its status is not 7 (the initial roll-out failed); equal
        scores resolve to the lowest index (`<` on doubles: -0.0 and 0.0 tie).  Returns (winner [G] int32, batch-absolute, -1
        where no slot is eligible; best [G], the winner's score, NaN for -1; n_eligible [G] int32).  Nothing in the batch
        changes.  numpy arrays, or with device=True torch tensors on the solver's GPU (score then None or a float64 CUDA tensor),
        filled in the order of torch's current stream without a host wait (ilqg_batch_best_of_device)."""
        return _best_of(self, "ilqg_batch_", K, score, device)

    def shift_winners(self, K, winner, steps, x0=None, u_tail=None, du=None):
        """shift(), except that every slot b of segment g takes the plan of slot w = winner[g] in place of its own
        (ilqg_batch_shift_winners): u'_b[k] = u_w[k+steps], tail = u_tail [G,steps,nu] or the winner's last control held, plus
        du [B,N,nu] where given (one fp64 add; zero one slot's rows to keep the incumbent unperturbed); x0'_b = x0 [G,nx] or the
        winner's x[steps]; then what init() does.  winner [G] integers, batch-absolute (best_of's); -1: the slots of that segment
        shift their own plans.  A winner outside its segment is refused — except on the device, which cannot look: there it
        counts as -1.  0 <= steps < N.  With any argument a CUDA torch tensor all of them must be (winner int32, the others
        float64, contiguous, on the solver's GPU): they are read where they are, in the order of torch's current stream,
        without a host copy or a host wait (ilqg_batch_shift_winners_device)."""
        _shift_winners(self, "ilqg_batch_", K, winner, steps, x0, u_tail, du, True)

    def head(self, steps, gains=False, device=False):
        """the first `steps` steps of every current plan, read where it lives (nothing in the batch changes):
        dict(x [B,steps,nx] = x_0 .. x_{steps-1}, u [B,steps,nu], cost [B]) and, with gains, l [B,steps,nu] and
        L [B,steps,nu*nx] (each step column-major, as gains()).  numpy arrays (ilqg_batch_head), or with device=True
        float64 torch tensors on the solver's GPU, filled in the order of torch's current stream without a host wait
        (ilqg_batch_head_device)."""
        if not device:
            out, ptr = _head_outputs(self, steps, gains)
            self._ck(_receding_entry(self.lib, "ilqg_batch_head")(self.h, int(steps), *ptr))
            return out
        entry = _receding_entry(self.lib, "ilqg_batch_head_device")
        torch, dev, stream = _torch_stream(self.device)
        out, ptr = _head_outputs(self, steps, gains, torch, dev)
        self._ck(entry(self.h, int(steps), *ptr, stream))
        return out

    def policy_rollout(self, x0, alpha=1.0, feedback=True, trajectories=False, device=False, params=None, disturbance=None, noise=None,
                       noise_shared=False, first_trajectory=0):
        """every plan's feedback policy rolled out from R starts per trajectory on the GPU (ilqg_batch_policy_rollout):
        x0 [B,R,nx], or [R,nx] for every trajectory; u_k = u_nom_k [+ alpha l_k if alpha != 0] [+ L_k (x_k - x_nom_k) if
        feedback], clamped, through the problem's dynamics and cost.  The policy is what head(N, gains=True) returns — behind
        an accepted step its gains were computed about the PREVIOUS nominal trajectory; nothing in the batch changes.
        dict(cost [B,R], ok [B,R] int32 (0: a value was NaN / Inf, the roll-out's other outputs are unspecified),
        x_end [B,R,nx]) and with trajectories x [B,R,N+1,nx], u [B,R,N,nu] (the clamped controls applied).
        numpy arrays, or with device=True a float64 torch tensor [B,R,nx] on the solver's GPU in and torch tensors out, in
        the order of torch's current stream without a host wait (ilqg_batch_policy_rollout_device).
        params = {name: array}: roll-out (b, r) runs under problem parameters of its own (ilqg_batch_policy_rollout_params) —
        the batch's, with every named fixed-size parameter replaced by array[b, r]: every array [B,R,size], or every array
        [R,size] for all trajectories (the last axis may be left out for size 1), R as in x0.  The policy stays the plan's:
        its gains were computed under the batch's parameters.  Per-time-step parameters stay shared and cannot be named;
        the batch's parameters do not change.  With device=True contiguous float64 torch tensors on the solver's GPU,
        packed with torch.cat on torch's current stream (a single tensor is read where it is).
        disturbance: process noise, a push on the state behind every step (ilqg_batch_policy_rollout_noise): roll-out (b, r)
        goes on from x_next + disturbance[b, r, k] behind step k = 0 .. N-1 — [B,R,N,nx], or [R,N,nx] for every trajectory
        (common random numbers).  The control of step k+1 is computed at the disturbed state; row N-1 moves x_end, x[N] and the
        state the final cost is evaluated at; ok is 0 too where a disturbed state is not finite.  A numpy array, or with
        device=True a contiguous float64 torch tensor on the solver's GPU.  None: the call without a table, unchanged.
        noise = (seed, sigma): the same push DRAWN ON THE DEVICE (ilqg_batch_policy_rollout_drawn; no table, no memory
        proportional to R): disturbance[b, r, k, i] = sigma[i] z, z a standard normal of the counter-based generator
        Philox4x32-10 under the 64-bit seed at the counter (k, r, first_trajectory + b, i // 4) (Box-Muller in double
        precision, the tail ends at 6.7 sigma).  sigma [nx] or a scalar, host memory in every form.  A draw depends on its
        counter alone: roll-out (b, r) has the same bits for any R, stream groups and shards, and a batch rolled out in chunks
        equals the whole with first_trajectory = each chunk's first trajectory.  noise_shared: every trajectory gets the
        draws of trajectory 0 (common random numbers).  noise_table(R, seed, sigma, ...) is the same noise as a table: given
        as `disturbance` it yields the same bits.  noise together with disturbance is refused."""
        nx, B, named = self.problem.nx, self.B, ()
        if not device:
            if _is_cuda(x0):
                raise IlqgError("policy_rollout: x0 is a tensor on the device: pass device=True")
            return _policy_rollout(self, "ilqg_batch_policy_rollout", x0, alpha, feedback, trajectories, params, disturbance, noise, noise_shared,
                                   first_trajectory)
        if not _is_cuda(x0):
            raise IlqgError("policy_rollout: device=True and x0 is in host memory: pass a float64 torch tensor on the solver's GPU")
        if len(x0.shape) != 3 or int(x0.shape[1]) < 1:
            raise IlqgError("policy_rollout: x0 has shape %s, expected (%d, R, %d) with n_starts = R >= 1" % (tuple(x0.shape), B, nx))
        R = int(x0.shape[1])
        px = _cuda_address(x0, (B, R, nx), self.device, "x0")
        if params is not None:
            names, cols, shared = _rollout_params(self, params, R, self.device)
        if noise is not None:
            drawn = _drawn_noise(self, "policy_rollout", noise, noise_shared, first_trajectory, disturbance)
            named = (0, None, None, 0)
        if disturbance is not None:
            dist, dist_shared, keep_dist = _rollout_disturbance(self, disturbance, R, self.device)
            named = (0, None, None, 0)
        entry = _receding_entry(self.lib, "ilqg_batch_policy_rollout_drawn_device" if noise is not None else
                                "ilqg_batch_policy_rollout_noise_device" if disturbance is not None else
                                "ilqg_batch_policy_rollout_device" if params is None else "ilqg_batch_policy_rollout_params_device")
        torch, dev, stream = _torch_stream(self.device)
        out, ptr = _rollout_outputs(self, R, trajectories, torch, dev)
        if params is not None:
            values, keep = _tensor_table(torch, dev, cols)
            named = (len(names), names, values, shared)
        if noise is not None:
            named = named + drawn
        elif disturbance is not None:
            named = named + (dist, dist_shared)
        self._ck(entry(self.h, R, px, *named, float(alpha), 1 if feedback else 0, *ptr, stream))
        return out

    def noise_table(self, R, seed, sigma, shared=False, first_trajectory=0, device=False):
        """the process noise policy_rollout(noise=(seed, sigma), noise_shared=shared, first_trajectory=...) draws for R roll-outs
        per trajectory, as a table (ilqg_batch_noise_table; k_noise_fill, the same device function): [B,R,N,nx], or with shared
        [R,N,nx].  policy_rollout(disturbance=table) yields what the drawn call yields, bit for bit; table[:, 0, :rounds*steps]
        is a disturbance for receding_plant; a caller adds a term of their own to it.  A numpy array, or with device=True a
        float64 torch tensor on the solver's GPU, written in the order of torch's current stream without a host wait
        (ilqg_batch_noise_table_device).  Nothing in the batch changes."""
        if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or R < 1:
            raise IlqgError("noise_table: R must be an integer >= 1 (roll-outs per trajectory), not %r" % (R,))
        drawn = _drawn_noise(self, "noise_table", (seed, sigma), shared, first_trajectory)
        shape = ((int(R), self.N, self.problem.nx) if shared else (self.B, int(R), self.N, self.problem.nx))
        if not device:
            w = np.zeros(shape)
            self._ck(_receding_entry(self.lib, "ilqg_batch_noise_table")(self.h, int(R), *drawn, _address(w)))
            return w
        entry = _receding_entry(self.lib, "ilqg_batch_noise_table_device")
        torch, dev, stream = _torch_stream(self.device)
        w = torch.empty(shape, dtype=torch.float64, device=dev)
        self._ck(entry(self.h, int(R), *drawn, C.c_void_p(w.data_ptr() or None), stream))
        return w

    def shift_param(self, name, steps, tail=None):
        """the window of ONE per-time-step parameter moves `steps` values on (ilqg_batch_shift_param): p'[k] = p[k+steps],
        the last `steps` values from tail [steps], or the last value held; what set_param(name, [p[steps:], tail]) gives
        without sending the table again"""
        if tail is not None:
            tail = np.ascontiguousarray(tail, dtype=np.float64)
            if tail.shape != (max(int(steps), 0),):
                raise IlqgError("shift_param: tail has shape %s, expected (%d,) = (steps,)" % (tail.shape, max(int(steps), 0)))
        self._ck(_receding_entry(self.lib, "ilqg_batch_shift_param")(self.h, name.encode(), int(steps), _address(tail)))

    def receding(self, rounds, steps, iterations, windows=None):
        """rounds x { iterate(iterations); record the first `steps` (x, u) of every plan and its cost; shift(steps) }
        (ilqg_batch_receding): dict(x [B,rounds*steps,nx], u [B,rounds*steps,nu], cost [B,rounds]), copied to the host once.
        A problem with a per-time-step parameter is refused unless windows is given: windows = {name: future or None}
        (ilqg_batch_receding_windows) moves EVERY per-time-step parameter's window `steps` on each round, between the record
        and the shift, on the device: future [B, rounds*steps] for a name that currently has rows (set_param_steps_batch),
        [rounds*steps] for a shared name — the values beyond the current window, sent once —, None or a name left out: the
        window holds its last value.  {} is valid.  Afterwards the windows have moved rounds*steps on (param_steps_batch)."""
        n = max(int(rounds), 0) * max(int(steps), 0)
        entry, moving = "ilqg_batch_receding", ()
        if windows is not None:
            n_windows, window_names, futures, keep = _windows(self, "receding", windows, rounds, steps)
            entry, moving = "ilqg_batch_receding_windows", (n_windows, window_names, futures)
        out = dict(x=np.zeros((self.B, n, self.problem.nx)), u=np.zeros((self.B, n, self.problem.nu)),
                   cost=np.zeros((self.B, max(int(rounds), 0))))
        ptr = (out["x"], out["u"], out["cost"]) if windows is None else tuple(_address(out[k]) for k in ("x", "u", "cost"))
        self._ck(_receding_entry(self.lib, entry)(self.h, int(rounds), int(steps), int(iterations), *moving, *ptr))
        return out

    def receding_plant(self, rounds, steps, iterations, feedback=True, x_plant=None, params=None, disturbance=None, windows=None):
        """the closed loop of planner and plant on the GPU for `rounds` control intervals (ilqg_batch_receding_plant):
        rounds x { iterate(iterations); every trajectory's plant advances `steps` steps from ITS OWN state under the plan's
        policy, u = u_nom_k [+ L_k (x_plant - x_nom_k) if feedback], clamped, through the problem's dynamics and cost under
        the PLANT's parameters, and behind each step disturbance[b, round*steps + k] is added to its state;
        shift(steps, x0 = the plants' states) }.
        x_plant [B,nx]: the plants' states at the start (None: every plan's x_0).  params = {name: array [B,size]} (the last
        axis may be left out for size 1): the plant of trajectory b runs under the batch's parameters with every named
        fixed-size parameter replaced by array[b] (None: the plant is the model); the planner keeps the batch's parameters,
        which do not change.  disturbance [B,rounds*steps,nx] or None.  Everything is host memory, sent once; the logs come
        back once: dict(x [B,rounds*steps,nx] the plant's state each control was applied at, u [B,rounds*steps,nu] the
        clamped control applied, cost [B,rounds] the sum of the round's running costs under the plant's parameters,
        plan_cost [B,rounds] the cost of the plan the round applied, ok [B] int32 (0: a step of that plant met NaN / Inf; it
        stayed at its last finite state and its later entries are unspecified), x_plant [B,nx] the plants' states behind
        the last round, or None where x_plant was None).  The gains behind an accepted step are those about the previous
        nominal trajectory (see policy_rollout).
        windows = {name: future or None} as in receding() (ilqg_batch_receding_plant_windows): the plant's step k reads
        p[name][k] of the round's not yet moved window (trajectory b's row where the name has rows), then every window moves
        `steps` on, then the plans shift; without it a problem with a per-time-step parameter is refused."""
        return _receding_plant(self, "ilqg_batch_receding_plant", rounds, steps, iterations, feedback, x_plant, params, disturbance, windows)

    def solve_stream(self, x0, u0, with_trajectories=False, params=None, param_steps=None, history=0):
        """a stream of len(x0) starts through this batch's slots (ilqg_batch_solve_stream): dict of cost, status, iterations
        per start, and x / u if asked for.
        Each start may bring its own (ilqg_batch_solve_stream_rows): params = {name: array [total, size]} (the last axis may
        be left out for size 1), rows of fixed-size parameters as in set_params_batch; param_steps = {name: array
        [total, n_hor+1]}, windows of per-time-step parameters as in set_param_steps_batch; history = a capacity: the result
        gains `history`, a dict like history()'s with `total` in place of B.  Start s gets, bit for bit, what solve() gives
        it in a batch that holds it under set_params_batch / set_param_steps_batch with its rows.  The solver itself must
        have no set, no rows and no history, and has none afterwards.  Without the three keywords the call is the one it has
        always been; with one of them on a library built before the entry existed it says so ("rebuild")."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
        total = x0.shape[0]
        assert u0.shape == (total, self.N, self.problem.nu) and x0.shape == (total, self.problem.nx)
        cost = np.zeros(total)
        status, iters = np.zeros(total, dtype=np.int32), np.zeros(total, dtype=np.int32)
        x = np.zeros((total, self.N + 1, self.problem.nx)) if with_trajectories else None
        u = np.zeros((total, self.N, self.problem.nu)) if with_trajectories else None
        vp = C.c_void_p
        xp, up = (x.ctypes.data_as(vp), u.ctypes.data_as(vp)) if with_trajectories else (None, None)
        if params is None and param_steps is None and isinstance(history, (int, np.integer)) and not isinstance(history, bool) and history == 0:
            self.lib.ilqg_batch_solve_stream.argtypes = [vp, C.c_int, _dp, _dp, _dp, _ip, _ip, vp, vp]
            self._ck(self.lib.ilqg_batch_solve_stream(self.h, total, x0, u0, cost, status, iters, xp, up))
            return dict(cost=cost, status=status, iterations=iters, x=x, u=u)
        who = "solve_stream"
        entry = _receding_entry(self.lib, "ilqg_batch_solve_stream_rows")
        for what, d in (("params", params), ("param_steps", param_steps)):
            if d is not None and not isinstance(d, dict):
                raise IlqgError("%s: %s must be a dict of parameter name -> array with a row per start, or None" % (who, what))
        if isinstance(history, bool) or not isinstance(history, (int, np.integer)):
            raise IlqgError("%s: history must be an integer (a capacity: that many entries per start, 0: no history), not %r" % (who, history))
        if history < 0:
            raise IlqgError("%s: history = %d, must not be negative (a capacity: that many entries per start, 0: no history)" % (who, history))
        names, values = None, None
        if params:
            names, values, _ = _pack_arrays(who, self.problem, params, ((total,),), "all starts", hint=", with total = %d as in x0" % total)
        step_names, step_ptrs, keep = None, None, []
        if param_steps:
            cnames = [_param_steps_name(self.problem, who, name) for name in param_steps]
            for name, a in param_steps.items():
                keep.append(_param_steps_rows(who, "param_steps['%s']" % name, a, (total, self.N + 1), False, self.device)[1])
            step_names = (C.c_char_p * len(cnames))(*cnames)
            step_ptrs = (vp * len(keep))(*[a.ctypes.data for a in keep])
        cap, hist, hist_names, hist_ptrs = int(history), None, None, None
        if cap > 0:
            me, mf = self.multiplier_dims()
            known = HISTORY_DOUBLES + (HISTORY_PENALTIES if me + mf else ()) + HISTORY_INTS + ("n",)
            hist = {name: np.zeros(total, dtype=np.int32) if name == "n" else
                    np.zeros((total, cap), dtype=np.int32 if name in HISTORY_INTS else np.float64) for name in known}
            hist_names = (C.c_char_p * len(known))(*[name.encode() for name in known])
            hist_ptrs = (vp * len(known))(*[hist[name].ctypes.data for name in known])
        self._ck(entry(self.h, total, _address(x0), _address(u0), 0 if names is None else len(names), names, _address(values),
                       0 if step_names is None else len(step_names), step_names, step_ptrs,
                       cap, 0 if hist is None else len(hist), hist_names, hist_ptrs, _address(cost), _address(status), _address(iters), xp, up))
        out = dict(cost=cost, status=status, iterations=iters, x=x, u=u)
        if hist is not None:
            out["history"] = hist
        return out

    def stream_counts(self):
        """the last solve_stream, counted (ilqg_batch_stream_counts): dict of polls (status reads), harvests (launches of
        k_harvest), harvest_bytes (what they copied to the host) and contexts (contexts made: the staging context)"""
        entry = _receding_entry(self.lib, "ilqg_batch_stream_counts")
        out = (C.c_longlong * 4)()
        entry(self.h, out)
        return dict(zip(("polls", "harvests", "harvest_bytes", "contexts"), (int(v) for v in out)))

    def solve_trace(self):
        """the last solve(), poll by poll: (iterations done, trajectories active, slots iterated over) arrays and the number
        of times the active set was gathered into a smaller context (option "compact")"""
        cap = 4096
        it, act, slots = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        comp = C.c_int(0)
        self.lib.ilqg_batch_solve_trace.argtypes = [C.c_void_p, _ip, _ip, _ip, C.c_int, C.POINTER(C.c_int)]
        n = min(cap, self.lib.ilqg_batch_solve_trace(self.h, it, act, slots, cap, C.byref(comp)))
        return it[:n].copy(), act[:n].copy(), slots[:n].copy(), comp.value

    def sync(self):
        self._ck(self.lib.ilqg_batch_sync(self.h))

    def active(self):
        n = np.zeros(1, dtype=np.int32)
        self._ck(self.lib.ilqg_batch_active(self.h, n))
        return int(n[0])

    def calc_derivs(self):
        self._ck(self.lib.ilqg_batch_calc_derivs(self.h))

    def back_pass(self, single_sweep=False, fused=False):
        """single_sweep: one sweep on stored records (the drop-in back_pass()); fused: derivatives on the fly"""
        self._ck(self.lib.ilqg_batch_back_pass(self.h, 1 if single_sweep else (2 if fused else 0)))

    def line_search(self):
        self._ck(self.lib.ilqg_batch_line_search(self.h))

    def update(self):
        self._ck(self.lib.ilqg_batch_update(self.h))

    # -- results -----------------------------------------------------------
    def x(self):
        out = np.zeros((self.B, self.N + 1, self.problem.nx))
        self._ck(self.lib.ilqg_batch_get_x(self.h, out))
        return out

    def u(self):
        out = np.zeros((self.B, self.N, self.problem.nu))
        self._ck(self.lib.ilqg_batch_get_u(self.h, out))
        return out

    def gains(self):
        l = np.zeros((self.B, self.N, self.problem.nu))
        L = np.zeros((self.B, self.N, self.problem.nu * self.problem.nx))
        self._ck(self.lib.ilqg_batch_get_gains(self.h, l, L))
        return l, L

    def set_x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.B, self.N + 1, self.problem.nx)
        self._ck(self.lib.ilqg_batch_set_x(self.h, x))

    def set_u(self, u):
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(self.B, self.N, self.problem.nu)
        self._ck(self.lib.ilqg_batch_set_u(self.h, u))

    def set_gains(self, l, L):
        self._ck(self.lib.ilqg_batch_set_gains(self.h, np.ascontiguousarray(l, dtype=np.float64),
                                               np.ascontiguousarray(L, dtype=np.float64)))

    def derivs(self):
        rec = np.zeros((self.B, self.N, self.problem.rec_host))
        fin = np.zeros((self.B, self.problem.nx + self.problem.sxx))
        self._ck(self.lib.ilqg_batch_get_derivs(self.h, rec, fin))
        return rec, fin

    def set_derivs(self, rec, fin):
        rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(self.B, self.N, self.problem.rec_host)
        fin = np.ascontiguousarray(fin, dtype=np.float64).reshape(self.B, self.problem.nx + self.problem.sxx)
        self._ck(self.lib.ilqg_batch_set_derivs(self.h, rec, fin))

    def multiplier_dims(self):
        d = np.zeros(2, dtype=np.int32)
        self.lib.ilqg_problem_multiplier_dims(d)
        return int(d[0]), int(d[1])

    def multipliers(self):
        """(running [B, N, el], final [B, fin]): multipliersEl_t / multipliersFin_t member by member"""
        me, mf = self.multiplier_dims()
        run = np.zeros((self.B, self.N, max(me, 1)))
        fin = np.zeros((self.B, max(mf, 1)))
        self._ck(self.lib.ilqg_batch_get_multipliers(self.h, run, fin))
        return run[:, :, :me], fin[:, :mf]

    def set_multipliers(self, running, final):
        me, mf = self.multiplier_dims()
        # a part the problem does not have is not read by the library: any buffer will do
        run = (np.ascontiguousarray(running, dtype=np.float64).reshape(self.B, self.N, me) if me
               else np.zeros((self.B, self.N, 1)))
        fin = np.ascontiguousarray(final, dtype=np.float64).reshape(self.B, mf) if mf else np.zeros((self.B, 1))
        self._ck(self.lib.ilqg_batch_set_multipliers(self.h, run, fin))

    def scalar(self, name):
        w = MAX_ALPHA if name == "alpha_cost" else 1
        out = np.zeros((self.B, w))
        self._ck(self.lib.ilqg_batch_get_scalar(self.h, name.encode(), out))
        return out if w > 1 else out[:, 0]

    def set_scalar(self, name, value):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64), (self.B,)))
        self._ck(self.lib.ilqg_batch_set_scalar(self.h, name.encode(), v))

    def ints(self, name):
        w = MAX_ALPHA if name == "alpha_ok" else 1
        out = np.zeros((self.B, w), dtype=np.int32)
        self._ck(self.lib.ilqg_batch_get_int(self.h, name.encode(), out))
        return out if w > 1 else out[:, 0]

    def set_ints(self, name, value):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.int32), (self.B,)))
        self._ck(self.lib.ilqg_batch_set_int(self.h, name.encode(), v))

    def set_history(self, cap):
        """the iteration history on the device (ilqg_batch_set_history): with cap > 0 every update of an iteration — in
        iterate, solve (compacted too), every receding* loop, or the stage update() — first appends one entry for every
        trajectory that is active then, i.e. whose line search has just run, at position n[b] of the trajectory's own count;
        entries at positions >= cap are dropped while n counts on.  set_history and init() clear counts and entries, shift()
        and the resident loops do not.  0 switches off and frees.  solve_stream refuses a solver with a history."""
        _set_history(self, "ilqg_batch_", cap)

    def history(self, names=None):
        """the recorded entries (ilqg_batch_get_history / _get_history_int): dict of arrays [B, cap] — float64 cost, new_cost,
        z, lambda, g_norm, dV0, dV1 (and w_pen_l, w_pen_f where the problem has multipliers), int32 alpha_idx, bp_calls,
        iterations — plus n [B] int32, the entries recorded per trajectory (it may exceed cap).  Entry e of trajectory b is
        valid for e < min(n[b], cap); unwritten entries are zero.  names: a name or a sequence of them (default: all)."""
        return _history(self, "ilqg_batch_", names)

    def success(self):
        """the reference's iLQG() return value per trajectory (what the drop-in iLQG() of this library returns too)"""
        status, iters = self.ints("status"), self.ints("iterations")
        return np.array([self.lib.ilqg_reference_success(int(s), int(it)) for s, it in zip(status, iters)], dtype=np.int32)

    # -- plumbing for collectives / profiling ------------------------------
    def cost_device_ptr(self):
        return self.lib.ilqg_batch_cost_device_ptr(self.h)

    def groups(self):
        return int(self.lib.ilqg_batch_groups(self.h))

    def scalar_to_device(self, name, device_ptr):
        """per-trajectory scalar of the whole batch into caller-owned device memory (B doubles), no host copy"""
        self._ck(self.lib.ilqg_batch_scalar_to_device(self.h, name.encode(), C.c_void_p(int(device_ptr))))

    def stream(self):
        return self.lib.ilqg_batch_stream(self.h)

    def timing(self, enable=True):
        self._ck(self.lib.ilqg_batch_timing(self.h, 1 if enable else 0))

    def kernel_times(self):
        """{kernel name: (launches, total ms)} measured with HIP events on the solver's stream"""
        out = {}
        n = np.zeros(1, dtype=np.int32)
        ms = np.zeros(1)
        for k in range(self.lib.ilqg_batch_kernel_count()):
            self._ck(self.lib.ilqg_batch_get_timing(self.h, k, n, ms))
            out[self.lib.ilqg_batch_kernel_name(k).decode()] = (int(n[0]), float(ms[0]))
        return out


    def kernel_busy(self):
        """{kernel name: ms of wall clock its launches occupied} (union of the launch intervals: launches of one kernel
        on two streams overlap in the event clock while they take turns on the chip)"""
        out = {}
        ms = np.zeros(1)
        for k in range(self.lib.ilqg_batch_kernel_count()):
            self._ck(self.lib.ilqg_batch_get_busy(self.h, k, ms))
            if ms[0] > 0:
                out[self.lib.ilqg_batch_kernel_name(k).decode()] = float(ms[0])
        return out


class MultiSolver:
    """B trajectories sharded over several GPUs of one node in ONE process (ilqg_multi_*): contiguous blocks of
    ceil(B / G) trajectories per device, no exchange except costs() = one RCCL gather to the first device."""

    def __init__(self, problem="carparking", full_ddp=0, batch=2, n_hor=500, devices=(0,), params=None, opts=None):
        self.problem = Problem(problem, full_ddp)
        self.lib = self.problem.lib
        self.B, self.N = int(batch), int(n_hor)
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        self.h = self.lib.ilqg_multi_create(devs.size, devs, self.B, self.N)
        if not self.h:
            raise IlqgError(self.lib.ilqg_multi_error(None).decode())
        for k, val in (params or {}).items():
            a = np.ascontiguousarray(np.atleast_1d(val), dtype=np.float64)
            self._ck(self.lib.ilqg_multi_set_param(self.h, k.encode(), a, a.size))
        for k, val in (opts or {}).items():
            a = np.ascontiguousarray(np.atleast_1d(val), dtype=np.float64)
            self._ck(self.lib.ilqg_multi_set_option(self.h, k.encode(), a, a.size))

    def _ck(self, rc):
        if rc:
            raise IlqgError(self.lib.ilqg_multi_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ilqg_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def devices(self):
        return int(self.lib.ilqg_multi_devices(self.h))

    def init(self, x0, u0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(self.B, self.problem.nx)
        u0 = np.ascontiguousarray(u0, dtype=np.float64).reshape(self.B, self.N, self.problem.nu)
        self._ck(self.lib.ilqg_multi_set_x0(self.h, x0))
        self._ck(self.lib.ilqg_multi_set_u(self.h, u0))
        self._ck(self.lib.ilqg_multi_init(self.h))

    def iterate(self, n=1):
        self._ck(self.lib.ilqg_multi_iterate(self.h, int(n)))

    def set_params_batch(self, params):
        """BatchSolver.set_params_batch on every shard, each with the rows of its trajectories (ilqg_multi_set_params_batch),
        numpy arrays"""
        if params is not None and not isinstance(params, dict):
            raise IlqgError("set_params_batch: params must be a dict of parameter name -> array [B, size]; {} or None clears the set")
        entry = _receding_entry(self.lib, "ilqg_multi_set_params_batch")
        if not params:
            self._ck(entry(self.h, 0, None, None))
            return
        names, values, _ = _pack_arrays("set_params_batch", self.problem, params, ((self.B,),), "all trajectories")
        self._ck(entry(self.h, len(names), names, _address(values)))

    def set_param_steps_batch(self, name, values):
        """BatchSolver.set_param_steps_batch on every shard, each with the rows of its trajectories
        (ilqg_multi_set_param_steps_batch), numpy arrays; None makes the name shared again"""
        who = "set_param_steps_batch"
        cname = _param_steps_name(self.problem, who, name)
        ptr, keep = (None, None) if values is None else _param_steps_rows(who, "values", values, (self.B, self.N + 1), False, None)
        self._ck(_receding_entry(self.lib, "ilqg_multi_set_param_steps_batch")(self.h, cname, ptr))
        _note_step_rows(self, name, values is not None)

    def shift_param_batch(self, name, steps, tail=None):
        """BatchSolver.shift_param_batch on every shard, each with the tails of its trajectories (ilqg_multi_shift_param_batch)"""
        who = "shift_param_batch"
        cname = _param_steps_name(self.problem, who, name)
        ptr, keep = (None, None) if tail is None else _param_steps_rows(who, "tail", tail, (self.B, max(int(steps), 0)), False, None)
        self._ck(_receding_entry(self.lib, "ilqg_multi_shift_param_batch")(self.h, cname, int(steps), ptr))

    def shift(self, steps, x0=None, u_tail=None):
        """BatchSolver.shift on every shard (ilqg_multi_shift)"""
        x0, u_tail = _optional(x0, (self.B, self.problem.nx)), _optional(u_tail, (self.B, max(int(steps), 0), self.problem.nu))
        self._ck(_receding_entry(self.lib, "ilqg_multi_shift")(self.h, int(steps), _address(x0), _address(u_tail)))

    def best_of(self, K, score=None):
        """BatchSolver.best_of of every shard (ilqg_multi_best_of), numpy arrays; winner is absolute in the whole batch.  Refused
        when a shard's first trajectory is not a multiple of K."""
        return _best_of(self, "ilqg_multi_", K, score, False)

    def shift_winners(self, K, winner, steps, x0=None, u_tail=None, du=None):
        """BatchSolver.shift_winners on every shard (ilqg_multi_shift_winners), numpy arrays"""
        _shift_winners(self, "ilqg_multi_", K, winner, steps, x0, u_tail, du, False)

    def head(self, steps, gains=False):
        """BatchSolver.head of every shard (ilqg_multi_head), numpy arrays"""
        out, ptr = _head_outputs(self, steps, gains)
        self._ck(_receding_entry(self.lib, "ilqg_multi_head")(self.h, int(steps), *ptr))
        return out

    def policy_rollout(self, x0, alpha=1.0, feedback=True, trajectories=False, params=None, disturbance=None, noise=None, noise_shared=False,
                       first_trajectory=0):
        """BatchSolver.policy_rollout of every shard (ilqg_multi_policy_rollout, with params ilqg_multi_policy_rollout_params,
        with a disturbance ilqg_multi_policy_rollout_noise: a [B,R,N,nx] table sharded by rows, a [R,N,nx] one given to every shard;
        with noise = (seed, sigma) ilqg_multi_policy_rollout_drawn: every shard draws under its own first trajectory, the bits of the single batch),
        numpy arrays"""
        return _policy_rollout(self, "ilqg_multi_policy_rollout", x0, alpha, feedback, trajectories, params, disturbance, noise, noise_shared,
                               first_trajectory)

    def receding_plant(self, rounds, steps, iterations, feedback=True, x_plant=None, params=None, disturbance=None, windows=None):
        """BatchSolver.receding_plant of every shard, one shard after the other (ilqg_multi_receding_plant, with windows
        ilqg_multi_receding_plant_windows: a future [B, rounds*steps] is sharded by rows), numpy arrays"""
        return _receding_plant(self, "ilqg_multi_receding_plant", rounds, steps, iterations, feedback, x_plant, params, disturbance, windows)

    def solve(self):
        self._ck(self.lib.ilqg_multi_solve(self.h))

    def sync(self):
        self._ck(self.lib.ilqg_multi_sync(self.h))

    def active(self):
        n = np.zeros(1, dtype=np.int32)
        self._ck(self.lib.ilqg_multi_active(self.h, n))
        return int(n[0])

    def costs(self):
        """the single collective: per-trajectory costs of all devices, gathered over RCCL"""
        out = np.zeros(self.B)
        self._ck(self.lib.ilqg_multi_gather_costs(self.h, out))
        return out

    def x(self):
        out = np.zeros((self.B, self.N + 1, self.problem.nx))
        self._ck(self.lib.ilqg_multi_get_x(self.h, out))
        return out

    def u(self):
        out = np.zeros((self.B, self.N, self.problem.nu))
        self._ck(self.lib.ilqg_multi_get_u(self.h, out))
        return out

    def multiplier_dims(self):
        d = np.zeros(2, dtype=np.int32)
        self.lib.ilqg_problem_multiplier_dims(d)
        return int(d[0]), int(d[1])

    def set_history(self, cap):
        """BatchSolver.set_history on every shard (ilqg_multi_set_history)"""
        _set_history(self, "ilqg_multi_", cap)

    def history(self, names=None):
        """BatchSolver.history of every shard, placed by rows (ilqg_multi_get_history / _get_history_int)"""
        return _history(self, "ilqg_multi_", names)

    def ints(self, name):
        out = np.zeros((self.B, MAX_ALPHA if name == "alpha_ok" else 1), dtype=np.int32)
        self._ck(self.lib.ilqg_multi_get_int(self.h, name.encode(), out))
        return out if name == "alpha_ok" else out[:, 0]


def solve_single(x0, u_nom, params, opts=None, problem="carparking", full_ddp=0, strict=False):
    """[success, x, u, cost] = iLQG<Problem>(x0, u_nom, params, opts) — the reference's MEX entry (iLQG_mex.c:19-144)
    through ilqg_solve_single: the drop-in iLQG() with back_pass() / line_search() on the GPU.
    Returns dict(success, x [N+1,nx], u [N,nu], cost, iterations, seconds)."""
    prob = Problem(problem, full_ddp, strict)
    u_nom = np.ascontiguousarray(u_nom, dtype=np.float64).reshape(-1, prob.nu)
    n_hor = u_nom.shape[0]
    x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(prob.nx)
    p_arr, p_n, keep1 = _named_list(params or {})
    o_arr, o_n, keep2 = _named_list(opts or {})
    x = np.zeros((n_hor + 1, prob.nx))
    u = np.zeros((n_hor, prob.nu))
    cost, secs, iters = np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.int32)
    err = C.create_string_buffer(512)
    rc = prob.lib.ilqg_solve_single(n_hor, x0, u_nom, p_arr, p_n, o_arr, o_n, x, u, cost, iters, secs, err, 512)
    if rc < 0:
        raise IlqgError(err.value.decode())
    return dict(success=int(rc), x=x, u=u, cost=float(cost[0]), iterations=int(iters[0]), seconds=float(secs[0]))


def boxqp_batch(n, H, g, lower, upper, x0, problem="carparking", full_ddp=0, device=0, strict=False, cooperative=False, active=None):
    """device box-QP on `count` independent problems (arrays [count, ...]); unit-test entry.
    cooperative: the form of the one-wavefront-per-trajectory mapping (one lane per variable; the one the library's
    backward step runs: box_qp_row, or box_qp_rows in the `elem` library);
    cooperative="table": the per-lane form with the factorisations of all clamp patterns made up front;
    cooperative="quad": the form of the quad mapping, four problems per wavefront (problems 4 w ... 4 w + 3 are the rows of
    wavefront w; libraries of the wave mapping only).  active [count] (quad only): 0 = the problem's row runs along and
    commits nothing — x as given, rc 0; None = all active"""
    lib = load_library(problem, full_ddp, strict)
    H = np.ascontiguousarray(H, dtype=np.float64)
    count = H.shape[0]
    t = n * (n + 1) // 2
    x = np.array(x0, dtype=np.float64).reshape(count, n).copy()
    clamp = np.zeros((count, n), dtype=np.int32)
    nfree = np.zeros(count, dtype=np.int32)
    invH = np.zeros((count, t))
    rc = np.zeros(count, dtype=np.int32)
    fn = lib.ilqg_boxqp_table_batch if cooperative == "table" else (lib.ilqg_boxqp_wave_batch if cooperative else lib.ilqg_boxqp_batch)
    more = ()
    if cooperative == "quad":
        if not hasattr(lib, "ilqg_boxqp_quad_batch"):
            raise IlqgError("boxqp_batch: %s has no ilqg_boxqp_quad_batch: build it again" % library_path(problem, full_ddp, strict))
        fn = lib.ilqg_boxqp_quad_batch
        if active is not None:
            active = np.ascontiguousarray(active, dtype=np.int32)
            if active.shape != (count,):
                raise IlqgError("boxqp_batch: active must hold one entry per problem")
        more = (None if active is None else active.ctypes.data,)
    elif active is not None:
        raise IlqgError('boxqp_batch: active goes with cooperative="quad"')
    r = fn(device, n, count, H.reshape(count, t), np.ascontiguousarray(g, dtype=np.float64),
           np.ascontiguousarray(lower, dtype=np.float64), np.ascontiguousarray(upper, dtype=np.float64),
           x, clamp, nfree, invH, rc, *more)
    if r:
        raise IlqgError(lib.ilqg_batch_error(None).decode() if cooperative == "quad" else "ilqg_boxqp_batch failed")
    return dict(rc=rc, x=x, clamp=clamp, n_free=nfree, invH=invH)


def sincos_batch(x, problem="carparking", full_ddp=0, device=0, strict=False):
    """device sin/cos exactly as the generated callbacks get them; unit-test entry"""
    lib = load_library(problem, full_ddp, strict)
    x = np.ascontiguousarray(x, dtype=np.float64)
    s, c = np.zeros_like(x), np.zeros_like(x)
    if lib.ilqg_sincos_batch(device, x.size, x, s, c):
        raise IlqgError("ilqg_sincos_batch failed")
    return s, c


# CarParking demo parameters, reference examples/CarParking/testCar.m:2-11
CAR_PARAMS = dict(
    d=[2.0], h=[0.03],
    pf=[0.01, 0.01, 0.01, 1.0], cf=[0.1, 0.1, 1.0, 0.3],
    cu=[1e-2, 1e-4], cx=[1e-3, 1e-3], px=[0.1, 0.1],
    limW=[-0.5, 0.5], limA=[-2.0, 2.0],
)
