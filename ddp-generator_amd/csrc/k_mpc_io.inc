// The control interval of a caller with its OWN plant (ilqg_dev_head*, ilqg_dev_put_*_device, ilqg_dev_shift_param): the
// first steps of every plan leave the solver's layouts for trajectory-major arrays, and the window of a per-time-step
// parameter moves with the horizon, without a field or a table crossing to the host.  No arithmetic.  The device-source
// forms of the x0 / tail writes are the existing k_nom_io, k_to_dev and k_put_u_steps fed from the caller's pointer.

// k_head: x_k, u_k, l_k, L_k for k < steps and the cost of every CURRENT plan into x [B][steps][NX], u [B][steps][NU],
// l [B][steps][NU], L [B][steps][NXU] (column-major per step, as the host getter), cost [B]; any pointer may be null.
// x / u are read where the current trajectory lives (cur_x / cur_u: the tiled X / U or a kept roll-out plane in the lane
// mapping, the packed records in the wave mapping), l / L from the packed records in both mappings (what the host
// getters read, has_tiled_scratch).
//
// Thread-to-element map.  The two sides want opposite orders: the tiled arrays are contiguous along the TRAJECTORY (one
// (step, component) of 8 consecutive trajectories is one 64-byte segment), the outputs — and the records — along the
// COMPONENT (for one trajectory the q = k * w + c, q < steps * w, are consecutive doubles).  Neither is favoured: a
// wavefront takes a block of 8 trajectories x 8 consecutive q, the trajectory on the low three lane bits.  Every tiled read
// of the wavefront is then a whole 64-byte segment (8 lanes each), and every write a run of 8 doubles = 64 bytes per
// trajectory (for steps * w < 8, e.g. CarParking's x with steps = 1, runs of w doubles that are adjacent from one
// trajectory to the next: the 8 trajectories' 256 bytes are contiguous); reads from the records are runs of up to 64 bytes
// too.  A map with the trajectory fastest over the whole wavefront (k_log_steps) would write one double per 64-byte
// segment for the 16 x 8 problem; one with the component fastest would read the tiled arrays that way.  The price is
// idle lanes where steps * w < 8, on a kernel that moves a few bytes per trajectory.
// Grid: x = blocks of 8 trajectories, y = groups of HEAD_WAVES tiles of 8 q over the four fields one behind the other.
constexpr int HEAD_WAVES = 4;
__global__ void __launch_bounds__(WAVE * HEAD_WAVES) k_head(DevPtrs P, int steps, double *__restrict__ ox, double *__restrict__ ou,
                                                          double *__restrict__ ol, double *__restrict__ oL, double *__restrict__ oc) {
    const int lane = (int)(threadIdx.x & 63);
    const int b = (int)blockIdx.x * 8 + (lane & 7);
    int tile = (int)blockIdx.y * HEAD_WAVES + (int)(threadIdx.x >> 6);  // wave-uniform
    if(oc && blockIdx.y == 0 && threadIdx.x < 8 && b < P.B) oc[b] = P.f[ILQG_F_COST][b];
    if(b >= P.B) return;
    const int tx = ox ? (steps * NX + 7) / 8 : 0, tu = ou ? (steps * NU + 7) / 8 : 0, tl = ol ? (steps * NU + 7) / 8 : 0,
              tL = oL ? (steps * NXU + 7) / 8 : 0;
    if(tile < tx) {
        const int q = tile * 8 + (lane >> 3);
        if(q < steps * NX) ox[(size_t)b * steps * NX + q] = cur_x(P, q / NX, b)[(size_t)(q % NX) * XSI];
        return;
    }
    tile -= tx;
    if(tile < tu) {
        const int q = tile * 8 + (lane >> 3);
        if(q < steps * NU) ou[(size_t)b * steps * NU + q] = cur_u(P, q / NU, b)[(size_t)(q % NU) * XSI];
        return;
    }
    tile -= tu;
    if(tile < tl) {
        const int q = tile * 8 + (lane >> 3);
        if(q < steps * NU) ol[(size_t)b * steps * NU + q] = nomp(P, q / NU, b)[NOM_L + q % NU];
        return;
    }
    tile -= tl;
    if(tile < tL) {
        const int q = tile * 8 + (lane >> 3);
        if(q < steps * NXU) oL[(size_t)b * steps * NXU + q] = nomp(P, q / NXU, b)[NOM_K + q % NXU];
    }
}

// The windows of a per-time-step parameter (n = n_hor + 1 doubles each, in global memory) move `steps` values on, in place:
// p'[k] = p[k + steps], the last `steps` values from the row's tail or, with tail null, p[n - 1] held — shift_row
// (k_shift.inc), one workgroup per row: rows [grid][n], tail [grid][steps] or null.  The per-trajectory windows
// (ilqg_dev_shift_param_batch) are B rows, the one shared window (param_bufs, ilqg_dev_shift_param) is one.  Index
// arithmetic over B n in size_t.
__global__ void __launch_bounds__(PARAM_BLOCK) k_shift_param_rows(double *__restrict__ rows, int n, int steps, const double *__restrict__ tail) {
    if(steps <= 0) return;
    shift_row(rows + (size_t)blockIdx.x * (size_t)n, n, steps, tail ? tail + (size_t)blockIdx.x * (size_t)steps : nullptr);
}

// ALL windows of a context move with the horizon in ONE launch, fed from futures that already lie on the device
// (ilqg_dev_loop_shift: the resident loops ilqg_batch_receding_windows / _receding_plant_windows).  Per size -1 parameter of
// the problem — its slot, grid.y — a descriptor by value: the window's base, its row count (B for a parameter with rows per
// trajectory, 1 for the shared window), the base of its future or null (hold the last value, per row) and the future's row
// stride (rounds * steps, or 0 for a shared future).  grid.x is the row; the workgroups beyond a slot's row count return at
// once.  The tail of this round is columns [col, col + steps) of the row's future, col = round * steps.  Within a row
// shift_row, one workgroup per row as in k_shift_param_rows.  Index arithmetic over B n and B rounds steps in size_t.  Plain
// loads and stores, no LDS.  A template on the number of slots, so that it exists only in libraries whose problem has a
// per-time-step parameter.
struct WindowDesc {
    double *base;
    const double *future;
    size_t stride;
    int rows;
};
template <int n_slots>
struct WindowSet {
    WindowDesc w[n_slots];
};
template <int n_slots>
__global__ void __launch_bounds__(PARAM_BLOCK) k_shift_windows(WindowSet<n_slots> S, int n, int steps, int col) {
    const WindowDesc w = S.w[blockIdx.y];
    if(steps <= 0 || (int)blockIdx.x >= w.rows) return;  // (uniform over the workgroup: nobody is left at the barrier)
    shift_row(w.base + (size_t)blockIdx.x * (size_t)n, n, steps, w.future ? w.future + (size_t)blockIdx.x * w.stride + (size_t)col : nullptr);
}
