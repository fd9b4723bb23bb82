// The extern-"C" shim (ilqg_shim.h) over the kernels: buffers, streams, launches, collectives.  Included by
// ilqg_kernels.hip behind the kernels; not a translation unit of its own.

// ===========================================================================
// shim
// ===========================================================================
#if ILQG_WAVE_MAP
// Wave mapping: the derivative records of a chunk of trajectories (trajEl_t structs, 48 KB each with the tensors of the
// n = 16 problem) live in ONE work buffer per device, shared by all solver contexts on it.  A context owns the buffer
// from the start of a derivatives + backward pass to its end; the hand-over is an event on the streams, so a second
// context's pass starts when the first one's has finished — which is also the schedule that pays: the backward pass
// fills the chip, the roll-outs (one lane per trajectory and step size) cannot, so with the batch advancing as two
// groups of trajectories the roll-outs of one run beside the backward pass of the other.
// (Reference-counted and process-wide, allocated by a loop that halves the request until the device has it: the one device
// allocation of a context that is NOT a Buffer below.)
struct SharedWork {
    trajEl_t *buf;
    size_t bytes;
    hipEvent_t free_ev;  // recorded when the current owner is done with the buffer
    int refs;
    // which constant record entries (init_running) the buffer holds: for whom, and where
    bool whole, half[2], factored, pv_set;
    int N, B, part, half_cap;
    ParamValues pv;
};
static SharedWork g_work[64];
#else
struct SharedWork;
#endif

constexpr int QUEUE_CELL = 32;  // ints between two counters: a cache line each

namespace {  // (internal linkage: the libraries export the C entries, no symbol of these types)

// The ONE owner of memory the shim allocates: device memory, or with PinnedMem as the second argument pinned host memory.
// Move-only; the destructor frees.  The acquiring calls return the shim's 0 / 1 with g_err set (HIP_TRY) and leave the
// buffer empty, bytes() == 0, when the allocation fails.  `drain`: the stream whose queued work may still read the old
// memory, synchronised before it is freed (nullptr: nothing can).
struct DeviceMem {
    static hipError_t take(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t give(void *p) { return hipFree(p); }
};
struct PinnedMem {
    static hipError_t take(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t give(void *p) { return hipHostFree(p); }
};
template <class T, class Mem = DeviceMem>
class Buffer {
    T *p_ = nullptr;
    size_t bytes_ = 0;

  public:
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept {
        if(this != &o) {
            (void)release();
            p_ = o.p_, bytes_ = o.bytes_;
            o.p_ = nullptr, o.bytes_ = 0;
        }
        return *this;
    }
    ~Buffer() {
        if(p_) (void)Mem::give(p_);
    }
    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }
    // frees and forgets (also where the free fails)
    int release() {
        T *old = p_;
        p_ = nullptr, bytes_ = 0;
        if(old) HIP_TRY(Mem::give(old));
        return 0;
    }
    // frees, then allocates exactly `bytes`
    int renew(size_t bytes) {
        if(release()) return 1;
        const hipError_t allocation = Mem::take((void **)&p_, bytes);
        if(allocation != hipSuccess) p_ = nullptr;
        HIP_TRY(allocation);
        bytes_ = bytes;
        return 0;
    }
    // grow-only: nothing if the buffer holds `bytes`; else drain, free, allocate
    int reserve(size_t bytes, hipStream_t drain = nullptr) {
        if(bytes <= bytes_) return 0;
        if(drain) HIP_TRY(hipStreamSynchronize(drain));
        return renew(bytes);
    }
    // the same for a buffer the caller can do without: 2 = the device does not have the memory (the error is cleared)
    int try_reserve(size_t bytes, hipStream_t drain) {
        if(bytes <= bytes_) return 0;
        HIP_TRY(hipStreamSynchronize(drain));
        if(release()) return 1;
        // (ILQG_TEST_NO_PLANES: the tests' way to a device that is out of memory)
        if(getenv("ILQG_TEST_NO_PLANES") || Mem::take((void **)&p_, bytes) != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
            return 2;
        }
        bytes_ = bytes;
        return 0;
    }
};
// A view in DevPtrs follows its owner in the statement that acquires, grows or releases it: `rc` is that call's result
template <class T>
static int repoint(T *&view, const Buffer<T> &owner, int rc) {
    view = owner.get();
    return rc;
}

// Everything a context allocates.  DevPtrs P holds plain views of these for the kernels; sizes live here, in bytes().
// ilqg_dev_destroy releases all of it in one statement; a new buffer is a member here and a reserve() where it is used.
struct DevBuffers {
    Buffer<double> f[ILQG_F_COUNT], nom;   // P.f[], P.nom
    Buffer<int> i[ILQG_I_COUNT], derivs_failed, pending_list, n_pending;  // P.i[], P.derivs_failed, P.pending, P.n_pending
    Buffer<trajEl_t> work;                 // P.work of stage-by-stage calls (own_work)
    Buffer<double *> param_table;          // P.p: the table of the pointers below
    std::vector<Buffer<double>> param_bufs;
    Buffer<int> counter;
    Buffer<int> queues;    // wave mapping: the backward kernel's trajectory counters (DevPtrs::queue), QUEUE_CELL ints apart
    Buffer<double> cand, cand1;            // P.cand, P.cand1
    Buffer<double> xpl, upl;               // P.xpl, P.upl (ls_keep = 2)
    Buffer<unsigned> spec_ints;            // quad mapping with speculative retries: the protocol's words
    Buffer<double> spec_doubles;           //   ... the rows' results and gains
    Buffer<double> log_x, log_u, log_c;    // receding horizon: the applied steps of every round (ilqg_dev_loop_begin), host layout
    // the plants of a closed loop (ilqg_dev_loop_begin): their states [B][NX], failure flags [B], the sums of the applied
    // running costs [B][rounds] (the applied steps and the plans' costs go to the log above), and what the caller sent:
    // the parameter rows [B][W] with their map, the disturbances [B][rounds * steps][NX]
    Buffer<double> plant_xp, plant_cost, plant_values, plant_dist;
    Buffer<int> plant_failed;
    Buffer<NoiseSpec> noise_spec;          // what a drawn launch reads of its caller (k_noise.inc), written in stream order by noise_spec_put
    // per-trajectory problem parameters (ilqg_dev_set_params_batch): the rows [B][W]; the buffer only grows and outlives a cleared set
    Buffer<double> pb_values;
    // per-time-step parameters per trajectory (ilqg_dev_set_param_steps_batch): for the s-th parameter of size -1 its rows
    // [Bp][N + 1] (trajectory-major; rows B .. Bp - 1 are zero and belong to nobody); grow-only like pb_values
    static constexpr int SR = N_STEP_PARAMS > 0 ? N_STEP_PARAMS : 1;
    Buffer<double> sr_rows[SR];
    // the futures of a resident loop's windows (ilqg_dev_loop_begin): per slot the values beyond the window, [B][rounds * steps]
    // for a parameter with rows, [rounds * steps] for the shared window; grow-only
    Buffer<double> win_future[SR];
    Buffer<double> hist_d;                 // the iteration history (ilqg_dev_set_history): History::d, History::i
    Buffer<int> hist_i;
    Buffer<double> hist_next_d;            //   ... and those of the capacity it is about to take (ilqg_dev_reserve_history)
    Buffer<int> hist_next_i;
    Buffer<unsigned long long> harvest;    // the packed records of ilqg_dev_harvest, and their copy on the host; both only grow
    Buffer<char, PinnedMem> harvest_host;
    Buffer<double> staging;                // see io_deferred
    Buffer<char, PinnedMem> pinned;
};

// What a launch of a wave-mapped derivative or sweep kernel is, stated ONCE per instantiation (wave_kernels_fill): dev_fill
// walks the descriptions for the scratch question and the LDS limit, wave_backward launches what derivs_kernel / sweep_kernel
// pick.  A launch over n items (trajectories; records for the derivatives) takes ceil(n / per_wg) workgroups, at most
// cap * CUs of them.
template <class Fn>
struct WaveKernel {
    Fn fn;
    int block;
    size_t lds;        // dynamic LDS of a launch
    int per_wg;        // items a workgroup takes
    int cap;           // most workgroups per CU in the grid (0: no cap; 1: the kernel's LDS leaves a CU one workgroup at a time)
    size_t lds_limit;  // hipFuncAttributeMaxDynamicSharedMemorySize where the kernel needs more than the default 64 KB (0: not set)
    bool scratch;      // the runtime gives it scratch memory (uses_scratch on the context's device): it runs on the shared roll-out stream
    dim3 grid(size_t n, int cus) const {
        const size_t wgs = (n + per_wg - 1) / per_wg, most = (size_t)cap * cus;
        return dim3((unsigned)(cap && most < wgs ? most : wgs));
    }
};
struct WaveKernels {
    WaveKernel<void (*)(DevPtrs, ilqg_dev_opts_t, ParamValues, int, int, int, int, int)> derivs[2];  // records: [factored, general]
    WaveKernel<void (*)(DevPtrs, ilqg_dev_opts_t, int, int, int)> sweep[6];  // quad, quad with speculative retries, row: [factored, general] each
};

}  // namespace

struct ilqg_dev : DevBuffers {
    int device, B, Bp, N;
    hipStream_t stream;
    DevPtrs P;
    ilqg_dev_opts_t O;
    ParamValues pv;       // fixed-size parameters, passed to the kernels by value
    // Deferred transfers (ilqg_dev_io_begin .. ilqg_dev_io_end): every write / read takes its own slice of the device
    // staging buffer and of a pinned host buffer and nothing waits; the stream is synchronised once, at the end, and
    // the reads are handed to the caller then.  (The drop-in back_pass() / line_search() move two dozen small arrays
    // per call: one wait instead of one per array.)
    bool io_deferred;
    size_t io_off;
    struct PendingRead { void *dst; const void *src; size_t bytes; int transpose_w; };
    std::vector<PendingRead> pending;
    bool keep_first;      // the roll-out launch in progress keeps the first stage's roll-outs in P.cand1
    size_t roll_pad;              // wave mapping: LDS on top of the records' buffer when the roll-outs' records go through LDS
    bool roll_dma;                // wave mapping: k_rollout_parts fetches the nominal records through LDS
    int loc_set;          // the set of planes current trajectories may live in (-1: none, all in X / U)
    bool defer_commit, commit_pending, pending_zero;  // ls_keep = 2: k_update commits / clears the pending counter
    int commit_s1, commit_set;
    bool winner_done;     // the last search ended with the accepted trajectories in place (two-stage search)
    int cus;              // compute units of the device
    bool work_consts;     // wave mapping: constant entries of the records written (init_running)
    bool half_consts[2];  // wave mapping: the same per half of the work buffer (chunks alternate between the halves)
    hipStream_t stream2;  // wave mapping: second stream of the chunk pipeline, fork / join events
    hipEvent_t fork, join;
    // Wave mapping: the roll-outs run through the generated callbacks with a trajEl_t per lane in scratch memory
    // (48 KB per lane for the n = 16 problem with its tensors) and the runtime reserves scratch per queue for every
    // wavefront the chip can hold — one queue works, a second one runs out of resources.  All roll-outs of all
    // contexts (groups) of a device therefore share ONE stream, tied to each context's own stream by events; the
    // backward passes of the other groups overlap with them.
    hipStream_t roll;
    hipEvent_t roll_in, roll_out;
    struct SharedWork *shared;  // wave mapping: the device's derivative work buffer (see SharedWork)
    bool per_step_params;       // some problem parameter has one value per time step
    // The resident loop that is open (ilqg_dev_loop_begin; rounds = 0: none): the shape of its logs and futures, and what its
    // per-round steps do
    struct Loop {
        int rounds, steps;
        bool plant, windows;
        bool named;             // the plants run under plant_values and this map
        PolicyParamMap map;
        bool given[SR];         // the slot has a future in win_future[s] (else its window holds)
    } loop;
    // pb_on: the lane-mapped kernels that take ParamValues run as the instantiation whose pack is the table pb_values and its map
    // (with_rows)
    bool pb_on;
    PolicyParamMap pb_map;
    bool sr_on[SR];             // sr_rows[s] is in use
    // what with_rows hands the rows twins: rows_on = pb_on or some sr_on; rows_map = pb_map (empty without a table) with the
    // step rows in use (rows_refresh, after every change of either set)
    bool rows_on;
    PolicyParamMap rows_map;
    int hist_next_cap;          // the capacity hist_next_d / hist_next_i were made for (0: none aside)
    History hist;               // views of hist_d / hist_i; cap = 0: no history, ilqg_dev_update launches nothing for it
    hipEvent_t ext_in, ext_out;  // ordering with a stream of the caller (ilqg_dev_stream_in / _out), made with the context
    // Switches of the environment (comparison runs, tests), read ONCE when the context is made: a change of the environment
    // between two calls of a solve does not switch mappings or piece layouts under it.
    // (read_env; roll_lds: wave mapping, the dynamic LDS asked for by the second-stage roll-outs — one workgroup per CU)
    struct EnvSwitches { bool no_quad, quad_stored, two_pieces, deriv_parts, no_dma, no_rollout_parts, quad_spec, second_stream; size_t roll_lds; } env;
    WaveKernels wave_kernels;  // wave mapping: the derivative and sweep kernels as THIS context's device runs them
    bool timing;
    struct Span { int kernel; hipEvent_t a, b; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;  // events of drained spans, reused: none is created while a window is timed
    double t_ms[ILQG_K_TOTAL];
    int t_n[ILQG_K_TOTAL];
    // launches of one kernel on the context's two streams overlap in the event clock (the later one waits for the chip):
    // t_busy is the length of the UNION of a kernel's launch intervals, measured against an event recorded when timing
    // was switched on
    hipEvent_t epoch;
    double t_busy[ILQG_K_TOTAL];
};

namespace {

static ilqg_dev *g_spec_last;  // the context whose backward pass ran with speculative retries last (measurement: ilqg_dev_spec_words)
struct FieldInfo { int steps_plus; int wd, wh; };  // steps = steps_plus<0 ? 1 : N + steps_plus

FieldInfo field_info(int f) {
    switch(f) {
        case ILQG_F_X: return {1, NX, NX};
        case ILQG_F_U: return {0, NU, NU};
        case ILQG_F_LG: return {0, NU, NU};
        case ILQG_F_KG: return {0, NXU, NXU};
        case ILQG_F_DER: return {0, WAVE_MAP ? REC_HOST : REC, REC_HOST};
        case ILQG_F_FIN: return {-1, FIN, FIN};
        case ILQG_F_MUL: return {0, MEW, MEW};
        case ILQG_F_MULF: return {-1, MFW, MFW};
        case ILQG_F_ALPHA_COST: return {-1, ILQG_MAX_ALPHA, ILQG_MAX_ALPHA};
        default: return {-1, 1, 1};
    }
}

// columns of the packed trajectory records (nomp): first column, or -1 for any other field
int nom_column(int field) {
    switch(field) {
        case ILQG_F_X: return NOM_X;
        case ILQG_F_U: return NOM_U;
        case ILQG_F_LG: return NOM_L;
        case ILQG_F_KG: return NOM_K;
        default: return -1;
    }
}
// lane mapping: X and U also exist as tiled arrays, the representation the host reads (see cur_x)
bool has_tiled_copy(int field) { return !WAVE_MAP && (field == ILQG_F_X || field == ILQG_F_U); }
// lane mapping: tiled l / L are the output of the backward pass over stored records only (see k_pack_records);
// the host reads and writes gains in the records
bool has_tiled_scratch(int field) { return !WAVE_MAP && (field == ILQG_F_LG || field == ILQG_F_KG); }
int field_steps(const ilqg_dev *d, int f) {
    const FieldInfo fi = field_info(f);
    return fi.steps_plus < 0 ? 1 : d->N + fi.steps_plus;
}

int int_field_width(int f) { return f == ILQG_I_ALPHA_OK ? ILQG_MAX_ALPHA : 1; }

// end of a deferred batch (or of a part of it): wait once, deliver the reads
int io_flush(ilqg_dev *d) {
    HIP_TRY(hipStreamSynchronize(d->stream));
    for(const auto &r : d->pending) {
        if(r.transpose_w) {  // int field: device [width][Bp] -> host [B][width]
            const int *src = (const int *)r.src;
            int *dst = (int *)r.dst;
            for(int b = 0; b < d->B; b++)
                for(int j = 0; j < r.transpose_w; j++) dst[(size_t)b * r.transpose_w + j] = src[(size_t)j * d->Bp + b];
        } else {
            memcpy(r.dst, r.src, r.bytes);
        }
    }
    d->pending.clear();
    d->io_off = 0;
    return 0;
}

// Staging for one transfer of `bytes`: *dev in the device staging buffer and, while transfers are deferred, *pin in the
// pinned host buffer (nullptr otherwise: the transfer then uses the caller's memory and is waited for at once).
int stage(ilqg_dev *d, size_t bytes, void **dev, void **pin) {
    if(!d->io_deferred) {
        if(d->staging.reserve(bytes)) return 1;
        *dev = d->staging.get();
        *pin = nullptr;
        return 0;
    }
    bytes = (bytes + 255) & ~(size_t)255;
    if(d->io_off + bytes > d->staging.bytes() || d->io_off + bytes > d->pinned.bytes()) {
        if(io_flush(d)) return 1;  // what is in flight uses the old buffers
        const size_t want = (bytes > (1u << 20) ? bytes : (1u << 20)) + 2 * d->pinned.bytes();
        if(d->staging.reserve(want) || d->pinned.reserve(want)) return 1;
    }
    *dev = (char *)d->staging.get() + d->io_off;
    *pin = d->pinned.get() + d->io_off;
    d->io_off += bytes;
    return 0;
}
// host -> staging slice / staging slice -> host, according to the mode
int stage_in(ilqg_dev *d, void *dev, void *pin, const void *host, size_t bytes) {
    if(pin) {
        memcpy(pin, host, bytes);
        host = pin;
    }
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, d->stream));
    return 0;
}
int stage_out(ilqg_dev *d, const void *dev, void *pin, void *host, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(pin ? pin : host, dev, bytes, hipMemcpyDeviceToHost, d->stream));
    if(pin) d->pending.push_back({host, pin, bytes, 0});
    else HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}
int io_done(ilqg_dev *d) {  // end of a single write
    if(!d->io_deferred) HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

// The transfers of one entry.  The entry declares its inputs, then its outputs — in(p, bytes) / out(p, bytes), p its own
// pointer variable —, opens the plan, launches on what p points to now, and closes the plan.
// Host form: open() makes ONE stage() reservation for all of them (a second one could, while transfers are deferred, flush and
// regrow the buffers under addresses already handed out), cut into slices 256 bytes apart in the order declared, sends every
// input there and points each p at its slice; NULL or 0 bytes takes no room and leaves p NULL.  close() queues one copy per
// output; deferred, they are delivered by ilqg_dev_io_end; else this is the entry's one wait (without outputs: as io_done).
// on_device: p is device memory of the caller and stays as it is; nothing is staged, copied or waited for.
struct Staged {
    struct Slice { void *var; void *host; size_t bytes, off; bool out; };
    ilqg_dev *d;
    Slice s[8];  // (ilqg_dev_policy_rollout declares eight)
    int n = 0;
    bool on_device;
    size_t total = 0;
    char *dev = nullptr, *pin = nullptr;
    Staged(ilqg_dev *d, int on_device = 0) : d(d), on_device(on_device != 0) {}
    template <class T> void add(T *&p, size_t bytes, bool out) {
        if(on_device) return;
        if(!p || !bytes) {
            p = nullptr;
            return;
        }
        s[n++] = {&p, const_cast<void *>((const void *)p), bytes, total, out};
        total += (bytes + 255) & ~(size_t)255;
    }
    template <class T> void in(const T *&p, size_t bytes) { add(p, bytes, false); }
    template <class T> void out(T *&p, size_t bytes) { add(p, bytes, true); }
    int open() {
        void *dv, *pv;
        if(!n) return 0;
        if(stage(d, total, &dv, &pv)) return 1;
        dev = (char *)dv, pin = (char *)pv;
        for(int i = 0; i < n; i++) {
            void *at = dev + s[i].off;
            memcpy(s[i].var, &at, sizeof(at));  // (the entry's pointer, whatever it points to)
            if(!s[i].out && stage_in(d, at, pin ? pin + s[i].off : nullptr, s[i].host, s[i].bytes)) return 1;
        }
        return 0;
    }
    int close() {
        if(!n) return 0;
        for(int i = 0; i < n; i++) {
            if(!s[i].out) continue;
            void *to = pin ? (void *)(pin + s[i].off) : s[i].host;
            HIP_TRY(hipMemcpyAsync(to, dev + s[i].off, s[i].bytes, hipMemcpyDeviceToHost, d->stream));
            if(pin) d->pending.push_back({s[i].host, to, s[i].bytes, 0});
        }
        return io_done(d);
    }
};

struct Timed {
    ilqg_dev *d;
    int kernel;
    hipEvent_t a, b;
    hipStream_t st;
    static hipEvent_t take(ilqg_dev *d) {
        hipEvent_t e = nullptr;
        if(!d->event_pool.empty()) {
            e = d->event_pool.back();
            d->event_pool.pop_back();
        } else {
            hipEventCreate(&e);
        }
        return e;
    }
    Timed(ilqg_dev *d_, int k, hipStream_t stream = nullptr) : d(d_), kernel(k), a(nullptr), b(nullptr) {
        st = stream ? stream : d->stream;
        if(d->timing) {
            a = take(d);
            b = take(d);
            hipEventRecord(a, st);
        }
    }
    ~Timed() {
        if(d->timing) {
            hipEventRecord(b, st);
            d->spans.push_back({kernel, a, b});
        }
    }
};

int drain_spans(ilqg_dev *d) {
    if(d->spans.empty()) return 0;
    HIP_TRY(hipStreamSynchronize(d->stream));
    if(d->stream2) HIP_TRY(hipStreamSynchronize(d->stream2));
    if(d->roll) HIP_TRY(hipStreamSynchronize(d->roll));
    std::vector<std::pair<float, float>> iv[ILQG_K_TOTAL];
    for(auto &s : d->spans) {
        float ms = 0.f, t0 = 0.f;
        hipEventElapsedTime(&ms, s.a, s.b);
        d->t_ms[s.kernel] += ms;
        d->t_n[s.kernel]++;
        if(d->epoch && hipEventElapsedTime(&t0, d->epoch, s.a) == hipSuccess) iv[s.kernel].push_back({t0, t0 + ms});
        d->event_pool.push_back(s.a);
        d->event_pool.push_back(s.b);
    }
    (void)hipGetLastError();
    for(int k = 0; k < ILQG_K_TOTAL; k++) {  // union of the intervals of this batch of spans
        std::sort(iv[k].begin(), iv[k].end());
        float end = -1.f;
        for(auto &q : iv[k]) {
            if(q.second <= end) continue;
            d->t_busy[k] += q.second - (q.first > end ? q.first : end);
            end = q.second;
        }
    }
    d->spans.clear();
    return 0;
}

inline dim3 grid1(size_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

// the plants' buffers (ilqg_dev_loop_begin makes them anew for every loop; the caller has synchronised)
int plant_release(ilqg_dev *d) {
    d->loop.named = false;
    return d->plant_xp.release() | d->plant_cost.release() | d->plant_values.release() | d->plant_dist.release() | d->plant_failed.release();
}

}  // namespace

// Kernels with scratch memory (spills, the frames of called generated functions) all go to that shared stream too.  The
// runtime hands out scratch per QUEUE, and a request larger than an eighth of its pool is a single-use one that takes
// the largest piece of the pool that is free and is given back some time after the dispatch has retired (ROCr: "large"
// allocations).  The scalar roll-outs of an n = 16 problem are such requests (48 KB per lane); a kernel with scratch
// that follows one on ANOTHER queue asks while the pool is still taken, the runtime answers
// HSA_STATUS_ERROR_OUT_OF_RESOURCES and aborts the process — seen as a silent abort in the first iterate() behind an
// init(), once in a few hundred pairs, depending on timing.  On one queue the runtime releases the previous piece before
// it acquires the next.  (which kernels have scratch is asked of the runtime: hipFuncGetAttributes)
template <class K>
static bool uses_scratch(K kernel) {
    hipFuncAttributes a;
    if(hipFuncGetAttributes(&a, reinterpret_cast<const void *>(kernel)) != hipSuccess) return true;
    return a.localSizeBytes != 0;
}
// launch(stream) on the shared stream between two hand-overs with `st` if `needed` and the context has one, else on st
template <class Fn>
static int on_scratch_stream(ilqg_dev_t *d, bool needed, hipStream_t st, Fn &&launch) {
    if(!needed || !d->roll) {
        launch(st);
        return 0;
    }
    HIP_TRY(hipEventRecord(d->roll_in, st));
    HIP_TRY(hipStreamWaitEvent(d->roll, d->roll_in, 0));
    launch(d->roll);
    HIP_TRY(hipEventRecord(d->roll_out, d->roll));
    HIP_TRY(hipStreamWaitEvent(st, d->roll_out, 0));
    return 0;
}

// the step rows in use into a map (rows_refresh)
template <class Map>
static bool step_rows_into(Map &m, const ilqg_dev_t *d) {  // (a template: the member exists only with N_STEP_PARAMS > 0)
    bool any = false;
    if constexpr(N_STEP_PARAMS > 0) {
        for(int s = 0; s < N_STEP_PARAMS; s++) {
            m.rows[s] = d->sr_on[s] ? d->sr_rows[s].get() : nullptr;
            any = any || d->sr_on[s];
        }
    }
    return any;
}

// The ONE place that picks the instantiation of a lane-mapped kernel that takes ParamValues: the kernel as it was before
// there were per-trajectory parameters — its old name, an empty pack, not one argument more — unless the context holds a
// table (ilqg_dev_set_params_batch) or rows of a per-time-step parameter (ilqg_dev_set_param_steps_batch); then the
// instantiation whose pack is the table and its map, behind the kernel's own arguments — with step rows only, a table that
// is not read under an empty map (rows_refresh).  with_rows hands the launch, a generic callable, nothing or that pair:
//     with_rows(d, [&](auto... tr) { hipLaunchKernelGGL((k_rollout<RK_INIT, decltype(tr)...>), ..., tr...); });
// Both forms share the kernel's timing slot.  The wave mapping has no second form (ilqg_dev_set_params_batch refuses), and
// its libraries do not instantiate one.
template <class Launch>
static void with_rows(ilqg_dev_t *d, Launch &&launch) {
    if constexpr(!WAVE_MAP) {
        if(d->rows_on) return launch((const double *)d->pb_values.get(), d->rows_map);
    }
    launch();
}
// the same shape for a kernel's OWN rows behind them (k_policy<true>: values, shared, map; k_plant<true>: values, map)
template <class Launch, class... Own>
static void with_own_rows(bool on, Launch &&launch, Own... own) {
    if(!on) return launch();
    launch(own...);
}
// The two kernels that are no templates, k_derivs and k_multipliers, have a rows twin of another name, K_rows<table, map>
#if !ILQG_WAVE_MAP
#define LAUNCH_TWIN(d, K, grid, block, lds, stream, ...)                                                               \
    with_rows(d, [&](auto... tr) {                                                                                     \
        if constexpr(sizeof...(tr) == 0) hipLaunchKernelGGL(K, grid, block, lds, stream, __VA_ARGS__);                 \
        else hipLaunchKernelGGL((K##_rows<decltype(tr)...>), grid, block, lds, stream, __VA_ARGS__, tr...);            \
    })
#else
#define LAUNCH_TWIN(d, K, grid, block, lds, stream, ...) hipLaunchKernelGGL(K, grid, block, lds, stream, __VA_ARGS__)
#endif

// The ONE place that reads the environment's switches (dev_fill, first thing): presence switches, but for two
static ilqg_dev::EnvSwitches read_env() {
    const auto set = [](const char *name) { return getenv(name) != nullptr; };
    const auto number = [](const char *name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; };
    ilqg_dev::EnvSwitches e;
    e.no_quad = set("ILQG_NO_QUAD");
    // stored tensors in the quad mapping (ilqg_quad.hpp): measured behind the row mapping at config 5 (1.66-1.71 against 1.82
    // iterations/s, profiles/r6_stored_path.txt — both kernels share the HBM with k_derivs_wave of the other half of the
    // buffer, and four trajectories' loads per wavefront gain nothing there); kept, tested, off unless ILQG_QUAD_STORED=1
    e.quad_stored = number("ILQG_QUAD_STORED", 0) != 0;
    e.two_pieces = set("ILQG_TWO_PIECES");
    e.deriv_parts = set("ILQG_DERIV_PARTS");
    e.no_dma = set("ILQG_NO_DMA");
    e.no_rollout_parts = set("ILQG_NO_ROLLOUT_PARTS");
    e.quad_spec = number("ILQG_QUAD_SPEC", 1) != 0;  // on unless ILQG_QUAD_SPEC=0
    e.second_stream = set("ILQG_SECOND_STREAM");
    // measured (config 5, ~300 busy workgroups in the second stage): 32.9 / 40.3 ms without, 33.0 / 28.5 ms with;
    // with fewer than 256 busy workgroups every one of them gets a CU to itself (ILQG_ROLL_LDS_KB=0: off)
    e.roll_lds = (size_t)number("ILQG_ROLL_LDS_KB", 84) * 1024;
    return e;
}

#if ILQG_WAVE_MAP
// The descriptions, in the order the code object lays the kernels out (the order of first reference in this file: another one
// moves pc-relative call offsets in the kernels' code).  FACTORED = false builds name the general kernel twice; nothing
// selects the first of a pair there (`fact` needs FACTORED).
static void wave_kernels_fill(WaveKernels &k) {
    constexpr size_t D = sizeof(double);
    constexpr size_t quad_rows = QUAD_WAVES * 4 * QRow::SIZE * D, quad_limit = QUAD_STEP ? TABLE_DOUBLES * D + quad_rows : 0;
    constexpr size_t fact_lds = (TABLE_DOUBLES + ILQG_FACT_WAVES * WAVE_LDS_DOUBLES) * D;
    k.derivs[0] = {k_derivs_wave<FACTORED>, ILQG_DERIVS_BLOCK, 0, ILQG_DERIVS_BLOCK, 0, 0};
    k.derivs[1] = {k_derivs_wave<false>, ILQG_DERIVS_BLOCK, DERIVS_DYN_LDS, ILQG_DERIVS_BLOCK, 0, 0};
    // quad mapping: four trajectories to a wavefront, one workgroup per CU at a time
    k.sweep[0] = {k_backward_quad<FACTORED>, 64 * QUAD_WAVES, TABLE_DOUBLES * D + quad_rows, 4 * QUAD_WAVES, 1, quad_limit};
    k.sweep[1] = {k_backward_quad<false>, 64 * QUAD_WAVES, quad_rows, 4 * QUAD_WAVES, 1, quad_limit};
    k.sweep[2] = {k_backward_quad<FACTORED, true>, 64 * QUAD_WAVES, TABLE_DOUBLES * D + quad_rows, 4 * QUAD_WAVES, 1, quad_limit};
    k.sweep[3] = {k_backward_quad<false, true>, 64 * QUAD_WAVES, quad_rows, 4 * QUAD_WAVES, 1, quad_limit};
    // row mapping: a wavefront per trajectory; the factored kernel's workgroups share the coefficient tables (one per CU at a time)
    k.sweep[4] = {k_backward_wave<FACTORED>, 64 * ILQG_FACT_WAVES, fact_lds, ILQG_FACT_WAVES, 1, FACTORED ? fact_lds : 0};
    k.sweep[5] = {k_backward_wave<false>, 64, WAVE_LDS_DOUBLES * D, 1, 8, 0};
}
static const auto &derivs_kernel(const ilqg_dev_t *d, bool fact) { return d->wave_kernels.derivs[fact ? 0 : 1]; }
static const auto &sweep_kernel(const ilqg_dev_t *d, bool fact, bool quad, bool spec) {
    return d->wave_kernels.sweep[(quad ? (spec ? 2 : 0) : 4) + (fact ? 0 : 1)];
}
#endif

extern "C" {

const char *ilqg_dev_error(void) { return g_err.c_str(); }

int ilqg_dev_count(void) {
    int n = 0;
    if(hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void ilqg_dev_multiplier_dims(int *out) {
    out[0] = ME;
    out[1] = MF;
}

void ilqg_dev_dims(int *out) {
    out[0] = NX;
    out[1] = NU;
    out[2] = FULL ? 1 : 0;
    out[3] = REC_HOST;
    out[4] = REC;
    out[5] = HX ? 1 : 0;
    out[6] = 0;
    out[7] = WAVE_MAP ? 1 : 0;
}

const char *ilqg_dev_kernel_name(int k) {
    static const char *names[ILQG_K_COUNT] = {"k_derivs", "k_backward", "k_rollout[search]", "k_select",
                                              "k_rollout[winner]", "k_update", "k_rollout[cost]", "k_rollout[init]",
                                              "layout kernels", "k_backward[fused derivs]", "k_rollout[stage 2 | winner]",
                                              "k_multipliers", "k_search[stage 1]", "k_search[stage 2]", "k_adopt_home + k_commit", "k_shift",
                                              "k_log_steps", "k_head", "k_shift_param", "k_policy", "k_policy_params", "k_plant", "k_shift_param_rows",
                                              "k_shift_windows", "k_history"};
    // (the slots behind the history's, in ilqg_shim.h's second list)
    static const char *later[ILQG_K_TOTAL - ILQG_K_COUNT] = {"k_best_of", "k_shift_winners", "k_policy_drawn", "k_policy_drawn_params", "k_noise_fill"};
    if(k >= ILQG_K_COUNT && k < ILQG_K_TOTAL) return later[k - ILQG_K_COUNT];
    return (k >= 0 && k < ILQG_K_COUNT) ? names[k] : "?";
}

static int dev_fill(ilqg_dev *d, int device, int batch, int n_hor);
int ilqg_dev_create(ilqg_dev_t **out, int device, int batch, int n_hor) {
    *out = nullptr;
    if(batch < 1 || n_hor < 2) {
        g_err = "ilqg_dev_create: need batch >= 1 and n_hor >= 2";
        return 1;
    }
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if(device < 0 || device >= ndev) {
        g_err = "ilqg_dev_create: no such HIP device";
        return 1;
    }
    HIP_TRY(hipSetDevice(device));
    ilqg_dev *d = new ilqg_dev();  // value-initialised: every handle, view, flag and count is null until dev_fill or a call sets it
    if(dev_fill(d, device, batch, n_hor)) {
        const std::string why = g_err;
        ilqg_dev_destroy(d);  // releases whatever the failed attempt had acquired
        g_err = why;
        return 1;
    }
    *out = d;
    return 0;
}

static int dev_fill(ilqg_dev *d, int device, int batch, int n_hor) {
    d->env = read_env();
    d->device = device;
    d->B = batch;
    d->Bp = (batch + WAVE - 1) / WAVE * WAVE;
    d->N = n_hor;
    d->loc_set = -1;
    d->P.B = d->B;
    d->P.Bp = d->Bp;
    d->P.N = d->N;
    HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&d->ext_in, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d->ext_out, hipEventDisableTiming));
#if ILQG_WAVE_MAP
    wave_kernels_fill(d->wave_kernels);
    const auto prepare = [](auto &k) {
        k.scratch = uses_scratch(k.fn);
        if(k.lds_limit) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds_limit));
        return 0;
    };
    for(auto &k : d->wave_kernels.derivs)
        if(prepare(k)) return 1;
    for(auto &k : d->wave_kernels.sweep)
        if(prepare(k)) return 1;
#endif
#if ILQG_WAVE_MAP && defined(ILQG_ROLLOUT_PARTS)
    if(d->env.roll_lds)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rollout_parts<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)d->env.roll_lds));
    // records through LDS (see k_rollout_parts; ILQG_NO_DMA=1: per-lane loads).  With them a workgroup takes more than
    // half of a CU's LDS whenever a record is 640 bytes or more; below that the same is asked for explicitly
    d->roll_dma = !d->env.no_dma;
    const size_t roll_need = (size_t)WAVE * RNP * sizeof(double);
    d->roll_pad = (d->env.roll_lds > roll_need + 40 * 1024) ? d->env.roll_lds - roll_need - 40 * 1024 : 0;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rollout_parts<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(roll_need + d->roll_pad)));
#endif
    // (the second stream is the wave mapping's chunk pipeline; the lane mapping does not make one: the streams of a process
    // share four hardware queues, and with two streams per context the four groups of a batch sit on two of them in pairs)
    if(WAVE_MAP || d->env.second_stream) HIP_TRY(hipStreamCreateWithFlags(&d->stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&d->fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d->join, hipEventDisableTiming));
    if(WAVE_MAP) {
        static std::vector<hipStream_t> shared_roll(64, nullptr);  // one per device, for the life of the process
        if(!shared_roll[device]) HIP_TRY(hipStreamCreateWithFlags(&shared_roll[device], hipStreamNonBlocking));
        d->roll = shared_roll[device];
        HIP_TRY(hipEventCreateWithFlags(&d->roll_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&d->roll_out, hipEventDisableTiming));
    }
    for(int f = 0; f < ILQG_F_COUNT; f++) {
        if(WAVE_MAP && f == ILQG_F_DER) {
#if ILQG_WAVE_MAP
            // derivative records = device trajEl_t structs for as many trajectories as fit the device's work buffer
            // (allocated by the first context: ILQG_WORK_GB if set, else half of the free device memory, at most what
            // this context needs); a private buffer for stage-by-stage calls is allocated when one is made
            SharedWork &W = g_work[device];
            const size_t per_traj = (size_t)d->N * sizeof(trajEl_t);
            if(!W.buf) {
                const char *e = getenv("ILQG_WORK_GB");
                size_t free_b = 0, total_b = 0;
                HIP_TRY(hipMemGetInfo(&free_b, &total_b));
                // Without ILQG_WORK_GB: what the whole batch needs in the record form ilqg_dev_iterate uses, if the device
                // has it once this context's other arrays (the packed records, the second line-search stage's kept
                // roll-outs, and a margin) are counted; else what is left then, but at least half of what is free.
                const double need = (double)d->B * (double)d->N * (double)(ILQG_DEV_EL ? STORED_STRIDE : FACT_STRIDE);
                const double others = (double)d->Bp * (d->N + 1) * (RN + (ILQG_MAX_ALPHA - 1) * CAND_W) * sizeof(double) + 6e9;
                double budget = (double)free_b - others;
                if(budget < 0.5 * (double)free_b) budget = 0.5 * (double)free_b;
                if(budget > need) budget = need;
                if(e) budget = atof(e) * 1e9;
                size_t bytes = (size_t)budget;
                if(bytes < per_traj) bytes = per_traj;
                if(bytes > (size_t)d->B * per_traj) bytes = (size_t)d->B * per_traj;
                memset(&W, 0, sizeof(W));
                // (+ one record: records may lie closer together than their size, see FACT_STRIDE, and the last one
                // still reaches sizeof(trajEl_t) beyond its start)
                bytes += sizeof(trajEl_t);
                // (what hipMemGetInfo calls free is not always available in one piece: take less rather than fail)
                while(hipMalloc((void **)&W.buf, bytes) != hipSuccess) {
                    (void)hipGetLastError();
                    W.buf = nullptr;
                    if(bytes / 2 < per_traj + sizeof(trajEl_t)) {
                        g_err = "ilqg_dev_create: no device memory for the derivative work buffer";
                        return 1;
                    }
                    bytes = bytes / 2 + sizeof(trajEl_t);
                }
                W.bytes = bytes;
                HIP_TRY(hipMemsetAsync(W.buf, 0, W.bytes, d->stream));
                HIP_TRY(hipStreamSynchronize(d->stream));
                HIP_TRY(hipEventCreateWithFlags(&W.free_ev, hipEventDisableTiming));
            }
            W.refs++;
            d->shared = &W;
            if((W.bytes - sizeof(trajEl_t)) / per_traj < 1) {
                g_err = "ilqg_dev_create: the device's derivative work buffer (made for a shorter horizon) does not hold one trajectory";
                return 1;
            }
#endif
            continue;
        }
        if(nom_column(f) >= 0 && !has_tiled_copy(f) && !has_tiled_scratch(f)) continue;  // columns of the packed records only
        const FieldInfo fi = field_info(f);
        const size_t bytes = (size_t)field_steps(d, f) * fi.wd * d->Bp * sizeof(double);
        if(repoint(d->P.f[f], d->f[f], d->f[f].reserve(bytes))) return 1;
        HIP_TRY(hipMemsetAsync(d->P.f[f], 0, bytes, d->stream));
    }
    {
        const size_t bytes = (size_t)d->Bp * (d->N + 1) * RN * sizeof(double);
        if(repoint(d->P.nom, d->nom, d->nom.reserve(bytes))) return 1;
        HIP_TRY(hipMemsetAsync(d->P.nom, 0, bytes, d->stream));
    }
    for(int f = 0; f < ILQG_I_COUNT; f++) {
        const size_t bytes = (size_t)int_field_width(f) * d->Bp * sizeof(int);
        if(repoint(d->P.i[f], d->i[f], d->i[f].reserve(bytes))) return 1;
        HIP_TRY(hipMemsetAsync(d->P.i[f], 0, bytes, d->stream));
    }
    if(repoint(d->P.derivs_failed, d->derivs_failed, d->derivs_failed.reserve(d->Bp * sizeof(int)))) return 1;
    HIP_TRY(hipMemsetAsync(d->P.derivs_failed, 0, d->Bp * sizeof(int), d->stream));
    if(d->counter.reserve(sizeof(int))) return 1;
    if(d->queues.reserve(2 * QUEUE_CELL * sizeof(int))) return 1;  // one cell per stream of the chunk pipeline
    {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        d->cus = cus > 0 ? cus : 256;
    }
    if(repoint(d->P.pending, d->pending_list, d->pending_list.reserve(d->Bp * sizeof(int)))) return 1;
    if(repoint(d->P.n_pending, d->n_pending, d->n_pending.reserve(sizeof(int)))) return 1;
    HIP_TRY(hipMemsetAsync(d->P.n_pending, 0, sizeof(int), d->stream));
    d->P.n_pending_next = d->P.n_pending;
    HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

void ilqg_dev_destroy(ilqg_dev_t *d) {
    if(!d) return;
    hipSetDevice(d->device);
    if(d->stream) hipStreamSynchronize(d->stream);
    if(d->stream2) hipStreamSynchronize(d->stream2);
    for(auto &s : d->spans) {
        hipEventDestroy(s.a);
        hipEventDestroy(s.b);
    }
    for(hipEvent_t e : d->event_pool) hipEventDestroy(e);
    // Memory goes HERE, in front of the streams, in this one statement — not in the members' destructors, which run at the
    // `delete` below, behind hipStreamDestroy: the order of this function is part of what it does.
    static_cast<DevBuffers &>(*d) = DevBuffers();
#if ILQG_WAVE_MAP
    if(d->shared && --d->shared->refs == 0) {  // the last context on the device: release the shared work buffer
        hipFree(d->shared->buf);
        hipEventDestroy(d->shared->free_ev);
        memset(d->shared, 0, sizeof(SharedWork));
    }
#endif
    if(g_spec_last == d) g_spec_last = nullptr;
    if(d->stream) hipStreamDestroy(d->stream);
    if(d->stream2) hipStreamDestroy(d->stream2);
    if(d->fork) hipEventDestroy(d->fork);
    if(d->join) hipEventDestroy(d->join);
    if(d->roll) hipStreamSynchronize(d->roll);
    if(d->roll_in) hipEventDestroy(d->roll_in);
    if(d->roll_out) hipEventDestroy(d->roll_out);
    if(d->epoch) hipEventDestroy(d->epoch);
    if(d->ext_in) hipEventDestroy(d->ext_in);
    if(d->ext_out) hipEventDestroy(d->ext_out);
    delete d;
}

int ilqg_dev_set_params(ilqg_dev_t *d, int n_params, const int *sizes, const double *const *values) {
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->stream));
    d->param_bufs.clear();
    if(repoint(d->P.p, d->param_table, d->param_table.release())) return 1;
    std::vector<double *> ptrs(n_params > 0 ? n_params : 1, nullptr);
    {
        constexpr int want[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
        constexpr int offs[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_POFFSETS;
        if(n_params != ILQG_NP) {
            g_err = "ilqg_dev_set_params: parameter count differs from the problem this library was built for";
            return 1;
        }
        for(int i = 0; i < n_params; i++) {
            if(sizes[i] != want[i]) {
                g_err = "ilqg_dev_set_params: parameter size differs from the problem's paramdesc[]";
                return 1;
            }
            for(int j = 0; j < sizes[i]; j++) d->pv.v[offs[i] + j] = values[i][j];
        }
        d->per_step_params = false;
        for(int i = 0; i < n_params; i++) d->per_step_params |= (sizes[i] == -1);
    }
    for(int i = 0; i < n_params; i++) {
        const int sz = sizes[i] == -1 ? d->N + 1 : sizes[i];
        Buffer<double> buf;
        if(buf.reserve(sz * sizeof(double))) return 1;
        HIP_TRY(hipMemcpy(buf.get(), values[i], sz * sizeof(double), hipMemcpyHostToDevice));
        ptrs[i] = buf.get();
        d->param_bufs.push_back(std::move(buf));
    }
    if(repoint(d->P.p, d->param_table, d->param_table.reserve(ptrs.size() * sizeof(double *)))) return 1;
    HIP_TRY(hipMemcpy(d->P.p, ptrs.data(), ptrs.size() * sizeof(double *), hipMemcpyHostToDevice));
    d->work_consts = d->half_consts[0] = d->half_consts[1] = false;  // constant record entries depend on the parameters
    return 0;
}

// Per-trajectory problem parameters.  Nothing here touches a trajectory: like ilqg_dev_set_params it only changes what the
// NEXT launch reads.  The copy is enqueued on the context's stream, behind every launch that still reads the old rows.
static const PolicyParamMap *policy_param_map(int n_named, const int *named, const double *values, PolicyParamMap &map);
// the map the rows twins get (with_rows): the table's, or an empty one, with the step rows in use
static void rows_refresh(ilqg_dev_t *d) {
    PolicyParamMap m;
    if(d->pb_on) {
        m = d->pb_map;
    } else {
        for(int j = 0; j < ILQG_PTOTAL; j++) m.src[j] = -1;
        m.W = 0;
    }
    const bool steps = step_rows_into(m, d);
    d->rows_map = m;
    d->rows_on = d->pb_on || steps;
}
// the table's buffer holds `bytes`; one that has to grow is out of use, and no longer described, before it is released
// (launches in flight read the old buffer: reserve drains the context's stream)
static int table_buffer(ilqg_dev_t *d, size_t bytes) {
    if(bytes <= d->pb_values.bytes()) return 0;
    d->pb_on = false;
    rows_refresh(d);
    return d->pb_values.reserve(bytes, d->stream);
}
int ilqg_dev_set_params_batch(ilqg_dev_t *d, int n_named, const int *named, const double *values, int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    if(WAVE_MAP) {
        g_err = "set_params_batch: this library maps one wavefront to a trajectory (wave mapping); its kernels do not carry "
                "parameters per lane, per-trajectory parameters need a lane-mapped library";
        return 1;
    }
    if(n_named < 0) {
        g_err = "set_params_batch: n_names must not be negative";
        return 1;
    }
    if(n_named == 0) {
        d->pb_on = false;  // (the buffer stays: a set that comes back allocates nothing)
        rows_refresh(d);
        return 0;
    }
    PolicyParamMap map;
    if(!policy_param_map(n_named, named, values, map)) return 1;
    const size_t bytes = (size_t)d->B * (size_t)map.W * sizeof(double);
    if(table_buffer(d, bytes)) return 1;
    HIP_TRY(hipMemcpyAsync(d->pb_values.get(), values, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, d->stream));
    if(!on_device) HIP_TRY(hipStreamSynchronize(d->stream));  // the one wait: the caller's array is its own again
    d->pb_map = map;
    d->pb_on = true;
    rows_refresh(d);
    return 0;
}

// Per-time-step parameters per trajectory.  The same contract: only what the NEXT launch reads changes, the copy goes onto
// the context's stream behind every launch that reads the old rows, the buffer of a parameter only grows.
// step_slot: which of the problem's size -1 parameters `index` is, or -1
static int step_slot(int index) {
    constexpr int sizes[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
    if(index < 0 || index >= ILQG_NP || sizes[index] != -1) return -1;
    int s = 0;
    for(int i = 0; i < index; i++) s += sizes[i] == -1 ? 1 : 0;
    return s;
}
// the buffer of slot s holds Bp rows, the rows beyond B zero (no lane reads them; a stray one would read zeros, not beyond)
static int step_rows_buffer(ilqg_dev_t *d, int s) {
    const size_t n = (size_t)d->N + 1, bytes = (size_t)d->Bp * n * sizeof(double);
    if(bytes > d->sr_rows[s].bytes()) {  // (as table_buffer)
        d->sr_on[s] = false;
        rows_refresh(d);
        if(d->sr_rows[s].reserve(bytes, d->stream)) return 1;
    }
    if(!d->sr_on[s] && d->Bp > d->B)
        HIP_TRY(hipMemsetAsync(d->sr_rows[s].get() + (size_t)d->B * n, 0, (size_t)(d->Bp - d->B) * n * sizeof(double), d->stream));
    return 0;
}
int ilqg_dev_set_param_steps_batch(ilqg_dev_t *d, int index, const double *values, int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    if(WAVE_MAP) {
        g_err = "set_param_steps_batch: this library maps one wavefront to a trajectory (wave mapping); its kernels do not carry "
                "parameters per lane, per-trajectory parameters need a lane-mapped library";
        return 1;
    }
    const int s = step_slot(index);
    if(s < 0) {
        g_err = "set_param_steps_batch: not a parameter with one value per time step";
        return 1;
    }
    if(!values) {
        d->sr_on[s] = false;  // (the buffer stays: rows that come back allocate nothing)
        rows_refresh(d);
        return 0;
    }
    if(step_rows_buffer(d, s)) return 1;
    const size_t bytes = (size_t)d->B * ((size_t)d->N + 1) * sizeof(double);
    HIP_TRY(hipMemcpyAsync(d->sr_rows[s].get(), values, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, d->stream));
    if(!on_device) HIP_TRY(hipStreamSynchronize(d->stream));  // the one wait: the caller's array is its own again
    d->sr_on[s] = true;
    rows_refresh(d);
    return 0;
}

int ilqg_dev_get_param_steps_batch(ilqg_dev_t *d, int index, double *rows) {
    HIP_TRY(hipSetDevice(d->device));
    const int s = step_slot(index);
    if(s < 0 || !d->sr_on[s]) {
        g_err = "get_param_steps_batch: the parameter has no rows per trajectory in this context";
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(rows, d->sr_rows[s].get(), (size_t)d->B * ((size_t)d->N + 1) * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

int ilqg_dev_get_params_batch(ilqg_dev_t *d, double *rows) {
    HIP_TRY(hipSetDevice(d->device));
    if(!d->pb_on) {
        g_err = "get_params_batch: the context has no per-trajectory parameters";
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(rows, d->pb_values.get(), (size_t)d->B * (size_t)d->pb_map.W * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

int ilqg_dev_set_opts(ilqg_dev_t *d, const ilqg_dev_opts_t *o) {
#if !ILQG_EXPERIMENTS
    if(o->bw_split) {
        g_err = "option bw_split: the two-wavefront backward pass (a measured negative result) is compiled into the -DILQG_EXPERIMENTS libraries only (lib*_exp.so)";
        return 1;
    }
#endif
    if(o->n_alpha < 1 || o->n_alpha > ILQG_MAX_ALPHA) {
        g_err = "ilqg_dev_set_opts: n_alpha must be in 1..16";
        return 1;
    }
    d->O = *o;
    return 0;
}

int ilqg_dev_field_width(int field) { return field_info(field).wh; }
int ilqg_dev_field_steps(ilqg_dev_t *d, int field) { return field_steps(d, field); }
void *ilqg_dev_field_ptr(ilqg_dev_t *d, int field) { return d->P.f[field]; }
void *ilqg_dev_stream(ilqg_dev_t *d) { return (void *)d->stream; }

// a per-trajectory scalar field (B doubles) into device memory of the caller, on the context's stream
int ilqg_dev_copy_scalar_to(ilqg_dev_t *d, int field, void *dst_device) {
    HIP_TRY(hipSetDevice(d->device));
    if(field < ILQG_F_COST || field >= ILQG_F_ALPHA_COST) {
        g_err = "ilqg_dev_copy_scalar_to: not a per-trajectory scalar field";
        return 1;
    }
    HIP_TRY(hipMemcpyAsync(dst_device, d->P.f[field], (size_t)d->B * sizeof(double), hipMemcpyDeviceToDevice, d->stream));
    return 0;
}

int ilqg_dev_write(ilqg_dev_t *d, int field, const double *host) {
    return ilqg_dev_write_steps(d, field, host, field_steps(d, field));
}

// trajectory-major on the device, i.e. already in host layout: copied without a kernel
static bool is_traj_major(int field) { return WAVE_MAP && field == ILQG_F_FIN; }

static int nom_io(ilqg_dev *d, int field, double *host_rw, const double *host_ro, int steps) {
    const FieldInfo fi = field_info(field);
    const size_t n = (size_t)d->B * steps * fi.wh;
    Staged io(d);
    io.in(host_ro, n * sizeof(double));
    io.out(host_rw, n * sizeof(double));
    if(io.open()) return 1;
    double *const slice = host_ro ? const_cast<double *>(host_ro) : host_rw;  // (one of the two is given)
    {
        Timed t(d, ILQG_K_TRANSPOSE);
        hipLaunchKernelGGL(k_nom_io, grid1(n, 256), dim3(256), 0, d->stream, d->P.nom, slice, d->B, d->N, steps,
                           fi.wh, nom_column(field), host_ro ? 1 : 0);
    }
    HIP_TRY(hipGetLastError());
    return io.close();
}

#if ILQG_WAVE_MAP
// derivative records live in device trajEl_t structs: convert to/from the packed host record
#define REC_FIELDS(OP)                                                                            \
    OP(cx, NX) OP(cxx, SXX) OP(cu, NU) OP(cuu, SUU) OP(cxu, NXU) OP(fx, NX * NX) OP(fu, NXU)     \
    OP(lower, NU) OP(upper, NU) REC_FIELDS_FULL(OP)                                               \
    OP(lower_sign, NU) OP(upper_sign, NU) OP(lower_hx, NXU) OP(upper_hx, NXU)
#if FULL_DDP
#define REC_FIELDS_FULL(OP) OP(fxx, NX * SXX) OP(fuu, NX * SUU) OP(fxu, NX * NXU)
#else
#define REC_FIELDS_FULL(OP)
#endif

// The context's PRIVATE record buffer, for calls that leave records behind or find them there (ilqg_dev_derivs, the
// single sweep of the drop-in back_pass(), reading / writing records): allocated when the first such call is made,
// for the whole batch (these calls exist for tests and for the single-trajectory drop-in path).
static int own_work(ilqg_dev *d) {
    if(d->P.work) return 0;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t per_traj = (size_t)d->N * sizeof(trajEl_t);
    if((double)d->B * (double)per_traj > 0.5 * (double)free_b) {
        g_err = "derivative records of the whole batch do not fit the device (wave mapping): stage-by-stage calls and "
                "record transfers need a smaller batch; ilqg_dev_iterate / ilqg_dev_backward(mode 2) work in chunks";
        return 1;
    }
    if(repoint(d->P.work, d->work, d->work.reserve((size_t)d->B * per_traj))) return 1;
    HIP_TRY(hipMemsetAsync(d->P.work, 0, (size_t)d->B * per_traj, d->stream));
    d->work_consts = false;
    return 0;
}

static int der_io(ilqg_dev *d, double *host_rw, const double *host_ro) {
    if(own_work(d)) return 1;
    const size_t n = (size_t)d->B * d->N;
    std::vector<trajEl_t> tmp(n);
    HIP_TRY(hipMemcpy(tmp.data(), d->P.work, n * sizeof(trajEl_t), hipMemcpyDeviceToHost));
    for(size_t e = 0; e < n; e++) {
        trajEl_t &t = tmp[e];
        if(host_ro) {
            const double *r = host_ro + e * REC_HOST;
#define OP(field, cnt) memcpy(t.field, r, sizeof(double) * (cnt)); r += (cnt);
            REC_FIELDS(OP)
#undef OP
        } else {
            double *r = host_rw + e * REC_HOST;
#define OP(field, cnt) memcpy(r, t.field, sizeof(double) * (cnt)); r += (cnt);
            REC_FIELDS(OP)
#undef OP
        }
    }
    if(host_ro) HIP_TRY(hipMemcpy(d->P.work, tmp.data(), n * sizeof(trajEl_t), hipMemcpyHostToDevice));
    return 0;
}
#endif

static int all_home(ilqg_dev_t *d);

int ilqg_dev_write_steps(ilqg_dev_t *d, int field, const double *host, int steps) {
    HIP_TRY(hipSetDevice(d->device));
    if(has_tiled_copy(field) && all_home(d)) return 1;
    const FieldInfo fi = field_info(field);
    if(steps < 1 || steps > field_steps(d, field)) {
        g_err = "ilqg_dev_write_steps: bad step count";
        return 1;
    }
#if ILQG_WAVE_MAP
    if(field == ILQG_F_DER) {
        if(io_flush(d)) return 1;
        return der_io(d, nullptr, host);
    }
#endif
    if(nom_column(field) >= 0) {
        if(nom_io(d, field, nullptr, host, steps)) return 1;
        if(!has_tiled_copy(field)) return 0;  // else: the tiled copy below as well
    }
    if(is_traj_major(field)) {
        const size_t row = (size_t)steps * fi.wd * sizeof(double);
        const size_t dpitch = (size_t)field_steps(d, field) * fi.wd * sizeof(double);
        const void *src = host;
        if(d->io_deferred) {
            void *dev, *pin;
            if(stage(d, row * d->B, &dev, &pin)) return 1;
            memcpy(pin, host, row * d->B);
            src = pin;
        }
        HIP_TRY(hipMemcpy2DAsync(d->P.f[field], dpitch, src, row, row, d->B, hipMemcpyHostToDevice, d->stream));
        return io_done(d);
    }
    const size_t n = (size_t)d->B * steps * fi.wh;
    void *dev, *pin;
    if(stage(d, n * sizeof(double), &dev, &pin)) return 1;
    if(stage_in(d, dev, pin, host, n * sizeof(double))) return 1;
    {
        Timed t(d, ILQG_K_TRANSPOSE);
        const size_t total = (size_t)d->B * steps * fi.wd;
        hipLaunchKernelGGL(k_to_dev, grid1(total, 256), dim3(256), 0, d->stream, (const double *)dev, d->P.f[field], d->B, d->Bp,
                           steps, fi.wh, fi.wd);
    }
    HIP_TRY(hipGetLastError());
    return io_done(d);
}

int ilqg_dev_read(ilqg_dev_t *d, int field, double *host) {
    HIP_TRY(hipSetDevice(d->device));
    if(has_tiled_copy(field) && all_home(d)) return 1;
    const FieldInfo fi = field_info(field);
    const int steps = field_steps(d, field);
    const size_t n = (size_t)d->B * steps * fi.wh;
#if ILQG_WAVE_MAP
    if(field == ILQG_F_DER) {
        if(io_flush(d)) return 1;
        return der_io(d, host, nullptr);
    }
#endif
    if(nom_column(field) >= 0 && !has_tiled_copy(field)) return nom_io(d, field, host, nullptr, steps);
    if(is_traj_major(field)) {
        void *dev = nullptr, *pin = nullptr;
        if(d->io_deferred && stage(d, n * sizeof(double), &dev, &pin)) return 1;
        return stage_out(d, d->P.f[field], pin, host, n * sizeof(double));
    }
    void *dev, *pin;
    if(stage(d, n * sizeof(double), &dev, &pin)) return 1;
    {
        Timed t(d, ILQG_K_TRANSPOSE);
        hipLaunchKernelGGL(k_from_dev, grid1(n, 256), dim3(256), 0, d->stream, d->P.f[field], (double *)dev, d->B, d->Bp,
                           steps, fi.wh, fi.wd);
    }
    HIP_TRY(hipGetLastError());
    return stage_out(d, dev, pin, host, n * sizeof(double));
}

// int fields are [width][Bp] on the device, [B][width] on the host
int ilqg_dev_write_int(ilqg_dev_t *d, int field, const int *host) {
    HIP_TRY(hipSetDevice(d->device));
    const int w = int_field_width(field);
    const size_t bytes = (size_t)w * d->Bp * sizeof(int);
    std::vector<int> tmp;
    int *src;
    if(d->io_deferred) {
        void *dev, *pin;
        if(stage(d, bytes, &dev, &pin)) return 1;
        src = (int *)pin;
    } else {
        tmp.resize((size_t)w * d->Bp);
        src = tmp.data();
    }
    memset(src, 0, bytes);
    for(int b = 0; b < d->B; b++)
        for(int j = 0; j < w; j++) src[(size_t)j * d->Bp + b] = host[(size_t)b * w + j];
    HIP_TRY(hipMemcpyAsync(d->P.i[field], src, bytes, hipMemcpyHostToDevice, d->stream));
    return io_done(d);
}

int ilqg_dev_read_int(ilqg_dev_t *d, int field, int *host) {
    HIP_TRY(hipSetDevice(d->device));
    const int w = int_field_width(field);
    const size_t bytes = (size_t)w * d->Bp * sizeof(int);
    if(d->io_deferred) {
        void *dev, *pin;
        if(stage(d, bytes, &dev, &pin)) return 1;
        HIP_TRY(hipMemcpyAsync(pin, d->P.i[field], bytes, hipMemcpyDeviceToHost, d->stream));
        d->pending.push_back({host, pin, bytes, w});
        return 0;
    }
    std::vector<int> tmp((size_t)w * d->Bp, 0);
    HIP_TRY(hipMemcpyAsync(tmp.data(), d->P.i[field], tmp.size() * sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    for(int b = 0; b < d->B; b++)
        for(int j = 0; j < w; j++) host[(size_t)b * w + j] = tmp[(size_t)j * d->Bp + b];
    return 0;
}

int ilqg_dev_io_begin(ilqg_dev_t *d) {
    d->io_deferred = true;
    d->io_off = 0;
    return 0;
}

int ilqg_dev_io_end(ilqg_dev_t *d) {
    HIP_TRY(hipSetDevice(d->device));
    d->io_deferred = false;
    return io_flush(d);
}

#define NEED_PARAMS(d)                                                   \
    if(!(d)->P.p) {                                                      \
        g_err = "problem parameters not set (ilqg_dev_set_params)";      \
        return 1;                                                        \
    }

// ls_keep = 2: every current trajectory back into the arrays X / U (the host is about to read or write them, an
// initial roll-out is about to store there, or a search that does not keep its roll-outs follows)
static int all_home(ilqg_dev_t *d) {
#if !ILQG_WAVE_MAP
    if(d->loc_set < 0) return 0;
    hipLaunchKernelGGL(k_all_home, dim3(8 * d->cus), dim3(256), 0, d->stream, d->P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(d->P.i[ILQG_I_LOC], 0, d->Bp * sizeof(int), d->stream));
    d->loc_set = -1;
#endif
    return 0;
}

int ilqg_dev_reset(ilqg_dev_t *d) {
    HIP_TRY(hipSetDevice(d->device));
    hipLaunchKernelGGL(k_reset, grid1(d->Bp, 256), dim3(256), 0, d->stream, d->P, d->O);
    if(HAS_MUL) {  // update_multipliers(o, 1) of the solver entry (iLQG.c:236)
        NEED_PARAMS(d);
        Timed t(d, ILQG_K_MULTIPLIERS);
        LAUNCH_TWIN(d, k_multipliers, dim3(d->Bp / WAVE), dim3(WAVE), 0, d->stream, d->P, d->O, d->pv, 1);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// the stream the roll-out family of a context runs on, and the two hand-overs with the context's own stream
static hipStream_t roll_stream(ilqg_dev_t *d) { return d->roll ? d->roll : d->stream; }
static int roll_enter(ilqg_dev_t *d) {  // what is queued on the context's stream happens before the roll-outs
    if(!d->roll) return 0;
    HIP_TRY(hipEventRecord(d->roll_in, d->stream));
    HIP_TRY(hipStreamWaitEvent(d->roll, d->roll_in, 0));
    return 0;
}
static int roll_leave(ilqg_dev_t *d) {  // ... and the roll-outs before whatever the context's stream gets next
    if(!d->roll) return 0;
    HIP_TRY(hipEventRecord(d->roll_out, d->roll));
    HIP_TRY(hipStreamWaitEvent(d->stream, d->roll_out, 0));
    return 0;
}

// (launch errors are picked up by the caller's hipGetLastError())
static void launch_rollout(ilqg_dev_t *d, int mode, int kernel_id, int a0, int n_alpha, hipStream_t stream = nullptr) {
    if(!stream) stream = d->stream;
    Timed t(d, kernel_id, stream);
    const dim3 grid((d->Bp + ROLL_BLOCK - 1) / ROLL_BLOCK, n_alpha), block(ROLL_BLOCK);
    if(mode == ROLL_INIT)
        with_rows(d, [&](auto... tr) { hipLaunchKernelGGL((k_rollout<RK_INIT, decltype(tr)...>), grid, block, 0, stream, d->P, d->O, d->pv, mode, a0, tr...); });
    else if(mode == ROLL_COST)
        with_rows(d, [&](auto... tr) { hipLaunchKernelGGL((k_rollout<RK_COST, decltype(tr)...>), grid, block, 0, stream, d->P, d->O, d->pv, mode, a0, tr...); });
#if ILQG_WAVE_MAP && defined(ILQG_ROLLOUT_PARTS)
    else if(!HAS_MUL && !d->env.no_rollout_parts) {  // the generated file offers the step in parts: several wavefronts per 64 trajectories
        DevPtrs Q = d->P;
        if(!d->keep_first) Q.cand1 = nullptr;
        // (second stage: a busy workgroup is a chain of N steps that keeps its CU's SIMDs issuing; two of them on one CU
        // take twice as long, and the dispatcher puts two on one CU while others idle.  Asking for more than half of
        // the CU's LDS leaves room for one.)
        if(d->roll_dma) {
            hipLaunchKernelGGL(k_rollout_parts<true>, dim3(d->Bp / WAVE, n_alpha), dim3(WAVE * RW), (size_t)WAVE * RNP * sizeof(double) + d->roll_pad,
                               stream, Q, d->O, d->pv, mode, a0);
        } else {
            const size_t lds = (n_alpha > 1) ? d->env.roll_lds : 0;
            hipLaunchKernelGGL(k_rollout_parts<false>, dim3(d->Bp / WAVE, n_alpha), dim3(WAVE * RW), lds, stream, Q, d->O, d->pv, mode, a0);
        }
    }
#endif
    else
        with_rows(d, [&](auto... tr) { hipLaunchKernelGGL((k_rollout<RK_GENERAL, decltype(tr)...>), grid, block, 0, stream, d->P, d->O, d->pv, mode, a0, tr...); });
}

int ilqg_dev_rollout_init(ilqg_dev_t *d) {
    NEED_PARAMS(d);
    HIP_TRY(hipSetDevice(d->device));
    if(all_home(d)) return 1;  // (the controls the roll-out starts from are read where they currently are)
    if(roll_enter(d)) return 1;
    HIP_TRY(hipMemsetAsync(d->P.i[ILQG_I_STATUS], 0, d->Bp * sizeof(int), roll_stream(d)));
    launch_rollout(d, ROLL_INIT, ILQG_K_ROLLOUT_INIT, 0, 1, roll_stream(d));
    HIP_TRY(hipGetLastError());
    return roll_leave(d);
}

}  // extern "C"
// (shift_plans is a template and cannot have C linkage: it stands between two extern blocks, as each_future / windows_move do)
// Receding horizon: the plan moves `steps` time steps towards the start where it is (k_shift.inc).  One pass over U in the
// lane mapping — the controls are read wherever the source's trajectory lives and land in the array U, so the location
// indices are cleared behind it and the all_home() of the initial roll-out that follows has nothing left to copy — and one
// over the records' u in the wave mapping.  What ilqg_dev_shift and ilqg_dev_shift_winners share: `steps` in range (who:
// the entry's name in front of the text; the winners entry asks before it plans its transfers), and ONE launch of this
// mapping's kernel (wave_grid: its workgroups in the wave mapping) under `slot` with the clear behind it.
static int shift_steps_ok(ilqg_dev_t *d, const char *who, int steps) {
    if(steps >= 0 && steps < d->N) return 1;
    g_err = std::string(who) + ": steps must be in 0 .. n_hor - 1";
    return 0;
}
template <class Kernel, class... Args>
static int shift_plans(ilqg_dev_t *d, int slot, Kernel kernel, int wave_grid, Args... args) {
    {
        Timed t(d, slot);
        const size_t grid = WAVE_MAP ? (size_t)wave_grid : (size_t)(NX > NU ? NX : NU) * d->Bp / WAVE;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(SHIFT_THREADS), 0, d->stream, d->P, args...);
    }
    HIP_TRY(hipGetLastError());
    if constexpr(!WAVE_MAP) {
        if(d->loc_set >= 0) HIP_TRY(hipMemsetAsync(d->P.i[ILQG_I_LOC], 0, d->Bp * sizeof(int), d->stream));
        d->loc_set = -1;
    }
    return 0;
}
extern "C" {
int ilqg_dev_shift(ilqg_dev_t *d, int steps, int use_plan_x0) {
    HIP_TRY(hipSetDevice(d->device));
    if(!shift_steps_ok(d, "ilqg_dev_shift", steps)) return 1;
    return shift_plans(d, ILQG_K_SHIFT, k_shift, d->B, steps, use_plan_x0);
}

int ilqg_dev_put_u_tail(ilqg_dev_t *d, const double *tail, int steps, int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    if(steps < 1 || steps > d->N) {
        g_err = "ilqg_dev_put_u_tail: bad step count";
        return 1;
    }
    if(all_home(d)) return 1;
    const size_t n = (size_t)d->B * steps * NU;
    Staged io(d, on_device);
    io.in(tail, n * sizeof(double));
    if(io.open()) return 1;
    {
        Timed t(d, ILQG_K_TRANSPOSE);
        hipLaunchKernelGGL(k_put_u_steps, grid1(n, 256), dim3(256), 0, d->stream, d->P, tail, d->N - steps, steps);
    }
    HIP_TRY(hipGetLastError());
    return io.close();
}

// ---------------------------------------------------------------------------------------------------------------------
// Candidates per agent (k_best.inc): the context's trajectories as segments of K consecutive slots
// ---------------------------------------------------------------------------------------------------------------------
// what the kernels rely on: K a power of two up to the wavefront, whole segments in the context (whose tiles are 64 wide)
static int segments_ok(ilqg_dev_t *d, int K, int first) {
    if(K < 1 || K > WAVE || (K & (K - 1)) != 0) {
        g_err = "K must be one of 1, 2, 4, 8, 16, 32, 64";
        return 0;
    }
    if(d->B % K != 0 || first < 0 || first % K != 0) {
        g_err = "K must divide the group's size and its first trajectory";
        return 0;
    }
    return 1;
}

// The one launch of k_best_of, on device memory.  Reads costs / the caller's scores and the status; writes nothing of the context.
static int launch_best_of(ilqg_dev_t *d, int K, int first, const double *score, int *winner, double *best, int *n_eligible) {
    {
        Timed t(d, ILQG_K_BEST_OF);
        hipLaunchKernelGGL(k_best_of, dim3(d->Bp / WAVE), dim3(WAVE), 0, d->stream, d->P, K, first, score, winner, best, n_eligible);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int ilqg_dev_best_of(ilqg_dev_t *d, int K, int first, const double *score, int *winner, double *best, int *n_eligible, int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    if(!segments_ok(d, K, first)) return 1;
    if(!winner) {
        g_err = "best_of: winner is NULL";
        return 1;
    }
    const size_t G = (size_t)(d->B / K);
    Staged io(d, on_device);
    io.in(score, d->B * sizeof(double));
    io.out(winner, G * sizeof(int));
    io.out(best, G * sizeof(double));
    io.out(n_eligible, G * sizeof(int));
    if(io.open() || launch_best_of(d, K, first, score, winner, best, n_eligible)) return 1;
    return io.close();
}

// ilqg_dev_shift with the winner's plan as every slot's source: the same check, launch and clear (shift_plans)
int ilqg_dev_shift_winners(ilqg_dev_t *d, int K, int first, const int *winner, int steps, const double *x0_new, const double *u_tail, const double *du,
                           int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    if(!segments_ok(d, K, first) || !shift_steps_ok(d, "ilqg_dev_shift_winners", steps)) return 1;
    if(!winner) {
        g_err = "ilqg_dev_shift_winners: winner is NULL";
        return 1;
    }
    if(steps == 0) u_tail = nullptr;  // (no tail step to fill)
    const size_t G = (size_t)(d->B / K);
    Staged io(d, on_device);
    io.in(winner, G * sizeof(int));
    io.in(x0_new, G * NX * sizeof(double));
    io.in(u_tail, G * steps * NU * sizeof(double));
    io.in(du, (size_t)d->B * d->N * NU * sizeof(double));
    if(io.open() || shift_plans(d, ILQG_K_SHIFT_WINNERS, k_shift_winners, d->B / K, K, first, winner, steps, x0_new, u_tail, du)) return 1;
    return io.close();
}

// ---------------------------------------------------------------------------------------------------------------------
// The control interval of a caller with its own plant (k_mpc_io.inc)
// ---------------------------------------------------------------------------------------------------------------------
static int launch_head(ilqg_dev_t *d, int steps, double *x, double *u, double *l, double *L, double *cost) {
    const int tiles = (x ? (steps * NX + 7) / 8 : 0) + ((u ? 1 : 0) + (l ? 1 : 0)) * ((steps * NU + 7) / 8) + (L ? (steps * NXU + 7) / 8 : 0);
    const int gy = tiles > 0 ? (tiles + HEAD_WAVES - 1) / HEAD_WAVES : 1;
    {
        Timed t(d, ILQG_K_HEAD);
        hipLaunchKernelGGL(k_head, dim3((unsigned)((d->B + 7) / 8), (unsigned)gy), dim3(WAVE * HEAD_WAVES), 0, d->stream, d->P, steps, x, u, l, L, cost);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
static int head_steps_ok(ilqg_dev_t *d, int steps) {
    if(steps >= 1 && steps <= d->N) return 1;
    g_err = "head: steps must be in 1 .. n_hor";
    return 0;
}

int ilqg_dev_head(ilqg_dev_t *d, int steps, double *x, double *u, double *l, double *L, double *cost, int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    if(!head_steps_ok(d, steps)) return 1;
    if(!x && !u && !l && !L && !cost) return 0;
    const size_t n = (size_t)d->B * steps * sizeof(double);
    Staged io(d, on_device);
    io.out(x, n * NX);
    io.out(u, n * NU);
    io.out(l, n * NU);
    io.out(L, n * NXU);
    io.out(cost, d->B * sizeof(double));
    if(io.open() || launch_head(d, steps, x, u, l, L, cost)) return 1;
    return io.close();
}

// ---------------------------------------------------------------------------------------------------------------------
// Roll-outs of the policy from the caller's starts (k_policy.inc).  On the stream of the roll-out family: in the wave
// mapping the kernel keeps a trajEl_t per lane in scratch memory like every scalar roll-out (see `roll`).
// ---------------------------------------------------------------------------------------------------------------------
static int policy_args_ok(ilqg_dev_t *d, int R, const double *x0) {
    if(R < 1) {
        g_err = "policy_rollout: n_starts must be at least 1";
        return 0;
    }
    if(!x0) {
        g_err = "policy_rollout: x0 is NULL";
        return 0;
    }
    if(((size_t)d->B * (size_t)R + ROLL_BLOCK - 1) / ROLL_BLOCK > (size_t)0x7fffffff) {
        g_err = "policy_rollout: n_starts is too large for one launch";
        return 0;
    }
    return 1;
}
// the map of the ParamValues slots for the named parameters (k_policy.inc), or nullptr with g_err set
static const PolicyParamMap *policy_param_map(int n_named, const int *named, const double *values, PolicyParamMap &map) {
    constexpr int sizes[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
    constexpr int offs[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_POFFSETS;
    if(n_named < 1 || !named) {
        g_err = "policy_rollout_params: n_names must be at least 1 and names not NULL";
        return nullptr;
    }
    if(!values) {
        g_err = "policy_rollout_params: values is NULL";
        return nullptr;
    }
    for(int j = 0; j < ILQG_PTOTAL; j++) map.src[j] = -1;
    map.W = 0;
    for(int n = 0; n < n_named; n++) {
        const int i = named[n];
        if(i < 0 || i >= ILQG_NP || sizes[i] < 1) {
            g_err = "policy_rollout_params: names must be fixed-size parameters of the problem (per-time-step parameters stay shared)";
            return nullptr;
        }
        if(map.src[offs[i]] >= 0) {
            g_err = "policy_rollout_params: a parameter is named twice";
            return nullptr;
        }
        for(int j = 0; j < sizes[i]; j++) map.src[offs[i] + j] = (short)(map.W + j);
        map.W += sizes[i];
    }
    return &map;
}
// map == nullptr: k_policy<false>; else the same under the rows of `values` (device memory), k_policy<true>.  Each has its
// own timing slot.
// spec == nullptr: no noise or the table `dist`; else the noise drawn from *spec (device memory; dist is not read), under the
// timing slots of the drawn form: k_policy_drawn where the library has that kernel, k_policy's third noise argument where it
// has one kernel (ILQG_POLICY_ONE_KERNEL, k_policy.inc).
static int launch_policy(ilqg_dev_t *d, int R, const double *x0, const PolicyParamMap *map, const double *values, int shared, const double *dist,
                         int dist_shared, const NoiseSpec *spec, double alpha, int feedback, double *cost, int *ok, double *x_end, double *x, double *u) {
    if(roll_enter(d)) return 1;
    const dim3 grid = grid1((size_t)d->B * (size_t)R, ROLL_BLOCK);
    {   // (with a per-trajectory table — lane mapping only — the trajectory's row goes first, the roll-out's behind it)
        Timed t(d, spec ? (map ? ILQG_K_POLICY_DRAWN_PARAMS : ILQG_K_POLICY_DRAWN) : (map ? ILQG_K_POLICY_PARAMS : ILQG_K_POLICY), roll_stream(d));
        with_rows(d, [&](auto... tr) {
            with_own_rows(map != nullptr, [&](auto... own) {
#if ILQG_POLICY_ONE_KERNEL
                hipLaunchKernelGGL((k_policy<sizeof...(own) != 0, decltype(tr)..., decltype(own)...>), grid, dim3(ROLL_BLOCK), 0, roll_stream(d), d->P, d->O,
                                   d->pv, R, x0, alpha, feedback ? 1 : 0, cost, ok, x_end, x, u, spec ? nullptr : dist, dist_shared ? 1 : 0, spec, tr...,
                                   own...);
#else
                if(spec)
                    hipLaunchKernelGGL((k_policy_drawn<sizeof...(own) != 0, decltype(tr)..., decltype(own)...>), grid, dim3(ROLL_BLOCK), 0,
                                       roll_stream(d), d->P, d->O, d->pv, R, x0, alpha, feedback ? 1 : 0, cost, ok, x_end, x, u, spec, tr..., own...);
                else
                    hipLaunchKernelGGL((k_policy<sizeof...(own) != 0, decltype(tr)..., decltype(own)...>), grid, dim3(ROLL_BLOCK), 0, roll_stream(d), d->P,
                                       d->O, d->pv, R, x0, alpha, feedback ? 1 : 0, cost, ok, x_end, x, u, dist, dist_shared ? 1 : 0, tr..., own...);
#endif
            }, values, shared ? 1 : 0, map ? *map : PolicyParamMap{});
        });
    }
    HIP_TRY(hipGetLastError());
    return roll_leave(d);
}

// n_named == 0 = no table (k_policy<false>), else roll-out (b, r) under its row of `values`; dist == nullptr = no disturbance,
// else roll-out (b, r) under its rows of `dist` (dist_shared: row r for every trajectory).  The host form stages the starts,
// then with a map the table of values, then the disturbance table if there is one, then the outputs.
int ilqg_dev_policy_rollout(ilqg_dev_t *d, int R, const double *x0, int n_named, const int *named, const double *values, int shared,
                            const double *dist, int dist_shared, double alpha, int feedback, double *cost, int *ok, double *x_end, double *x, double *u,
                            int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    NEED_PARAMS(d);
    PolicyParamMap table;
    const PolicyParamMap *map = nullptr;
    if(!policy_args_ok(d, R, x0) || (n_named != 0 && !(map = policy_param_map(n_named, named, values, table)))) return 1;
    if(!cost && !ok && !x_end && !x && !u) return 0;
    const size_t n = (size_t)d->B * (size_t)R;
    Staged io(d, on_device);
    io.in(x0, n * NX * sizeof(double));
    io.in(values, map ? (shared ? (size_t)R : n) * (size_t)map->W * sizeof(double) : 0);
    io.in(dist, (dist_shared ? (size_t)R : n) * (size_t)d->N * NX * sizeof(double));
    io.out(cost, n * sizeof(double));
    io.out(ok, n * sizeof(int));
    io.out(x_end, n * NX * sizeof(double));
    io.out(x, n * (size_t)(d->N + 1) * NX * sizeof(double));
    io.out(u, n * (size_t)d->N * NU * sizeof(double));
    if(io.open() || launch_policy(d, R, x0, map, values, shared, dist, dist_shared, nullptr, alpha, feedback, cost, ok, x_end, x, u)) return 1;
    return io.close();
}

// ---------------------------------------------------------------------------------------------------------------------
// Process noise drawn on the device (k_noise.inc).  The caller's seed, sigma (HOST memory in every form), shared flag and
// first trajectory travel as ONE NoiseSpec in the context's own device buffer, copied in the order of the context's stream:
// a launch that follows on that stream (or, between roll_enter and roll_leave, on the roll-out family's) reads this call's
// block, and the next call's copy waits for it.  sigma and first_trajectory arrive checked (ilqg_host.c drawn_refused: sigma
// N_X finite doubles >= 0, 0 <= first_trajectory, first_trajectory + batch <= 2^32).
// ---------------------------------------------------------------------------------------------------------------------
static int noise_spec_put(ilqg_dev_t *d, const char *who, unsigned long long seed, const double *sigma, int noise_shared, long long first_trajectory) {
    NoiseSpec s;
    s.key0 = (unsigned)(seed & 0xffffffffull);
    s.key1 = (unsigned)(seed >> 32);
    s.first = (unsigned)first_trajectory;
    s.shared = noise_shared ? 1 : 0;
    for(int i = 0; i < NX; i++) s.sigma[i] = sigma[i];
    if(d->noise_spec.reserve(sizeof(NoiseSpec))) return 1;
    // (pageable memory of this frame: the runtime has taken its copy when the call returns)
    HIP_TRY(hipMemcpyAsync(d->noise_spec.get(), &s, sizeof(NoiseSpec), hipMemcpyHostToDevice, d->stream));
    return 0;
}
int ilqg_dev_policy_rollout_drawn(ilqg_dev_t *d, int R, const double *x0, int n_named, const int *named, const double *values, int shared,
                                  unsigned long long seed, const double *sigma, int noise_shared, long long first_trajectory, double alpha, int feedback,
                                  double *cost, int *ok, double *x_end, double *x, double *u, int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    NEED_PARAMS(d);
    PolicyParamMap table;
    const PolicyParamMap *map = nullptr;
    if(!policy_args_ok(d, R, x0) || (n_named != 0 && !(map = policy_param_map(n_named, named, values, table)))) return 1;
    if(!cost && !ok && !x_end && !x && !u) return 0;
    const size_t n = (size_t)d->B * (size_t)R;
    if(noise_spec_put(d, "policy_rollout_drawn", seed, sigma, noise_shared, first_trajectory)) return 1;
    Staged io(d, on_device);
    io.in(x0, n * NX * sizeof(double));
    io.in(values, map ? (shared ? (size_t)R : n) * (size_t)map->W * sizeof(double) : 0);
    io.out(cost, n * sizeof(double));
    io.out(ok, n * sizeof(int));
    io.out(x_end, n * NX * sizeof(double));
    io.out(x, n * (size_t)(d->N + 1) * NX * sizeof(double));
    io.out(u, n * (size_t)d->N * NU * sizeof(double));
    if(io.open() || launch_policy(d, R, x0, map, values, shared, nullptr, 0, d->noise_spec.get(), alpha, feedback, cost, ok, x_end, x, u)) return 1;
    return io.close();
}

int ilqg_dev_noise_table(ilqg_dev_t *d, int R, unsigned long long seed, const double *sigma, int noise_shared, long long first_trajectory, double *w,
                         int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    if(R < 1) {
        g_err = "noise_table: n_starts must be at least 1";
        return 1;
    }
    if(!w) {
        g_err = "noise_table: w is NULL (the table, [batch][n_starts][n_hor][N_X] or shared [n_starts][n_hor][N_X])";
        return 1;
    }
    const size_t rows = (noise_shared ? (size_t)1 : (size_t)d->B) * (size_t)R * (size_t)d->N;
    if((rows + 255) / 256 > (size_t)0x7fffffff) {
        g_err = "noise_table: n_starts is too large for one launch";
        return 1;
    }
    if(noise_spec_put(d, "noise_table", seed, sigma, noise_shared, first_trajectory)) return 1;
    Staged io(d, on_device);
    io.out(w, rows * NX * sizeof(double));
    if(io.open()) return 1;
    {
        Timed t(d, ILQG_K_NOISE_FILL);
        hipLaunchKernelGGL(k_noise_fill, grid1(rows, 256), dim3(256), 0, d->stream, (const NoiseSpec *)d->noise_spec.get(), rows, R, d->N, w);
    }
    HIP_TRY(hipGetLastError());
    return io.close();
}

int ilqg_dev_put_x0_device(ilqg_dev_t *d, const double *x0) {
    HIP_TRY(hipSetDevice(d->device));
    if(all_home(d)) return 1;  // (behind ilqg_dev_shift nothing is left to move)
    const size_t n = (size_t)d->B * NX;
    {
        Timed t(d, ILQG_K_TRANSPOSE);
        hipLaunchKernelGGL(k_nom_io, grid1(n, 256), dim3(256), 0, d->stream, d->P.nom, const_cast<double *>(x0), d->B, d->N, 1, NX, NOM_X, 1);
        if(!WAVE_MAP) hipLaunchKernelGGL(k_to_dev, grid1(n, 256), dim3(256), 0, d->stream, x0, d->P.f[ILQG_F_X], d->B, d->Bp, 1, NX, NX);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int ilqg_dev_stream_in(ilqg_dev_t *d, void *stream) {
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipEventRecord(d->ext_in, (hipStream_t)stream));
    HIP_TRY(hipStreamWaitEvent(d->stream, d->ext_in, 0));
    return 0;
}
int ilqg_dev_stream_out(ilqg_dev_t *d, void *stream) {
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipEventRecord(d->ext_out, d->stream));
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, d->ext_out, 0));
    return 0;
}

int ilqg_dev_check_device_ptr(ilqg_dev_t *d, const void *ptr, const char *what) {
    HIP_TRY(hipSetDevice(d->device));
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    const hipError_t e = hipPointerGetAttributes(&a, ptr);
    if(e != hipSuccess) (void)hipGetLastError();  // (memory the runtime does not know: plain host memory)
    if(e != hipSuccess || a.type != hipMemoryTypeDevice || a.device != d->device) {
        g_err = std::string(what) + " must point to device memory on the context's device";
        return 1;
    }
    return 0;
}

int ilqg_dev_shift_param(ilqg_dev_t *d, int index, int steps, const double *tail) {
    HIP_TRY(hipSetDevice(d->device));
    NEED_PARAMS(d);
    constexpr int want[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
    if(index < 0 || index >= ILQG_NP || index >= (int)d->param_bufs.size() || want[index] != -1) {
        g_err = "ilqg_dev_shift_param: not a parameter with one value per time step";
        return 1;
    }
    if(steps < 0 || steps > d->N) {
        g_err = "ilqg_dev_shift_param: steps must be in 0 .. n_hor";
        return 1;
    }
    if(steps == 0) return 0;
    Staged io(d);
    io.in(tail, (size_t)steps * sizeof(double));
    if(io.open()) return 1;
    {
        Timed t(d, ILQG_K_SHIFT_PARAM);
        hipLaunchKernelGGL(k_shift_param_rows, dim3(1), dim3(PARAM_BLOCK), 0, d->stream, d->param_bufs[index].get(), d->N + 1, steps, tail);  // (one row)
    }
    HIP_TRY(hipGetLastError());
    d->work_consts = d->half_consts[0] = d->half_consts[1] = false;  // constant record entries depend on the parameters
    return io.close();
}

// the same per row of a per-trajectory window: k_shift_param_rows, one workgroup per trajectory
int ilqg_dev_shift_param_batch(ilqg_dev_t *d, int index, int steps, const double *tail, int on_device) {
    HIP_TRY(hipSetDevice(d->device));
    const int s = step_slot(index);
    if(s < 0 || !d->sr_on[s]) {
        g_err = "ilqg_dev_shift_param_batch: the parameter has no rows per trajectory in this context";
        return 1;
    }
    if(steps < 0 || steps > d->N) {
        g_err = "ilqg_dev_shift_param_batch: steps must be in 0 .. n_hor";
        return 1;
    }
    if(steps == 0) return 0;
    Staged io(d, on_device);
    io.in(tail, (size_t)d->B * (size_t)steps * sizeof(double));
    if(io.open()) return 1;
    {
        Timed t(d, ILQG_K_SHIFT_PARAM_ROWS);
        hipLaunchKernelGGL(k_shift_param_rows, dim3(d->B), dim3(PARAM_BLOCK), 0, d->stream, d->sr_rows[s].get(), d->N + 1, steps, tail);
    }
    HIP_TRY(hipGetLastError());
    return io.close();
}

// ---------------------------------------------------------------------------------------------------------------------
// The resident receding-horizon loop (ilqg_shim.h ilqg_dev_loop_t): what it is lives in d->loop, written by begin alone; the
// per-round steps and read ask it.  k_plant runs where k_policy runs: on the stream of the roll-out family, between the two
// hand-overs with the context's stream, so behind the iteration that made the plan and in front of the k_shift_* that moves
// it.  k_shift_windows runs on the context's stream: behind the log or the plant step of the round (both hand back to it) and
// in front of ilqg_dev_shift and the initial roll-out that reads the moved windows.
// ---------------------------------------------------------------------------------------------------------------------
static int slot_index(int s) {  // the paramdesc[] index of the s-th size -1 parameter
    constexpr int sizes[ILQG_NP > 0 ? ILQG_NP : 1] = ILQG_PSIZES;
    for(int i = 0; i < ILQG_NP; i++)
        if(sizes[i] == -1 && s-- == 0) return i;
    return -1;
}
}  // extern "C"
// (templates on the slot count: the discarded branch, and with it the kernel, is not instantiated where there is no slot)
// each(s, f, bytes) for every slot s the caller gave a future f of the open loop's shape
template <int n_slots, class Each>
static int each_future(ilqg_dev_t *d, const double *const *future, Each &&each) {
    if constexpr(n_slots > 0) {
        const size_t per = (size_t)d->loop.rounds * (size_t)d->loop.steps;
        for(int s = 0; s < n_slots; s++) {
            const double *f = future ? future[slot_index(s)] : nullptr;
            if(f && each(s, f, (d->sr_on[s] ? (size_t)d->B : (size_t)1) * per * sizeof(double))) return 1;
        }
    }
    return 0;
}
template <int n_slots>
static int windows_move(ilqg_dev_t *d, int round) {
    if constexpr(n_slots > 0) {
        NEED_PARAMS(d);
        WindowSet<n_slots> S;
        int most = 1;
        for(int s = 0; s < n_slots; s++) {
            const bool rows = d->sr_on[s];
            S.w[s].base = rows ? d->sr_rows[s].get() : d->param_bufs[slot_index(s)].get();
            S.w[s].rows = rows ? d->B : 1;
            S.w[s].future = d->loop.given[s] ? d->win_future[s].get() : nullptr;
            S.w[s].stride = rows ? (size_t)d->loop.rounds * (size_t)d->loop.steps : 0;
            if(S.w[s].rows > most) most = S.w[s].rows;
        }
        {
            Timed t(d, ILQG_K_SHIFT_WINDOWS);
            hipLaunchKernelGGL(k_shift_windows<n_slots>, dim3(most, n_slots), dim3(PARAM_BLOCK), 0, d->stream, S, d->N + 1, d->loop.steps,
                               round * d->loop.steps);
        }
        HIP_TRY(hipGetLastError());
        d->work_consts = d->half_consts[0] = d->half_consts[1] = false;  // constant record entries depend on the parameters
    }
    return 0;
}
// no loop, no log and no plant: as before the first begin
static int loop_close(ilqg_dev_t *d) {
    d->loop.rounds = 0;
    return d->log_x.release() | d->log_u.release() | d->log_c.release() | plant_release(d);
}
static int loop_round_ok(const ilqg_dev_t *d, int round, const char *who) {
    if(round >= 0 && round < d->loop.rounds) return 1;
    g_err = std::string(who) + ": no such round of an open loop (ilqg_dev_loop_begin)";
    return 0;
}
extern "C" {
int ilqg_dev_loop_begin(ilqg_dev_t *d, const ilqg_dev_loop_t *loop) {
    HIP_TRY(hipSetDevice(d->device));
    const ilqg_dev_loop_t &L = *loop;
    const bool windows = L.windows && N_STEP_PARAMS > 0, named = L.plant && L.n_named > 0;
    if(L.rounds < 1 || L.steps < 1 || L.steps >= d->N) {
        g_err = "ilqg_dev_loop_begin: need rounds >= 1 and 1 <= steps < n_hor";
        return 1;
    }
    if(L.plant || windows) NEED_PARAMS(d);
    PolicyParamMap map;
    if(L.plant && L.n_named < 0) {
        g_err = "ilqg_dev_loop_begin: n_names must not be negative";
        return 1;
    }
    if(named && !policy_param_map(L.n_named, L.named, L.values, map)) return 1;
    // nothing in flight reads what is made anew or grows below
    HIP_TRY(hipStreamSynchronize(d->stream));
    if(L.plant && d->roll) HIP_TRY(hipStreamSynchronize(d->roll));
    d->loop.rounds = L.rounds, d->loop.steps = L.steps, d->loop.plant = L.plant != 0, d->loop.windows = L.windows != 0;
    for(bool &given : d->loop.given) given = false;
    const size_t B = (size_t)d->B, rounds = (size_t)L.rounds, per = B * rounds * (size_t)L.steps;
    // the logs and the plants anew, the futures grow-only; all or none
    if(d->log_x.renew(per * NX * sizeof(double)) || d->log_u.renew(per * NU * sizeof(double)) || d->log_c.renew(B * rounds * sizeof(double)) ||
       (L.plant && (plant_release(d) || d->plant_xp.renew(B * NX * sizeof(double)) || d->plant_failed.renew(B * sizeof(int)) ||
                    d->plant_cost.renew(B * rounds * sizeof(double)) || (named && d->plant_values.renew(B * (size_t)map.W * sizeof(double))) ||
                    (L.disturbance && d->plant_dist.renew(per * NX * sizeof(double))))) ||
       (windows && each_future<N_STEP_PARAMS>(d, L.future, [&](int s, const double *, size_t bytes) {
            d->loop.given[s] = true;
            return d->win_future[s].reserve(bytes);
        }))) {
        (void)loop_close(d);
        return 1;
    }
    bool sent = L.plant != 0;
    if(L.plant) {
        HIP_TRY(hipMemsetAsync(d->plant_failed.get(), 0, B * sizeof(int), d->stream));
        // (what a failed plant leaves unwritten reaches the host as zeros)
        HIP_TRY(hipMemsetAsync(d->log_x.get(), 0, per * NX * sizeof(double), d->stream));
        HIP_TRY(hipMemsetAsync(d->log_u.get(), 0, per * NU * sizeof(double), d->stream));
        HIP_TRY(hipMemsetAsync(d->plant_cost.get(), 0, B * rounds * sizeof(double), d->stream));
        if(named) {
            d->loop.map = map;
            d->loop.named = true;
            HIP_TRY(hipMemcpyAsync(d->plant_values.get(), L.values, B * (size_t)map.W * sizeof(double), hipMemcpyHostToDevice, d->stream));
        }
        if(L.disturbance) HIP_TRY(hipMemcpyAsync(d->plant_dist.get(), L.disturbance, per * NX * sizeof(double), hipMemcpyHostToDevice, d->stream));
        if(L.x_plant) HIP_TRY(hipMemcpyAsync(d->plant_xp.get(), L.x_plant, B * NX * sizeof(double), hipMemcpyHostToDevice, d->stream));
        else if(launch_head(d, 1, d->plant_xp.get(), nullptr, nullptr, nullptr, nullptr)) return 1;  // x_0 of every plan, where it lives
    }
    if(windows && each_future<N_STEP_PARAMS>(d, L.future, [&](int s, const double *f, size_t bytes) {
           HIP_TRY(hipMemcpyAsync(d->win_future[s].get(), f, bytes, hipMemcpyHostToDevice, d->stream));
           sent = true;
           return 0;
       }))
        return 1;
    if(sent) HIP_TRY(hipStreamSynchronize(d->stream));  // the one wait: the caller's arrays are its own again
    return 0;
}

int ilqg_dev_loop_apply(ilqg_dev_t *d, int round, int feedback) {
    HIP_TRY(hipSetDevice(d->device));
    if(!loop_round_ok(d, round, "ilqg_dev_loop_apply")) return 1;
    const int steps = d->loop.steps, rounds = d->loop.rounds;
    if(!d->loop.plant) {
        {
            Timed t(d, ILQG_K_LOG);
            hipLaunchKernelGGL(k_log_steps, grid1((size_t)d->B * steps * (NX + NU), 256), dim3(256), 0, d->stream, d->P, d->log_x.get(), d->log_u.get(),
                               d->log_c.get(), round, rounds, steps);
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }
    NEED_PARAMS(d);
    if(roll_enter(d)) return 1;
    {
        Timed t(d, ILQG_K_PLANT, roll_stream(d));
        // (with a per-trajectory table the trajectory's row — the model's — goes first, the plant's behind it)
        with_rows(d, [&](auto... tr) {
            with_own_rows(d->loop.named, [&](auto... own) {
                hipLaunchKernelGGL((k_plant<sizeof...(own) != 0, decltype(tr)..., decltype(own)...>), grid1((size_t)d->B, ROLL_BLOCK), dim3(ROLL_BLOCK), 0,
                                   roll_stream(d), d->P, d->O, d->pv, steps, feedback ? 1 : 0, d->plant_xp.get(), d->plant_failed.get(),
                                   (const double *)d->plant_dist.get(), round * steps, rounds * steps, round, rounds, d->log_x.get(), d->log_u.get(),
                                   d->plant_cost.get(), d->log_c.get(), tr..., own...);
            }, (const double *)d->plant_values.get(), d->loop.map);
        });
    }
    HIP_TRY(hipGetLastError());
    return roll_leave(d);
}

int ilqg_dev_loop_shift(ilqg_dev_t *d, int round) {
    HIP_TRY(hipSetDevice(d->device));
    if(!loop_round_ok(d, round, "ilqg_dev_loop_shift")) return 1;
    if(d->loop.windows && windows_move<N_STEP_PARAMS>(d, round)) return 1;
    if(ilqg_dev_shift(d, d->loop.steps, !d->loop.plant)) return 1;
    return d->loop.plant ? ilqg_dev_put_x0_device(d, d->plant_xp.get()) : 0;
}

int ilqg_dev_loop_read(ilqg_dev_t *d, double *x_plant, double *x, double *u, double *cost_applied, double *plan_cost, int *ok) {
    HIP_TRY(hipSetDevice(d->device));
    if(d->loop.rounds < 1 || ((x_plant || cost_applied || ok) && !d->loop.plant)) {
        g_err = "ilqg_dev_loop_read: no loop, or none with plants (ilqg_dev_loop_begin)";
        return 1;
    }
    const size_t B = (size_t)d->B, rounds = (size_t)d->loop.rounds, per = B * rounds * (size_t)d->loop.steps;
    if(x_plant) HIP_TRY(hipMemcpyAsync(x_plant, d->plant_xp.get(), B * NX * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if(cost_applied) HIP_TRY(hipMemcpyAsync(cost_applied, d->plant_cost.get(), B * rounds * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if(ok) HIP_TRY(hipMemcpyAsync(ok, d->plant_failed.get(), B * sizeof(int), hipMemcpyDeviceToHost, d->stream));
    if(x) HIP_TRY(hipMemcpyAsync(x, d->log_x.get(), per * NX * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if(u) HIP_TRY(hipMemcpyAsync(u, d->log_u.get(), per * NU * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if(plan_cost) HIP_TRY(hipMemcpyAsync(plan_cost, d->log_c.get(), B * rounds * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    if(ok)
        for(size_t b = 0; b < B; b++) ok[b] = ok[b] ? 0 : 1;  // the device keeps failure flags
    return 0;
}

#if ILQG_WAVE_MAP
// wave mapping: derivative records are evaluated chunk by chunk into the work buffer and consumed by
// the backward kernel of the same chunk (wave_backward: work_plan, then launch_derivs and launch_sweep piece by piece).

// the most backward sweeps one call of the retry loop can make under these options (iLQG.c:261-283): sweep 0 at the lambda the
// trajectory has, sweep j at the lambda j increases later (lambda_up, the step k_backward_quad's attempts take), while
// lambda <= lambdaMax.  The longest schedule starts from lambda = 0 with the smallest dlambda (every increase then
// multiplies by lambdaFactor only once more than the one before).
static int spec_sweeps_at_most(const ilqg_dev_opts_t &O) {
    double lam = 0.0, dlam = 0.0;
    int sweeps = 1;
    while(sweeps <= 4096) {
        lambda_up(O.lambdaFactor, O.lambdaMin, &lam, &dlam);
        if(lam > O.lambdaMax || !(lam == lam)) break;
        sweeps++;
    }
    return sweeps;
}

// Where the records of a derivatives / backward call go and how the batch is divided (work_plan)
struct WorkPlan {
    SharedWork *shared;          // transient records (made and consumed in this call): the device's buffer; null: the context's private one
    bool fact, quad;             // factored records; the quad mapping sweeps them
    char *work;
    size_t stride;               // bytes between two records
    int chunk;                   // trajectories whose records the buffer holds
    bool split;                  // the pieces alternate between the two halves of the buffer, on two streams
    int half_cap, part, pieces;  // trajectories a half holds, trajectories of a piece, pieces
    bool *whole, *half;          // which constant entries (init_running) the buffer already holds: all of it, each half
};

static int work_plan(ilqg_dev_t *d, int do_derivs, int do_backward, WorkPlan &w) {
    // Records produced and consumed in one go use the device's shared work buffer, chunk by chunk; records that are
    // left behind or found (ilqg_dev_derivs, the drop-in back_pass()) the context's private one, whole batch.
    w.shared = do_derivs && do_backward ? d->shared : nullptr;
    // factored records (FACTORED builds, option fuse_derivs): only in the transient case — records the caller reads or
    // writes are always the complete ones
    w.fact = FACTORED && d->O.fuse_derivs && w.shared;
    w.stride = w.fact ? FACT_STRIDE : (w.shared ? STORED_STRIDE : sizeof(trajEl_t));
    if(w.shared) {
        w.work = reinterpret_cast<char *>(w.shared->buf);
        // (the last record reaches sizeof(trajEl_t) beyond its start whatever the distance between records)
        const size_t fit = (w.shared->bytes - sizeof(trajEl_t)) / ((size_t)d->N * w.stride);
        w.chunk = (int)(fit > (size_t)d->B ? (size_t)d->B : fit);
        if(w.chunk < 1) {
            g_err = "the device's derivative work buffer does not hold one trajectory of this horizon";
            return 1;
        }
    } else {
        if(own_work(d)) return 1;
        w.work = reinterpret_cast<char *>(d->P.work);
        w.chunk = d->B;  // (own_work holds the whole batch)
    }
    // A batch that needs several chunks alternates between the two halves of the work buffer on two streams, so that
    // the derivatives of one chunk are evaluated while the other's backward pass runs and the end of one backward
    // kernel (few wavefronts still busy) is filled by the next.  The pieces are of equal size.
    // (a batch that fits as a whole goes in two pieces as well, if it is large enough to fill the chip twice)
    // (Quad mapping: a batch whose records fit goes as ONE piece.  Its rows are workers that take trajectories from a queue,
    // four to a wavefront: the more trajectories a queue holds per worker, the less the workers' last ones — 1 to 4 sweeps
    // each — stick out at the end; measured, config 5: 197.8 ms per iteration in two pieces, 181.6 in one.
    // ILQG_TWO_PIECES=1 restores the halves.)
    // quad mapping (16 lanes per trajectory) where it applies; ILQG_NO_QUAD=1: the row mapping (comparison)
    w.quad = QUAD_STEP && d->O.regType == 1 && (w.fact || !FULL || d->env.quad_stored) && !d->env.no_quad;
    w.split = w.shared && w.chunk >= 2 && (d->B > w.chunk || (d->B >= 16 * d->cus && (!w.quad || d->env.two_pieces)));
    w.half_cap = w.split ? w.chunk / 2 : w.chunk;
    w.pieces = (d->B + w.half_cap - 1) / w.half_cap;
    w.part = w.chunk;
    if(w.split) {
        w.part = ((d->B + w.pieces - 1) / w.pieces + 7) / 8 * 8;  // whole workgroups of the factored backward kernel
        if(w.part > w.half_cap) w.part = w.half_cap;
    }
    w.whole = &d->work_consts, w.half = d->half_consts;
    if(w.shared) {  // the shared buffer's constants are another context's, or of another division: none count
        SharedWork *W = w.shared;
        const bool same = W->pv_set && W->N == d->N && W->B == d->B && W->part == w.part && W->half_cap == w.half_cap &&
                          W->factored == w.fact && !d->per_step_params && memcmp(&W->pv, &d->pv, sizeof(ParamValues)) == 0;
        if(!same) {
            W->whole = W->half[0] = W->half[1] = false;
            W->pv = d->pv, W->pv_set = !d->per_step_params;
            W->N = d->N, W->B = d->B, W->part = w.part, W->half_cap = w.half_cap, W->factored = w.fact;
        }
        w.whole = &W->whole, w.half = W->half;
    }
    return 0;
}

// the derivative records of one piece (trajectories c0 .. c0 + cnt - 1 into half h of the buffer, P.work)
static int launch_derivs(ilqg_dev_t *d, const WorkPlan &w, const DevPtrs &P, hipStream_t st, int h, int c0, int cnt) {
    const auto &k = derivs_kernel(d, w.fact);
    const bool have_consts = *w.whole || (w.split && w.half[h]);
    // (transient records are read by the backward pass alone: the limits' signs and gradients, which it does not
    // use unless the limits depend on the state, are left out of them)
    const int limit_gradients = (w.shared && !HX) ? 0 : 1;
#if ILQG_HAVE_DERIV_PARTS
    // records of the steps assembled on chip, whole lines out (k_derivs_parts) once the buffer holds the constant
    // entries; the final records from the derivative kernel.  MEASURED SLOWER than the generated code on a struct per lane
    // (51 against 44 ms per iteration of config 5, see the kernel): off unless ILQG_DERIV_PARTS=1
    if(w.fact && have_consts && d->env.deriv_parts) {
        if(on_scratch_stream(d, true, st, [&](hipStream_t q) {
               Timed t(d, ILQG_K_DERIVS, q);
               hipLaunchKernelGGL(k_derivs_parts, grid1((size_t)cnt * d->N, 64 * DP_WAVES), dim3(64 * DP_WAVES), 0, q, P, d->O, d->pv, c0, cnt);
               hipLaunchKernelGGL(k.fn, k.grid((size_t)cnt, d->cus), dim3(k.block), k.lds, q, P, d->O, d->pv, c0, cnt, 0, 0, 1);
           }))
            return 1;
    } else
#endif
    if(on_scratch_stream(d, k.scratch, st, [&](hipStream_t q) {
           Timed t(d, ILQG_K_DERIVS, q);
           hipLaunchKernelGGL(k.fn, k.grid((size_t)cnt * (d->N + 1), d->cus), dim3(k.block), k.lds, q, P, d->O, d->pv, c0, cnt, have_consts ? 0 : 1,
                              limit_gradients, 0);
       }))
        return 1;
    if(cnt == w.part) {  // every element of this (half of the) buffer that is ever used has its constants now
        if(w.split) w.half[h] = true;
        else *w.whole = w.half[0] = w.half[1] = true;
    }
    return 0;
}

// Speculative retries (k_backward_quad<FACT, true>): rows whose queue is used up run other trajectories' next attempts.
// The rows of a sweep over cnt trajectories, with the buffers of their protocol reserved; 0 = the device cannot spare them (the
// rows' gains buffers are 1.1 MB per row at N = 1 000) and the caller sweeps without; -1 = error
static int spec_rows(ilqg_dev_t *d, int cnt, hipStream_t st) {
    const int rows = (int)sweep_kernel(d, false, true, true).grid((size_t)cnt, d->cus).x * 4 * QUAD_WAVES;
    const int ri = d->spec_ints.try_reserve(((size_t)(3 + SPEC_ATTEMPTS) * d->B + rows) * sizeof(unsigned), st);
    const int rd = ri ? ri : d->spec_doubles.try_reserve((size_t)rows * (SPEC_SLOTS + (size_t)d->N * SPEC_GW) * sizeof(double), st);
    return rd == 0 ? rows : (rd == 2 ? 0 : -1);
}
// P.spec_* into those buffers, and the protocol's words cleared on the stream of the launch
static void spec_point(ilqg_dev_t *d, DevPtrs &P, int rows, hipStream_t q) {
    unsigned *w = d->spec_ints.get();
    const size_t nb = (size_t)d->B;
    P.spec_word = w;
    P.spec_done = w + nb;
    P.spec_out = w + 2 * nb;
    P.spec_best = w + (2 + SPEC_ATTEMPTS) * nb;
    P.spec_row_b = reinterpret_cast<int *>(w + (3 + SPEC_ATTEMPTS) * nb);
    P.spec_res = d->spec_doubles.get();
    P.spec_gains = d->spec_doubles.get() + (size_t)rows * SPEC_SLOTS;
    P.spec_rows = rows;
    g_spec_last = d;
    (void)hipMemsetAsync(w, 0, (2 + SPEC_ATTEMPTS) * nb * sizeof(unsigned), q);
    (void)hipMemsetAsync(P.spec_best, 0xff, (nb + (size_t)rows) * sizeof(unsigned), q);
}

// the backward sweep of one piece
static int launch_sweep(ilqg_dev_t *d, const WorkPlan &w, DevPtrs &P, hipStream_t st, int single_sweep, int c0, int cnt) {
    HIP_TRY(hipMemsetAsync(P.queue, 0, sizeof(int), st));
    // speculative retries: one piece, the retry loop on the device (ILQG_QUAD_SPEC=0: off)
    // (round 6: in the layout of two wavefronts per SIMD as well, -DILQG_QUAD_LEAN=63: 255 registers, 2 spilled)
    bool spec = w.quad && d->env.quad_spec && !single_sweep && !w.split && c0 == 0 && cnt == d->B;
    // the kernel numbers a trajectory's sweeps 0 .. SPEC_ATTEMPTS - 1: options whose lambda schedule (iLQG.c:271-274,
    // user-settable lambdaFactor / lambdaMin / lambdaMax) allows more sweeps than that take the sequential loop
    if(spec && spec_sweeps_at_most(d->O) > SPEC_ATTEMPTS) spec = false;
    const int rows = spec ? spec_rows(d, cnt, st) : 0;
    if(rows < 0) return 1;
    // (the product builds' backward kernels have no scratch; the -ffp-contract=off twins of the tests spill)
    const auto &k = sweep_kernel(d, w.fact, w.quad, rows > 0);
    return on_scratch_stream(d, k.scratch, st, [&](hipStream_t q) {
        Timed t(d, ILQG_K_BACKWARD, q);
        if(rows) spec_point(d, P, rows, q);
        hipLaunchKernelGGL(k.fn, k.grid((size_t)cnt, d->cus), dim3(k.block), k.lds, q, P, d->O, single_sweep, c0, cnt);
    });
}

// The pieces of a call, each on the stream of its half of the buffer.  do_derivs = 0 uses the records already in the buffer.
static int wave_backward(ilqg_dev_t *d, int single_sweep, int do_derivs, int do_backward) {
    WorkPlan w;
    if(work_plan(d, do_derivs, do_backward, w)) return 1;
    if(w.shared) HIP_TRY(hipStreamWaitEvent(d->stream, w.shared->free_ev, 0));  // the previous owner's pass has finished
    if(w.split) {
        HIP_TRY(hipEventRecord(d->fork, d->stream));
        HIP_TRY(hipStreamWaitEvent(d->stream2, d->fork, 0));
    }
    int piece = 0;
    for(int c0 = 0; c0 < d->B; c0 += w.part, piece++) {
        const int cnt = (d->B - c0 < w.part) ? d->B - c0 : w.part;
        const int h = w.split ? (piece & 1) : 0;
        hipStream_t st = h ? d->stream2 : d->stream;
        DevPtrs P = d->P;
        P.work = reinterpret_cast<trajEl_t *>(w.work + (size_t)h * w.half_cap * d->N * w.stride);
        P.work_stride = w.stride;
        P.queue = d->queues.get() + h * QUEUE_CELL;
        if(do_derivs && launch_derivs(d, w, P, st, h, c0, cnt)) return 1;
        if(do_backward && launch_sweep(d, w, P, st, single_sweep, c0, cnt)) return 1;
    }
    if(do_derivs) {  // every slot a batch of this size and division uses has been visited
        if(w.split) w.half[0] = w.half[1] = true;
        else *w.whole = w.half[0] = w.half[1] = true;
    }
    if(w.split) {
        HIP_TRY(hipEventRecord(d->join, d->stream2));
        HIP_TRY(hipStreamWaitEvent(d->stream, d->join, 0));
    }
    if(w.shared) HIP_TRY(hipEventRecord(w.shared->free_ev, d->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}
#endif

int ilqg_dev_derivs(ilqg_dev_t *d) {
    NEED_PARAMS(d);
    HIP_TRY(hipSetDevice(d->device));
#if ILQG_WAVE_MAP
    return wave_backward(d, 0, 1, 0);
#else
    {
        Timed t(d, ILQG_K_DERIVS);
        const size_t total = (size_t)d->Bp * (d->N + 1);
        LAUNCH_TWIN(d, k_derivs, grid1(total, 256), dim3(256), 0, d->stream, d->P, d->O, d->pv);
    }
    HIP_TRY(hipGetLastError());
    return 0;
#endif
}

int ilqg_dev_backward(ilqg_dev_t *d, int mode) {
    HIP_TRY(hipSetDevice(d->device));
    if(mode < 0 || mode > 2) {
        g_err = "ilqg_dev_backward: mode must be 0, 1 or 2";
        return 1;
    }
    if(mode == 2) NEED_PARAMS(d);

#if ILQG_WAVE_MAP
    return wave_backward(d, mode == 1, mode == 2, 1);
#else
    {
        Timed t(d, mode == 2 ? ILQG_K_BACKWARD_FUSED : ILQG_K_BACKWARD);
        const dim3 grid(d->Bp / WAVE), block(WAVE);
        if(mode == 0)
            with_rows(d, [&](auto... tr) { hipLaunchKernelGGL((k_backward<0, decltype(tr)...>), grid, block, 0, d->stream, d->P, d->O, d->pv, tr...); });
        else if(mode == 1)
            with_rows(d, [&](auto... tr) { hipLaunchKernelGGL((k_backward<1, decltype(tr)...>), grid, block, 0, d->stream, d->P, d->O, d->pv, tr...); });
#if ILQG_HAVE_SPLIT
        else if(d->O.bw_split && !HAS_MUL && !d->rows_on)  // (k_backward_split knows the shared parameters only)
            hipLaunchKernelGGL(k_backward_split, grid, dim3(2 * WAVE), 0, d->stream, d->P, d->O, d->pv);
#endif
        else
            with_rows(d, [&](auto... tr) { hipLaunchKernelGGL((k_backward<2, decltype(tr)...>), grid, block, 0, d->stream, d->P, d->O, d->pv, tr...); });
    }
    if(mode != 2) {
        Timed t(d, ILQG_K_TRANSPOSE);
        hipLaunchKernelGGL(k_pack_records, dim3(d->Bp / WAVE, (d->N + 1 + PACK_WAVES - 1) / PACK_WAVES),
                           dim3(WAVE * PACK_WAVES), 0, d->stream, d->P);
    }
    HIP_TRY(hipGetLastError());
    return 0;
#endif
}

// What the three searches below share: the selection among step sizes [a0, a1) (second: of the second stage) ...
static void launch_select(ilqg_dev_t *d, hipStream_t rs, int a0, int a1, int second) {
    Timed t(d, ILQG_K_SELECT, rs);
    hipLaunchKernelGGL(k_select, grid1(d->Bp, 256), dim3(256), 0, rs, d->P, d->O, a0, a1, second);
}
// ... and the buffer of the roll-outs a stage of n_alpha step sizes keeps (P.cand, P.cand1)
static int reserve_kept(ilqg_dev_t *d, double *&view, Buffer<double> &owner, int n_alpha, hipStream_t rs) {
    return repoint(view, owner, owner.reserve((size_t)d->Bp * n_alpha * (d->N + 1) * CAND_W * sizeof(double), rs));
}

#if !ILQG_WAVE_MAP
}  // extern "C"
// a stage of the search that keeps planes: step sizes [a0, a0 + n), T trajectories to a wavefront
template <int STAGE>
static void launch_search_stage(ilqg_dev_t *d, hipStream_t rs, int a0, int n, int set) {
    Timed t(d, STAGE ? ILQG_K_SEARCH2 : ILQG_K_SEARCH, rs);
    const int T = WAVE / n;
    const dim3 grid((d->B + T - 1) / T), block(WAVE);
    if(T * (RN / 2) <= WAVE * DMA_LOADS && !d->env.no_dma)  // the nominal records through LDS
        with_rows(d, [&](auto... tr) { hipLaunchKernelGGL((k_search<STAGE, true, decltype(tr)...>), grid, block, 2 * T * RN * sizeof(double), rs, d->P, d->O, d->pv, a0, n, set, tr...); });
    else
        with_rows(d, [&](auto... tr) { hipLaunchKernelGGL((k_search<STAGE, false, decltype(tr)...>), grid, block, 0, rs, d->P, d->O, d->pv, a0, n, set, tr...); });
}
extern "C" {

// Lane mapping, ls_keep = 2: every roll-out of the search is kept and the accepted one becomes the current trajectory by a
// change of its location index (k_search, k_adopt_home, k_commit; see cur_x).  2 = the device does not have the planes.
static int search_kept_planes(ilqg_dev_t *d, int A, int s1) {
    hipStream_t rs = roll_stream(d);
    const size_t xplane = (size_t)(d->N + 1) * NX * d->Bp, uplane = (size_t)d->N * NU * d->Bp;
    // Two sets of s1 planes of the size of X resp. U (12.6 GB for the benchmark: 2 x 4 planes of 65 536 x 501 x 6
    // doubles).  The planes are laid out s1 to a set: a first stage of another size re-homes the trajectories first.
    // A device that cannot provide them (a larger batch, several contexts sharing it) searches without keeping
    // every roll-out instead of failing: the ls_keep = 1 form needs none of this memory.
    if(d->P.plane_n != s1) {
        if(all_home(d)) return 1;
        d->P.plane_n = s1;
    }
    const int rx = repoint(d->P.xpl, d->xpl, d->xpl.try_reserve(2 * (size_t)s1 * xplane * sizeof(double), rs));
    const int ru = rx ? rx : repoint(d->P.upl, d->upl, d->upl.try_reserve(2 * (size_t)s1 * uplane * sizeof(double), rs));
    if(rx == 1 || ru == 1) return 1;
    if(rx == 2 || ru == 2) {
        if(repoint(d->P.xpl, d->xpl, d->xpl.release())) return 1;
        d->loc_set = -1;  // nothing lives in a plane any more — there are none
        HIP_TRY(hipMemsetAsync(d->P.i[ILQG_I_LOC], 0, d->Bp * sizeof(int), d->stream));
        return 2;
    }
    const int n2 = A - s1, set = (d->loc_set == 0) ? 1 : 0;
    d->P.xplane = xplane;
    d->P.uplane = uplane;
    if(n2 > 0 && reserve_kept(d, d->P.cand, d->cand, n2, rs)) return 1;
    if(!d->pending_zero) HIP_TRY(hipMemsetAsync(d->P.n_pending, 0, sizeof(int), rs));
    d->pending_zero = false;
    launch_search_stage<0>(d, rs, 0, s1, set);
    if(n2 > 0) {  // the grid covers the worst case; wavefronts beyond the pending count return at once
        launch_search_stage<1>(d, rs, s1, n2, set);
        Timed t(d, ILQG_K_ADOPT, rs);
        hipLaunchKernelGGL(k_adopt_home, dim3(8 * d->cus), dim3(256), 0, rs, d->P, s1);
    } else {
        Timed t(d, ILQG_K_ADOPT, rs);
        hipLaunchKernelGGL(k_rejected_home, dim3(8 * d->cus), dim3(256), 0, rs, d->P);
    }
    if(d->defer_commit) {  // inside ilqg_dev_iterate: the update kernel of this iteration commits
        d->commit_pending = true;
        d->commit_s1 = s1;
        d->commit_set = set;
    } else {
        Timed t(d, ILQG_K_ADOPT, rs);
        hipLaunchKernelGGL(k_commit, grid1(d->Bp, 256), dim3(256), 0, rs, d->P, s1, set);
    }
    d->loc_set = set;
    d->winner_done = true;
    HIP_TRY(hipGetLastError());
    return 0;
}
#endif

#if ILQG_WAVE_MAP && defined(ILQG_ROLLOUT_PARTS)
// Wave mapping with the roll-outs in parts: BOTH stages keep what they roll out and the accepted roll-outs are
// copied into the records — no winner pass (16 384 chains of N steps beside the second stage's: the second
// launch needed two rounds of workgroups, 50 ms; the second stage alone fits one).
static int search_rollout_parts(ilqg_dev_t *d, int A, int s1) {
    hipStream_t rs = roll_stream(d);
    const int n2 = A - s1;
    if(reserve_kept(d, d->P.cand1, d->cand1, s1, rs)) return 1;
    if(n2 > 0 && reserve_kept(d, d->P.cand, d->cand, n2, rs)) return 1;
    d->keep_first = true;
    launch_rollout(d, ROLL_SEARCH, ILQG_K_ROLLOUT_SEARCH, 0, s1, rs);
    d->keep_first = false;
    launch_select(d, rs, 0, s1, 0);
    if(n2 > 0) {
        launch_rollout(d, ROLL_LIST_KEEP, ILQG_K_ROLLOUT_SEARCH2, s1, n2, rs);
        launch_select(d, rs, s1, A, 1);
        Timed t(d, ILQG_K_ROLLOUT_WINNER, rs);
        hipLaunchKernelGGL(k_adopt, dim3(8 * d->cus), dim3(256), 0, rs, d->P, s1, n2);
    }
    {
        Timed t(d, ILQG_K_ROLLOUT_WINNER, rs);
        hipLaunchKernelGGL(k_adopt_first, dim3(16 * d->cus), dim3(256), 0, rs, d->P, s1);
    }
    d->winner_done = true;
    return 0;
}
#endif

// The plain search: the roll-out kernel per stage; accepted trajectories are stored in place, by the second stage's launch
// where there is one, else by ilqg_dev_winner
static int search_plain(ilqg_dev_t *d, int A, int s1) {
    hipStream_t rs = roll_stream(d);
    launch_rollout(d, ROLL_SEARCH, ILQG_K_ROLLOUT_SEARCH, 0, s1, rs);
    launch_select(d, rs, 0, s1, 0);
    d->winner_done = false;
    if(s1 < A && !d->O.ls_keep) {
        // the grid covers the worst case; blocks beyond the pending count return at once
        launch_rollout(d, ROLL_SEARCH_LIST, ILQG_K_ROLLOUT_SEARCH2, s1, A - s1, rs);
        launch_select(d, rs, s1, A, 1);
    } else if(s1 < A) {
        // Second stage and the winner pass of the trajectories the first stage settled in ONE launch (ROLL_SECOND);
        // the grid covers the worst case, blocks beyond the pending count return at once.
        const int n2 = A - s1;
        if(reserve_kept(d, d->P.cand, d->cand, n2, rs)) return 1;
        launch_rollout(d, ROLL_SECOND, ILQG_K_ROLLOUT_SEARCH2, s1, n2 + 1, rs);
        launch_select(d, rs, s1, A, 1);
        Timed t(d, ILQG_K_ROLLOUT_WINNER, rs);
        hipLaunchKernelGGL(k_adopt, dim3(8 * d->cus), dim3(256), 0, rs, d->P, s1, n2);
        d->winner_done = true;
    }
    return 0;
}

// Line search (line_search.c:33-78) in up to two stages, see k_select / k_rollout:
//   stage 1: step sizes [0, s1) for every trajectory; selection
//   stage 2: step sizes [s1, n_alpha) for the trajectories still without an acceptable one; selection
int ilqg_dev_search(ilqg_dev_t *d) {
    NEED_PARAMS(d);
    HIP_TRY(hipSetDevice(d->device));
    const int A = d->O.n_alpha;
    const int s1 = (d->O.ls_split > 0 && d->O.ls_split < A) ? d->O.ls_split : A;
#if !ILQG_WAVE_MAP
    if(d->O.ls_keep >= 2 && s1 <= PLANE_A && WAVE / s1 >= 1 && (A == s1 || WAVE / (A - s1) >= 1)) {
        const int rc = search_kept_planes(d, A, s1);
        if(rc != 2) return rc;
    }
    if(all_home(d)) return 1;  // the searches below store accepted trajectories in place: in X / U
#endif
    if(roll_enter(d)) return 1;
    HIP_TRY(hipMemsetAsync(d->P.n_pending, 0, sizeof(int), roll_stream(d)));
    d->pending_zero = false;
    bool parts = false;
#if ILQG_WAVE_MAP && defined(ILQG_ROLLOUT_PARTS)
    parts = d->O.ls_keep >= 2 && !HAS_MUL && !d->env.no_rollout_parts;
    if(parts && search_rollout_parts(d, A, s1)) return 1;
#endif
    if(!parts && search_plain(d, A, s1)) return 1;
    HIP_TRY(hipGetLastError());
    return roll_leave(d);
}

// the two launches of the iteration history, defined at the end of this file (see k_history in k_common.inc for why there)
static void launch_history(ilqg_dev_t *d, hipStream_t stream);
static void launch_move_history(ilqg_dev_t *dst, ilqg_dev_t *src, const int *to, const int *from, int count);
static void launch_harvest(ilqg_dev_t *d, const HarvestPlan &plan, const int *from);

int ilqg_dev_winner(ilqg_dev_t *d) {
    NEED_PARAMS(d);
    HIP_TRY(hipSetDevice(d->device));
    if(d->winner_done) {  // the two-stage search has stored the accepted trajectories already (ROLL_SECOND, k_adopt)
        d->winner_done = false;
        return 0;
    }
    if(roll_enter(d)) return 1;
    launch_rollout(d, ROLL_WINNER, ILQG_K_ROLLOUT_WINNER, 0, 1, roll_stream(d));
    HIP_TRY(hipGetLastError());
    return roll_leave(d);
}

int ilqg_dev_update(ilqg_dev_t *d) {
    NEED_PARAMS(d);
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t rs = roll_stream(d);
    if(roll_enter(d)) return 1;
    if(d->hist.cap > 0) {  // the record of the search that has just run, before the update moves what it holds
        Timed t(d, ILQG_K_HISTORY, rs);
        launch_history(d, rs);
    }
    {
        Timed t(d, ILQG_K_UPDATE, rs);
        const int reset = (!WAVE_MAP && d->defer_commit) ? 1 : 0;
        hipLaunchKernelGGL(k_update, grid1(d->Bp, 256), dim3(256), 0, rs, d->P, d->O, d->commit_pending ? d->commit_s1 : -1, d->commit_set, reset);
        d->commit_pending = false;
        d->pending_zero = reset != 0;
    }
    if(HAS_MUL) {
        Timed t(d, ILQG_K_MULTIPLIERS, rs);
        LAUNCH_TWIN(d, k_multipliers, dim3(d->Bp / WAVE), dim3(WAVE), 0, rs, d->P, d->O, d->pv, 0);
    }
    if(d->O.resweep || HAS_MUL) launch_rollout(d, ROLL_COST, ILQG_K_ROLLOUT_COST, 0, 1, rs);
    HIP_TRY(hipGetLastError());
    return roll_leave(d);
}

int ilqg_dev_iterate(ilqg_dev_t *d, int n) {
    struct Defer {  // search and update of one iteration are launched together: the update commits for the search
        ilqg_dev_t *d;
        explicit Defer(ilqg_dev_t *d_) : d(d_) { d->defer_commit = true; }
        ~Defer() { d->defer_commit = false; }
    } defer(d);
    for(int it = 0; it < n; it++) {
        if(d->O.fuse_derivs || WAVE_MAP) {  // wave mapping: derivatives + sweep chunk by chunk
            if(ilqg_dev_backward(d, 2)) return 1;
        } else {
            if(ilqg_dev_derivs(d)) return 1;
            if(ilqg_dev_backward(d, 0)) return 1;
        }
        if(ilqg_dev_search(d)) return 1;
        if(ilqg_dev_winner(d)) return 1;
        if(ilqg_dev_update(d)) return 1;
    }
    return 0;
}

// Full solves retire finished trajectories (ilqg_host.c): the solver state of trajectories from[0..count) of `src` becomes
// that of trajectories to[0..count) of `dst` (both contexts on one device; k_move_traj).  Both streams are drained around the
// copy — it happens a handful of times per solve, between iterations.
int ilqg_dev_move(ilqg_dev_t *dst, ilqg_dev_t *src, int count, const int *to, const int *from, int with_records) {
    if(count < 1) return 0;
    if(dst->device != src->device || dst->N != src->N) {
        g_err = "ilqg_dev_move: the two contexts differ in device or horizon";
        return 1;
    }
    HIP_TRY(hipSetDevice(dst->device));
    for(int j = 0; j < count; j++)
        if(to[j] < 0 || to[j] >= dst->B || from[j] < 0 || from[j] >= src->B) {
            g_err = "ilqg_dev_move: trajectory index out of range";
            return 1;
        }
    HIP_TRY(hipStreamSynchronize(src->stream));
    if(io_flush(dst)) return 1;
    if(dst->staging.reserve(2 * (size_t)count * sizeof(int))) return 1;
    int *idx = reinterpret_cast<int *>(dst->staging.get());
    HIP_TRY(hipMemcpyAsync(idx, to, (size_t)count * sizeof(int), hipMemcpyHostToDevice, dst->stream));
    HIP_TRY(hipMemcpyAsync(idx + count, from, (size_t)count * sizeof(int), hipMemcpyHostToDevice, dst->stream));
    hipLaunchKernelGGL(k_move_traj, grid1((size_t)count * (src->N + 1), 256), dim3(256), 0, dst->stream, dst->P, src->P, idx, idx + count, count,
                       (with_records && !WAVE_MAP) ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if(src->pb_on) {  // the trajectories' parameter rows travel with them; a destination without a table gets the source's map
        const size_t W = (size_t)src->pb_map.W, bytes = (size_t)dst->B * W * sizeof(double);
        bool same = dst->pb_on && dst->pb_map.W == src->pb_map.W;
        for(int j = 0; same && j < ILQG_PTOTAL; j++) same = dst->pb_map.src[j] == src->pb_map.src[j];
        if(!same) {
            if(table_buffer(dst, bytes)) return 1;
            HIP_TRY(hipMemsetAsync(dst->pb_values.get(), 0, bytes, dst->stream));  // (rows nothing has moved into yet)
            dst->pb_map = src->pb_map;
            dst->pb_on = true;
        }
        rows_refresh(dst);
        hipLaunchKernelGGL(k_move_rows, grid1((size_t)count * W, 256), dim3(256), 0, dst->stream, dst->pb_values.get(), (const double *)src->pb_values.get(), idx,
                           idx + count, count, (int)W);
        HIP_TRY(hipGetLastError());
    }
    for(int s = 0; s < N_STEP_PARAMS; s++) {  // ... and their rows of the per-time-step parameters, W = n_hor + 1
        if(!src->sr_on[s]) continue;
        const size_t W = (size_t)src->N + 1;
        if(!dst->sr_on[s]) {  // (rows nothing has moved into yet are zero)
            if(step_rows_buffer(dst, s)) return 1;
            HIP_TRY(hipMemsetAsync(dst->sr_rows[s].get(), 0, (size_t)dst->B * W * sizeof(double), dst->stream));
            dst->sr_on[s] = true;
            rows_refresh(dst);
        }
        hipLaunchKernelGGL(k_move_rows, grid1((size_t)count * W, 256), dim3(256), 0, dst->stream, dst->sr_rows[s].get(), (const double *)src->sr_rows[s].get(), idx,
                           idx + count, count, (int)W);
        HIP_TRY(hipGetLastError());
    }
    if(src->hist.cap > 0) {  // ... and their histories; a destination without one gets one of the source's capacity
        if(dst->hist.cap == 0 && ilqg_dev_set_history(dst, src->hist.cap)) return 1;
        launch_move_history(dst, src, idx, idx + count, count);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(dst->stream));
    return 0;
}

// A stream of starts brings its finished trajectories back (ilqg_host.c stream_solve): what `what` asks for of trajectories
// from[0..count) is gathered into the context's packed buffer by ONE launch (k_harvest, which states the record's layout) and
// reaches pinned host memory by ONE copy.  Everything is checked before anything is queued; ilqg_dev_harvest queues and
// returns, ilqg_dev_harvest_wait waits for the context's stream and hands the records out — a caller with several contexts
// queues on all of them before it waits for any.
int ilqg_dev_harvest(ilqg_dev_t *d, int count, const int *from, const ilqg_dev_harvest_t *what, int *words, int *offsets) {
    if(count < 1) return 0;
    HIP_TRY(hipSetDevice(d->device));
    if(!from || !what || !words || !offsets) {
        g_err = "ilqg_dev_harvest: from, what, words or offsets is NULL";
        return 1;
    }
    for(int j = 0; j < count; j++)
        if(from[j] < 0 || from[j] >= d->B) {
            g_err = "ilqg_dev_harvest: trajectory index out of range";
            return 1;
        }
    if(what->n_hist < 0 || what->n_hist > HARVEST_FIELDS || (what->n_hist > 0 && (!what->hist_int || !what->hist_field))) {
        g_err = "ilqg_dev_harvest: n_hist = " + std::to_string(what->n_hist) + ", must be 0 .. " + std::to_string(HARVEST_FIELDS) + " fields, each with its kind and index";
        return 1;
    }
    if(what->n_hist > 0 && d->hist.cap == 0) {
        g_err = "ilqg_dev_harvest: the context has no history (ilqg_dev_set_history with cap > 0 switches one on)";
        return 1;
    }
    HarvestPlan plan = {};
    plan.count = count, plan.n_hist = what->n_hist;
    int w = 2;
    plan.ox = what->x ? w : -1;
    w += what->x ? (d->N + 1) * NX : 0;
    plan.ou = what->u ? w : -1;
    w += what->u ? d->N * NU : 0;
    offsets[0] = plan.ox, offsets[1] = plan.ou;
    for(int i = 0; i < what->n_hist; i++) {
        const int f = what->hist_field[i], is_int = what->hist_int[i];
        if(is_int ? (f != ILQG_HI_N && (f < 0 || f >= ILQG_HI_COUNT)) : (f < 0 || f >= HIST_DOUBLES)) {
            g_err = "ilqg_dev_harvest: no such history field (w_pen_l / w_pen_f are recorded in libraries of problems with multipliers only)";
            return 1;
        }
        plan.kind[i] = !is_int ? HARVEST_DOUBLE : f == ILQG_HI_N ? HARVEST_N : HARVEST_INT;
        plan.field[i] = f == ILQG_HI_N ? 0 : f;
        plan.off[i] = offsets[2 + i] = w;
        w += !is_int ? d->hist.cap : f == ILQG_HI_N ? 1 : (d->hist.cap + 1) / 2;
    }
    for(int i = what->n_hist; i <= HARVEST_FIELDS; i++) plan.off[i] = w;
    plan.W = *words = w;
    const size_t bytes = (size_t)count * w * sizeof(unsigned long long), index_bytes = (size_t)count * sizeof(int);
    if(io_flush(d)) return 1;
    if(d->harvest.reserve(bytes + index_bytes, d->stream) || d->harvest_host.reserve(bytes, d->stream)) return 1;
    int *idx = reinterpret_cast<int *>(d->harvest.get() + (size_t)count * w);  // (behind the records: 8-byte aligned)
    // (the list goes up from the pinned buffer, which the records overwrite behind the kernel in stream order: `from` is the
    // caller's again when this returns)
    memcpy(d->harvest_host.get(), from, index_bytes);
    HIP_TRY(hipMemcpyAsync(idx, d->harvest_host.get(), index_bytes, hipMemcpyHostToDevice, d->stream));
    {
        Timed t(d, ILQG_K_TRANSPOSE);
        launch_harvest(d, plan, idx);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d->harvest_host.get(), d->harvest.get(), bytes, hipMemcpyDeviceToHost, d->stream));
    return 0;
}
int ilqg_dev_harvest_wait(ilqg_dev_t *d, const void **records) {
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->stream));
    *records = d->harvest_host.get();
    return 0;
}

// The iteration history.  Both buffers are made before the old ones go, so a capacity that does not fit leaves the history
// as it was; the context's stream is drained in front of the exchange (k_history runs on the roll-outs' stream, which
// hands back to the context's stream in ilqg_dev_update).
static size_t history_doubles(const ilqg_dev_t *d, int cap) { return (size_t)HIST_DOUBLES * cap * d->Bp; }
static size_t history_ints(const ilqg_dev_t *d, int cap) { return ((size_t)ILQG_HI_COUNT * cap + 1) * d->Bp; }
int ilqg_dev_history_cap(const ilqg_dev_t *d) { return d->hist.cap; }
// the buffers of a history of capacity cap, made aside (hist_next_*): ilqg_dev_set_history(d, cap) takes them.  cap <= 0 or
// the capacity the context has: whatever was aside is released, nothing is made.
int ilqg_dev_reserve_history(ilqg_dev_t *d, int cap) {
    HIP_TRY(hipSetDevice(d->device));
    d->hist_next_cap = 0;
    if(d->hist_next_d.release() | d->hist_next_i.release()) return 1;
    if(cap <= 0 || cap == d->hist.cap) return 0;
    if(d->hist_next_d.renew(history_doubles(d, cap) * sizeof(double)) || d->hist_next_i.renew(history_ints(d, cap) * sizeof(int))) {
        const std::string why = g_err;
        (void)hipGetLastError();
        (void)d->hist_next_d.release();
        g_err = "set_history: no device memory for a history of cap = " + std::to_string(cap) + " entries per trajectory (" +
                std::to_string(history_doubles(d, cap) * sizeof(double) + history_ints(d, cap) * sizeof(int)) + " bytes); the history stays as it was: " + why;
        return 1;
    }
    d->hist_next_cap = cap;
    return 0;
}
int ilqg_dev_set_history(ilqg_dev_t *d, int cap) {
    HIP_TRY(hipSetDevice(d->device));
    if(cap < 0) {
        g_err = "set_history: cap must not be negative (cap > 0: a history of that many entries per trajectory, 0: none)";
        return 1;
    }
    if(cap != d->hist.cap) {
        if(cap > 0 && d->hist_next_cap != cap && ilqg_dev_reserve_history(d, cap)) return 1;
        HIP_TRY(hipStreamSynchronize(d->stream));
        d->hist_d = std::move(d->hist_next_d);  // (cap = 0: nothing is aside, the old buffers go)
        d->hist_i = std::move(d->hist_next_i);
        d->hist_next_cap = 0;
        d->hist = History{d->hist_d.get(), d->hist_i.get(), cap, d->Bp};
    }
    if(cap > 0) {
        HIP_TRY(hipMemsetAsync(d->hist.d, 0, d->hist_d.bytes(), d->stream));
        HIP_TRY(hipMemsetAsync(d->hist.i, 0, d->hist_i.bytes(), d->stream));
    }
    return 0;
}
}  // extern "C"
// one field's slab [cap][Bp] to the host, turned into [B][cap]
template <class T>
static int history_field(ilqg_dev_t *d, const T *slab, T *out) {
    const int cap = d->hist.cap;
    std::vector<T> host((size_t)cap * d->Bp);
    HIP_TRY(hipMemcpyAsync(host.data(), slab, host.size() * sizeof(T), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    for(int b = 0; b < d->B; b++)
        for(int e = 0; e < cap; e++) out[(size_t)b * cap + e] = host[(size_t)e * d->Bp + b];
    return 0;
}
extern "C" {
static int history_readable(ilqg_dev_t *d, const char *who, const void *out) {
    if(d->hist.cap == 0) {
        g_err = std::string(who) + ": the context has no history (ilqg_dev_set_history with cap > 0 switches one on)";
        return 1;
    }
    if(!out) {
        g_err = std::string(who) + ": out is NULL";
        return 1;
    }
    return 0;
}
int ilqg_dev_get_history(ilqg_dev_t *d, int field, double *out) {
    HIP_TRY(hipSetDevice(d->device));
    if(history_readable(d, "get_history", out)) return 1;
    if(field < 0 || field >= ILQG_H_COUNT) {
        g_err = "get_history: no such field";
        return 1;
    }
    if(field >= HIST_DOUBLES) {
        g_err = "get_history: w_pen_l / w_pen_f are recorded in libraries of problems with multipliers only; this problem has none";
        return 1;
    }
    return history_field(d, d->hist.d + d->hist.at(field, 0, 0), out);
}
int ilqg_dev_get_history_int(ilqg_dev_t *d, int field, int *out) {
    HIP_TRY(hipSetDevice(d->device));
    if(history_readable(d, "get_history_int", out)) return 1;
    if(field == ILQG_HI_N) {
        HIP_TRY(hipMemcpyAsync(out, d->hist.i, (size_t)d->B * sizeof(int), hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        return 0;
    }
    if(field < 0 || field >= ILQG_HI_COUNT) {
        g_err = "get_history_int: no such field";
        return 1;
    }
    return history_field(d, d->hist.ints() + d->hist.at(field, 0, 0), out);
}

int ilqg_dev_sync(ilqg_dev_t *d) {
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

int ilqg_dev_count_active(ilqg_dev_t *d, int *n_active) {
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipMemsetAsync(d->counter.get(), 0, sizeof(int), d->stream));
    hipLaunchKernelGGL(k_count_active, grid1(d->Bp, 256), dim3(256), 0, d->stream, d->P.i[ILQG_I_STATUS], d->B,
                       d->counter.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(n_active, d->counter.get(), sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

// cycle accounting of -DILQG_PROFILE_SECTIONS builds: reads and clears the 8 section counters (zeros otherwise)
int ilqg_dev_section_cycles(unsigned long long *out) {
#ifdef ILQG_PROFILE_SECTIONS
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(ilqg_prof_cycles), 8 * sizeof(unsigned long long)));
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(ilqg_prof_cycles), z, sizeof(z)));
#else
    for(int i = 0; i < 8; i++) out[i] = 0;
#endif
    return 0;
}

// k_derivs_wave's probes (ILQG_PROFILE_SECTIONS builds of the wave mapping; zeros otherwise), 32 sums, cleared by the call
int ilqg_dev_derivs_cycles(unsigned long long *out) {
#if defined(ILQG_PROFILE_SECTIONS) && ILQG_WAVE_MAP
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(ilqg_dprof_cycles), 32 * sizeof(unsigned long long)));
    unsigned long long z[32] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(ilqg_dprof_cycles), z, sizeof(z)));
#else
    for(int i = 0; i < 32; i++) out[i] = 0;
#endif
    return 0;
}

// quad mapping with speculative retries (ILQG_QUAD_SPEC=1): the protocol's words as the last backward launch left them —
// [B] attempts handed out | rows at work << 16, [B] written, [B][16] how attempt j ended (kind | direct << 2 | row << 3), [B] smallest
// attempt with a result, [rows] trajectory per row; returns the number of words through *count (0: not in use)
int ilqg_dev_spec_words(unsigned *out, size_t max_words, size_t *count) {
    *count = 0;
    ilqg_dev_t *d = g_spec_last;
    if(!d) return 0;
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipDeviceSynchronize());
    if(!d->spec_ints.get()) return 0;
    size_t n = d->spec_ints.bytes() / sizeof(unsigned);
    if(n > max_words) n = max_words;
    HIP_TRY(hipMemcpy(out, d->spec_ints.get(), n * sizeof(unsigned), hipMemcpyDeviceToHost));
    *count = n;
    return 0;
}

// -DILQG_WAVE_PLACES builds: the log of wavefront places (3 words per entry: kind / XCC / HW_ID, clock at entry, clock at
// exit), cleared by the call; returns the number of entries copied through *count (0 in other builds)
int ilqg_dev_wave_places(unsigned long long *out, int max_entries, int *count) {
    *count = 0;
#ifdef ILQG_WAVE_PLACES
    HIP_TRY(hipDeviceSynchronize());
    unsigned n = 0, zero = 0;
    HIP_TRY(hipMemcpyFromSymbol(&n, HIP_SYMBOL(ilqg_places_n), sizeof(n)));
    if(n > PLACES_MAX) n = PLACES_MAX;
    if((int)n > max_entries) n = (unsigned)max_entries;
    if(n) HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(ilqg_places), (size_t)n * 3 * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(ilqg_places_n), &zero, sizeof(zero)));
    *count = (int)n;
#else
    (void)out;
    (void)max_entries;
#endif
    return 0;
}

int ilqg_dev_timing(ilqg_dev_t *d, int enable) {
    HIP_TRY(hipSetDevice(d->device));
    if(drain_spans(d)) return 1;
    if(enable)
        while(d->event_pool.size() < 1024) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreate(&e));
            d->event_pool.push_back(e);
        }
    d->timing = enable != 0;
    memset(d->t_ms, 0, sizeof(d->t_ms));
    memset(d->t_n, 0, sizeof(d->t_n));
    memset(d->t_busy, 0, sizeof(d->t_busy));
    if(enable) {
        if(!d->epoch) HIP_TRY(hipEventCreate(&d->epoch));
        HIP_TRY(hipEventRecord(d->epoch, d->stream));
    }
    return 0;
}

/* length of the union of the launch intervals of a kernel since timing was switched on (ms): what the kernel occupied
 * of the wall clock, however its launches on different streams overlap in the event clock */
int ilqg_dev_get_busy(ilqg_dev_t *d, int kernel, double *busy_ms) {
    if(kernel < 0 || kernel >= ILQG_K_TOTAL) {
        g_err = "ilqg_dev_get_busy: bad kernel id";
        return 1;
    }
    if(drain_spans(d)) return 1;
    *busy_ms = d->t_busy[kernel];
    return 0;
}

int ilqg_dev_get_timing(ilqg_dev_t *d, int kernel, int *launches, double *total_ms) {
    if(kernel < 0 || kernel >= ILQG_K_TOTAL) {
        g_err = "ilqg_dev_get_timing: bad kernel id";
        return 1;
    }
    if(drain_spans(d)) return 1;
    *launches = d->t_n[kernel];
    *total_ms = d->t_ms[kernel];
    return 0;
}

// op / shape as in k_dense_test; in*/out are host arrays of n_in0/n_in1/n_in2/n_out doubles (out is in/out)
int ilqg_dev_dense(int device, int op, int shape, const double *in0, int n_in0, const double *in1, int n_in1,
                   const double *in2, int n_in2, double *out, int n_out, int *flag) {
    HIP_TRY(hipSetDevice(device));
    Buffer<double> d0, d1, d2, dout;
    Buffer<int> dflag;
    if(d0.reserve((n_in0 > 0 ? n_in0 : 1) * 8) || d1.reserve((n_in1 > 0 ? n_in1 : 1) * 8) || d2.reserve((n_in2 > 0 ? n_in2 : 1) * 8) ||
       dout.reserve((n_out > 0 ? n_out : 1) * 8) || dflag.reserve(4))
        return 1;
    if(n_in0 > 0) HIP_TRY(hipMemcpy(d0.get(), in0, n_in0 * 8, hipMemcpyHostToDevice));
    if(n_in1 > 0) HIP_TRY(hipMemcpy(d1.get(), in1, n_in1 * 8, hipMemcpyHostToDevice));
    if(n_in2 > 0) HIP_TRY(hipMemcpy(d2.get(), in2, n_in2 * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dout.get(), out, n_out * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_dense_test, dim3(1), dim3(64), 0, 0, op, shape, 0, 0, d0.get(), d1.get(), d2.get(), dout.get(), dflag.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.get(), n_out * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flag, dflag.get(), 4, hipMemcpyDeviceToHost));
    return 0;
}

int ilqg_dev_sincos_batch(int device, int n, const double *x, double *s, double *c) {
    HIP_TRY(hipSetDevice(device));
    Buffer<double> dx, ds, dc;
    if(dx.reserve(n * 8) || ds.reserve(n * 8) || dc.reserve(n * 8)) return 1;
    HIP_TRY(hipMemcpy(dx.get(), x, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_sincos_test, grid1(n, 256), dim3(256), 0, 0, n, dx.get(), ds.get(), dc.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(s, ds.get(), n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c, dc.get(), n * 8, hipMemcpyDeviceToHost));
    return 0;
}

// The first uses of k_history and k_move_history in this translation unit: where a template is first used is where its code
// lands in the code object (see k_history in k_common.inc) — here, behind every kernel of the solver and in front of the
// box QP's unit-test kernels, which call nothing out of line.
static void launch_history(ilqg_dev_t *d, hipStream_t stream) {
    hipLaunchKernelGGL(k_history<>, grid1(d->Bp, 256), dim3(256), 0, stream, d->P, d->hist);
}
static void launch_move_history(ilqg_dev_t *dst, ilqg_dev_t *src, const int *to, const int *from, int count) {
    hipLaunchKernelGGL(k_move_history<>, grid1((size_t)count * dst->hist.cap, 256), dim3(256), 0, dst->stream, dst->hist, src->hist, to, from, count);
}
// ... and of k_harvest, behind them for the same reason.  Grid: x = blocks of HARVEST_WAVES entries, y = blocks of 64 words.
static void launch_harvest(ilqg_dev_t *d, const HarvestPlan &plan, const int *from) {
    hipLaunchKernelGGL(k_harvest<>, dim3((unsigned)((plan.count + HARVEST_WAVES - 1) / HARVEST_WAVES), (unsigned)((plan.W + WAVE - 1) / WAVE)),
                       dim3(WAVE * HARVEST_WAVES), 0, d->stream, d->P, d->hist, plan, from, d->harvest.get());
}

// rows: 0 box_qp (one problem per lane), 1 the cooperative form of the wave mapping (one per wavefront), 2 box_qp with the
// pattern tables, 3 box_qp_quad (four per wavefront; `active`: one int per problem, NULL = all active)
static int boxqp_batch(int rows, int device, int n, int count, const double *H, const double *g, const double *lower,
                       const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc, const int *active = nullptr) {
    if(n != 2 && n != 8 && n != NU) {
        g_err = "ilqg_dev_boxqp_batch: n must be 2, 8 or N_U";
        return 1;
    }
    if(rows == 3) {
#if ILQG_WAVE_MAP
        if(n != 2 && n != NU) {
            g_err = "ilqg_dev_boxqp_quad_batch: n must be 2 or N_U";
            return 1;
        }
#else
        g_err = "ilqg_dev_boxqp_quad_batch: the quad form is compiled into the libraries of the wave mapping only (N_X > 8, lib*_wave.so)";
        return 1;
#endif
    }
    HIP_TRY(hipSetDevice(device));
    const size_t T = n * (n + 1) / 2;
    Buffer<double> oH, oinv, og, olo, oup, ox;
    Buffer<int> ocl, onf, orc, oact;
    if(oH.reserve(count * T * 8) || oinv.reserve(count * T * 8) || og.reserve(count * n * 8) || olo.reserve(count * n * 8) ||
       oup.reserve(count * n * 8) || ox.reserve(count * n * 8) || ocl.reserve(count * n * 4) || onf.reserve(count * 4) || orc.reserve(count * 4))
        return 1;
    double *const dH = oH.get(), *const dinv = oinv.get(), *const dg = og.get(), *const dlo = olo.get(), *const dup = oup.get(), *const dx = ox.get();
    int *const dcl = ocl.get(), *const dnf = onf.get(), *const drc = orc.get();
    HIP_TRY(hipMemcpy(dH, H, count * T * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dg, g, count * n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dlo, lower, count * n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dup, upper, count * n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dx, x, count * n * 8, hipMemcpyHostToDevice));
    const dim3 grid = rows == 1 ? dim3(count) : (rows == 3 ? grid1(count, 4) : grid1(count, 64)), block(64);
#if ILQG_WAVE_MAP
    if(rows == 3) {
        if(oact.reserve(count * 4)) return 1;
        int *const dact = oact.get();
        const std::vector<int> every(count, 1);
        HIP_TRY(hipMemcpy(dact, active ? active : every.data(), count * 4, hipMemcpyHostToDevice));
        if(n == NU)
            hipLaunchKernelGGL(k_boxqp_quad_test<NU>, grid, block, 0, 0, count, dact, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
        else
            hipLaunchKernelGGL(k_boxqp_quad_test<2>, grid, block, 0, 0, count, dact, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
    } else
#endif
#if ILQG_EXPERIMENTS
    if(rows == 2 && n == 2)
        hipLaunchKernelGGL((k_boxqp_test<2, true>), grid, block, 0, 0, count, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
    else if(rows == 2 && n == NU)
        hipLaunchKernelGGL((k_boxqp_test<NU, true>), grid, block, 0, 0, count, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
    else if(rows == 2) {
        g_err = "ilqg_dev_boxqp_table_batch: n must be 2 or N_U";
        return 1;
    } else
#else
    if(rows == 2) {
        g_err = "ilqg_dev_boxqp_table_batch: the pattern-table form is compiled into the -DILQG_EXPERIMENTS libraries only (lib*_exp.so)";
        return 1;
    } else
#endif
    if(rows && n == 2)
        hipLaunchKernelGGL(k_boxqp_rows_test<2>, grid, block, 0, 0, count, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
    else if(rows && n == 8)
        hipLaunchKernelGGL(k_boxqp_rows_test<8>, grid, block, 0, 0, count, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
    else if(rows)
        hipLaunchKernelGGL(k_boxqp_rows_test<NU>, grid, block, 0, 0, count, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
    else if(n == 2)
        hipLaunchKernelGGL(k_boxqp_test<2>, grid, block, 0, 0, count, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
    else if(n == 8)
        hipLaunchKernelGGL(k_boxqp_test<8>, grid, block, 0, 0, count, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
    else
        hipLaunchKernelGGL(k_boxqp_test<NU>, grid, block, 0, 0, count, dH, dg, dlo, dup, dx, dcl, dnf, dinv, drc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(x, dx, count * n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(invH, dinv, count * T * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(clamp, dcl, count * n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_free, dnf, count * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rc, drc, count * 4, hipMemcpyDeviceToHost));
    return 0;
}

int ilqg_dev_boxqp_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                         const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc) {
    return boxqp_batch(0, device, n, count, H, g, lower, upper, x, clamp, n_free, invH, rc);
}

int ilqg_dev_boxqp_wave_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                              const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc) {
    return boxqp_batch(1, device, n, count, H, g, lower, upper, x, clamp, n_free, invH, rc);
}

int ilqg_dev_boxqp_table_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                               const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc) {
    return boxqp_batch(2, device, n, count, H, g, lower, upper, x, clamp, n_free, invH, rc);
}

int ilqg_dev_boxqp_quad_batch(int device, int n, int count, const double *H, const double *g, const double *lower,
                              const double *upper, double *x, int *clamp, int *n_free, double *invH, int *rc, const int *active) {
    return boxqp_batch(3, device, n, count, H, g, lower, upper, x, clamp, n_free, invH, rc, active);
}

// ---------------------------------------------------------------------------
// Several GPUs of one node in ONE process (SURVEY 8(e)): the trajectory batch is sharded, every device advances its
// shard by itself, and the only exchange is one RCCL gather of a per-trajectory scalar (the costs) to a root device.
// ---------------------------------------------------------------------------
// (send[] and recv stay raw pointers: each is freed with ITS device current, which a Buffer does not remember)
struct ilqg_comm {
    int n;
    std::vector<int> devices;
    std::vector<ncclComm_t> comms;
    std::vector<double *> send;   // per device: its shard of the scalar, padded to `per`
    double *recv;                 // root device: n * per doubles
    int per;
    bool loopback;                // every shard on ONE device (tests, rehearsals): the gather is device-to-device copies
};

#define NCCL_TRY(expr)                                                              \
    do {                                                                            \
        ncclResult_t r_ = (expr);                                                   \
        if(r_ != ncclSuccess) {                                                     \
            g_err = std::string(#expr) + ": " + ncclGetErrorString(r_);             \
            return 1;                                                               \
        }                                                                           \
    } while(0)

void ilqg_comm_destroy(ilqg_comm_t *c) {
    if(!c) return;
    for(size_t g = 0; g < c->comms.size(); g++)
        if(c->comms[g]) ncclCommDestroy(c->comms[g]);
    for(size_t g = 0; g < c->send.size(); g++) {
        hipSetDevice(c->devices[g]);
        if(c->send[g]) hipFree(c->send[g]);
    }
    if(c->recv) {
        hipSetDevice(c->devices[0]);
        hipFree(c->recv);
    }
    delete c;
}

static int comm_fill(ilqg_comm *c, int n, const int *devices, int per) {
    c->n = n;
    c->per = per;
    c->devices.assign(devices, devices + n);
    c->comms.assign(n, nullptr);
    c->send.assign(n, nullptr);
    // RCCL wants distinct devices.  Several shards on one device (n > 1, all the same id) is how the sharding, the
    // offsets and the cost hand-over are rehearsed where only one GPU is present: no communicator, the gather copies.
    c->loopback = n > 1;
    for(int g = 1; g < n; g++)
        if(devices[g] != devices[0]) c->loopback = false;
    if(!c->loopback) NCCL_TRY(ncclCommInitAll(c->comms.data(), n, devices));
    for(int g = 0; g < n; g++) {
        HIP_TRY(hipSetDevice(devices[g]));
        HIP_TRY(hipMalloc((void **)&c->send[g], (size_t)per * sizeof(double)));
        HIP_TRY(hipMemset(c->send[g], 0, (size_t)per * sizeof(double)));
    }
    HIP_TRY(hipSetDevice(devices[0]));
    HIP_TRY(hipMalloc((void **)&c->recv, (size_t)n * per * sizeof(double)));
    return 0;
}

// one communicator over `n` distinct devices; `per` = doubles every device contributes to a gather
int ilqg_comm_create(ilqg_comm_t **out, int n, const int *devices, int per) {
    *out = nullptr;
    if(n < 1 || per < 1) {
        g_err = "ilqg_comm_create: need at least one device and one value per device";
        return 1;
    }
    ilqg_comm *c = new ilqg_comm();
    if(comm_fill(c, n, devices, per)) {
        const std::string why = g_err;
        ilqg_comm_destroy(c);
        g_err = why;
        return 1;
    }
    *out = c;
    return 0;
}

void *ilqg_comm_send_buffer(ilqg_comm_t *c, int g) { return (g >= 0 && g < c->n) ? c->send[g] : nullptr; }

// The single collective of the path: the send buffers (filled by the caller, `per` doubles per device, all copies
// complete) -> device 0 by ONE ncclGather, enqueued on the stream of each device's context devs[g], and on to the
// host: host[first[g] .. first[g] + counts[g]) = what device g sent.
int ilqg_comm_gather(ilqg_comm_t *c, ilqg_dev_t *const *devs, const int *first, const int *counts, double *host) {
    for(int g = 0; g < c->n; g++)
        if(counts[g] > c->per) {
            g_err = "ilqg_comm_gather: a shard is larger than the communicator's send buffers";
            return 1;
        }
    if(c->loopback) {
        HIP_TRY(hipSetDevice(c->devices[0]));
        for(int g = 0; g < c->n; g++) {
            HIP_TRY(hipMemcpyAsync(c->recv + (size_t)g * c->per, c->send[g], (size_t)c->per * sizeof(double),
                                   hipMemcpyDeviceToDevice, devs[g]->stream));
            if(g > 0) HIP_TRY(hipStreamSynchronize(devs[g]->stream));
        }
    } else {
        NCCL_TRY(ncclGroupStart());
        for(int g = 0; g < c->n; g++)
            NCCL_TRY(ncclGather(c->send[g], c->recv, (size_t)c->per, ncclDouble, 0, c->comms[g], devs[g]->stream));
        NCCL_TRY(ncclGroupEnd());
    }
    HIP_TRY(hipSetDevice(c->devices[0]));
    std::vector<double> tmp((size_t)c->n * c->per);
    HIP_TRY(hipMemcpyAsync(tmp.data(), c->recv, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, devs[0]->stream));
    HIP_TRY(hipStreamSynchronize(devs[0]->stream));
    for(int g = 0; g < c->n; g++) memcpy(host + first[g], tmp.data() + (size_t)g * c->per, sizeof(double) * counts[g]);
    return 0;
}

}  // extern "C"
