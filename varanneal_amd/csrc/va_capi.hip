// va_capi.hip -- host side of libvaranneal_amd.so: the C-ABI of include/varanneal_amd.h.
//
// Owns the device image of one annealing problem (B seeds resident in HBM), moves
// paths in/out, and drives the three-launch kernel cycle
//     k_eval (+ line-search / ladder step) -> k_update (+ direction coefficients) -> k_direction
// until every seed has climbed its whole RF ladder.  No per-iteration host sync:
// the host only polls a device counter of unfinished seeds every few cycles.
//
// Creation.  A handle under construction has ONE owner (HandleOwner: va_problem_destroy on every way out but success), and
// both constructors share their front and back halves:
//     begin_create         device, stream, zeroed Dev, lbfgs_m / max_beta, default options
//     ... the action's own steps ...
//     alloc_solver_state   per-seed vectors, L-BFGS history, result tables
//     finish_create        pinned poll word, events, the stream sync that ends the life of the host staging buffers
// va_problem_create:       validate_desc (every check that needs neither HIP nor the plan) -> begin_create -> plan_problem
//                          (plan_eval / plan_module, va_eval_geo.h) -> fill_dims (Dims / Dev from the descriptor and the
//                          plan) -> prepare_kernels (LDS check, opt-in) -> alloc_problem_data -> alloc_solver_state ->
//                          upload_problem_data -> choose_persist -> finish_create
// va_nnet_problem_create:  plan_nnet (va_nnet_geo.h: the descriptor's checks and the whole launch plan, host arithmetic a
//                          CPU test records) -> begin_create -> fill_nnet_dims -> create_nnet_image -> finish_create
#include <dlfcn.h>
#include <link.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/varanneal_amd.h"
#include "va_device.h"
#include "va_eval_geo.h"
#include "va_nnet.h"
#include "va_eval_flat.h"
#include "va_persist.h"
#include "va_predict.h"
#include "va_predict_tlm.h"
#include "va_predict_adj.h"
#include "va_shoot.h"
#include "va_shoot_box.h"
#include "va_lyap.h"
#include "va_enkf.h"
#include "va_hvp.h"
#include "va_selinv.h"
#include "va_hmc.h"
#include "va_hmc_box.h"

using namespace va;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(e_ == hipErrorOutOfMemory ? VA_ENOMEM : VA_EHIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                 \
    } while (0)

// a step that returns a code: pass the first failure on
#define TRY(expr)                       \
    do {                                \
        if (int rc_ = (expr)) return rc_; \
    } while (0)
// an upload into a handle's buffer, whose name a failure reports
#define UPLOAD(dst, src, n) h->upload(dst, src, n, #dst)

// generated right-hand-side modules (va_rhs_load_module); ids are VA_RHS_USER_BASE + index
struct UserRhs {
    ModuleVariant variant;     // the ONE column-run instantiation the module carries besides its flat kernel, if any (va_user_rhs.hip)
    std::string path;
    void *dl = nullptr;
    RhsTable table = {};       // the module's launchers and sizes (va_user_rhs_table)
    HvpTable hvp = {};         // ... and the Hessian-vector kernel's (va_user_hvp_table); hvp.hvp NULL: the module has none
    // variant.n_colp_vectors > 0: the column-run instantiation is of the model's column-parameter form (RhsUserColP); its map
    // (va_user_colp_map): shared scalars S, vectors V, then the global index of each shared scalar and of each vector entry
    std::vector<int> colp;
};
struct UserAct {
    std::string path;
    void *dl = nullptr;
    NnetActLaunch launch = nullptr;
};
std::vector<UserAct> g_user_act;      // (guarded by g_user_rhs_mutex, like the right-hand-side registry)
std::vector<UserRhs> g_user_rhs;
std::mutex g_user_rhs_mutex;            // the registry is process-wide; handles are not shared

}  // namespace

struct va_problem_s {
    Dev dv;
    int device = 0, rhs = 0, keep_paths = 0;
    RhsTable rt = {};                  // the right-hand side's launchers (a copy; eval: the kernel THIS handle runs)
    HvpTable rt_hvp = {};              // the Hessian-vector kernel's launcher (va_hvp.h), hvp NULL: none
    NnetActLaunch nn_act = nullptr;    // generated activation module's launcher (nn.act >= NNET_USER)
    // few seeds, short paths: the whole ladder in ONE launch, every vector of the minimisation resident in
    // the LDS of pz_G workgroups per seed (va_persist.h); chosen at create when the slices fit and all are co-resident
    bool persist = false, tune_persist = true;
    int pz_G = 0, pz_T = 0, pz_maxG = 0;
    void *pz_misc = nullptr;           // device: [abort flag (int), pad, cycles (unsigned long long), stamps (PZ_NSTAMP doubles)]
    size_t pz_xch_bytes = 0;
    bool is_nnet = false;              // feed-forward-network action (va_nnet.hip) instead of an ODE path
    bool fold = false;                 // the evaluation kernel runs the tail itself (last arriver of each seed)
    bool tune_graph = true;            // ladder cycles / timed evaluations replayed from a hipGraph (va_problem_tune)
    int wg4_plan = 1;                  // k_eval4: the planner's row groups per workgroup (dv.wg4: what the handle runs, VA_TUNE_WIDE)
    hipGraphExec_t timed_gexec = nullptr;   // va_eval_timed's chunk of launches
    int timed_chunk = 0;
    Dev timed_dv;                      // the device image the chunk was captured with (kernels take it by value):
    NnetDev timed_nn;                  //   the graph is replayed only while h->dv / h->nn still equal these bytes
    double timed_armed_rf = -1.0;      // >= 0: every seed sits in PH_START at this rf_scale (S1 launches leave it so);
                                       //   what an S1 launch carries by value as Dev::s1_rf (run_eval)
    NnetDev nn;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<void *> allocs;
    int *h_nactive = nullptr;          // pinned: [0] live seeds; bytes 8..15: evaluation counter
    double *d_rf = nullptr;            // ladder on device [max_beta]
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int64_t n_eval_launch = 0, n_seed_evals = 0, n_seed_evals_direct = 0, n_cycles = 0;
    int last_nbeta = 0;
    std::vector<int> lidx_user;        // the observed columns in the caller's order (the device keeps them sorted): va_predict_adjoint's Y

    template <class T> int alloc(T **p, size_t n, bool zero = true)
    {
        void *q = nullptr;
        size_t bytes = sizeof(T) * (n ? n : 1);
        HIPCHK(hipMalloc(&q, bytes));
        allocs.push_back(q);
        if (zero) HIPCHK(hipMemsetAsync(q, 0, bytes, stream));
        *p = (T *)q;
        return VA_OK;
    }
    // n elements host -> device on the handle's stream.  Asynchronous, and from pageable memory during creation: src stays
    // untouched until the stream is synchronised (finish_create)
    template <class T> int upload(T *dst, const T *src, size_t n, const char *name)
    {
        hipError_t e = hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) return fail(VA_EHIP, "H2D %s: %s", name, hipGetErrorString(e));
        return VA_OK;
    }
};

// the one owner of a handle under construction: whatever way a constructor returns before `*out = h.release()`, the
// handle and everything it allocated so far go through va_problem_destroy
struct HandleDeleter { void operator()(va_problem_s *h) const { va_problem_destroy(h); } };
typedef std::unique_ptr<va_problem_s, HandleDeleter> HandleOwner;

namespace {

// one batched evaluation.  epi: what the last-arriving wave of each seed does with the partial sums
// (EPI_FINALIZE: S1 outputs; EPI_LS: one line-search / ladder step).  The network action's
// evaluation is several kernels, so its tail stays a launch of its own.
void run_eval(va_handle h, int epi)
{
    if (epi != EPI_FINALIZE) h->timed_armed_rf = -1.0;      // (line-search launches move the seeds' states)
    h->dv.lsrun = epi == EPI_LS ? 1 : 0;       // (S1 evaluations put every seed in PH_START: no line-search points)
    // An S1 launch takes phase and RF from its argument instead of the seeds' states -- while the handle KNOWS them: the
    // caller armed every seed with this RF and nothing has moved a state since (each path that does resets timed_armed_rf).
    // Every other launch kind reads the states.
    h->dv.s1_rf = epi == EPI_FINALIZE ? h->timed_armed_rf : -1.0;
    EvalOp op{false, h->stream, hipSuccess};
    if (h->is_nnet ? !h->nn.small : !h->fold) {
        // (large grids: a workgroup that waits for its arrival to come back holds its LDS and wave
        // slots ~1 us longer, which costs more than the 64-wave tail kernel it saves)
        h->dv.epi = EPI_NONE;
        if (h->is_nnet) launch_nnet_eval(h->dv, h->nn, h->stream, h->nn_act);
        else h->rt.eval(h->dv, op);
        if (epi == EPI_FINALIZE) launch_finalize_eval(h->dv, h->stream);
        else if (epi == EPI_LS) launch_ls(h->dv, h->stream);
        return;
    }
    h->dv.epi = epi;
    if (h->is_nnet) { launch_nnet_eval(h->dv, h->nn, h->stream, h->nn_act); return; }   // (small nets: k_nnet_small carries the tail)
    h->rt.eval(h->dv, op);
}

// per-seed vectors, L-BFGS history, partial tables and result tables: the part of the device
// image that does not depend on which action is being minimised
int alloc_solver_state(va_handle h)
{
    Dev &dv = h->dv;
    const Dims &dm = dv.dm;
    const size_t B = dm.B, ld = dm.ld, m = dm.m, max_beta = dv.max_beta;
    // x and d carry a zero-filled guard in front and behind: the evaluation kernels stage whole
    // tiles (+ halo rows) without clamping, so the first / last tile of the first / last seed reads
    // up to one tile beyond its path (such rows are masked out of the arithmetic)
    // (k_eval4: a workgroup of up to three row groups, whatever VA_TUNE_WIDE asks for later)
    const size_t guard = (((size_t)((dm.emode == 4 ? 3 : 1) * dm.T + 8) * dm.D + 15) / 16) * 16;
    TRY(h->alloc(&dv.x, B * ld + 2 * guard)); TRY(h->alloc(&dv.g, B * ld));
    TRY(h->alloc(&dv.gt, B * ld)); TRY(h->alloc(&dv.d, B * ld + 2 * guard));
    dv.x += guard; dv.d += guard;
    TRY(h->alloc(&dv.S, B * m * ld)); TRY(h->alloc(&dv.Y, B * m * ld));
    TRY(h->alloc(&dv.st, B));
    TRY(h->alloc(&dv.evp, B * dm.nprow * EP_N));
    dv.npbig = (!h->is_nnet && !dv.cpv && dm.NPt > RHS_MAX_NP) ? dm.NPt - RHS_MAX_NP : 0;
    if (dv.npbig) TRY(h->alloc(&dv.evp_big, B * dm.nprow * dv.npbig));
    if (dv.cpv) TRY(h->alloc(&dv.evv, B * dm.nprow * dv.cpv));
    TRY(h->alloc(&dv.upp, B * dm.nchunks * dv.ups));
    TRY(h->alloc(&dv.dpp, B * dm.nchunks * DP_N));
    TRY(h->alloc(&h->d_rf, max_beta));
    TRY(h->alloc(&dv.ame, B * max_beta * 3));
    TRY(h->alloc(&dv.pest, B * max_beta * (dm.NPest ? dm.NPest : 1)));
    TRY(h->alloc(&dv.status, B * max_beta)); TRY(h->alloc(&dv.nit, B * max_beta));
    TRY(h->alloc(&dv.nfev, B * max_beta));
    if (h->keep_paths) TRY(h->alloc(&dv.minpaths, B * max_beta * (size_t)(dm.ND + dm.NP), false));
    if (dm.bounded) {
        TRY(h->alloc(&dv.lb_z, B * ld)); TRY(h->alloc(&dv.lb_r, B * ld)); TRY(h->alloc(&dv.lb_xp, B * ld));
        TRY(h->alloc(&dv.lb_t, B * ld)); TRY(h->alloc(&dv.lb_iwhere, B * ld));
        TRY(h->alloc(&dv.lb_mat, B * 3 * m * m)); TRY(h->alloc(&dv.lb_dtd, B));
    }
    TRY(h->alloc(&dv.cnt_eval, B * CNT_STRIDE)); TRY(h->alloc(&dv.cnt_upd, B * CNT_STRIDE)); TRY(h->alloc(&dv.cnt_dir, B * CNT_STRIDE));
    TRY(h->alloc(&dv.n_active, 1));
    TRY(h->alloc(&dv.n_evals, 1));
    TRY(h->alloc(&dv.outA, B)); TRY(h->alloc(&dv.outme, B)); TRY(h->alloc(&dv.outfe, B));
    dv.rf_ladder = h->d_rf;
    return VA_OK;
}

// pinned poll word, timing events, initial seed states
int finish_create(va_handle h)
{
    hipError_t e = hipHostMalloc((void **)&h->h_nactive, 4 * sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) return fail(VA_ENOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
    e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    if (e != hipSuccess) return fail(VA_EHIP, "hipEventCreate: %s", hipGetErrorString(e));
    e = hipStreamSynchronize(h->stream);     // host staging buffers must be consumed before we return
    if (e != hipSuccess) return fail(VA_EHIP, "create sync: %s", hipGetErrorString(e));
    launch_init_states(h->dv, PH_IDLE, 1.0, h->stream);
    return VA_OK;
}

int copy_in(va_handle h, const double *XP, int64_t ld, int32_t mem)
{
    const Dims &dm = h->dv.dm;
    const size_t w = sizeof(double) * (dm.ND + dm.NPest);
    HIPCHK(hipMemcpy2DAsync(h->dv.x, sizeof(double) * dm.ld, XP, sizeof(double) * ld, w, dm.B,
                            mem == VA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                            h->stream));
    return VA_OK;
}

int copy_out(va_handle h, const double *src, double *dst, int64_t ld, int32_t mem)
{
    const Dims &dm = h->dv.dm;
    const size_t w = sizeof(double) * (dm.ND + dm.NPest);
    HIPCHK(hipMemcpy2DAsync(dst, sizeof(double) * ld, src, sizeof(double) * dm.ld, w, dm.B,
                            mem == VA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                            h->stream));
    return VA_OK;
}

int check_xp(va_handle h, const void *XP, int64_t ld, int32_t mem)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!XP) return fail(VA_EINVAL, "XP is NULL");
    if (ld < h->dv.dm.ND + h->dv.dm.NPest) return fail(VA_EINVAL, "ld (%lld) < n_var (%d)", (long long)ld, h->dv.dm.ND + h->dv.dm.NPest);
    if (mem != VA_MEM_HOST && mem != VA_MEM_DEVICE) return fail(VA_EINVAL, "bad mem kind %d", mem);
    return VA_OK;
}

int set_opts(va_handle h, const va_lbfgs_opts *o)
{
    if (!o) return fail(VA_EINVAL, "opts is NULL");
    if (o->maxls <= 0) return fail(VA_EINVAL, "maxls must be positive");
    if (o->maxcor <= 0) return fail(VA_EINVAL, "maxcor must be positive");
    Opts &d = h->dv.o;
    d.m = o->maxcor < h->dv.dm.m ? o->maxcor : h->dv.dm.m;
    d.maxiter = o->maxiter; d.maxls = o->maxls; d.maxfun = o->maxfun;
    d.ftol = o->ftol; d.gtol = o->gtol;
    return VA_OK;
}

// Is a rocprofiler-sdk tool (rocprofv3, rocprof-compute) loaded into this process?  Replaying ONE hipGraphExec of 192
// kernel nodes ~900 times under rocprofv3 --kernel-trace ends in a SIGSEGV 13 frames below hipGraphLaunch, inside the
// runtime / tool libraries (round 4: tools/ex1_probe.py --nbeta 101 --graph 1 under the profiler, at a 1 MiB-aligned
// address; the same ladder with plain launches under the profiler, and with the graph without it, runs).  A fault
// inside a HIP call cannot be turned into an error code, so the ladder does not replay graphs while such a tool is
// attached -- the profiler then also sees every kernel as a dispatch of its own.  (HIP itself links only
// librocprofiler-register.so; the sdk and its tool library arrive with the profiler.)
bool profiler_attached()
{
    static const bool attached = [] {
        bool found = false;
        dl_iterate_phdr([](struct dl_phdr_info *info, size_t, void *out) -> int {
            const char *n = info->dlpi_name;
            if (n && (strstr(n, "librocprofiler-sdk.so") || strstr(n, "librocprofiler-sdk-tool"))) { *(bool *)out = true; return 1; }
            return 0;
        }, &found);
        return found;
    }();
    return attached;
}

// the most cycles a ladder of nbeta rungs may take: every cycle costs each live seed at least one evaluation
long long ladder_cycle_bound(const Dev &dv, int nbeta)
{
    const double per_step = (double)dv.o.maxfun + dv.o.maxls + 4.0;
    const double bound = per_step * nbeta;
    return bound > 4e18 ? (long long)4e18 : (long long)bound;
}

// the ladder on the device, every seed counted live and put in PH_START (zero_dpp: the three-launch cycle's direction
// partials are zeroed where they always were on the stream, ahead of the state kernel)
int arm_ladder(va_handle h, const double *rf_scale, int nbeta, bool zero_dpp)
{
    Dev &dv = h->dv;
    HIPCHK(hipMemcpyAsync(h->d_rf, rf_scale, sizeof(double) * nbeta, hipMemcpyHostToDevice, h->stream));
    dv.nbeta = nbeta; h->last_nbeta = nbeta;
    *h->h_nactive = dv.dm.B;
    HIPCHK(hipMemcpyAsync(dv.n_active, h->h_nactive, sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (zero_dpp) HIPCHK(hipMemsetAsync(dv.dpp, 0, sizeof(double) * dv.dm.B * dv.dm.nchunks * DP_N, h->stream));
    launch_init_states(dv, PH_START, -1.0, h->stream);
    h->timed_armed_rf = -1.0;
    return VA_OK;
}

// the count of live seeds and the evaluation counter into the pinned words (and 16 bytes of the persistent kernel's
// flags into misc, if given); returns once they are there
int read_progress(va_handle h, void *misc = nullptr)
{
    const Dev &dv = h->dv;
    HIPCHK(hipMemcpyAsync(h->h_nactive, dv.n_active, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->h_nactive + 2, dv.n_evals, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    if (misc) HIPCHK(hipMemcpyAsync(misc, h->pz_misc, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return VA_OK;
}

// a ladder ended after cyc cycles: the handle's counters, from what read_progress left
void book_ladder(va_handle h, long long cyc)
{
    h->n_cycles += cyc; h->n_eval_launch += cyc;
    h->n_seed_evals = h->n_seed_evals_direct + (int64_t)*(unsigned long long *)(h->h_nactive + 2);
}

// the kernel cycle until no seed is left (or the evaluation budget bound is hit)
int run_ladder_persist(va_handle h, const double *rf_scale, int nbeta, bool *fell_back);

int run_ladder(va_handle h, const double *rf_scale, int nbeta)
{
    Dev &dv = h->dv;
    if (nbeta < 1 || nbeta > dv.max_beta) return fail(VA_EINVAL, "nbeta=%d outside [1, max_beta=%d]", nbeta, dv.max_beta);
    if (h->persist && h->tune_persist) {
        bool fell_back = false;
        const int rc = run_ladder_persist(h, rf_scale, nbeta, &fell_back);
        if (!fell_back) return rc;
    }
    TRY(arm_ladder(h, rf_scale, nbeta, true));
    if (dv.dm.bounded) launch_clamp_x(dv, h->stream);
    const long long max_cycles = ladder_cycle_bound(dv, nbeta);
    long long cyc = 0;
    int poll = 4;
    // Long ladders on small problems are bound by the host's launch rate (3 launches per cycle at
    // ~4 us each against ~25 us of device time): once the polling interval has grown to 64 cycles,
    // that batch of 192 launches is captured ONCE into a hipGraph and replayed.  The kernels take the device image
    // by value, so the graph is private to this call (ladder length, options).
    hipGraphExec_t gexec = nullptr;
    bool use_graph = h->tune_graph && !profiler_attached();
    auto enqueue = [&](int n) {
        for (int k = 0; k < n; ++k) {
            run_eval(h, EPI_LS);
            launch_update(dv, h->stream);
            if (dv.dm.bounded) launch_lbfgsb_dir(dv, h->stream);      // L-BFGS-B: Cauchy point + subspace minimisation
            else launch_direction(dv, h->stream);
        }
    };
    struct GraphGuard { hipGraphExec_t &g; ~GraphGuard() { if (g) (void)hipGraphExecDestroy(g); } } guard{gexec};
    for (;;) {
        if (poll == 64 && use_graph) {
            if (!gexec) {
                // any failure here just means plain launches for the rest of this call
                hipGraph_t g = nullptr;
                if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                    enqueue(poll);
                    if (hipStreamEndCapture(h->stream, &g) != hipSuccess || !g ||
                        hipGraphInstantiate(&gexec, g, nullptr, nullptr, 0) != hipSuccess) gexec = nullptr;
                    if (g) (void)hipGraphDestroy(g);
                }
                if (!gexec) { (void)hipGetLastError(); use_graph = false; }
            }
            if (gexec) HIPCHK(hipGraphLaunch(gexec, h->stream));
            else enqueue(poll);
        } else enqueue(poll);
        cyc += poll;
        HIPCHK(hipGetLastError());            // a failed launch surfaces here, with its cause, not as a stalled ladder
        TRY(read_progress(h));
        if (*h->h_nactive <= 0) break;
        if (cyc > max_cycles) return fail(VA_ESTATE, "ladder did not finish within %lld cycles", max_cycles);
        if (poll < 64) poll *= 2;
    }
    book_ladder(h, cyc);
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// The same ladder as ONE launch of the persistent per-seed kernel.  *fell_back: the launch was refused, or its workgroups
// turned out not to be all resident (e.g. another process holds CUs): nothing was kept, take the three-launch cycle.
int run_ladder_persist(va_handle h, const double *rf_scale, int nbeta, bool *fell_back)
{
    Dev &dv = h->dv;
    *fell_back = false;
    const long long max_cycles = ladder_cycle_bound(dv, nbeta);
    Dev dvp = dv;
    dvp.dm.T = h->pz_T; dvp.dm.ntiles = h->pz_G; dvp.dm.nprow = h->pz_G;
    dvp.nbeta = nbeta; dvp.pz.max_cycles = max_cycles;
    HIPCHK(hipMemsetAsync(dv.pz.xch, 0, h->pz_xch_bytes, h->stream));           // (tags restart at 1 with every launch)
    HIPCHK(hipMemsetAsync(h->pz_misc, 0, 16, h->stream));
    TRY(arm_ladder(h, rf_scale, nbeta, false));
    EvalOp op{false, h->stream, hipSuccess};
    h->rt.seed(dvp, op);
    if (op.err != hipSuccess) {
        (void)hipGetLastError();
        h->persist = false;           // (for the rest of this handle's life)
        *fell_back = true;
        return VA_OK;
    }
    struct { int abort_flag, pad; unsigned long long cycles; } misc = {0, 0, 0ull};
    TRY(read_progress(h, &misc));
    HIPCHK(hipGetLastError());
    book_ladder(h, (long long)misc.cycles);
    if (misc.abort_flag == 1) {
        // a poll timed out: the seed's workgroups were not all resident.  Nothing was written back (x still holds the start
        // point, the result tables are rewritten from rung 0): this handle takes the three-launch cycle from now on
        h->persist = false;
        *fell_back = true;
        return VA_OK;
    }
    if (misc.abort_flag == 2) return fail(VA_ESTATE, "ladder did not finish within %lld cycles", max_cycles);
    if (*h->h_nactive > 0) return fail(VA_ESTATE, "persistent ladder ended with %d live seeds", *h->h_nactive);
    return VA_OK;
}

template <class T>
int fetch_table(va_handle h, const T *dev, T *host, int nbeta, int per)
{
    if (!host) return VA_OK;
    const Dev &dv = h->dv;
    HIPCHK(hipMemcpy2DAsync(host, sizeof(T) * nbeta * per, dev, sizeof(T) * dv.max_beta * per,
                            sizeof(T) * nbeta * per, dv.dm.B, hipMemcpyDeviceToHost, h->stream));
    return VA_OK;
}

// Why a problem of a module in column-parameter form cannot run that form (the module then has no kernel for it when it has
// more than RHS_BIG_NP parameters): the first reason that applies.
void colp_refusal(const va_problem_desc *d, const ModuleVariant &mv, char *msg, size_t n)
{
    if (const char *flat_only = flat_only_reason(d)) snprintf(msg, n, "%s", flat_only);
    else if (d->D > 64 && (d->D & 1)) snprintf(msg, n, "odd D = %d > 64 (k_eval3, which has no column-parameter form)", d->D);
    else if (d->D > 64 && mv.kernel != 5) snprintf(msg, n, "a non-autonomous model (model time or stimulus) on the streaming kernel k_eval5");
    else if (d->D <= 64 && !tile4_ok(d->D)) snprintf(msg, n, "D = %d fits neither k_eval4 (even D <= 64 filling a wave) nor k_eval5", d->D);
    else if (d->eval_kernel != 0 && d->eval_kernel != mv.kernel) snprintf(msg, n, "eval_kernel = %d (the module carries kernel %d)", d->eval_kernel, mv.kernel);
    else snprintf(msg, n, "the module's column-run instantiation does not fit this problem (weights, discretisation or run length): regenerate it");
}

// The plan of a problem that comes with a generated module.  The module holds ONE instantiation of a column-run kernel
// (va_eval_plan named it when the module was generated): `variant` says whether the problem runs it, with cps shared scalars
// and cpv vector entries when it is of the column-parameter form; a problem that calls for any other geometry runs the
// module's flat kernel.  VA_OK, or the refusal of a problem no kernel of the module carries.
struct ModulePlan {
    EvalPlan plan;
    bool variant = false;
    int cps = 0, cpv = 0;
};
int plan_module(const va_problem_desc *d, const UserRhs &u, ModulePlan &mp)
{
    const ModuleVariant &mv = u.variant;
    // more than RHS_MAX_NP parameters: the flat kernel carries them (their gradient partials in a table of their own), or
    // a column-parameter form, which carries any number: its vectors' partials have a table of their own
    const bool bigp = d->NP > RHS_MAX_NP;
    mp.plan = plan_eval(d, bigp && !mv.column_params() ? mv.flat_form() : mv.form());
    mp.variant = mp.plan.emode != 1 && variant_key(mp.plan, d) == mv.key();
    if (!mp.variant && mp.plan.emode != 1) mp.plan = plan_eval(d, mv.flat_form());
    if (mp.variant && mv.column_params()) { mp.cps = u.colp[0]; mp.cpv = u.colp[1] * d->D; }
    if (d->NP > RHS_BIG_NP && !mp.cpv) {
        char why[192];
        colp_refusal(d, mv, why, sizeof why);
        return fail(VA_EUNSUPPORTED, "%d parameters: only the column-parameter form on k_eval4 / k_eval5 carries more than %d, "
                                     "and this problem cannot run it: %s", d->NP, RHS_BIG_NP, why);
    }
    if (mp.plan.emode == 4 && mp.cpv > mp.plan.g4.XW)       // (k_eval4 leaves the vector partials in the wave's x image)
        return fail(VA_EUNSUPPORTED, "runs of %d rows are too short for %d vector entries on k_eval4", mp.plan.g4.K, mp.cpv);
    return VA_OK;
}

// ---------------------------------------------------------------- creation: the steps of the two constructors

// The front half of both constructors: the device, a handle with its stream, a zeroed device image, the history length
// and ladder capacity (their defaults), the default options.  Leaves h owning the handle, also when it fails.
int begin_create(int device, void *stream, int lbfgs_m, int max_beta, int keep_paths, HandleOwner &h)
{
    const int m = lbfgs_m > 0 ? lbfgs_m : 10;
    if (m > MAX_M) return fail(VA_EINVAL, "lbfgs_m=%d > %d", m, MAX_M);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VA_EINVAL, "device %d of %d", device, ndev);
    HIPCHK(hipSetDevice(device));

    h.reset(new va_problem_s());
    h->dv.s1_rf = -1.0;
    h->device = device; h->keep_paths = keep_paths;
    if (stream) h->stream = (hipStream_t)stream;
    else {
        hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e != hipSuccess) return fail(VA_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
        h->own_stream = true;
    }
    Dev &dv = h->dv;
    memset(&dv, 0, sizeof dv);
    dv.dm.m = m;
    dv.ups = UP_OLD + 4 * m; dv.max_beta = max_beta > 0 ? max_beta : 1; dv.nbeta = 1;
    dv.o.m = m; dv.o.maxiter = 15000; dv.o.maxls = 20; dv.o.maxfun = 15000; dv.o.ftol = 2.2204460492503131e-09; dv.o.gtol = 1e-5;
    return VA_OK;
}

// the padded length of a seed's vector and its chunks, once ND and NPest stand
void set_ld(Dims &dm)
{
    dm.ld = ((dm.ND + dm.NPest + 15) / 16) * 16;
    dm.chunk = VEC_CHUNK; dm.nchunks = (dm.ld + VEC_CHUNK - 1) / VEC_CHUNK;
}

// Step 1 of va_problem_create: every check of the descriptor that needs neither HIP nor the plan, the first that fails
// first.  *user: the registered module the descriptor names (a copy: the registry may grow under another thread), or NULL.
int validate_desc(const va_problem_desc *d, UserRhs &user_copy, const UserRhs **user)
{
    if (d->struct_size != (int32_t)sizeof(va_problem_desc)) return fail(VA_EINVAL, "struct_size %d != %zu", d->struct_size, sizeof(va_problem_desc));
    if (d->batch < 1 || d->D < 1 || d->N_model < 2 || d->N_data < 1 || d->L < 0 || d->merr_nskip < 1)
        return fail(VA_EINVAL, "bad sizes (batch=%d D=%d N_model=%d N_data=%d L=%d nskip=%d)", d->batch, d->D, d->N_model, d->N_data, d->L, d->merr_nskip);
    if ((int64_t)(d->N_data - 1) * d->merr_nskip + 1 != d->N_model)      /* va_ode.py:557 */
        return fail(VA_EINVAL, "N_model (%d) must equal (N_data-1)*merr_nskip+1 (%lld)", d->N_model,
                    (long long)(d->N_data - 1) * d->merr_nskip + 1);
    if (d->disc < VA_DISC_EULER || d->disc > VA_DISC_FORWARDMAP) return fail(VA_EINVAL, "unknown disc %d", d->disc);
    if (d->disc == VA_DISC_SIMPSON_HERMITE && (d->N_model % 2) == 0)
        return fail(VA_EINVAL, "SimpsonHermite needs an odd number of time points (N_model=%d)", d->N_model);
    *user = nullptr;
    if (d->rhs >= VA_RHS_USER_BASE) {
        std::lock_guard<std::mutex> lock(g_user_rhs_mutex);
        if ((size_t)(d->rhs - VA_RHS_USER_BASE) >= g_user_rhs.size()) return fail(VA_EINVAL, "rhs module id %d was never registered", d->rhs);
        user_copy = g_user_rhs[d->rhs - VA_RHS_USER_BASE];
        *user = &user_copy;
        const RhsTable &t = user_copy.table;
        if (t.NP != d->NP || t.D != d->D || t.NSTIM != d->n_stim)
            return fail(VA_EINVAL, "rhs module %s was generated for D=%d NP=%d n_stim=%d, problem has D=%d NP=%d n_stim=%d",
                        user_copy.path.c_str(), t.D, t.NP, t.NSTIM, d->D, d->NP, d->n_stim);
    } else if (d->rhs != VA_RHS_LORENZ96) return fail(VA_EUNSUPPORTED, "unknown built-in rhs %d", d->rhs);
    if (d->rhs == VA_RHS_LORENZ96 && (d->NP != RhsL96::NP || d->D < 4))
        return fail(VA_EINVAL, "Lorenz-96 needs NP=1 and D>=4 (NP=%d D=%d)", d->NP, d->D);
    if (d->n_stim < 0 || (d->n_stim > 0 && !d->stim)) return fail(VA_EINVAL, "n_stim=%d without a stimulus array", d->n_stim);
    // (more than RHS_BIG_NP parameters: a module in column-parameter form only, on k_eval4 / k_eval5 -- plan_module checks the kernel)
    if (d->NP > RHS_BIG_NP && !(*user && !user_copy.colp.empty()))
        return fail(VA_EUNSUPPORTED, "NP=%d > %d: only a generated module in column-parameter form (shared scalars + per-column "
                                     "vectors) carries more, and this model has none", d->NP, RHS_BIG_NP);
    if (d->NPest < 0 || d->NPest > d->NP) return fail(VA_EINVAL, "bad NP/NPest (%d/%d)", d->NP, d->NPest);
    const bool tdp = d->p_time_dependent != 0;
    // more than RHS_MAX_NP parameters: the flat kernel carries them (their gradient partials in a table of their own)
    if (d->NP > RHS_MAX_NP && tdp) return fail(VA_EUNSUPPORTED, "time-dependent parameters: at most %d of them", RHS_MAX_NP);
    if (tdp && d->disc != VA_DISC_TRAPEZOID && d->disc != VA_DISC_SIMPSON_HERMITE)
        return fail(VA_EUNSUPPORTED, "time-dependent parameters: trapezoid and SimpsonHermite only (upstream's euler/forwardmap "
                                     "branches are inconsistent, va_ode.py:345-349)");
    if (tdp && (int64_t)d->N_model * (d->D + d->NPest) > 2000000000LL) return fail(VA_EUNSUPPORTED, "n_var does not fit 32-bit indexing");
    if (!d->Y || (d->L > 0 && !d->Lidx) || !d->P || (d->NPest > 0 && !d->Pidx)) return fail(VA_EINVAL, "null array in desc");
    if ((d->rm_kind && !d->rm_array) || (d->rf_kind && !d->rf0_array)) return fail(VA_EINVAL, "rm/rf array kind without array");
    if ((d->lower != nullptr) != (d->upper != nullptr)) return fail(VA_EINVAL, "lower and upper bounds come together");
    std::vector<char> seen(d->D, 0);
    for (int l = 0; l < d->L; ++l) {
        if (d->Lidx[l] < 0 || d->Lidx[l] >= d->D) return fail(VA_EINVAL, "Lidx[%d]=%d outside [0,D)", l, d->Lidx[l]);
        // any order is fine (data column l pairs with state column Lidx[l], va_ode.py:141); a state
        // column observed twice has no slot in the column -> data-column map the kernels use
        if (seen[d->Lidx[l]] && d->rm_kind != 2) return fail(VA_EUNSUPPORTED, "Lidx lists state column %d twice", d->Lidx[l]);
        seen[d->Lidx[l]] = 1;
    }
    for (int k = 0; k < d->NPest; ++k)
        if (d->Pidx[k] < 0 || d->Pidx[k] >= d->NP) return fail(VA_EINVAL, "Pidx[%d]=%d outside [0,NP)", k, d->Pidx[k]);
    // (begin_create refuses it for both constructors; here it keeps its place ahead of the two checks that follow)
    if (d->lbfgs_m > MAX_M) return fail(VA_EINVAL, "lbfgs_m=%d > %d", d->lbfgs_m, MAX_M);
    if (d->rm_kind < 0 || d->rm_kind > 2) return fail(VA_EINVAL, "rm_kind %d", d->rm_kind);
    if (d->lower) {
        const int nv = tdp ? d->N_model * (d->D + d->NPest) : d->D * d->N_model + d->NPest;
        for (int i = 0; i < nv; ++i)
            if (!(d->lower[i] <= d->upper[i])) return fail(VA_EINVAL, "lower[%d] > upper[%d] (or NaN)", i, i);
    }
    return VA_OK;
}

// Step 2: the evaluation kernel and its geometry (va_eval_geo.h); for a generated module also which of its kernels the
// handle launches and the sizes of its column-parameter form
int plan_problem(va_handle h, const va_problem_desc *d, const UserRhs *user, EvalPlan &plan)
{
    Dev &dv = h->dv;
    h->rhs = d->rhs;
    if (!user) {
        builtin_rhs_table(h->rt);
        builtin_hvp_table(h->rt_hvp);
        EvalForm l96;
        l96.ne = RhsL96s::NE; l96.nb = RhsL96s::NB; l96.ghost = RhsL96g::GHOST; l96.has_reach5 = true;
        l96.reach5[0] = t5_xl<RhsL96s>(); l96.reach5[1] = t5_xr<RhsL96s>(); l96.reach5[2] = t5_gl<RhsL96s>(); l96.reach5[3] = t5_gr<RhsL96s>();
        plan = plan_eval(d, l96);
        return VA_OK;
    }
    ModulePlan mp;
    TRY(plan_module(d, *user, mp));
    plan = mp.plan;
    h->rt = user->table;
    h->rt_hvp = user->hvp;
    if (mp.variant) h->rt.eval = user->table.eval_var;
    dv.dm.lin = user->variant.has_linear;
    dv.cps = mp.cps; dv.cpv = mp.cpv;
    dv.cpnsg = (mp.cpv && plan.emode == 5) ? plan.g5.NSG : 0;
    return VA_OK;
}

// k_eval4's workgroup width and what follows from it: G row groups per workgroup, nwg = ceil(ntiles / G) workgroups per
// seed (nwg <= ntiles, so the 2^32 bound fill_dims checks covers every G)
void set_eval4_groups(Dev &dv, int G)
{
    dv.wg4 = G;
    const int nwg = eval4_nwg(dv);
    dv.nwg_magic = (unsigned)(((1ull << 32) + nwg - 1) / nwg);
}

// Step 3: Dims and the rest of Dev that follow from the descriptor and the plan
int fill_dims(va_handle h, const va_problem_desc *d, const EvalPlan &plan)
{
    Dev &dv = h->dv;
    Dims &dm = dv.dm;
    const bool tdp = d->p_time_dependent != 0;
    dm.D = d->D; dm.N = d->N_model; dm.ND = dm.D * dm.N; dm.L = d->L; dm.N_data = d->N_data;
    dm.nskip = d->merr_nskip; dm.NP = d->NP; dm.NPest = d->NPest; dm.B = d->batch;
    dm.disc = d->disc;
    dm.tdp = tdp ? 1 : 0; dm.NPt = d->NP; dm.NPe = d->NPest;
    dm.bounded = (d->lower && d->upper) ? 1 : 0;
    if (tdp) { dm.ND = dm.N * (dm.D + dm.NPe); dm.NP = 0; dm.NPest = 0; }   // one flat run for the L-BFGS kernels
    set_ld(dm);
    dm.emode = plan.emode; dm.RY = plan.RY; dm.NT = plan.NT; dm.maxr = plan.maxr; dm.T = plan.T; dm.ntiles = plan.ntiles;
    dm.ghost = plan.ghost;
    dv.g4 = plan.g4; dv.g5 = plan.g5;
    if (dm.emode == 4 && (unsigned long long)dm.B * dm.ntiles * dm.ntiles >= (1ull << 32))      // (umulhi by nwg_magic would no longer be an exact division)
        return fail(VA_EUNSUPPORTED, "batch x tiles too large for the wave-private kernel: pass eval_kernel=3");
    h->wg4_plan = dm.emode == 4 ? plan.wg4 : 1;
    set_eval4_groups(dv, EVAL4_WIDE_DEFAULT ? h->wg4_plan : 1);
    // fold the tail into the evaluation kernel while the whole grid is resident at once (<= 8 workgroups per CU)
    h->fold = (long)dm.B * dm.ntiles <= 8L * 256;
    dm.nprow = dm.ntiles;                                                    // one partial row per workgroup (k_eval4: per row group)
    dm.dt = d->dt_model;
    dm.cme = d->L > 0 ? 1.0 / ((double)dm.L * dm.N_data) : 0.0;
    dm.cfe = 1.0 / ((double)dm.D * (dm.N - 1));
    dm.rm = d->rm; dm.rf0 = d->rf0;
    const int npcols = dv.cpv ? dv.cps : d->NP;          // (column-parameter form: the shared scalars only)
    dv.evcols = EP_GP + npcols <= 8 ? 8 : (EP_GP + npcols <= 16 ? 16 : 32);
    // write-through gradient stores pay where the grid is one resident round and the end-of-kernel write-back
    // of 10 MB is on the critical path (C3: -1.3 us); on large grids they cost 10 % (4096 seeds: 446 vs 404 us)
    dv.gaux = h->fold ? 1 : 0;
    return VA_OK;
}

// Step 4: does the tile fit the LDS, and the kernels' opt-in to more than 64 KiB of it (per kernel AND per device: once per handle)
int prepare_kernels(va_handle h)
{
    Dev &dv = h->dv;
    const Dims &dm = dv.dm;
    // the flat kernel keeps 3 staged arrays of (T + halo) rows: up to the CU's 160 KiB
    size_t need = eval_lds_bytes(dv);
    if (dm.emode == 5) { dv.lsrun = 1; need = std::max(need, eval_lds_bytes(dv)); dv.lsrun = 0; }
    const size_t cap = 160 * 1024;
    if (need > cap)
        return fail(VA_EUNSUPPORTED, "a tile of %d rows x D=%d needs %zu B of LDS (> %zu): state too wide for this kernel",
                    dm.T, dm.D, need, cap);
    EvalOp op{true, nullptr, hipSuccess};
    h->rt.eval(dv, op);
    hipError_t e = op.err;
    if (e == hipSuccess && dm.bounded) e = prepare_lbfgsb(dv);
    if (e != hipSuccess) return fail(VA_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(e));
    return VA_OK;
}

// The problem data of an ODE handle between its allocation and its upload: the device buffers, and the host images the
// uploads read.  The uploads are asynchronous copies from this pageable memory, so ONE of these lives in the frame of
// va_problem_create, declared before the first step that fills it, and must not be destroyed, resized or refilled until
// finish_create has synchronised the stream.  It is declared BEFORE the HandleOwner: destruction order is part of the rule,
// since on a failing return it is the owner's va_problem_destroy that synchronises the stream, and that must happen while
// these vectors still exist.  (No helper keeps a staging vector of its own.)
struct OdeData {
    std::vector<double> Ys, rms, rf_fill, lo, hi;
    std::vector<int> lmap, colp_map;
    size_t LY = 0, np_seed = 0, rm_elems = 0;
    bool warr5 = false;        // k_eval5 streams both weight images: scalar weights are spread out into arrays
    int *lmap_d = nullptr, *pidx_d = nullptr, *ystrip_d = nullptr, *lidx_d = nullptr;
    double *Y_d = nullptr, *rm_d = nullptr, *rf_d = nullptr, *P_d = nullptr, *t_d = nullptr, *st_d = nullptr, *lo_d = nullptr, *hi_d = nullptr;
};

// Step 5a: the device buffers of the problem data (zero-filled on the stream, ahead of the uploads into them)
int alloc_problem_data(va_handle h, const va_problem_desc *d, const EvalPlan &plan, OdeData &o)
{
    Dev &dv = h->dv;
    Dims &dm = dv.dm;
    const size_t B = dm.B;
    TRY(h->alloc(&o.lmap_d, dm.D));
    // (two rows + a line of padding: the streaming kernel stages observation rows by whole 16-byte pieces, two rows at a time)
    const size_t LY = dm.emode == 5 ? (size_t)dv.g5.LY : (size_t)dm.L;        // row pitch of Y (and of the RM image of k_eval5) on the device
    o.LY = LY;
    TRY(h->alloc(&o.Y_d, (size_t)dm.N_data * LY + 4 * LY + 16));   // (k_eval5 stages row pairs: one pair before the first row, one past the last)
    o.Y_d += 2 * (LY / 2) + (LY & 1) * 2;                   // an even number of doubles >= L: the data keep their 16-byte alignment
    if (dm.emode == 5) TRY(h->alloc(&o.ystrip_d, plan.ystrip.size()));
    o.np_seed = dm.tdp ? (size_t)dm.N * dm.NPt : (size_t)dm.NPt;       // parameters stored per seed
    TRY(h->alloc(&o.pidx_d, dm.NPe));
    TRY(h->alloc(&o.P_d, B * o.np_seed));
    o.rm_elems = (size_t)dm.N_data * dm.L * (d->rm_kind == 2 ? dm.L : 1);
    o.warr5 = dm.emode == 5 && dv.g5.warr;
    if (o.warr5) {
        // (as Y: one row pair in front and behind; L is even on this path)
        TRY(h->alloc(&o.rm_d, (size_t)dm.N_data * LY + 4 * LY + 16));
        o.rm_d += LY;
    } else if (d->rm_kind) TRY(h->alloc(&o.rm_d, o.rm_elems));
    if (d->rm_kind == 2) TRY(h->alloc(&o.lidx_d, dm.L));
    if (o.warr5) {
        TRY(h->alloc(&o.rf_d, (size_t)(dm.N + 3) * dm.D + 16));
        o.rf_d += dm.D;
    } else if (d->rf_kind) TRY(h->alloc(&o.rf_d, (size_t)(dm.N - 1) * dm.D * (d->rf_kind == 2 ? dm.D : 1)));
    if (dm.bounded) {
        const int nv = dm.ND + dm.NPest;
        o.lo.assign(dm.ld, -HUGE_VAL); o.hi.assign(dm.ld, HUGE_VAL);
        for (int i = 0; i < nv; ++i) { o.lo[i] = d->lower[i]; o.hi[i] = d->upper[i]; }
        bool boxed = true;
        for (int i = 0; i < nv; ++i) boxed = boxed && o.lo[i] > -HUGE_VAL && o.hi[i] < HUGE_VAL;
        if (boxed) dm.bounded |= 2;
        TRY(h->alloc(&o.lo_d, (size_t)dm.ld)); TRY(h->alloc(&o.hi_d, (size_t)dm.ld));
    }
    if (d->t_model) TRY(h->alloc(&o.t_d, (size_t)dm.N));
    if (d->n_stim > 0) TRY(h->alloc(&o.st_d, (size_t)dm.N * d->n_stim));
    return VA_OK;
}

// Step 5b: stage the problem data in o and upload it.
// On the device Lidx is ascending: data column l pairs with state column Lidx[l] in any order
// (va_ode.py:141), so sorting Lidx and permuting the columns of Y (and of a weight array) the same
// way changes nothing, and the kernels of narrow states find a column's data by counting the
// observed columns below it (obsmask) instead of loading a map.
int upload_problem_data(va_handle h, const va_problem_desc *d, const UserRhs *user, const EvalPlan &plan, OdeData &o)
{
    Dev &dv = h->dv;
    Dims &dm = dv.dm;
    const size_t B = dm.B, LY = o.LY;
    std::vector<int> perm(dm.L), lidx_sorted(dm.L);
    for (int l = 0; l < dm.L; ++l) perm[l] = l;
    if (d->rm_kind != 2) std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return d->Lidx[a] < d->Lidx[b]; });
    for (int l = 0; l < dm.L; ++l) lidx_sorted[l] = d->Lidx[perm[l]];
    h->lidx_user.assign(d->Lidx, d->Lidx + dm.L);
    o.Ys.assign((size_t)dm.N_data * LY, 0.0);
    for (int n = 0; n < dm.N_data; ++n)
        for (int l = 0; l < dm.L; ++l) o.Ys[(size_t)n * LY + l] = d->Y[(size_t)n * dm.L + perm[l]];
    if (o.warr5 && d->rm_kind == 0) o.rms.assign((size_t)dm.N_data * LY, d->rm);
    if (d->rm_kind == 1) {
        o.rms.assign((size_t)dm.N_data * LY, 0.0);
        for (int n = 0; n < dm.N_data; ++n)
            for (int l = 0; l < dm.L; ++l) o.rms[(size_t)n * LY + l] = d->rm_array[(size_t)n * dm.L + perm[l]];
    }
    o.lmap.assign(dm.D, -1);
    for (int l = 0; l < dm.L; ++l) o.lmap[lidx_sorted[l]] = l;
    dm.obsmask = 0ull;
    if (dm.D <= 64) for (int l = 0; l < dm.L; ++l) dm.obsmask |= 1ull << lidx_sorted[l];
    TRY(UPLOAD(o.lmap_d, o.lmap.data(), dm.D));
    if (dm.emode == 5) { TRY(UPLOAD(o.ystrip_d, plan.ystrip.data(), plan.ystrip.size())); dv.ystrip = o.ystrip_d; }
    TRY(UPLOAD(o.Y_d, o.Ys.data(), (size_t)dm.N_data * LY));
    if (dm.NPe) TRY(UPLOAD(o.pidx_d, d->Pidx, dm.NPe));
    TRY(UPLOAD(o.P_d, d->P, B * o.np_seed));
    if (d->rm_kind || o.warr5) TRY(UPLOAD(o.rm_d, d->rm_kind != 2 ? o.rms.data() : d->rm_array, d->rm_kind != 2 ? o.rms.size() : o.rm_elems));
    if (d->rm_kind == 2) TRY(UPLOAD(o.lidx_d, d->Lidx, dm.L));
    if (o.warr5 && d->rf_kind == 0) o.rf_fill.assign((size_t)(dm.N - 1) * dm.D, d->rf0);
    if (d->rf_kind || o.warr5) TRY(UPLOAD(o.rf_d, d->rf_kind ? d->rf0_array : o.rf_fill.data(), (size_t)(dm.N - 1) * dm.D * (d->rf_kind == 2 ? dm.D : 1)));
    if (dm.bounded) { TRY(UPLOAD(o.lo_d, o.lo.data(), (size_t)dm.ld)); TRY(UPLOAD(o.hi_d, o.hi.data(), (size_t)dm.ld)); }
    dv.pp.lo = o.lo_d; dv.pp.hi = o.hi_d;
    if (d->t_model) TRY(UPLOAD(o.t_d, d->t_model, (size_t)dm.N));
    if (d->n_stim > 0) TRY(UPLOAD(o.st_d, d->stim, (size_t)dm.N * d->n_stim));
    dv.pp.lmap = o.lmap_d; dv.pp.Y = o.Y_d; dv.pp.rf0_arr = (d->rf_kind == 1 || o.warr5) ? o.rf_d : nullptr;
    dv.pp.rf0_full = d->rf_kind == 2 ? o.rf_d : nullptr;
    dv.pp.rm_arr = (d->rm_kind == 1 || o.warr5) ? o.rm_d : nullptr;
    dv.pp.rm_full = d->rm_kind == 2 ? o.rm_d : nullptr; dv.pp.Lidx = o.lidx_d;
    dv.pp.Pidx = o.pidx_d; dv.pp.Pfull = o.P_d;
    if (dv.cpv) {
        // column-parameter form: each shared scalar / vector entry -> its global index, then its index in p_est or -1
        const int NT = dv.cps + dv.cpv;
        std::vector<int> pest(d->NP, -1);
        o.colp_map.assign(2 * (size_t)NT, 0);
        for (int k = 0; k < d->NPest; ++k) pest[d->Pidx[k]] = k;
        for (int j = 0; j < NT; ++j) { o.colp_map[j] = user->colp[2 + j]; o.colp_map[NT + j] = pest[o.colp_map[j]]; }
        int *cm_d = nullptr;
        TRY(h->alloc(&cm_d, o.colp_map.size()));
        TRY(UPLOAD(cm_d, o.colp_map.data(), o.colp_map.size()));
        dv.cpmap = cm_d;
    }
    dv.pp.tmodel = o.t_d; dv.pp.stim = o.st_d; dv.pp.nstim = d->n_stim;
    return VA_OK;
}

// Step 6: few seeds, short paths: can the whole minimisation live in LDS?  (flat tile phases: any right-hand side, any
// discretisation, weight arrays, merr_nskip, full weight matrices; not bounds, time-dependent parameters, a dense
// linear part, more than RHS_MAX_NP parameters, or the padded observation rows of the streaming kernel)
int choose_persist(va_handle h, const va_problem_desc *d)
{
    Dev &dv = h->dv;
    const Dims &dm = dv.dm;
    const size_t B = dm.B;
    if (dm.bounded || dm.tdp || dm.lin || d->NP > RHS_MAX_NP || dm.emode == 5 || !h->rt.seed) return VA_OK;
    int G = 0, T = 0, ncu = 0;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, d->device));
    h->pz_maxG = ncu / (int)B;
    if (h->pz_maxG < 1 || !persist_geometry(dm.N, dm.D, dm.L, dm.NP, dm.NPest, dm.m, dm.disc, PZ_LDS_BYTES, h->pz_maxG, 0, &G, &T)) return VA_OK;
    Dev dvp = dv;
    dvp.dm.T = T; dvp.dm.ntiles = G;
    EvalOp op{true, nullptr, hipSuccess};
    h->rt.seed(dvp, op);
    if (op.err != hipSuccess) { (void)hipGetLastError(); return VA_OK; }
    h->persist = true; h->pz_G = G; h->pz_T = T;
    // (sized for the most workgroups a seed may get: va_problem_tune may choose other slices)
    const size_t units = B * 2 * (size_t)h->pz_maxG * (size_t)pz_row_granules(dm.D) * 2;     // 8-byte units: 16 per granule pair
    TRY(h->alloc(&dv.pz.xch, units));
    h->pz_xch_bytes = units * 8;
    unsigned long long *misc = nullptr;
    TRY(h->alloc(&misc, 2 + PZ_NSTAMP));
    h->pz_misc = misc;
    dv.pz.abort_flag = (int *)misc; dv.pz.cycles = misc + 1; dv.pz.stamps = (double *)(misc + 2);
    return VA_OK;
}

// CUs of a device, or 256 where it cannot be asked (a device that does not exist is refused by begin_create, after the
// descriptor's own checks)
int cu_count(int device)
{
    int ncu = 256;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) { (void)hipGetLastError(); ncu = 256; }
    return ncu;
}

// Dims and NnetDev of a network handle, from the descriptor and its plan
void fill_nnet_dims(va_handle h, const va_nnet_desc *d, const NnetPlan &p)
{
    Dev &dv = h->dv;
    NnetDev &nn = h->nn;
    memset(&nn, 0, sizeof nn);
    Dims &dm = dv.dm;
    // to the L-BFGS kernels the unknown vector is one flat run of ND doubles with no tail
    dm.D = p.NDnet; dm.N = d->M; dm.ND = (int)p.nvar; dm.NP = 0; dm.NPest = 0; dm.B = d->batch;
    dm.L = d->L_in + d->L_out; dm.N_data = d->M; dm.nskip = 1; dm.disc = VA_DISC_FORWARDMAP;
    set_ld(dm);
    dm.cme = 1.0 / ((double)(d->L_in + d->L_out) * d->M);                 /* va_nnet.py:173 */
    dm.cfe = d->rf0 / ((double)(p.NDnet - p.s[0]) * d->M);                /* va_nnet.py:255 */
    dm.rm = d->rm_in; dm.rf0 = d->rf0;
    dv.evcols = 8;                 // the network kernels fill EP_ME .. EP_GMAX only
    dm.nprow = p.nprow;
    dm.ntiles = dm.nprow; dm.T = NN_TILE; dm.emode = 0;

    nn.NL = d->n_layers; nn.M = d->M; nn.NDnet = p.NDnet; nn.NDens = p.NDnet * d->M; nn.NP = d->NP; nn.NPest = d->NPest;
    nn.act = d->activation; nn.Lin = d->L_in; nn.Lout = d->L_out; nn.rm_in = d->rm_in; nn.rm_out = d->rm_out;
    nn.mch = p.mch; nn.nmch = p.nmch;
    nn.n0 = p.n0; nn.n1 = p.n1; nn.n2 = p.n2; nn.n3 = p.n3; nn.n4 = p.n4; nn.nraw = p.nraw;
    nn.small = p.small;
    nn.nfb = p.nfb; nn.wfsz = p.wfsz; nn.fb_slots = p.fb_slots; nn.fused = p.fused;
}

// The device image of a network: its buffers, then the solver state, then the uploads.  The uploads read the plan's
// vectors and the caller's arrays: p lives in the frame of va_nnet_problem_create until finish_create has synchronised.
int create_nnet_image(va_handle h, const va_nnet_desc *d, const NnetPlan &p)
{
    Dev &dv = h->dv;
    NnetDev &nn = h->nn;
    const Dims &dm = dv.dm;
    const int NL = d->n_layers;
    const size_t B = dm.B;
    int *s_d = nullptr, *off_d = nullptr, *woff_d = nullptr, *boff_d = nullptr, *lin_d = nullptr, *lout_d = nullptr, *pmap_d = nullptr;
    double *din_d = nullptr, *dout_d = nullptr, *P_d = nullptr;
    NnetTile *t1_d = nullptr, *t2_d = nullptr, *t3_d = nullptr;
    TRY(h->alloc(&s_d, NL)); TRY(h->alloc(&off_d, NL + 1)); TRY(h->alloc(&woff_d, NL - 1)); TRY(h->alloc(&boff_d, NL - 1));
    TRY(h->alloc(&lin_d, p.s[0])); TRY(h->alloc(&lout_d, p.s[NL - 1])); TRY(h->alloc(&pmap_d, d->NP));
    TRY(h->alloc(&din_d, (size_t)d->M * d->L_in)); TRY(h->alloc(&dout_d, (size_t)d->M * d->L_out));
    TRY(h->alloc(&P_d, B * d->NP)); TRY(h->alloc(&nn.Pw, B * d->NP));
    TRY(h->alloc(&nn.delta, B * dm.ld));
    TRY(h->alloc(&nn.Xw, B * dm.ld));
    if (p.fold_rows) TRY(h->alloc(&nn.raw, B * nn.nraw * EP_GP));
    TRY(h->alloc(&nn.gpart, B * nn.nmch * (size_t)d->NP));
    int *wfoff_d = nullptr;
    if (p.fb_ok) {
        TRY(h->alloc(&nn.Wf, B * (size_t)nn.wfsz));
        TRY(h->alloc(&wfoff_d, 2 * (NL - 1)));
        TRY(h->alloc(&dv.pz.stamps, (size_t)PZ_NSTAMP));       // (measurement builds of k_nnet_fb: va_measure.h)
        TRY(h->alloc(&nn.fb_cu, (size_t)16));
    }
    TRY(h->alloc(&t1_d, p.t1.size())); TRY(h->alloc(&t2_d, p.t2.size())); TRY(h->alloc(&t3_d, p.t3.size()));
    TRY(alloc_solver_state(h));
    TRY(UPLOAD(s_d, p.s.data(), NL)); TRY(UPLOAD(off_d, p.off.data(), NL + 1));
    TRY(UPLOAD(woff_d, p.woff.data(), NL - 1)); TRY(UPLOAD(boff_d, p.boff.data(), NL - 1));
    TRY(UPLOAD(lin_d, p.lin.data(), p.s[0])); TRY(UPLOAD(lout_d, p.lout.data(), p.s[NL - 1])); TRY(UPLOAD(pmap_d, p.pmap.data(), d->NP));
    if (d->L_in) TRY(UPLOAD(din_d, d->data_in, (size_t)d->M * d->L_in));
    if (d->L_out) TRY(UPLOAD(dout_d, d->data_out, (size_t)d->M * d->L_out));
    TRY(UPLOAD(P_d, d->P, B * d->NP));
    if (p.fb_ok) { TRY(UPLOAD(wfoff_d, p.wfoff.data(), 2 * (NL - 1))); nn.wfoff = wfoff_d; }
    TRY(UPLOAD(t1_d, p.t1.data(), p.t1.size())); TRY(UPLOAD(t2_d, p.t2.data(), p.t2.size()));
    if (!p.t3.empty()) TRY(UPLOAD(t3_d, p.t3.data(), p.t3.size()));
    nn.s = s_d; nn.off = off_d; nn.woff = woff_d; nn.boff = boff_d; nn.lmap_in = lin_d; nn.lmap_out = lout_d;
    nn.pmap = pmap_d; nn.din = din_d; nn.dout = dout_d; nn.Pfix = P_d; nn.t1 = t1_d; nn.t2 = t2_d; nn.t3 = t3_d;
    if (d->rm_in_matrix) {
        // full measurement matrices (va_nnet.py:136-139): the kernels walk the layer's observed neurons
        double *ri = nullptr, *ro = nullptr; int *li = nullptr, *lo = nullptr;
        TRY(h->alloc(&ri, (size_t)d->L_in * d->L_in + 1)); TRY(h->alloc(&ro, (size_t)d->L_out * d->L_out + 1));
        TRY(h->alloc(&li, d->L_in + 1)); TRY(h->alloc(&lo, d->L_out + 1));
        if (d->L_in) { TRY(UPLOAD(ri, d->rm_in_matrix, (size_t)d->L_in * d->L_in)); TRY(UPLOAD(li, d->Lidx_in, d->L_in)); }
        if (d->L_out) { TRY(UPLOAD(ro, d->rm_out_matrix, (size_t)d->L_out * d->L_out)); TRY(UPLOAD(lo, d->Lidx_out, d->L_out)); }
        nn.rmm_in = ri; nn.rmm_out = ro; nn.lidx_in = li; nn.lidx_out = lo;
    }
    if (p.fb_ok) {
        const hipError_t e = prepare_nnet_fb(nn, h->nn_act);
        if (e != hipSuccess) { (void)hipGetLastError(); nn.Wf = nullptr; }      // (the tune knob then refuses)
    }
    return VA_OK;
}

}  // namespace

extern "C" {

int32_t va_abi_version(void) { return VA_ABI_VERSION; }
const char *va_last_error(void) { return g_err.c_str(); }

int va_device_count(int32_t *count)
{
    if (!count) return fail(VA_EINVAL, "count is NULL");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    *count = n;
    return VA_OK;
}

int va_eval_plan_reach(const va_problem_desc *d, int32_t ne, int32_t ghost, const int32_t *reach, int32_t *out)
{
    if (!d || !out) return fail(VA_EINVAL, "null argument");
    if (d->struct_size != (int32_t)sizeof(va_problem_desc)) return fail(VA_EINVAL, "struct_size %d != %zu", d->struct_size, sizeof(va_problem_desc));
    out[0] = out[1] = out[2] = out[3] = 0;
    if ((ne <= 0 && ghost <= 0) || d->D < 1 || d->N_model < 2 || d->batch < 1) return VA_OK;
    if (d->L > 0 && !d->Lidx) return fail(VA_EINVAL, "Lidx is NULL");
    EvalForm form;
    form.ne = ne; form.ghost = ghost; form.has_reach5 = reach != nullptr;
    if (reach) for (int k = 0; k < 4; ++k) form.reach5[k] = reach[k];
    const VariantKey key = variant_key(plan_eval(d, form), d);
    out[0] = key.kernel; out[1] = key.disc; out[2] = key.K; out[3] = key.W;
    return VA_OK;
}

int va_eval_plan(const va_problem_desc *d, int32_t ne, int32_t ghost, int32_t *out)
{
    return va_eval_plan_reach(d, ne, ghost, nullptr, out);
}

int va_rhs_load_module(const char *path, int32_t *rhs_id)
{
    if (!path || !rhs_id) return fail(VA_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(g_user_rhs_mutex);
    for (size_t i = 0; i < g_user_rhs.size(); ++i)
        if (g_user_rhs[i].path == path) { *rhs_id = VA_RHS_USER_BASE + (int32_t)i; return VA_OK; }
    UserRhs u;
    u.path = path;
    u.dl = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!u.dl) return fail(VA_EINVAL, "dlopen(%s): %s", path, dlerror());
    typedef void (*info_fn)(int *);
    typedef int (*table_fn)(RhsTable *, int);
    table_fn table = (table_fn)dlsym(u.dl, "va_user_rhs_table");
    if (!table) { dlclose(u.dl); return fail(VA_EINVAL, "%s lacks va_user_rhs_table", path); }
    RhsTable &t = u.table;
    const int table_bytes = table(&t, (int)sizeof(RhsTable));         // (fills t only when the sizes agree)
    if (table_bytes != (int)sizeof(RhsTable) || t.dev_bytes != (int)sizeof(Dev) || t.seed_bytes != (int)sizeof(SeedState)
        || t.predict_bytes != (int)sizeof(PredictArgs)) {
        dlclose(u.dl);
        return fail(VA_EINVAL, "%s was built against different headers (table %d vs %zu bytes, Dev %d vs %zu bytes): rebuild it", path,
                    table_bytes, sizeof(RhsTable), t.dev_bytes, sizeof(Dev));
    }
    typedef int (*hvp_fn)(HvpTable *, int);
    if (hvp_fn hv = (hvp_fn)dlsym(u.dl, "va_user_hvp_table")) {
        const int hb = hv(&u.hvp, (int)sizeof(HvpTable));
        if (hb != (int)sizeof(HvpTable) || u.hvp.hvp_bytes != (int)sizeof(HvpArgs) || u.hvp.tlm_bytes != (int)sizeof(PredictTlmArgs)
            || u.hvp.lyap_bytes != (int)sizeof(LyapArgs) || u.hvp.adj_bytes != (int)sizeof(PredictAdjArgs)
            || u.hvp.shoot_bytes != (int)sizeof(ShootArgs) || u.hvp.enkf_bytes != (int)sizeof(EnkfArgs)
            || u.hvp.shoot_box_bytes != (int)sizeof(ShootBoxArgs)) {
            dlclose(u.dl);
            return fail(VA_EINVAL, "%s was built against different headers (HvpTable %d vs %zu bytes): rebuild it", path, hb, sizeof(HvpTable));
        }
    }
    if (info_fn vinfo = (info_fn)dlsym(u.dl, "va_user_variant_info")) {
        int uv[UV_N];
        vinfo(uv);
        u.variant = ModuleVariant::decode(uv);
        if (!t.eval_var) u.variant.kernel = 0;
        typedef int (*nb_fn)(void);
        if (nb_fn nb = (nb_fn)dlsym(u.dl, "va_user_col_neighbours")) u.variant.nb = nb();
    }
    if (info_fn cmap = (info_fn)dlsym(u.dl, "va_user_colp_map")) {
        // (S <= RHS_MAX_NP and V <= CP_VMAX by construction: the generator checks both)
        u.colp.assign(2 + RHS_MAX_NP + (size_t)CP_VMAX * (t.D > 0 ? t.D : 1), 0);
        cmap(u.colp.data());
        u.colp.resize(2 + (size_t)u.colp[0] + (size_t)u.colp[1] * t.D);
    }
    if (u.colp.empty()) u.variant.n_colp_vectors = 0;
    // past RHS_BIG_NP parameters a module has no flat kernel: it must carry the column-parameter form (the kernels that
    // run it are checked problem by problem, va_problem_create)
    if (t.NP < 0 || (t.NP > RHS_BIG_NP && u.colp.empty())) {
        dlclose(u.dl);
        return fail(VA_EUNSUPPORTED, "%s: NP=%d > %d and no column-parameter form", path, t.NP, RHS_BIG_NP);
    }
    g_user_rhs.push_back(u);
    *rhs_id = VA_RHS_USER_BASE + (int32_t)g_user_rhs.size() - 1;
    return VA_OK;
}

int va_act_load_module(const char *path, int32_t *act_id)
{
    if (!path || !act_id) return fail(VA_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(g_user_rhs_mutex);
    for (size_t i = 0; i < g_user_act.size(); ++i)
        if (g_user_act[i].path == path) { *act_id = VA_ACT_USER_BASE + (int32_t)i; return VA_OK; }
    UserAct u;
    u.path = path;
    u.dl = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!u.dl) return fail(VA_EINVAL, "dlopen(%s): %s", path, dlerror());
    typedef void (*info_fn)(int *);
    info_fn info = (info_fn)dlsym(u.dl, "va_user_act_info");
    u.launch = (NnetActLaunch)dlsym(u.dl, "va_user_act_launch");
    if (!info || !u.launch) { dlclose(u.dl); return fail(VA_EINVAL, "%s lacks va_user_act_info / va_user_act_launch", path); }
    int ai[3] = {0, 0, 0};                 // (sizeof(Dev), sizeof(NnetDev), sizeof(SeedState))
    info(ai);
    if (ai[0] != (int)sizeof(Dev) || ai[1] != (int)sizeof(NnetDev) || ai[2] != (int)sizeof(SeedState)) {
        dlclose(u.dl);
        return fail(VA_EINVAL, "%s was built against different headers: rebuild it", path);
    }
    g_user_act.push_back(u);
    *act_id = VA_ACT_USER_BASE + (int32_t)g_user_act.size() - 1;
    return VA_OK;
}

int va_problem_create(const va_problem_desc *d, va_handle *out)
{
    if (!d || !out) return fail(VA_EINVAL, "null argument");
    *out = nullptr;
    UserRhs user_copy;
    const UserRhs *user = nullptr;
    TRY(validate_desc(d, user_copy, &user));
    // declared AHEAD of the owner: locals die in reverse order, so on a failing return the owner's va_problem_destroy
    // synchronises the stream while the memory the queued uploads read is still there
    EvalPlan plan;       // (its observation strips are uploaded: it lives as long as the staging below)
    OdeData data;        // device buffers and host staging: alive until finish_create has synchronised the stream
    HandleOwner h;
    TRY(begin_create(d->device, d->stream, d->lbfgs_m, d->max_beta, d->keep_paths, h));
    TRY(plan_problem(h.get(), d, user, plan));
    TRY(fill_dims(h.get(), d, plan));
    TRY(prepare_kernels(h.get()));
    TRY(alloc_problem_data(h.get(), d, plan, data));
    TRY(alloc_solver_state(h.get()));         // (reads dv.cpv / dv.cps: after plan_problem)
    TRY(upload_problem_data(h.get(), d, user, plan, data));
    TRY(choose_persist(h.get(), d));
    TRY(finish_create(h.get()));
    *out = h.release();
    return VA_OK;
}

int va_nnet_problem_create(const va_nnet_desc *d, va_handle *out)
{
    if (!d || !out) return fail(VA_EINVAL, "null argument");
    *out = nullptr;
    if (d->struct_size != (int32_t)sizeof(va_nnet_desc)) return fail(VA_EINVAL, "struct_size %d != %zu", d->struct_size, sizeof(va_nnet_desc));
    if (d->batch < 1 || d->n_layers < 2 || d->M < 1 || !d->structure) return fail(VA_EINVAL, "bad sizes (batch=%d n_layers=%d M=%d)", d->batch, d->n_layers, d->M);
    if ((d->rm_in_matrix != nullptr) != (d->rm_out_matrix != nullptr)) return fail(VA_EINVAL, "rm_in_matrix and rm_out_matrix come together");
    NnetActLaunch user_act = nullptr;
    if (d->activation >= VA_ACT_USER_BASE) {
        std::lock_guard<std::mutex> lock(g_user_rhs_mutex);
        if ((size_t)(d->activation - VA_ACT_USER_BASE) >= g_user_act.size()) return fail(VA_EINVAL, "activation module id %d was never registered", d->activation);
        user_act = g_user_act[d->activation - VA_ACT_USER_BASE].launch;
    } else if (d->activation < VA_ACT_SIGMOID || d->activation > VA_ACT_SOFTPLUS) return fail(VA_EUNSUPPORTED, "unknown activation %d", d->activation);
    NnetPlan plan;       // (its tables are uploaded: alive until finish_create has synchronised the stream, or, on a failing
                         // return, until the owner declared after it has destroyed the handle)
    const char *why = "";
    if (int rc = plan_nnet(d, cu_count(d->device), plan, &why)) return fail(rc, "%s", why);
    HandleOwner h;
    TRY(begin_create(d->device, d->stream, d->lbfgs_m, d->max_beta, d->keep_paths, h));
    h->rhs = -1; h->is_nnet = true; h->nn_act = user_act;
    fill_nnet_dims(h.get(), d, plan);
    TRY(create_nnet_image(h.get(), d, plan));
    TRY(finish_create(h.get()));
    *out = h.release();
    return VA_OK;
}

void va_problem_destroy(va_handle h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->timed_gexec) (void)hipGraphExecDestroy(h->timed_gexec);
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->h_nactive) (void)hipHostFree(h->h_nactive);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int va_problem_info(va_handle h, int64_t *n_var, int64_t *ld_internal, int32_t *tile_rows, int32_t *ntiles)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (n_var) *n_var = h->dv.dm.ND + h->dv.dm.NPest;
    if (ld_internal) *ld_internal = h->dv.dm.ld;
    if (tile_rows) *tile_rows = h->dv.dm.T;
    if (ntiles) *ntiles = h->dv.dm.ntiles;
    return VA_OK;
}

int va_problem_eval_grid(va_handle h, int32_t *row_groups_per_workgroup, int32_t *workgroups)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    const bool e4 = !h->is_nnet && h->dv.dm.emode == 4;
    if (row_groups_per_workgroup) *row_groups_per_workgroup = e4 ? eval4_groups(h->dv) : 1;
    if (workgroups) *workgroups = h->is_nnet ? 0 : h->dv.dm.B * (e4 ? eval4_nwg(h->dv) : h->dv.dm.ntiles);
    return VA_OK;
}

int va_problem_eval_kernel(va_handle h, int32_t *eval_kernel, int32_t *run_rows)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (eval_kernel) *eval_kernel = h->is_nnet ? 0 : h->dv.dm.emode;
    if (run_rows) *run_rows = h->is_nnet ? 0 : h->dv.dm.maxr;
    return VA_OK;
}

int va_problem_persistent(va_handle h, int32_t *workgroups_per_seed, int32_t *rows_per_workgroup)
{
    if (!h) return 0;
    const bool on = h->persist && h->tune_persist;
    if (workgroups_per_seed) *workgroups_per_seed = on ? h->pz_G : 0;
    if (rows_per_workgroup) *rows_per_workgroup = on ? h->pz_T : 0;
    return on ? 1 : 0;
}

int va_action_grad(va_handle h, const double *XP, int64_t ld, int32_t mem, double rf_scale,
                   double *A, double *me, double *fe, double *grad, int64_t ldg)
{
    int rc = check_xp(h, XP, ld, mem);
    if (rc) return rc;
    if (!A || !me || !fe) return fail(VA_EINVAL, "A/me/fe must not be NULL");
    if (grad && ldg < h->dv.dm.ND + h->dv.dm.NPest) return fail(VA_EINVAL, "ldg < n_var");
    HIPCHK(hipSetDevice(h->device));
    Dev &dv = h->dv;
    if ((rc = copy_in(h, XP, ld, mem))) return rc;
    launch_init_states(dv, PH_START, rf_scale, h->stream);
    h->timed_armed_rf = rf_scale;
    run_eval(h, EPI_FINALIZE);
    const hipMemcpyKind k = mem == VA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(A, dv.outA, sizeof(double) * dv.dm.B, k, h->stream));
    HIPCHK(hipMemcpyAsync(me, dv.outme, sizeof(double) * dv.dm.B, k, h->stream));
    HIPCHK(hipMemcpyAsync(fe, dv.outfe, sizeof(double) * dv.dm.B, k, h->stream));
    if (grad && (rc = copy_out(h, dv.gt, grad, ldg, mem))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    h->n_eval_launch += 1; h->n_seed_evals += dv.dm.B; h->n_seed_evals_direct += dv.dm.B;
    return VA_OK;
}

int va_anneal(va_handle h, double *XP, int64_t ld, int32_t mem, const double *rf_scale, int32_t nbeta,
              const va_lbfgs_opts *opts, double *ame, double *pest, int32_t *status, int32_t *nit,
              int64_t *nfev, double *minpaths)
{
    int rc = check_xp(h, XP, ld, mem);
    if (rc) return rc;
    if (!rf_scale) return fail(VA_EINVAL, "rf_scale is NULL");
    if (minpaths && !h->dv.minpaths) return fail(VA_ESTATE, "minpaths requested but the problem was created with keep_paths=0");
    if ((rc = set_opts(h, opts))) return rc;
    HIPCHK(hipSetDevice(h->device));
    Dev &dv = h->dv;
    if ((rc = copy_in(h, XP, ld, mem))) return rc;
    if ((rc = run_ladder(h, rf_scale, nbeta))) return rc;
    if ((rc = copy_out(h, dv.x, XP, ld, mem))) return rc;
    if ((rc = fetch_table(h, dv.ame, ame, nbeta, 3))) return rc;
    if (dv.dm.NPest && (rc = fetch_table(h, dv.pest, pest, nbeta, dv.dm.NPest))) return rc;
    if ((rc = fetch_table(h, dv.status, status, nbeta, 1))) return rc;
    if ((rc = fetch_table(h, dv.nit, nit, nbeta, 1))) return rc;
    if ((rc = fetch_table(h, (const int64_t *)dv.nfev, nfev, nbeta, 1))) return rc;
    if ((rc = fetch_table(h, dv.minpaths, minpaths, nbeta, dv.dm.ND + dv.dm.NP))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return VA_OK;
}

int va_minimize_lbfgs(va_handle h, double *XP, int64_t ld, int32_t mem, double rf_scale,
                      const va_lbfgs_opts *opts, double *Amin, double *me, double *fe,
                      int32_t *status, int32_t *nit, int64_t *nfev)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    const int B = h->dv.dm.B;
    std::vector<double> ame((size_t)B * 3);
    int rc = va_anneal(h, XP, ld, mem, &rf_scale, 1, opts, ame.data(), nullptr, status, nit, nfev, nullptr);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        if (Amin) Amin[b] = ame[3 * b];
        if (me) me[b] = ame[3 * b + 1];
        if (fe) fe[b] = ame[3 * b + 2];
    }
    return VA_OK;
}

// Forecast: T trajectories of the handle's model from x0 with the parameters p, classical RK4 (va_predict.h).  Works on
// buffers of its own: the handle's resident paths, seed states and captured graphs are not touched.
int va_predict(va_handle h, const double *x0, const double *p, int32_t T, double t0, int32_t n_steps, int32_t substeps,
               int32_t every, const double *stim, double *out)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!x0 || !p || !out) return fail(VA_EINVAL, "x0 / p / out must not be NULL");
    if (T < 1 || n_steps < 1 || substeps < 1 || every < 1)
        return fail(VA_EINVAL, "T, n_steps, substeps and every must be at least 1 (T=%d n_steps=%d substeps=%d every=%d)", T, n_steps, substeps, every);
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "a network handle has no differential equation to integrate");
    const Dims &dm = h->dv.dm;
    const int nstim = h->dv.pp.nstim;
    if (nstim > 0 && !stim) return fail(VA_EINVAL, "the model takes a stimulus of %d column(s): pass its %d rows from t0 on", nstim, n_steps + 1);
    if (nstim == 0 && stim) return fail(VA_EINVAL, "the model takes no stimulus, but one was passed");
    if (!h->rt.predict)
        return fail(VA_EUNSUPPORTED, "the model has no flat form f(x, i, p) for the integrator to call (more than %d parameters: "
                                     "its module carries the column-parameter form only)", RHS_BIG_NP);
    if ((int64_t)n_steps * substeps > 2000000000LL) return fail(VA_EUNSUPPORTED, "n_steps x substeps does not fit 32-bit indexing");
    PredictArgs a;
    a.T = T; a.D = dm.D; a.NP = dm.NPt; a.nstim = nstim; a.n_steps = n_steps; a.substeps = substeps; a.every = every;
    a.n_out = n_steps / every + 1; a.t0 = t0; a.dt = dm.dt;
    if (!plan_predict(a.D, T, a.NP, nstim, a.geo)) return fail(VA_EUNSUPPORTED, "va_predict: D=%d: %s", a.D, a.geo.why);
    HIPCHK(hipSetDevice(h->device));
    // one allocation: [x0 | p | stim | out]
    const size_t nx = (size_t)T * a.D, np = (size_t)T * a.NP, ns = (size_t)(n_steps + 1) * nstim, no = (size_t)T * a.n_out * a.D;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (nx + np + ns + no + 1)));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *x0_d = buf, *p_d = x0_d + nx, *st_d = p_d + np, *out_d = st_d + ns;
    HIPCHK(hipMemcpyAsync(x0_d, x0, sizeof(double) * nx, hipMemcpyHostToDevice, h->stream));
    if (np) HIPCHK(hipMemcpyAsync(p_d, p, sizeof(double) * np, hipMemcpyHostToDevice, h->stream));
    if (ns) HIPCHK(hipMemcpyAsync(st_d, stim, sizeof(double) * ns, hipMemcpyHostToDevice, h->stream));
    a.x0 = x0_d; a.p = p_d; a.stim = ns ? st_d : nullptr; a.out = out_d;
    const hipError_t e = h->rt.predict(a, h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);       // (the uploads read the caller's arrays)
        return fail(VA_EHIP, "k_predict launch: %s", hipGetErrorString(e));
    }
    HIPCHK(hipMemcpyAsync(out, out_d, sizeof(double) * no, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// Forecast spread: the nominal trajectories of va_predict and, along nvec directions each, the tangent-linear model of the
// discrete RK4 map (va_predict_tlm.h); the tangents stay in a device workspace [T][nvec][n_out][D], which k_spread reduces
// to variances and same-time covariance blocks.  Chunked over trajectories: the buffers of a chunk stay under 1 GiB.  Works
// on buffers of its own, like va_predict.
int va_predict_tangent(va_handle h, const double *x0, const double *p, const double *V0, int32_t T, int32_t nvec, double t0,
                       int32_t n_steps, int32_t substeps, int32_t every, const double *stim, double *out, double *dX, double *var,
                       double *cov)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!x0 || !p || !V0 || !out) return fail(VA_EINVAL, "x0 / p / V0 / out must not be NULL");
    if (T < 1 || n_steps < 1 || substeps < 1 || every < 1)
        return fail(VA_EINVAL, "T, n_steps, substeps and every must be at least 1 (T=%d n_steps=%d substeps=%d every=%d)", T, n_steps, substeps, every);
    if (nvec < 1) return fail(VA_EINVAL, "nvec must be at least 1 (nvec=%d)", nvec);
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "a network handle has no differential equation to integrate");
    const Dims &dm = h->dv.dm;
    const int nstim = h->dv.pp.nstim;
    if (nstim > 0 && !stim) return fail(VA_EINVAL, "the model takes a stimulus of %d column(s): pass its %d rows from t0 on", nstim, n_steps + 1);
    if (nstim == 0 && stim) return fail(VA_EINVAL, "the model takes no stimulus, but one was passed");
    if (dm.lin) return fail(VA_EUNSUPPORTED, "va_predict_tangent: the module's dense linear part was split off (LINEAR): build it with linear=False");
    if (!h->rt.predict || !h->rt_hvp.predict_tlm)
        return fail(VA_EUNSUPPORTED, "va_predict_tangent: the model has no flat form f(x, i, p) to differentiate (more than %d parameters: "
                                     "its module carries the column-parameter form only)", RHS_BIG_NP);
    if ((int64_t)n_steps * substeps > 2000000000LL) return fail(VA_EUNSUPPORTED, "n_steps x substeps does not fit 32-bit indexing");
    PredictTlmArgs a;
    a.T = T; a.D = dm.D; a.NP = dm.NPt; a.NPest = dm.NPest; a.nvec = nvec; a.nstim = nstim; a.n_steps = n_steps; a.substeps = substeps;
    a.every = every; a.n_out = n_steps / every + 1; a.t0 = t0; a.dt = dm.dt; a.Pidx = h->dv.pp.Pidx;
    const bool reduce = var || cov;
    const size_t per = predict_tlm_traj_doubles(a.D, a.NP, a.NPest, nvec, a.n_out, cov != nullptr);
    const long C = predict_tlm_chunk_trajs(per, T);
    if (C < 1)
        return fail(VA_EUNSUPPORTED, "va_predict_tangent: one trajectory with %d direction(s) and %d output row(s) takes %.1f MiB of device "
                                     "workspace, the limit is %zu MiB: fewer directions, or a larger `every`", nvec, a.n_out,
                    (double)per * 8.0 / 1048576.0, PREDICT_TLM_WORKSPACE_BYTES >> 20);
    if (!plan_predict_tlm(a.D, C, nvec, a.NP, nstim, a.geo)) return fail(VA_EUNSUPPORTED, "va_predict_tangent: D=%d nvec=%d: %s", a.D, nvec, a.geo.why);
    HIPCHK(hipSetDevice(h->device));
    // one allocation: [stim | x0 | p | V0 | out | dX | var | cov], all but the stimulus for one chunk of C trajectories
    const size_t nw = (size_t)a.D + a.NPest, row = (size_t)a.n_out * a.D;
    const size_t ns = (size_t)(n_steps + 1) * nstim, nx = (size_t)C * a.D, np = (size_t)C * a.NP, nv0 = (size_t)C * nvec * nw, no = C * row,
                 ndx = (dX || reduce) ? C * nvec * row : 0, nvar = var ? C * row : 0, ncov = cov ? C * row * a.D : 0;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (ns + nx + np + nv0 + no + ndx + nvar + ncov + 1)));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *st_d = buf, *x0_d = st_d + ns, *p_d = x0_d + nx, *v0_d = p_d + np, *out_d = v0_d + nv0, *dx_d = out_d + no, *var_d = dx_d + ndx,
           *cov_d = var_d + nvar;
    if (ns) HIPCHK(hipMemcpyAsync(st_d, stim, sizeof(double) * ns, hipMemcpyHostToDevice, h->stream));
    for (long t1 = 0; t1 < T; t1 += C) {
        const long n = T - t1 < C ? T - t1 : C;
        HIPCHK(hipMemcpyAsync(x0_d, x0 + (size_t)t1 * a.D, sizeof(double) * n * a.D, hipMemcpyHostToDevice, h->stream));
        if (a.NP) HIPCHK(hipMemcpyAsync(p_d, p + (size_t)t1 * a.NP, sizeof(double) * n * a.NP, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(v0_d, V0 + (size_t)t1 * nvec * nw, sizeof(double) * n * nvec * nw, hipMemcpyHostToDevice, h->stream));
        a.T = (int)n;
        if (!plan_predict_tlm(a.D, n, nvec, a.NP, nstim, a.geo)) {      // (the last chunk: the same plan on fewer workgroups)
            (void)hipStreamSynchronize(h->stream);
            return fail(VA_EUNSUPPORTED, "va_predict_tangent: D=%d nvec=%d: %s", a.D, nvec, a.geo.why);
        }
        a.x0 = x0_d; a.p = p_d; a.V0 = v0_d; a.stim = ns ? st_d : nullptr; a.out = out_d; a.dX = ndx ? dx_d : nullptr;
        hipError_t e = h->rt_hvp.predict_tlm(a, h->stream);
        if (e == hipSuccess && reduce) {
            SpreadArgs sa;
            sa.dX = dx_d; sa.var = var ? var_d : nullptr; sa.cov = cov ? cov_d : nullptr; sa.T = (int)n; sa.nvec = nvec; sa.n_out = a.n_out; sa.D = a.D;
            e = launch_spread(sa, h->stream);
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);       // (the uploads read the caller's arrays)
            return fail(VA_EHIP, "k_predict_tlm / k_spread launch: %s", hipGetErrorString(e));
        }
        HIPCHK(hipMemcpyAsync(out + (size_t)t1 * row, out_d, sizeof(double) * n * row, hipMemcpyDeviceToHost, h->stream));
        if (dX) HIPCHK(hipMemcpyAsync(dX + (size_t)t1 * nvec * row, dx_d, sizeof(double) * n * nvec * row, hipMemcpyDeviceToHost, h->stream));
        if (var) HIPCHK(hipMemcpyAsync(var + (size_t)t1 * row, var_d, sizeof(double) * n * row, hipMemcpyDeviceToHost, h->stream));
        if (cov) HIPCHK(hipMemcpyAsync(cov + (size_t)t1 * row * a.D, cov_d, sizeof(double) * n * row * a.D, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));      // (the next chunk reuses the buffers; pageable destinations)
    }
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// Adjoint of the forecast (va_predict_adj.h): the nominal trajectories of va_predict and, for ncot cotangent sets each, the
// transpose of the derivative of the discrete RK4 map va_predict_tangent applies -- gx0 = (d out / d x0)^T G and
// gp = (d out / d p_est)^T G.  Cotangent mode: the caller's G.  Misfit mode (G NULL, ncot = 1): the cotangents are
// 2 w_l (x_l - y_l) at the handle's observed columns and cost = sum w_l (x_l - y_l)^2 comes back with them.  Chunked over
// trajectories: the buffers of a chunk, checkpoints included, stay under 1 GiB.  Works on buffers of its own, like va_predict.
int va_predict_adjoint(va_handle h, const double *x0, const double *p, const double *G, const double *Y, const double *weights,
                       int32_t y_shared, int32_t T, int32_t ncot, double t0, int32_t n_steps, int32_t substeps, int32_t every,
                       const double *stim, double *out, double *gx0, double *gp, double *cost)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!x0 || !p || !out || !gx0) return fail(VA_EINVAL, "x0 / p / out / gx0 must not be NULL");
    if (T < 1 || n_steps < 1 || substeps < 1 || every < 1)
        return fail(VA_EINVAL, "T, n_steps, substeps and every must be at least 1 (T=%d n_steps=%d substeps=%d every=%d)", T, n_steps, substeps, every);
    if ((G != nullptr) == (Y != nullptr)) return fail(VA_EINVAL, "va_predict_adjoint: pass exactly one of G (cotangent mode) and Y (misfit mode)");
    if (ncot < 1) return fail(VA_EINVAL, "ncot must be at least 1 (ncot=%d)", ncot);
    if (Y && (ncot != 1 || !weights || !cost)) return fail(VA_EINVAL, "va_predict_adjoint: misfit mode takes ncot = 1, weights and cost (ncot=%d)", ncot);
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "a network handle has no differential equation to integrate");
    const Dims &dm = h->dv.dm;
    const int nstim = h->dv.pp.nstim;
    if (dm.NPest > 0 && !gp) return fail(VA_EINVAL, "gp must not be NULL (%d estimated parameter(s))", dm.NPest);
    if (nstim > 0 && !stim) return fail(VA_EINVAL, "the model takes a stimulus of %d column(s): pass its %d rows from t0 on", nstim, n_steps + 1);
    if (nstim == 0 && stim) return fail(VA_EINVAL, "the model takes no stimulus, but one was passed");
    if (dm.lin) return fail(VA_EUNSUPPORTED, "va_predict_adjoint: the module's dense linear part was split off (LINEAR): build it with linear=False");
    if (!h->rt.predict || !h->rt_hvp.predict_adj)
        return fail(VA_EUNSUPPORTED, "va_predict_adjoint: the model has no flat form f(x, i, p) to differentiate (more than %d parameters: "
                                     "its module carries the column-parameter form only)", RHS_BIG_NP);
    if ((int64_t)n_steps * substeps > 2000000000LL) return fail(VA_EUNSUPPORTED, "n_steps x substeps does not fit 32-bit indexing");
    PredictAdjArgs a;
    a.T = T; a.D = dm.D; a.NP = dm.NPt; a.NPest = dm.NPest; a.ncot = ncot; a.L = Y ? dm.L : 0; a.nstim = nstim; a.n_steps = n_steps;
    a.substeps = substeps; a.every = every; a.n_out = n_steps / every + 1; a.t0 = t0; a.dt = dm.dt; a.Pidx = h->dv.pp.Pidx;
    const long long Q = (long long)n_steps * substeps;
    const size_t row = (size_t)a.n_out * a.D, yrow = (size_t)a.n_out * a.L;
    if (!plan_predict_adj(a.D, T, ncot, a.NP, nstim, a.geo)) return fail(VA_EUNSUPPORTED, "va_predict_adjoint: D=%d ncot=%d: %s", a.D, ncot, a.geo.why);
    const size_t per = predict_adj_traj_doubles(a.D, a.NP, a.NPest, ncot, a.n_out, Q, a.geo.nchunks, G ? ncot * row : (y_shared ? 0 : yrow));
    const size_t spare = (size_t)a.geo.RW * a.geo.nchunks * (size_t)Q * a.D + (size_t)(n_steps + 1) * nstim + yrow + 2 * (size_t)a.L + 8;
    const long C = predict_adj_chunk_trajs(per, spare, T);
    if (C < 1)
        return fail(VA_EUNSUPPORTED, "va_predict_adjoint: one trajectory with %d cotangent set(s), %d output row(s) and %lld checkpoints takes "
                                     "%.1f MiB of device workspace, the limit is %zu MiB: fewer steps or sets, or a larger `every`", ncot,
                    a.n_out, Q * a.geo.nchunks, (double)(per + spare) * 8.0 / 1048576.0, PREDICT_ADJ_WORKSPACE_BYTES >> 20);
    if (!plan_predict_adj(a.D, C, ncot, a.NP, nstim, a.geo)) return fail(VA_EUNSUPPORTED, "va_predict_adjoint: D=%d ncot=%d: %s", a.D, ncot, a.geo.why);
    HIPCHK(hipSetDevice(h->device));
    // one allocation: [stim | w | Lidx | x0 | p | G or Y | out | gx0 | gp | cost | checkpoints], all but the first three (and a
    // shared Y) for one chunk of C trajectories
    const size_t ns = (size_t)(n_steps + 1) * nstim, nwt = a.L, nli = ((size_t)a.L + 1) / 2, nx = (size_t)C * a.D, np = (size_t)C * a.NP,
                 ncg = G ? (size_t)C * ncot * row : (y_shared ? yrow : (size_t)C * yrow), no = C * row, ngx = (size_t)C * ncot * a.D,
                 ngp = (size_t)C * ncot * a.NPest, nc = Y ? (size_t)C : 0, nck = predict_adj_ckpt_doubles(a.geo, a.D, Q);
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (ns + nwt + nli + nx + np + ncg + no + ngx + ngp + nc + nck + 1)));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *st_d = buf, *w_d = st_d + ns, *li_d = w_d + nwt, *x0_d = li_d + nli, *p_d = x0_d + nx, *cg_d = p_d + np, *out_d = cg_d + ncg,
           *gx_d = out_d + no, *gp_d = gx_d + ngx, *c_d = gp_d + ngp, *ck_d = c_d + nc;
    if (ns) HIPCHK(hipMemcpyAsync(st_d, stim, sizeof(double) * ns, hipMemcpyHostToDevice, h->stream));
    if (a.L) {
        HIPCHK(hipMemcpyAsync(w_d, weights, sizeof(double) * a.L, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(li_d, h->lidx_user.data(), sizeof(int) * a.L, hipMemcpyHostToDevice, h->stream));
        if (y_shared) HIPCHK(hipMemcpyAsync(cg_d, Y, sizeof(double) * yrow, hipMemcpyHostToDevice, h->stream));
    }
    for (long t1 = 0; t1 < T; t1 += C) {
        const long n = T - t1 < C ? T - t1 : C;
        HIPCHK(hipMemcpyAsync(x0_d, x0 + (size_t)t1 * a.D, sizeof(double) * n * a.D, hipMemcpyHostToDevice, h->stream));
        if (a.NP) HIPCHK(hipMemcpyAsync(p_d, p + (size_t)t1 * a.NP, sizeof(double) * n * a.NP, hipMemcpyHostToDevice, h->stream));
        if (G) HIPCHK(hipMemcpyAsync(cg_d, G + (size_t)t1 * ncot * row, sizeof(double) * n * ncot * row, hipMemcpyHostToDevice, h->stream));
        else if (!y_shared && yrow) HIPCHK(hipMemcpyAsync(cg_d, Y + (size_t)t1 * yrow, sizeof(double) * n * yrow, hipMemcpyHostToDevice, h->stream));
        a.T = (int)n;
        if (!plan_predict_adj(a.D, n, ncot, a.NP, nstim, a.geo) || predict_adj_ckpt_doubles(a.geo, a.D, Q) > nck) {      // (the last chunk: the same plan on fewer workgroups)
            (void)hipStreamSynchronize(h->stream);
            return fail(VA_EUNSUPPORTED, "va_predict_adjoint: D=%d ncot=%d: %s", a.D, ncot, a.geo.why);
        }
        a.x0 = x0_d; a.p = p_d; a.G = G ? cg_d : nullptr; a.Y = Y ? cg_d : nullptr; a.w = w_d; a.Lidx = (const int *)li_d;
        a.y_stride = y_shared ? 0 : yrow; a.stim = ns ? st_d : nullptr; a.out = out_d; a.gx0 = gx_d; a.gp = gp_d; a.cost = c_d; a.ckpt = ck_d;
        const hipError_t e = h->rt_hvp.predict_adj(a, h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);       // (the uploads read the caller's arrays)
            return fail(VA_EHIP, "k_predict_adj launch: %s", hipGetErrorString(e));
        }
        HIPCHK(hipMemcpyAsync(out + (size_t)t1 * row, out_d, sizeof(double) * n * row, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(gx0 + (size_t)t1 * ncot * a.D, gx_d, sizeof(double) * n * ncot * a.D, hipMemcpyDeviceToHost, h->stream));
        if (a.NPest) HIPCHK(hipMemcpyAsync(gp + (size_t)t1 * ncot * a.NPest, gp_d, sizeof(double) * n * ncot * a.NPest, hipMemcpyDeviceToHost, h->stream));
        if (Y) HIPCHK(hipMemcpyAsync(cost + t1, c_d, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));      // (the next chunk reuses the buffers; pageable destinations)
    }
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// Strong-constraint shooting (va_shoot.h): the whole L-BFGS minimisation of va_predict_adjoint's misfit over (x0, p_est), for
// all T points in one launch per chunk.  One allocation, one upload, one download; chunked over points as va_predict_adjoint
// chunks its trajectories (the checkpoints and the L-BFGS history of a chunk stay under PREDICT_ADJ_WORKSPACE_BYTES).
// Works on buffers of its own: the handle's resident state is left alone.
int va_shoot(va_handle h, const double *x0, const double *p, const double *Y, const double *weights, int32_t y_shared, int32_t T,
             double t0, int32_t n_steps, int32_t substeps, int32_t every, const double *stim, int32_t m, int64_t maxiter,
             int64_t maxfun, int32_t maxls, double ftol, double gtol, double *x0_out, double *p_out, double *cost,
             double *cost_start, double *grad_max, int32_t *nit, int32_t *nfev, int32_t *status)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!x0 || !p || !Y || !weights) return fail(VA_EINVAL, "va_shoot: x0 / p / Y / weights must not be NULL");
    if (!x0_out || !p_out || !cost || !cost_start || !grad_max || !nit || !nfev || !status) return fail(VA_EINVAL, "va_shoot: the outputs must not be NULL");
    if (T < 1 || n_steps < 1 || substeps < 1 || every < 1)
        return fail(VA_EINVAL, "T, n_steps, substeps and every must be at least 1 (T=%d n_steps=%d substeps=%d every=%d)", T, n_steps, substeps, every);
    char why[192];
    if (!shoot_check_args(m, maxiter, maxfun, maxls, why, sizeof why)) return fail(VA_EINVAL, "va_shoot: %s", why);
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "a network handle has no differential equation to integrate");
    const Dims &dm = h->dv.dm;
    const int nstim = h->dv.pp.nstim;
    if (nstim > 0 && !stim) return fail(VA_EINVAL, "the model takes a stimulus of %d column(s): pass its %d rows from t0 on", nstim, n_steps + 1);
    if (nstim == 0 && stim) return fail(VA_EINVAL, "the model takes no stimulus, but one was passed");
    if (dm.bounded) return fail(VA_EUNSUPPORTED, "va_shoot: the handle has box bounds; the device minimiser takes no projected step");
    if (dm.lin) return fail(VA_EUNSUPPORTED, "va_shoot: the module's dense linear part was split off (LINEAR): build it with linear=False");
    if (dm.D > SHOOT_MAX_D)
        return fail(VA_EUNSUPPORTED, "va_shoot: D=%d: the shooting kernel carries states of at most %d columns; minimise on the host around va_predict_adjoint",
                    dm.D, SHOOT_MAX_D);
    if (!h->rt.predict || !h->rt_hvp.predict_adj || !h->rt_hvp.shoot)
        return fail(VA_EUNSUPPORTED, "va_shoot: the model has no flat form f(x, i, p) to differentiate (more than %d parameters: "
                                     "its module carries the column-parameter form only)", RHS_BIG_NP);
    if ((int64_t)n_steps * substeps > 2000000000LL) return fail(VA_EUNSUPPORTED, "n_steps x substeps does not fit 32-bit indexing");
    ShootArgs sa;
    PredictAdjArgs &a = sa.adj;
    a.T = T; a.D = dm.D; a.NP = dm.NPt; a.NPest = dm.NPest; a.ncot = 1; a.L = dm.L; a.nstim = nstim; a.n_steps = n_steps;
    a.substeps = substeps; a.every = every; a.n_out = n_steps / every + 1; a.t0 = t0; a.dt = dm.dt; a.Pidx = h->dv.pp.Pidx;
    a.G = nullptr; a.out = nullptr;
    sa.m = m; sa.maxls = maxls; sa.maxiter = maxiter; sa.maxfun = maxfun; sa.ftol = ftol; sa.gtol = gtol;
    const long long Q = (long long)n_steps * substeps;
    const size_t yrow = (size_t)a.n_out * a.L;
    ShootGeo geo;
    if (!plan_shoot(a.D, T, a.NP, a.NPest, nstim, m, geo)) return fail(VA_EUNSUPPORTED, "va_shoot: D=%d: %s", a.D, geo.why);
    const size_t per = shoot_traj_doubles(a.D, a.NP, a.NPest, Q, m, y_shared ? 0 : yrow);
    const size_t spare = (size_t)geo.adj.RW * (size_t)Q * a.D + (size_t)(n_steps + 1) * nstim + yrow + 2 * (size_t)a.L + 8;
    const long C = predict_adj_chunk_trajs(per, spare, T);
    if (C < 1)
        return fail(VA_EUNSUPPORTED, "va_shoot: one point with %d output row(s), %lld checkpoints and %d history pair(s) takes %.1f MiB of "
                                     "device workspace, the limit is %zu MiB: fewer steps, or a larger `every`", a.n_out, Q, m,
                    (double)(per + spare) * 8.0 / 1048576.0, PREDICT_ADJ_WORKSPACE_BYTES >> 20);
    if (!plan_shoot(a.D, C, a.NP, a.NPest, nstim, m, geo)) return fail(VA_EUNSUPPORTED, "va_shoot: D=%d: %s", a.D, geo.why);
    HIPCHK(hipSetDevice(h->device));
    // one allocation: [stim | w | Lidx | x0 | p | Y | gx0 | gp | cost | states | minimiser workspace | checkpoints], all but
    // the first three (and a shared Y) for one chunk of C points
    const size_t sd = shoot_state_doubles();
    const size_t ns = (size_t)(n_steps + 1) * nstim, nwt = a.L, nli = ((size_t)a.L + 1) / 2, nx = (size_t)C * a.D, np = (size_t)C * a.NP,
                 ny = y_shared ? yrow : (size_t)C * yrow, ngp = (size_t)C * a.NPest, nc = (size_t)C, nst = (size_t)C * sd,
                 nwk = (size_t)C * geo.point_doubles, nck = predict_adj_ckpt_doubles(geo.adj, a.D, Q);
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (ns + nwt + nli + nx + np + ny + nx + ngp + nc + nst + nwk + nck + 1)));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *st_d = buf, *w_d = st_d + ns, *li_d = w_d + nwt, *x0_d = li_d + nli, *p_d = x0_d + nx, *y_d = p_d + np, *gx_d = y_d + ny,
           *gp_d = gx_d + nx, *c_d = gp_d + ngp, *s_d = c_d + nc, *wk_d = s_d + nst, *ck_d = wk_d + nwk;
    if (ns) HIPCHK(hipMemcpyAsync(st_d, stim, sizeof(double) * ns, hipMemcpyHostToDevice, h->stream));
    if (a.L) {
        HIPCHK(hipMemcpyAsync(w_d, weights, sizeof(double) * a.L, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(li_d, h->lidx_user.data(), sizeof(int) * a.L, hipMemcpyHostToDevice, h->stream));
        if (y_shared) HIPCHK(hipMemcpyAsync(y_d, Y, sizeof(double) * yrow, hipMemcpyHostToDevice, h->stream));
    }
    std::vector<ShootState> states((size_t)C);
    for (long t1 = 0; t1 < T; t1 += C) {
        const long n = T - t1 < C ? T - t1 : C;
        HIPCHK(hipMemcpyAsync(x0_d, x0 + (size_t)t1 * a.D, sizeof(double) * n * a.D, hipMemcpyHostToDevice, h->stream));
        if (a.NP) HIPCHK(hipMemcpyAsync(p_d, p + (size_t)t1 * a.NP, sizeof(double) * n * a.NP, hipMemcpyHostToDevice, h->stream));
        if (!y_shared && yrow) HIPCHK(hipMemcpyAsync(y_d, Y + (size_t)t1 * yrow, sizeof(double) * n * yrow, hipMemcpyHostToDevice, h->stream));
        a.T = (int)n;
        if (!plan_shoot(a.D, n, a.NP, a.NPest, nstim, m, geo) || predict_adj_ckpt_doubles(geo.adj, a.D, Q) > nck) {      // (the last chunk: the same plan on fewer workgroups)
            (void)hipStreamSynchronize(h->stream);
            return fail(VA_EUNSUPPORTED, "va_shoot: D=%d: %s", a.D, geo.why);
        }
        a.geo = geo.adj;
        a.x0 = x0_d; a.p = p_d; a.Y = y_d; a.w = w_d; a.Lidx = (const int *)li_d; a.y_stride = y_shared ? 0 : yrow;
        a.stim = ns ? st_d : nullptr; a.gx0 = gx_d; a.gp = gp_d; a.cost = c_d; a.ckpt = ck_d;
        sa.x = x0_d; sa.p = p_d; sa.st = (ShootState *)s_d; sa.work = wk_d; sa.point_doubles = geo.point_doubles;
        const hipError_t e = h->rt_hvp.shoot(sa, h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);       // (the uploads read the caller's arrays)
            return fail(VA_EHIP, "k_shoot launch: %s", hipGetErrorString(e));
        }
        HIPCHK(hipMemcpyAsync(x0_out + (size_t)t1 * a.D, x0_d, sizeof(double) * n * a.D, hipMemcpyDeviceToHost, h->stream));
        if (a.NP) HIPCHK(hipMemcpyAsync(p_out + (size_t)t1 * a.NP, p_d, sizeof(double) * n * a.NP, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(states.data(), s_d, sizeof(ShootState) * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));      // (the next chunk reuses the buffers; pageable destinations)
        for (long k = 0; k < n; ++k) {
            const ShootState &s = states[(size_t)k];
            cost[t1 + k] = s.f; cost_start[t1 + k] = s.f_start; grad_max[t1 + k] = s.gmax;
            nit[t1 + k] = s.iter; nfev[t1 + k] = (int32_t)s.nfev; status[t1 + k] = s.status;
        }
    }
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// Strong-constraint shooting inside a box (va_shoot_box.h): va_shoot's launch with L-BFGS-B as the step.  The caller's box is
// the box: the handle's own `bounds` table is not looked at (as va_hess_vec ignores it), so bounded and unbounded handles
// both run.  Buffers and chunking as va_shoot, with the larger per-point workspace and, when every point has its own box,
// 2 n doubles more per point.
int va_shoot_box(va_handle h, const double *x0, const double *p, const double *Y, const double *weights, int32_t y_shared, int32_t T,
                 double t0, int32_t n_steps, int32_t substeps, int32_t every, const double *stim, int32_t m, int64_t maxiter,
                 int64_t maxfun, int32_t maxls, double ftol, double gtol, const double *lower, const double *upper, int32_t box_shared,
                 double *x0_out, double *p_out, double *cost, double *cost_start, double *grad_max, int32_t *nit, int32_t *nfev,
                 int32_t *status)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!x0 || !p || !Y || !weights) return fail(VA_EINVAL, "va_shoot_box: x0 / p / Y / weights must not be NULL");
    if (!lower || !upper) return fail(VA_EINVAL, "va_shoot_box: lower / upper must not be NULL (-inf / +inf entries: no bound)");
    if (!x0_out || !p_out || !cost || !cost_start || !grad_max || !nit || !nfev || !status) return fail(VA_EINVAL, "va_shoot_box: the outputs must not be NULL");
    if (T < 1 || n_steps < 1 || substeps < 1 || every < 1)
        return fail(VA_EINVAL, "T, n_steps, substeps and every must be at least 1 (T=%d n_steps=%d substeps=%d every=%d)", T, n_steps, substeps, every);
    char why[192];
    if (!shoot_check_args(m, maxiter, maxfun, maxls, why, sizeof why)) return fail(VA_EINVAL, "va_shoot_box: %s", why);
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "a network handle has no differential equation to integrate");
    const Dims &dm = h->dv.dm;
    const int nstim = h->dv.pp.nstim;
    if (nstim > 0 && !stim) return fail(VA_EINVAL, "the model takes a stimulus of %d column(s): pass its %d rows from t0 on", nstim, n_steps + 1);
    if (nstim == 0 && stim) return fail(VA_EINVAL, "the model takes no stimulus, but one was passed");
    if (dm.lin) return fail(VA_EUNSUPPORTED, "va_shoot_box: the module's dense linear part was split off (LINEAR): build it with linear=False");
    if (dm.D > SHOOT_MAX_D)
        return fail(VA_EUNSUPPORTED, "va_shoot_box: D=%d: the shooting kernel carries states of at most %d columns; minimise on the host around va_predict_adjoint",
                    dm.D, SHOOT_MAX_D);
    if (!h->rt.predict || !h->rt_hvp.predict_adj || !h->rt_hvp.shoot_box)
        return fail(VA_EUNSUPPORTED, "va_shoot_box: the model has no flat form f(x, i, p) to differentiate (more than %d parameters: "
                                     "its module carries the column-parameter form only)", RHS_BIG_NP);
    if ((int64_t)n_steps * substeps > 2000000000LL) return fail(VA_EUNSUPPORTED, "n_steps x substeps does not fit 32-bit indexing");
    const int nvar = dm.D + dm.NPest;
    if (!shoot_box_check_bounds(lower, upper, box_shared ? 1 : (long)T, nvar, why, sizeof why)) return fail(VA_EINVAL, "va_shoot_box: %s", why);
    ShootBoxArgs ba;
    ShootArgs &sa = ba.sh;
    PredictAdjArgs &a = sa.adj;
    a.T = T; a.D = dm.D; a.NP = dm.NPt; a.NPest = dm.NPest; a.ncot = 1; a.L = dm.L; a.nstim = nstim; a.n_steps = n_steps;
    a.substeps = substeps; a.every = every; a.n_out = n_steps / every + 1; a.t0 = t0; a.dt = dm.dt; a.Pidx = h->dv.pp.Pidx;
    a.G = nullptr; a.out = nullptr;
    sa.m = m; sa.maxls = maxls; sa.maxiter = maxiter; sa.maxfun = maxfun; sa.ftol = ftol; sa.gtol = gtol; sa.st = nullptr;
    ba.box_shared = box_shared ? 1 : 0;
    const long long Q = (long long)n_steps * substeps;
    const size_t yrow = (size_t)a.n_out * a.L, brow = 2 * (size_t)nvar;
    ShootGeo geo;
    if (!plan_shoot_box(a.D, T, a.NP, a.NPest, nstim, m, geo)) return fail(VA_EUNSUPPORTED, "va_shoot_box: D=%d: %s", a.D, geo.why);
    const size_t per = shoot_box_traj_doubles(a.D, a.NP, a.NPest, Q, m, y_shared ? 0 : yrow, box_shared ? 0 : brow);
    const size_t spare = (size_t)geo.adj.RW * (size_t)Q * a.D + (size_t)(n_steps + 1) * nstim + yrow + brow + 2 * (size_t)a.L + 8;
    const long C = predict_adj_chunk_trajs(per, spare, T);
    if (C < 1)
        return fail(VA_EUNSUPPORTED, "va_shoot_box: one point with %d output row(s), %lld checkpoints and %d history pair(s) takes %.1f MiB of "
                                     "device workspace, the limit is %zu MiB: fewer steps, or a larger `every`", a.n_out, Q, m,
                    (double)(per + spare) * 8.0 / 1048576.0, PREDICT_ADJ_WORKSPACE_BYTES >> 20);
    if (!plan_shoot_box(a.D, C, a.NP, a.NPest, nstim, m, geo)) return fail(VA_EUNSUPPORTED, "va_shoot_box: D=%d: %s", a.D, geo.why);
    HIPCHK(hipSetDevice(h->device));
    // one allocation: [stim | w | Lidx | x0 | p | Y | lower | upper | gx0 | gp | cost | states | minimiser workspace | checkpoints]
    const size_t sd = shoot_box_state_doubles();
    const size_t ns = (size_t)(n_steps + 1) * nstim, nwt = a.L, nli = ((size_t)a.L + 1) / 2, nx = (size_t)C * a.D, np = (size_t)C * a.NP,
                 ny = y_shared ? yrow : (size_t)C * yrow, nbx = box_shared ? (size_t)nvar : (size_t)C * nvar, ngp = (size_t)C * a.NPest,
                 nc = (size_t)C, nst = (size_t)C * sd, nwk = (size_t)C * geo.point_doubles, nck = predict_adj_ckpt_doubles(geo.adj, a.D, Q);
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (ns + nwt + nli + nx + np + ny + 2 * nbx + nx + ngp + nc + nst + nwk + nck + 1)));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *st_d = buf, *w_d = st_d + ns, *li_d = w_d + nwt, *x0_d = li_d + nli, *p_d = x0_d + nx, *y_d = p_d + np, *lo_d = y_d + ny,
           *hi_d = lo_d + nbx, *gx_d = hi_d + nbx, *gp_d = gx_d + nx, *c_d = gp_d + ngp, *s_d = c_d + nc, *wk_d = s_d + nst, *ck_d = wk_d + nwk;
    if (ns) HIPCHK(hipMemcpyAsync(st_d, stim, sizeof(double) * ns, hipMemcpyHostToDevice, h->stream));
    if (a.L) {
        HIPCHK(hipMemcpyAsync(w_d, weights, sizeof(double) * a.L, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(li_d, h->lidx_user.data(), sizeof(int) * a.L, hipMemcpyHostToDevice, h->stream));
        if (y_shared) HIPCHK(hipMemcpyAsync(y_d, Y, sizeof(double) * yrow, hipMemcpyHostToDevice, h->stream));
    }
    if (box_shared) {
        HIPCHK(hipMemcpyAsync(lo_d, lower, sizeof(double) * nvar, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(hi_d, upper, sizeof(double) * nvar, hipMemcpyHostToDevice, h->stream));
    }
    std::vector<ShootBoxState> states((size_t)C);
    for (long t1 = 0; t1 < T; t1 += C) {
        const long n = T - t1 < C ? T - t1 : C;
        HIPCHK(hipMemcpyAsync(x0_d, x0 + (size_t)t1 * a.D, sizeof(double) * n * a.D, hipMemcpyHostToDevice, h->stream));
        if (a.NP) HIPCHK(hipMemcpyAsync(p_d, p + (size_t)t1 * a.NP, sizeof(double) * n * a.NP, hipMemcpyHostToDevice, h->stream));
        if (!y_shared && yrow) HIPCHK(hipMemcpyAsync(y_d, Y + (size_t)t1 * yrow, sizeof(double) * n * yrow, hipMemcpyHostToDevice, h->stream));
        if (!box_shared) {
            HIPCHK(hipMemcpyAsync(lo_d, lower + (size_t)t1 * nvar, sizeof(double) * n * nvar, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(hi_d, upper + (size_t)t1 * nvar, sizeof(double) * n * nvar, hipMemcpyHostToDevice, h->stream));
        }
        a.T = (int)n;
        if (!plan_shoot_box(a.D, n, a.NP, a.NPest, nstim, m, geo) || predict_adj_ckpt_doubles(geo.adj, a.D, Q) > nck) {      // (the last chunk: the same plan on fewer workgroups)
            (void)hipStreamSynchronize(h->stream);
            return fail(VA_EUNSUPPORTED, "va_shoot_box: D=%d: %s", a.D, geo.why);
        }
        a.geo = geo.adj;
        a.x0 = x0_d; a.p = p_d; a.Y = y_d; a.w = w_d; a.Lidx = (const int *)li_d; a.y_stride = y_shared ? 0 : yrow;
        a.stim = ns ? st_d : nullptr; a.gx0 = gx_d; a.gp = gp_d; a.cost = c_d; a.ckpt = ck_d;
        sa.x = x0_d; sa.p = p_d; sa.work = wk_d; sa.point_doubles = geo.point_doubles;
        ba.st = (ShootBoxState *)s_d; ba.lower = lo_d; ba.upper = hi_d;
        const hipError_t e = h->rt_hvp.shoot_box(ba, h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);       // (the uploads read the caller's arrays)
            return fail(VA_EHIP, "k_shoot_box launch: %s", hipGetErrorString(e));
        }
        HIPCHK(hipMemcpyAsync(x0_out + (size_t)t1 * a.D, x0_d, sizeof(double) * n * a.D, hipMemcpyDeviceToHost, h->stream));
        if (a.NP) HIPCHK(hipMemcpyAsync(p_out + (size_t)t1 * a.NP, p_d, sizeof(double) * n * a.NP, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(states.data(), s_d, sizeof(ShootBoxState) * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));      // (the next chunk reuses the buffers; pageable destinations)
        for (long k = 0; k < n; ++k) {
            const ShootBoxState &s = states[(size_t)k];
            cost[t1 + k] = s.f; cost_start[t1 + k] = s.f_start; grad_max[t1 + k] = s.gmax;
            nit[t1 + k] = s.iter; nfev[t1 + k] = (int32_t)s.nfev; status[t1 + k] = s.status;
        }
    }
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// Lyapunov spectra (va_lyap.h): T trajectories with K tangents each, one workgroup per trajectory (or several trajectories
// per wave), all QRs on the device; only the sums, the end points and (when asked for) the trace come back.  Chunked over
// trajectories under a workspace limit; buffers of its own, like va_predict_tangent.
int va_lyapunov(va_handle h, const double *x0, const double *p, const double *Q0, const double *coupling, int32_t T, int32_t K,
                double t0, int32_t n_steps, int32_t substeps, int32_t qr_every, int32_t n_skip, const double *stim,
                double *logsum, double *x_end, double *Q_end, double *trace, int32_t *status)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!x0 || !p || !logsum || !x_end || !Q_end || !status) return fail(VA_EINVAL, "x0 / p / logsum / x_end / Q_end / status must not be NULL");
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "a network handle has no differential equation to integrate");
    const Dims &dm = h->dv.dm;
    char why[192];
    if (!lyap_check_args(T, dm.D, K, n_steps, substeps, qr_every, n_skip, coupling, why, sizeof why)) return fail(VA_EINVAL, "va_lyapunov: %s", why);
    const int nstim = h->dv.pp.nstim;
    if (nstim > 0 && !stim) return fail(VA_EINVAL, "the model takes a stimulus of %d column(s): pass its %d rows from t0 on", nstim, n_steps + 1);
    if (nstim == 0 && stim) return fail(VA_EINVAL, "the model takes no stimulus, but one was passed");
    if (dm.lin) return fail(VA_EUNSUPPORTED, "va_lyapunov: the module's dense linear part was split off (LINEAR): build it with linear=False");
    if (!h->rt.predict || !h->rt_hvp.predict_tlm)
        return fail(VA_EUNSUPPORTED, "va_lyapunov: the model has no flat form f(x, i, p) to differentiate (more than %d parameters: "
                                     "its module carries the column-parameter form only)", RHS_BIG_NP);
    if ((int64_t)n_steps * substeps > 2000000000LL) return fail(VA_EUNSUPPORTED, "n_steps x substeps does not fit 32-bit indexing");
    LyapArgs a;
    a.T = T; a.D = dm.D; a.NP = dm.NPt; a.K = K; a.nstim = nstim; a.n_steps = n_steps; a.substeps = substeps; a.qr_every = qr_every;
    a.n_skip = n_skip; a.t0 = t0; a.dt = dm.dt;
    const int n_qr = n_steps / qr_every;
    const size_t per = lyap_traj_doubles(a.D, a.NP, K, n_qr, trace != nullptr);
    const long C = lyap_chunk_trajs(per, T);
    if (C < 1)
        return fail(VA_EUNSUPPORTED, "va_lyapunov: one trajectory with a trace of %d QRs takes %.1f MiB of device workspace, the limit is "
                                     "%zu MiB: a larger qr_every, or no trace", n_qr, (double)per * 8.0 / 1048576.0, LYAP_WORKSPACE_BYTES >> 20);
    if (!plan_lyap(a.D, C, K, a.NP, nstim, a.geo)) return fail(VA_EUNSUPPORTED, "va_lyapunov: D=%d K=%d: %s", a.D, K, a.geo.why);
    if (!h->rt_hvp.lyap) return fail(VA_EUNSUPPORTED, "va_lyapunov: the model's module carries no k_lyap for D=%d", a.D);
    HIPCHK(hipSetDevice(h->device));
    // one allocation: [stim | x0 | p | Q0 | coupling | logsum | x_end | Q_end | trace | status], all but the stimulus for one
    // chunk of C trajectories
    const size_t ns = (size_t)(n_steps + 1) * nstim, nx = (size_t)C * a.D, np = (size_t)C * a.NP, nq = (size_t)C * K * a.D, nq0 = Q0 ? nq : 0,
                 ng = coupling ? nx : 0, nl = (size_t)C * K, ntr = trace ? (size_t)C * n_qr * K : 0;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (ns + nx + np + nq0 + ng + nl + nx + nq + ntr + (size_t)C + 1)));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *st_d = buf, *x0_d = st_d + ns, *p_d = x0_d + nx, *q0_d = p_d + np, *g_d = q0_d + nq0, *ls_d = g_d + ng, *xe_d = ls_d + nl,
           *qe_d = xe_d + nx, *tr_d = qe_d + nq;
    int *stat_d = (int *)(tr_d + ntr);
    if (ns) HIPCHK(hipMemcpyAsync(st_d, stim, sizeof(double) * ns, hipMemcpyHostToDevice, h->stream));
    for (long t1 = 0; t1 < T; t1 += C) {
        const long n = T - t1 < C ? T - t1 : C;
        HIPCHK(hipMemcpyAsync(x0_d, x0 + (size_t)t1 * a.D, sizeof(double) * n * a.D, hipMemcpyHostToDevice, h->stream));
        if (a.NP) HIPCHK(hipMemcpyAsync(p_d, p + (size_t)t1 * a.NP, sizeof(double) * n * a.NP, hipMemcpyHostToDevice, h->stream));
        if (Q0) HIPCHK(hipMemcpyAsync(q0_d, Q0 + (size_t)t1 * K * a.D, sizeof(double) * n * K * a.D, hipMemcpyHostToDevice, h->stream));
        if (coupling) HIPCHK(hipMemcpyAsync(g_d, coupling + (size_t)t1 * a.D, sizeof(double) * n * a.D, hipMemcpyHostToDevice, h->stream));
        a.T = (int)n;
        if (!plan_lyap(a.D, n, K, a.NP, nstim, a.geo)) {      // (the last chunk: the same plan on fewer workgroups)
            (void)hipStreamSynchronize(h->stream);
            return fail(VA_EUNSUPPORTED, "va_lyapunov: D=%d K=%d: %s", a.D, K, a.geo.why);
        }
        a.x0 = x0_d; a.p = p_d; a.Q0 = Q0 ? q0_d : nullptr; a.coupling = coupling ? g_d : nullptr; a.stim = ns ? st_d : nullptr;
        a.logsum = ls_d; a.x_end = xe_d; a.Q_end = qe_d; a.trace = trace ? tr_d : nullptr; a.status = stat_d;
        const hipError_t e = h->rt_hvp.lyap(a, h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);       // (the uploads read the caller's arrays)
            return fail(VA_EHIP, "k_lyap launch: %s", hipGetErrorString(e));
        }
        HIPCHK(hipMemcpyAsync(logsum + (size_t)t1 * K, ls_d, sizeof(double) * n * K, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(x_end + (size_t)t1 * a.D, xe_d, sizeof(double) * n * a.D, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(Q_end + (size_t)t1 * K * a.D, qe_d, sizeof(double) * n * K * a.D, hipMemcpyDeviceToHost, h->stream));
        if (trace) HIPCHK(hipMemcpyAsync(trace + (size_t)t1 * n_qr * K, tr_d, sizeof(double) * n * n_qr * K, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(status + t1, stat_d, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));      // (the next chunk reuses the buffers; pageable destinations)
    }
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// The ensemble Kalman filter (va_enkf.h): T points of M members each, one workgroup per point, forecast and analysis
// alternating inside one launch per chunk; the statistics of every observation row, the final members and their parameters
// come back.  Chunked over points under a workspace limit; buffers of its own, like va_predict.
int va_enkf(va_handle h, const double *x0, const double *p, const int32_t *est, int32_t NQ, const double *Y, const double *obs_var,
            double inflation, int32_t T, int32_t M, double t0, int32_t n_obs, int32_t obs_every, int32_t substeps, const double *stim,
            double *mean_f, double *sd_f, double *mean_a, double *sd_a, double *x_end, double *p_end, int32_t *status)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!x0 || !p || !Y || !obs_var) return fail(VA_EINVAL, "va_enkf: x0 / p / Y / obs_var must not be NULL");
    if (!mean_f || !sd_f || !mean_a || !sd_a || !x_end || !p_end || !status) return fail(VA_EINVAL, "va_enkf: the outputs must not be NULL");
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "a network handle has no differential equation to integrate");
    const Dims &dm = h->dv.dm;
    char why[192];
    if (!enkf_check_args(T, M, dm.NPt, NQ, dm.L, n_obs, obs_every, substeps, est, obs_var, inflation, why, sizeof why))
        return fail(VA_EINVAL, "va_enkf: %s", why);
    const int nstim = h->dv.pp.nstim;
    if ((int64_t)n_obs * obs_every * substeps > 2000000000LL) return fail(VA_EUNSUPPORTED, "n_obs x obs_every x substeps does not fit 32-bit indexing");
    const int n_steps = n_obs * obs_every;
    if (nstim > 0 && !stim) return fail(VA_EINVAL, "the model takes a stimulus of %d column(s): pass its %d rows from t0 on", nstim, n_steps + 1);
    if (nstim == 0 && stim) return fail(VA_EINVAL, "the model takes no stimulus, but one was passed");
    // (a module whose dense linear part was split off is carried: the members move through predict_f, as va_predict's do)
    if (!h->rt.predict || !h->rt_hvp.enkf)
        return fail(VA_EUNSUPPORTED, "va_enkf: the model has no flat form f(x, i, p) to integrate (more than %d parameters: "
                                     "its module carries the column-parameter form only)", RHS_BIG_NP);
    EnkfArgs a;
    a.T = T; a.D = dm.D; a.NP = dm.NPt; a.NQ = NQ; a.L = dm.L; a.M = M; a.nstim = nstim; a.n_obs = n_obs; a.obs_every = obs_every;
    a.substeps = substeps; a.t0 = t0; a.dt = dm.dt; a.inflation = inflation;
    const int NV = a.D + NQ;
    const size_t per = enkf_point_doubles(a.D, a.NP, NQ, a.L, M, n_obs);
    const long C = enkf_chunk_points(per, T);
    if (C < 1)
        return fail(VA_EUNSUPPORTED, "va_enkf: one point with %d observation rows takes %.1f MiB of device workspace, the limit is %zu MiB: "
                                     "fewer rows per call (x_end / p_end continue a run)", n_obs, (double)per * 8.0 / 1048576.0,
                    ENKF_WORKSPACE_BYTES >> 20);
    if (!plan_enkf(a.D, C, M, a.NP, NQ, nstim, a.geo)) return fail(VA_EUNSUPPORTED, "va_enkf: D=%d M=%d: %s", a.D, M, a.geo.why);
    HIPCHK(hipSetDevice(h->device));
    // one allocation: [stim | obs_var | est | Lidx | x0 | p | Y | mean_f | sd_f | mean_a | sd_a | x_end | p_end | status], all
    // but the first four for one chunk of C points
    const size_t ns = (size_t)(n_steps + 1) * nstim, nov = a.L, nes = ((size_t)NQ + 1) / 2, nli = ((size_t)a.L + 1) / 2,
                 nx = (size_t)C * M * a.D, np = (size_t)C * M * a.NP, ny = (size_t)C * n_obs * a.L, nst = (size_t)C * n_obs * NV;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (ns + nov + nes + nli + 2 * nx + 2 * np + ny + 4 * nst + (size_t)C + 1)));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *st_d = buf, *ov_d = st_d + ns, *es_d = ov_d + nov, *li_d = es_d + nes, *x0_d = li_d + nli, *p_d = x0_d + nx, *y_d = p_d + np,
           *mf_d = y_d + ny, *sf_d = mf_d + nst, *ma_d = sf_d + nst, *sa_d = ma_d + nst, *xe_d = sa_d + nst, *pe_d = xe_d + nx;
    int *stat_d = (int *)(pe_d + np);
    if (ns) HIPCHK(hipMemcpyAsync(st_d, stim, sizeof(double) * ns, hipMemcpyHostToDevice, h->stream));
    if (a.L) {
        HIPCHK(hipMemcpyAsync(ov_d, obs_var, sizeof(double) * a.L, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(li_d, h->lidx_user.data(), sizeof(int) * a.L, hipMemcpyHostToDevice, h->stream));
    }
    if (NQ) HIPCHK(hipMemcpyAsync(es_d, est, sizeof(int) * NQ, hipMemcpyHostToDevice, h->stream));
    for (long t1 = 0; t1 < T; t1 += C) {
        const long n = T - t1 < C ? T - t1 : C;
        HIPCHK(hipMemcpyAsync(x0_d, x0 + (size_t)t1 * M * a.D, sizeof(double) * n * M * a.D, hipMemcpyHostToDevice, h->stream));
        if (a.NP) HIPCHK(hipMemcpyAsync(p_d, p + (size_t)t1 * M * a.NP, sizeof(double) * n * M * a.NP, hipMemcpyHostToDevice, h->stream));
        if (a.L) HIPCHK(hipMemcpyAsync(y_d, Y + (size_t)t1 * n_obs * a.L, sizeof(double) * n * n_obs * a.L, hipMemcpyHostToDevice, h->stream));
        a.T = (int)n;
        if (!plan_enkf(a.D, n, M, a.NP, NQ, nstim, a.geo)) {      // (the last chunk: the same plan on fewer workgroups)
            (void)hipStreamSynchronize(h->stream);
            return fail(VA_EUNSUPPORTED, "va_enkf: D=%d M=%d: %s", a.D, M, a.geo.why);
        }
        a.x0 = x0_d; a.p = p_d; a.Y = y_d; a.obs_var = ov_d; a.stim = ns ? st_d : nullptr; a.est = (const int *)es_d; a.Lidx = (const int *)li_d;
        a.mean_f = mf_d; a.sd_f = sf_d; a.mean_a = ma_d; a.sd_a = sa_d; a.x_end = xe_d; a.p_end = pe_d; a.status = stat_d;
        const hipError_t e = h->rt_hvp.enkf(a, h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);       // (the uploads read the caller's arrays)
            return fail(VA_EHIP, "k_enkf launch: %s", hipGetErrorString(e));
        }
        const size_t so = (size_t)t1 * n_obs * NV, sb = sizeof(double) * n * n_obs * NV;
        HIPCHK(hipMemcpyAsync(mean_f + so, mf_d, sb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(sd_f + so, sf_d, sb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(mean_a + so, ma_d, sb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(sd_a + so, sa_d, sb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(x_end + (size_t)t1 * M * a.D, xe_d, sizeof(double) * n * M * a.D, hipMemcpyDeviceToHost, h->stream));
        if (a.NP) HIPCHK(hipMemcpyAsync(p_end + (size_t)t1 * M * a.NP, pe_d, sizeof(double) * n * M * a.NP, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(status + t1, stat_d, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));      // (the next chunk reuses the buffers; pageable destinations)
    }
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// Hamiltonian Monte Carlo on the resident paths (va_hmc.h): B chains of n_iter iterations at one rf_scale, n_leap evaluations
// each through run_eval -- whatever kernel the handle evaluates with -- and one element-wise launch between two of them.
// Plain launches on the handle's stream; the workspace is the call's own.  The handle's resident paths are saved and put
// back device-to-device, the seeds are left idle as a fresh handle has them, the evaluations are booked as va_action_grad's.
int va_hmc(va_handle h, double *XP, int64_t ld, int32_t mem, double rf_scale, int32_t n_iter, int32_t n_leap, const double *eps,
           double jitter, const double *minv, int64_t minv_n, uint64_t seed, const double *noise, int32_t thin,
           const int64_t *keep_idx, int32_t n_keep_idx, double *mean, double *var, double *A_trace, double *dH, int32_t *accepted,
           int32_t *n_divergent, double *kept)
{
    TRY(check_xp(h, XP, ld, mem));
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "va_hmc: network handles are not sampled (ODE handles only)");
    Dev &dv = h->dv;
    const Dims &dm = dv.dm;
    if (dm.bounded) return fail(VA_EUNSUPPORTED, "va_hmc: the handle has box bounds; va_hmc_box samples them through a transform");
    const long n_var = dm.ND + dm.NPest, B = dm.B;
    char why[192];
    if (hmc_check_args(n_var, B, n_iter, n_leap, thin, eps, jitter, minv, (long)minv_n, keep_idx, n_keep_idx, why, sizeof why))
        return fail(VA_EINVAL, "va_hmc: %s", why);
    if (!std::isfinite(rf_scale)) return fail(VA_EINVAL, "va_hmc: rf_scale is not finite");
    HmcArgs a = {};
    if (!plan_hmc(n_var, B, a.geo, why, sizeof why)) return fail(VA_EUNSUPPORTED, "va_hmc: %s", why);
    HIPCHK(hipSetDevice(h->device));
    // the inverse mass and its square root (IEEE on the host: the momentum is z / sqrt(minv) on every platform)
    const bool per_chain = minv && minv_n == B * n_var && B > 1;
    const size_t nm = per_chain ? (size_t)B * n_var : (size_t)n_var;
    std::vector<double> mh(nm, 1.0), sh(nm, 1.0), dh((size_t)B * n_iter);      // (dh: the energy errors' way back, below)
    if (minv) for (size_t i = 0; i < nm; ++i) { mh[i] = minv[i]; sh[i] = sqrt(minv[i]); }
    // one allocation, zeroed: [save | p | xs | gs | minv | sminv | eps | noise | A_cur | part | mean | m2 | A_trace | dH | kept |
    // keep_idx (int64) | accepted (int32)]
    const size_t nv = (size_t)B * dm.ld, nn = noise ? (size_t)n_iter * B * (n_var + 2) : 0, nt = (size_t)B * n_iter,
                 nk = (size_t)B * (n_iter / thin) * n_keep_idx, ns = (size_t)B * n_var;
    const size_t total = 4 * nv + 2 * nm + B + nn + 2 * B + 2 * (size_t)a.geo.grid + 2 * ns + 2 * nt + nk + (size_t)n_keep_idx + (nt + 1) / 2 + 1;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * total));
    // (last declared, first destroyed: the stream has consumed the host arrays above before they go, on every way out)
    struct Free { double *q; hipStream_t s; ~Free() { (void)hipStreamSynchronize(s); (void)hipFree(q); } } guard{buf, h->stream};
    HIPCHK(hipMemsetAsync(buf, 0, sizeof(double) * total, h->stream));
    double *q = buf;
    auto take = [&q](size_t n) { double *r = q; q += n; return r; };
    double *save = take(nv), *minv_d = nullptr, *sminv_d = nullptr, *eps_d = nullptr, *noise_d = nullptr;
    a.p = take(nv); a.xs = take(nv); a.gs = take(nv);
    minv_d = take(nm); sminv_d = take(nm); eps_d = take(B); noise_d = take(nn);
    a.A_cur = take(2 * B); a.part = take(2 * (size_t)a.geo.grid); a.mean = take(ns); a.m2 = take(ns);
    a.A_trace = take(nt); a.dH = take(nt); a.kept = take(nk);
    int64_t *keep_d = (int64_t *)take(n_keep_idx);
    a.accepted = (int32_t *)take((nt + 1) / 2);
    HIPCHK(hipMemcpyAsync(minv_d, mh.data(), sizeof(double) * nm, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(sminv_d, sh.data(), sizeof(double) * nm, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(eps_d, eps, sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    if (nn) HIPCHK(hipMemcpyAsync(noise_d, noise, sizeof(double) * nn, hipMemcpyHostToDevice, h->stream));
    if (n_keep_idx) HIPCHK(hipMemcpyAsync(keep_d, keep_idx, sizeof(int64_t) * n_keep_idx, hipMemcpyHostToDevice, h->stream));
    a.x = dv.x; a.g = dv.gt; a.minv = minv_d; a.sminv = sminv_d; a.minv_stride = per_chain ? n_var : 0; a.eps = eps_d; a.jitter = jitter;
    a.noise = nn ? noise_d : nullptr; a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.chain0 = 0u; a.A_eval = dv.outA;
    a.keep_idx = keep_d; a.n_keep = n_keep_idx; a.ld = dm.ld; a.n_var = n_var; a.B = (int)B; a.n_iter = n_iter; a.thin = thin;
    // the resident paths aside, the caller's in; the start point's action and gradient
    HIPCHK(hipMemcpyAsync(save, dv.x, sizeof(double) * nv, hipMemcpyDeviceToDevice, h->stream));
    // whatever ends the sampling from here on, the handle goes back to what it was: paths restored, seeds idle,
    // evaluations booked
    int64_t n_evals = 0;
    auto leave = [&]() {
        (void)hipMemcpyAsync(dv.x, save, sizeof(double) * nv, hipMemcpyDeviceToDevice, h->stream);
        launch_init_states(dv, PH_IDLE, 1.0, h->stream);
        h->timed_armed_rf = -1.0;
        h->n_eval_launch += n_evals; h->n_seed_evals += n_evals * B; h->n_seed_evals_direct += n_evals * B;
    };
    if (int rc_in = copy_in(h, XP, ld, mem)) { leave(); return rc_in; }      // (a failed copy may have overwritten part of dv.x)
    launch_init_states(dv, PH_START, rf_scale, h->stream);
    h->timed_armed_rf = rf_scale;
    run_eval(h, EPI_FINALIZE); ++n_evals;
    hipError_t e = hipMemcpyAsync(a.A_cur, dv.outA, sizeof(double) * B, hipMemcpyDeviceToDevice, h->stream);
    for (int it = 0; it < n_iter && e == hipSuccess; ++it) {
        a.it = it;
        e = launch_hmc(a, HMC_BEGIN, h->stream);
        for (int l = 0; l < n_leap && e == hipSuccess; ++l) {
            if (l) e = launch_hmc(a, HMC_MID, h->stream);
            if (e == hipSuccess) { run_eval(h, EPI_FINALIZE); ++n_evals; e = hipGetLastError(); }
        }
        if (e == hipSuccess) e = launch_hmc(a, HMC_END, h->stream);
        if (e == hipSuccess) e = launch_hmc(a, HMC_COMMIT, h->stream);
    }
    if (e != hipSuccess) {
        leave();
        return fail(VA_EHIP, "va_hmc launch: %s", hipGetErrorString(e));
    }
    int rc = copy_out(h, dv.x, XP, ld, mem);
    leave();
    if (rc) return rc;
    if (mean) HIPCHK(hipMemcpyAsync(mean, a.mean, sizeof(double) * ns, hipMemcpyDeviceToHost, h->stream));
    if (var) HIPCHK(hipMemcpyAsync(var, a.m2, sizeof(double) * ns, hipMemcpyDeviceToHost, h->stream));
    if (A_trace) HIPCHK(hipMemcpyAsync(A_trace, a.A_trace, sizeof(double) * nt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(dh.data(), a.dH, sizeof(double) * nt, hipMemcpyDeviceToHost, h->stream));
    if (accepted) HIPCHK(hipMemcpyAsync(accepted, a.accepted, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, h->stream));
    if (kept && nk) HIPCHK(hipMemcpyAsync(kept, a.kept, sizeof(double) * nk, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    // sample variance from the sum of squared deviations; a non-finite dH was a rejection and counts as divergent
    if (var) for (size_t i = 0; i < ns; ++i) var[i] = n_iter > 1 ? var[i] / (double)(n_iter - 1) : 0.0;
    for (long b = 0; b < B; ++b) {
        int nd = 0;
        for (int it = 0; it < n_iter; ++it) {
            const double v = dh[(size_t)b * n_iter + it];
            if (!std::isfinite(v)) ++nd;
            if (dH) dH[(size_t)b * n_iter + it] = v;
        }
        if (n_divergent) n_divergent[b] = nd;
    }
    return VA_OK;
}

// The sampler for box-bounded problems (va_hmc_box.h): va_hmc's call with the chain run in z, x = T(z) written into the
// handle's paths before every evaluation.  Kinds, start check and T^-1 on the host (va_hmc_geo.h, hmc_box_inverse); the
// start's x = T(z) too (IEEE + - * / sqrt: the bits the device's map gives), so the chain's first x is its z's own image.
int va_hmc_box(va_handle h, double *XP, int64_t ld, int32_t mem, double rf_scale, int32_t n_iter, int32_t n_leap, const double *eps,
               double jitter, const double *minv, int64_t minv_n, uint64_t seed, const double *noise, int32_t thin,
               const int64_t *keep_idx, int32_t n_keep_idx, const double *lower, const double *upper, const double *Z0, double *Z_out,
               double *mean, double *var, double *A_trace, double *dH, int32_t *accepted, int32_t *n_divergent, double *kept)
{
    TRY(check_xp(h, XP, ld, mem));
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "va_hmc_box: network handles are not sampled (ODE handles only)");
    Dev &dv = h->dv;
    const Dims &dm = dv.dm;
    if ((lower != nullptr) != (upper != nullptr)) return fail(VA_EINVAL, "va_hmc_box: lower and upper come together");
    if (!lower && !dm.bounded)
        return fail(VA_EUNSUPPORTED, "va_hmc_box: no bounds: the handle has none and lower / upper are NULL (va_hmc samples unbounded problems)");
    const long n_var = dm.ND + dm.NPest, B = dm.B;
    char why[256];
    if (hmc_check_args(n_var, B, n_iter, n_leap, thin, eps, jitter, minv, (long)minv_n, keep_idx, n_keep_idx, why, sizeof why))
        return fail(VA_EINVAL, "va_hmc_box: %s", why);
    if (!std::isfinite(rf_scale)) return fail(VA_EINVAL, "va_hmc_box: rf_scale is not finite");
    HmcBoxArgs a = {};
    if (!plan_hmc(n_var, B, a.h.geo, why, sizeof why)) return fail(VA_EUNSUPPORTED, "va_hmc_box: %s", why);
    HIPCHK(hipSetDevice(h->device));
    // bounds (the handle's own come back from its device tables), kinds, the start in x and in z
    std::vector<double> lo_h((size_t)n_var), hi_h((size_t)n_var);
    std::vector<int32_t> kind_h((size_t)n_var);
    if (lower) {
        for (long i = 0; i < n_var; ++i) { lo_h[i] = lower[i]; hi_h[i] = upper[i]; }
    } else {
        HIPCHK(hipMemcpyAsync(lo_h.data(), dv.pp.lo, sizeof(double) * n_var, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(hi_h.data(), dv.pp.hi, sizeof(double) * n_var, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    const long n_bounded = hmc_box_kinds(n_var, lo_h.data(), hi_h.data(), kind_h.data(), why, sizeof why);
    if (n_bounded < 0) return fail(VA_EINVAL, "va_hmc_box: %s", why);
    if (n_bounded == 0) return fail(VA_EUNSUPPORTED, "va_hmc_box: %s", why);
    const size_t nvv = (size_t)B * n_var;
    std::vector<double> x_h(nvv), z_h(nvv);
    if (Z0) {
        if (hmc_box_check_z(n_var, B, n_var, Z0, why, sizeof why)) return fail(VA_EINVAL, "va_hmc_box: %s", why);
        for (size_t k = 0; k < nvv; ++k) z_h[k] = Z0[k];
    } else {
        if (mem == VA_MEM_DEVICE) {
            HIPCHK(hipMemcpy2DAsync(x_h.data(), sizeof(double) * n_var, XP, sizeof(double) * ld, sizeof(double) * n_var, B, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        } else {
            for (long b = 0; b < B; ++b)
                for (long i = 0; i < n_var; ++i) x_h[(size_t)b * n_var + i] = XP[(size_t)b * ld + i];
        }
        if (hmc_box_check_start(n_var, B, n_var, x_h.data(), lo_h.data(), hi_h.data(), why, sizeof why)) return fail(VA_EINVAL, "va_hmc_box: %s", why);
        for (long b = 0; b < B; ++b)
            for (long i = 0; i < n_var; ++i) {
                const size_t k = (size_t)b * n_var + i;
                z_h[k] = hmc_box_inverse(kind_h[i], lo_h[i], hi_h[i], x_h[k]);
            }
    }
    for (long b = 0; b < B; ++b)
        for (long i = 0; i < n_var; ++i) {
            const size_t k = (size_t)b * n_var + i;
            double dx, dlj, lj;
            hmc_box_map(kind_h[i], lo_h[i], hi_h[i], z_h[k], &x_h[k], &dx, &dlj, &lj);
        }
    // the inverse mass of z and its square root (IEEE on the host)
    const bool per_chain = minv && minv_n == B * n_var && B > 1;
    const size_t nm = per_chain ? (size_t)B * n_var : (size_t)n_var;
    std::vector<double> mh(nm, 1.0), sh(nm, 1.0), dh((size_t)B * n_iter);
    if (minv) for (size_t i = 0; i < nm; ++i) { mh[i] = minv[i]; sh[i] = sqrt(minv[i]); }
    // one allocation, zeroed: [save | p | xs | gs | z | zs | minv | sminv | eps | noise | A_cur | part | lpart | mean | m2 |
    // A_trace | dH | kept | lo | hi | keep_idx (int64) | accepted (int32) | kind (int32)]
    const size_t nv = (size_t)B * dm.ld, nn = noise ? (size_t)n_iter * B * (n_var + 2) : 0, nt = (size_t)B * n_iter,
                 nk = (size_t)B * (n_iter / thin) * n_keep_idx, ns = (size_t)B * n_var, ng = (size_t)a.h.geo.grid;
    const size_t total = 6 * nv + 2 * nm + B + nn + 2 * B + 4 * ng + 2 * ns + 2 * nt + nk + 2 * (size_t)n_var + (size_t)n_keep_idx +
                         (nt + 1) / 2 + ((size_t)n_var + 1) / 2 + 1;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * total));
    struct Free { double *q; hipStream_t s; ~Free() { (void)hipStreamSynchronize(s); (void)hipFree(q); } } guard{buf, h->stream};
    HIPCHK(hipMemsetAsync(buf, 0, sizeof(double) * total, h->stream));
    double *q = buf;
    auto take = [&q](size_t n) { double *r = q; q += n; return r; };
    HmcArgs &ha = a.h;
    double *save = take(nv);
    ha.p = take(nv); ha.xs = take(nv); ha.gs = take(nv); a.z = take(nv); a.zs = take(nv);
    double *minv_d = take(nm), *sminv_d = take(nm), *eps_d = take(B), *noise_d = take(nn);
    ha.A_cur = take(2 * B); ha.part = take(2 * ng); a.lpart = take(2 * ng); ha.mean = take(ns); ha.m2 = take(ns);
    ha.A_trace = take(nt); ha.dH = take(nt); ha.kept = take(nk);
    double *lo_d = take(n_var), *hi_d = take(n_var);
    int64_t *keep_d = (int64_t *)take(n_keep_idx);
    ha.accepted = (int32_t *)take((nt + 1) / 2);
    int32_t *kind_d = (int32_t *)take(((size_t)n_var + 1) / 2);
    HIPCHK(hipMemcpyAsync(minv_d, mh.data(), sizeof(double) * nm, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(sminv_d, sh.data(), sizeof(double) * nm, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(eps_d, eps, sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    if (nn) HIPCHK(hipMemcpyAsync(noise_d, noise, sizeof(double) * nn, hipMemcpyHostToDevice, h->stream));
    if (n_keep_idx) HIPCHK(hipMemcpyAsync(keep_d, keep_idx, sizeof(int64_t) * n_keep_idx, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(lo_d, lo_h.data(), sizeof(double) * n_var, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(hi_d, hi_h.data(), sizeof(double) * n_var, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(kind_d, kind_h.data(), sizeof(int32_t) * n_var, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpy2DAsync(a.z, sizeof(double) * dm.ld, z_h.data(), sizeof(double) * n_var, sizeof(double) * n_var, B, hipMemcpyHostToDevice, h->stream));
    ha.x = dv.x; ha.g = dv.gt; ha.minv = minv_d; ha.sminv = sminv_d; ha.minv_stride = per_chain ? n_var : 0; ha.eps = eps_d; ha.jitter = jitter;
    ha.noise = nn ? noise_d : nullptr; ha.k0 = (uint32_t)seed; ha.k1 = (uint32_t)(seed >> 32); ha.chain0 = 0u; ha.A_eval = dv.outA;
    ha.keep_idx = keep_d; ha.n_keep = n_keep_idx; ha.ld = dm.ld; ha.n_var = n_var; ha.B = (int)B; ha.n_iter = n_iter; ha.thin = thin;
    a.kind = kind_d; a.lo = lo_d; a.hi = hi_d;
    HIPCHK(hipMemcpyAsync(save, dv.x, sizeof(double) * nv, hipMemcpyDeviceToDevice, h->stream));
    // whatever ends the sampling from here on, the handle goes back to what it was (as va_hmc)
    int64_t n_evals = 0;
    auto leave = [&]() {
        (void)hipMemcpyAsync(dv.x, save, sizeof(double) * nv, hipMemcpyDeviceToDevice, h->stream);
        launch_init_states(dv, PH_IDLE, 1.0, h->stream);
        h->timed_armed_rf = -1.0;
        h->n_eval_launch += n_evals; h->n_seed_evals += n_evals * B; h->n_seed_evals_direct += n_evals * B;
    };
    if (int rc_in = copy_in(h, x_h.data(), n_var, VA_MEM_HOST)) { leave(); return rc_in; }
    launch_init_states(dv, PH_START, rf_scale, h->stream);
    h->timed_armed_rf = rf_scale;
    run_eval(h, EPI_FINALIZE); ++n_evals;
    hipError_t e = hipMemcpyAsync(ha.A_cur, dv.outA, sizeof(double) * B, hipMemcpyDeviceToDevice, h->stream);
    for (int it = 0; it < n_iter && e == hipSuccess; ++it) {
        ha.it = it;
        e = launch_hmc_box(a, HMC_BEGIN, h->stream);
        for (int l = 0; l < n_leap && e == hipSuccess; ++l) {
            if (l) e = launch_hmc_box(a, HMC_MID, h->stream);
            if (e == hipSuccess) { run_eval(h, EPI_FINALIZE); ++n_evals; e = hipGetLastError(); }
        }
        if (e == hipSuccess) e = launch_hmc_box(a, HMC_END, h->stream);
        if (e == hipSuccess) e = launch_hmc_box(a, HMC_COMMIT, h->stream);
    }
    if (e != hipSuccess) {
        leave();
        return fail(VA_EHIP, "va_hmc_box launch: %s", hipGetErrorString(e));
    }
    int rc = copy_out(h, dv.x, XP, ld, mem);
    leave();
    if (rc) return rc;
    if (Z_out) HIPCHK(hipMemcpy2DAsync(Z_out, sizeof(double) * n_var, a.z, sizeof(double) * dm.ld, sizeof(double) * n_var, B, hipMemcpyDeviceToHost, h->stream));
    if (mean) HIPCHK(hipMemcpyAsync(mean, ha.mean, sizeof(double) * ns, hipMemcpyDeviceToHost, h->stream));
    if (var) HIPCHK(hipMemcpyAsync(var, ha.m2, sizeof(double) * ns, hipMemcpyDeviceToHost, h->stream));
    if (A_trace) HIPCHK(hipMemcpyAsync(A_trace, ha.A_trace, sizeof(double) * nt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(dh.data(), ha.dH, sizeof(double) * nt, hipMemcpyDeviceToHost, h->stream));
    if (accepted) HIPCHK(hipMemcpyAsync(accepted, ha.accepted, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, h->stream));
    if (kept && nk) HIPCHK(hipMemcpyAsync(kept, ha.kept, sizeof(double) * nk, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    if (var) for (size_t i = 0; i < ns; ++i) var[i] = n_iter > 1 ? var[i] / (double)(n_iter - 1) : 0.0;
    for (long b = 0; b < B; ++b) {
        int nd = 0;
        for (int it = 0; it < n_iter; ++it) {
            const double v = dh[(size_t)b * n_iter + it];
            if (!std::isfinite(v)) ++nd;
            if (dH) dH[(size_t)b * n_iter + it] = v;
        }
        if (n_divergent) n_divergent[b] = nd;
    }
    return VA_OK;
}

// hmc_box_map as the current device computes it, over a table of n entries (HOST arrays; lower / upper -/+HUGE_VAL: none).
// Needs no handle.
int va_hmc_box_map(int64_t n, const double *lower, const double *upper, const double *z, double *x, double *dx, double *dlj, double *lj)
{
    if (n < 1 || n > 2147483647LL || !lower || !upper || !z || !x || !dx || !dlj || !lj) return fail(VA_EINVAL, "va_hmc_box_map: n from 1 to 2^31 - 1 and no NULL array");
    char why[256];
    std::vector<int32_t> kind((size_t)n);
    if (hmc_box_kinds((long)n, lower, upper, kind.data(), why, sizeof why) < 0) return fail(VA_EINVAL, "va_hmc_box_map: %s", why);
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (7 * (size_t)n + ((size_t)n + 1) / 2)));
    struct Free { double *q; ~Free() { (void)hipDeviceSynchronize(); (void)hipFree(q); } } guard{buf};
    double *lo_d = buf, *hi_d = buf + n, *z_d = buf + 2 * n, *out_d = buf + 3 * n;
    int32_t *kind_d = (int32_t *)(buf + 7 * n);
    HIPCHK(hipMemcpy(lo_d, lower, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(hi_d, upper, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(z_d, z, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(kind_d, kind.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
    const hipError_t e = launch_hmc_box_map((long)n, kind_d, lo_d, hi_d, z_d, out_d, out_d + n, out_d + 2 * n, out_d + 3 * n, nullptr);
    if (e != hipSuccess) return fail(VA_EHIP, "k_hmc_box_map launch: %s", hipGetErrorString(e));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(x, out_d, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dx, out_d + n, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dlj, out_d + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lj, out_d + 3 * n, sizeof(double) * n, hipMemcpyDeviceToHost));
    return VA_OK;
}

// What the sampler's kernels draw for (seed, chain, iteration), computed by the device they would run on (the current one):
// words [(n + 1) * 4] the Philox words of the n element counters and of the extra stream's, normals [n], uniforms [2] (accept,
// jitter); any may be NULL.  HOST arrays.
int va_hmc_noise(uint64_t seed, int32_t chain, int32_t iteration, int64_t n, uint32_t *words, double *normals, double *uniforms)
{
    if (chain < 0 || iteration < 0 || n < 0 || n > 2147483647LL) return fail(VA_EINVAL, "va_hmc_noise: chain, iteration and n must not be negative (n below 2^31)");
    const size_t nw = ((size_t)n + 1) * 4;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * ((size_t)n + 2) + sizeof(uint32_t) * nw));
    struct Free { double *q; ~Free() { (void)hipDeviceSynchronize(); (void)hipFree(q); } } guard{buf};
    double *nrm_d = buf, *uni_d = buf + n;
    uint32_t *w_d = (uint32_t *)(buf + n + 2);
    const hipError_t e = launch_hmc_noise((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)chain, (uint32_t)iteration, (long)n, w_d, nrm_d, uni_d, nullptr);
    if (e != hipSuccess) return fail(VA_EHIP, "k_hmc_noise launch: %s", hipGetErrorString(e));
    HIPCHK(hipDeviceSynchronize());
    if (words) HIPCHK(hipMemcpy(words, w_d, sizeof(uint32_t) * nw, hipMemcpyDeviceToHost));
    if (normals && n) HIPCHK(hipMemcpy(normals, nrm_d, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (uniforms) HIPCHK(hipMemcpy(uniforms, uni_d, sizeof(double) * 2, hipMemcpyDeviceToHost));
    return VA_OK;
}

// Hessian-vector products of the action at npts points along nvec directions each (va_hvp.h): HV = (d^2 A / dXP^2) V, or the
// Gauss-Newton part of it.  Works on buffers of its own, like va_predict: the handle's resident paths, seed states and
// captured graphs are not touched.  The handle's bounds play no part: this is the Hessian of the unconstrained action.
// hvp_refusals: what the handle cannot do (`who` names the caller); hvp_on_device: the launch on device buffers
// (x_d [npts][ld], p_d [npts][NP], v_d / hv_d [npts][nvec][ld], part_d [npts][nvec][ntiles][NP]); va_hess_vec wraps both
// around host arrays, va_laplace runs them on the chunks of its workspace.
static int hvp_refusals(va_handle h, const char *who)
{
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "%s: the network action has no second derivatives here (ODE handles only)", who);
    const Dev &dv = h->dv;
    const Dims &hd = dv.dm;
    if (hd.tdp) return fail(VA_EUNSUPPORTED, "%s: time-dependent parameters are not carried", who);
    if (dv.pp.rm_full || dv.pp.rf0_full)
        return fail(VA_EUNSUPPORTED, "%s: full %s matrices (kind 2) are not carried: scalar or per-entry weights only", who, dv.pp.rm_full ? "RM" : "RF");
    if (hd.lin) return fail(VA_EUNSUPPORTED, "%s: the module's dense linear part was split off (LINEAR): build it with linear=False", who);
    if (!h->rt_hvp.hvp)
        return fail(VA_EUNSUPPORTED, "%s: the model has no flat form f(x, i, p) to differentiate (more than %d parameters: "
                                     "its module carries the column-parameter form only)", who, RHS_BIG_NP);
    return VA_OK;
}

static hipError_t hvp_on_device(va_handle h, const HvpGeo &geo, const double *x_d, const double *p_d, const double *v_d, double *hv_d,
                                double *part_d, int32_t npts, int32_t nvec, int64_t ld, double rf_scale, int32_t gauss_newton)
{
    const Dev &dv = h->dv;
    const Dims &hd = dv.dm;
    HvpArgs a;
    a.dm = hd; a.dm.T = geo.T; a.dm.ntiles = geo.ntiles; a.dm.bounded = 0; a.dm.B = npts;
    a.pp = dv.pp; a.pp.lo = a.pp.hi = nullptr;
    a.npts = npts; a.nvec = nvec; a.ld = (long)ld; a.gn = gauss_newton ? 1 : 0;
    a.rm_ld = hd.emode == 5 ? dv.g5.LY : hd.L;              // (the streaming kernel pads its observation rows)
    a.c = 2.0 * rf_scale * hd.cfe;
    a.X = x_d; a.pp.Pfull = p_d; a.V = v_d; a.HV = hv_d; a.part = part_d;
    return h->rt_hvp.hvp(a, geo.lds_bytes, h->stream);
}

int va_hess_vec(va_handle h, const double *XP, const double *P, const double *V, int32_t npts, int32_t nvec, int64_t ld,
                double rf_scale, int32_t gauss_newton, int32_t tile_rows, double *HV)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!XP || !V || !HV) return fail(VA_EINVAL, "XP / V / HV must not be NULL");
    if (npts < 1 || nvec < 1) return fail(VA_EINVAL, "npts and nvec must be at least 1 (npts=%d nvec=%d)", npts, nvec);
    TRY(hvp_refusals(h, "va_hess_vec"));
    const Dims &hd = h->dv.dm;
    const int64_t n_var = (int64_t)hd.ND + hd.NPest;
    if (ld < n_var) return fail(VA_EINVAL, "ld < n_var (%lld < %lld)", (long long)ld, (long long)n_var);
    if (hd.NPt > 0 && !P) return fail(VA_EINVAL, "P must not be NULL (the model has %d parameter(s))", hd.NPt);
    if (tile_rows < 0) return fail(VA_EINVAL, "tile_rows %d", tile_rows);
    HvpGeo geo;
    if (!plan_hvp(hd.D, hd.N, hd.disc, hd.NPt, npts, nvec, tile_rows, geo)) {
        if (hd.D > geo.maxD && geo.maxD > 0)
            return fail(VA_EUNSUPPORTED, "va_hess_vec: D=%d: %s (at most D=%d with this discretisation)", hd.D, geo.why, geo.maxD);
        return fail(tile_rows > 0 ? VA_EINVAL : VA_EUNSUPPORTED, "va_hess_vec: %s (tile_rows=%d, at most %d)", geo.why, tile_rows, geo.Tmax);
    }
    HIPCHK(hipSetDevice(h->device));
    // one allocation: [X | P | V | HV | partial parameter rows]
    const size_t nx = (size_t)npts * ld, np = (size_t)npts * hd.NPt, nv = (size_t)npts * nvec * ld,
                 npart = (size_t)npts * nvec * geo.ntiles * hd.NPt;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (nx + np + 2 * nv + npart + 1)));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *x_d = buf, *p_d = x_d + nx, *v_d = p_d + np, *hv_d = v_d + nv, *part_d = hv_d + nv;
    HIPCHK(hipMemcpyAsync(x_d, XP, sizeof(double) * nx, hipMemcpyHostToDevice, h->stream));
    if (np) HIPCHK(hipMemcpyAsync(p_d, P, sizeof(double) * np, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(v_d, V, sizeof(double) * nv, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(hv_d, 0, sizeof(double) * nv, h->stream));      // (the padding between n_var and ld)
    const hipError_t e = hvp_on_device(h, geo, x_d, p_d, v_d, hv_d, part_d, npts, nvec, ld, rf_scale, gauss_newton);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);       // (the uploads read the caller's arrays)
        return fail(VA_EHIP, "k_hvp launch: %s", hipGetErrorString(e));
    }
    HIPCHK(hipMemcpyAsync(HV, hv_d, sizeof(double) * nv, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// Selected inverse and log-determinant of npts block-tridiagonal arrow matrices given by their blocks (va_selinv.h), on the
// handle's device and stream, on buffers of its own.  Any handle serves: the blocks are the caller's.
int va_blocktri_selinv(va_handle h, int32_t npts, int32_t K, int32_t W, int32_t NPe, const double *Dk, const double *Bk,
                       const double *Pk, const double *Hpp, double *Skk, double *Snk, double *Spk, double *Spp, double *logdet,
                       int32_t *status)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (npts < 1 || K < 1 || W < 1 || NPe < 0) return fail(VA_EINVAL, "bad sizes (npts=%d K=%d W=%d NPe=%d)", npts, K, W, NPe);
    if (!Dk || (K > 1 && !Bk) || (NPe > 0 && (!Pk || !Hpp)) || !logdet || !status)
        return fail(VA_EINVAL, "Dk, Bk (K > 1), Pk and Hpp (NPe > 0), logdet and status must not be NULL");
    SelinvArgs a;
    if (!plan_selinv(W, K, NPe, npts, a.g)) return fail(VA_EUNSUPPORTED, "va_blocktri_selinv: W=%d NPe=%d: %s", W, NPe, a.g.why);
    HIPCHK(hipSetDevice(h->device));
    const size_t ww = (size_t)W * W, pw = (size_t)NPe * W;
    const size_t nd = npts * K * ww, nb = npts * (K - 1) * ww, np = npts * K * pw, nh = (size_t)npts * NPe * NPe;
    const size_t nws = (size_t)npts * a.g.ws_doubles;
    // one allocation: [D | B | P | Hpp | Skk | Snk | Spk | Spp | logdet | workspace | status]
    const size_t tot = 2 * (nd + nb + np + nh) + npts + nws;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (tot + 1) + sizeof(int) * npts));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *d_d = buf, *b_d = d_d + nd, *p_d = b_d + nb, *h_d = p_d + np, *skk_d = h_d + nh, *snk_d = skk_d + nd,
           *spk_d = snk_d + nb, *spp_d = spk_d + np, *ld_d = spp_d + nh, *ws_d = ld_d + npts;
    int *st_d = (int *)(ws_d + nws + 1);
    HIPCHK(hipMemcpyAsync(d_d, Dk, sizeof(double) * nd, hipMemcpyHostToDevice, h->stream));
    if (nb) HIPCHK(hipMemcpyAsync(b_d, Bk, sizeof(double) * nb, hipMemcpyHostToDevice, h->stream));
    if (np) HIPCHK(hipMemcpyAsync(p_d, Pk, sizeof(double) * np, hipMemcpyHostToDevice, h->stream));
    if (nh) HIPCHK(hipMemcpyAsync(h_d, Hpp, sizeof(double) * nh, hipMemcpyHostToDevice, h->stream));
    a.Dk = d_d; a.Bk = b_d; a.Pk = p_d; a.Hpp = h_d;
    a.Skk = Skk ? skk_d : nullptr; a.Snk = Snk ? snk_d : nullptr; a.Spk = Spk ? spk_d : nullptr; a.Spp = Spp ? spp_d : nullptr;
    a.logdet = ld_d; a.status = st_d; a.ws = ws_d; a.npts = npts;
    const hipError_t e = launch_selinv(a, h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);       // (the uploads read the caller's arrays)
        return fail(VA_EHIP, "k_selinv launch: %s", hipGetErrorString(e));
    }
    if (Skk) HIPCHK(hipMemcpyAsync(Skk, skk_d, sizeof(double) * nd, hipMemcpyDeviceToHost, h->stream));
    if (Snk && nb) HIPCHK(hipMemcpyAsync(Snk, snk_d, sizeof(double) * nb, hipMemcpyDeviceToHost, h->stream));
    if (Spk && np) HIPCHK(hipMemcpyAsync(Spk, spk_d, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
    if (Spp && nh) HIPCHK(hipMemcpyAsync(Spp, spp_d, sizeof(double) * nh, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(logdet, ld_d, sizeof(double) * npts, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(status, st_d, sizeof(int) * npts, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return VA_OK;
}

// Laplace approximation at npts points: the coloured directions, k_hvp, k_hblocks, k_selinv and k_laplace_unpack per chunk of
// points, each point with its own rf_scale (consecutive points of equal rf_scale share a k_hvp launch).  Like va_hess_vec it
// ignores bounds and leaves the resident paths, seed states and captured graphs alone.
int va_laplace(va_handle h, const double *XP, const double *P, int32_t npts, int64_t ld, const double *rf_scale,
               int32_t gauss_newton, int32_t chunk_pts, double *var_x, double *cov_xx, double *cov_px, double *cov_pp,
               double *logdet, int32_t *status)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (!XP || !rf_scale || !var_x || !logdet || !status) return fail(VA_EINVAL, "XP / rf_scale / var_x / logdet / status must not be NULL");
    if (npts < 1 || chunk_pts < 0) return fail(VA_EINVAL, "npts must be at least 1 and chunk_pts at least 0 (npts=%d chunk_pts=%d)", npts, chunk_pts);
    TRY(hvp_refusals(h, "va_laplace"));
    const Dims &hd = h->dv.dm;
    const int64_t n_var = (int64_t)hd.ND + hd.NPest;
    if (ld < n_var) return fail(VA_EINVAL, "ld < n_var (%lld < %lld)", (long long)ld, (long long)n_var);
    if (hd.NPt > 0 && !P) return fail(VA_EINVAL, "P must not be NULL (the model has %d parameter(s))", hd.NPt);
    HblocksGeo hg;
    hg.N = hd.N; hg.D = hd.D; hg.hb = hd.disc == DISC_SH ? 2 : 1; hg.NPe = hd.NPest; hg.ld = (long)ld;
    const int W = hblocks_W(hg), K = hblocks_K(hg), NPe = hd.NPest, nvec = hblocks_nvec(hg);
    SelinvGeo sg;
    if (hd.D > SELINV_MAX_W || !plan_selinv(W, K, NPe, npts, sg))
        return fail(VA_EUNSUPPORTED, "va_laplace: D=%d (blocks of %d time row(s): W=%d) NPest=%d: %s", hd.D, hg.hb, W, NPe,
                    hd.D > SELINV_MAX_W ? "block wider than 64 (D <= 64, or D <= 32 with SimpsonHermite)" : sg.why);
    HvpGeo geo;
    if (!plan_hvp(hd.D, hd.N, hd.disc, hd.NPt, 1, nvec, 0, geo)) return fail(VA_EUNSUPPORTED, "va_laplace: D=%d: %s", hd.D, geo.why);
    const size_t per = laplace_point_doubles(hg, sg, hd.NPt, geo.ntiles);
    const long fit = laplace_chunk_points(per, npts);
    if (chunk_pts > 0 ? (size_t)chunk_pts * per * sizeof(double) > LAPLACE_WORKSPACE_BYTES : fit < 1)
        return fail(VA_EINVAL, "va_laplace: a chunk of %d point(s) takes %.1f MiB of device workspace (%zu B per point), the limit is %zu MiB",
                    chunk_pts > 0 ? chunk_pts : 1, (chunk_pts > 0 ? chunk_pts : 1) * (double)per * 8.0 / 1048576.0, per * sizeof(double),
                    LAPLACE_WORKSPACE_BYTES >> 20);
    const int C = (int)(chunk_pts > 0 ? (chunk_pts < npts ? chunk_pts : npts) : fit);
    HIPCHK(hipSetDevice(h->device));
    const size_t ww = (size_t)W * W, pw = (size_t)NPe * W, ND = (size_t)hd.N * hd.D;
    const size_t nx = (size_t)C * ld, np = (size_t)C * hd.NPt, nv = (size_t)C * nvec * ld, npart = (size_t)C * nvec * geo.ntiles * (hd.NPt > 0 ? hd.NPt : 1),
                 nd = C * K * ww, nb = C * (K - 1) * ww, npk = C * K * pw, nh = (size_t)C * NPe * NPe, nws = (size_t)C * sg.ws_doubles,
                 nvar = C * ND, nxx = C * ND * hd.D, npx = C * NPe * ND;
    // one allocation: [X | P | V | HV | partial parameter rows | D | B | P_k | Hpp | workspace | Skk | Spk | Spp | logdet |
    //                  var_x | cov_xx | cov_px | status]
    const size_t tot = nx + np + 2 * nv + npart + nd + nb + npk + nh + nws + nd + npk + nh + C + nvar + nxx + npx;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, sizeof(double) * (tot + 1) + sizeof(int) * C));
    struct Free { double *q; ~Free() { (void)hipFree(q); } } guard{buf};
    double *x_d = buf, *p_d = x_d + nx, *v_d = p_d + np, *hv_d = v_d + nv, *part_d = hv_d + nv, *d_d = part_d + npart, *b_d = d_d + nd,
           *pk_d = b_d + nb, *h_d = pk_d + npk, *ws_d = h_d + nh, *skk_d = ws_d + nws, *spk_d = skk_d + nd, *spp_d = spk_d + npk,
           *ld_d = spp_d + nh, *var_d = ld_d + C, *xx_d = var_d + nvar, *px_d = xx_d + nxx;
    int *st_d = (int *)(px_d + npx + 1);
    hipError_t e = launch_hcolour(hg, v_d, C, h->stream);                 // (the same directions for every chunk)
    if (e != hipSuccess) return fail(VA_EHIP, "k_hcolour launch: %s", hipGetErrorString(e));
    for (int p0 = 0; p0 < npts; p0 += C) {
        const int n = npts - p0 < C ? npts - p0 : C;
        HIPCHK(hipMemcpyAsync(x_d, XP + (size_t)p0 * ld, sizeof(double) * n * ld, hipMemcpyHostToDevice, h->stream));
        if (hd.NPt) HIPCHK(hipMemcpyAsync(p_d, P + (size_t)p0 * hd.NPt, sizeof(double) * n * hd.NPt, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemsetAsync(hv_d, 0, sizeof(double) * (size_t)n * nvec * ld, h->stream));      // (the padding between n_var and ld)
        for (int q0 = 0; q0 < n;) {                                       // runs of one rf_scale
            int q1 = q0 + 1;
            while (q1 < n && rf_scale[p0 + q1] == rf_scale[p0 + q0]) ++q1;
            e = hvp_on_device(h, geo, x_d + (size_t)q0 * ld, p_d + (size_t)q0 * hd.NPt, v_d, hv_d + (size_t)q0 * nvec * ld,
                              part_d + (size_t)q0 * nvec * geo.ntiles * hd.NPt, q1 - q0, nvec, ld, rf_scale[p0 + q0], gauss_newton);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(h->stream);
                return fail(VA_EHIP, "k_hvp launch: %s", hipGetErrorString(e));
            }
            q0 = q1;
        }
        HblocksArgs ba;
        ba.h = hg; ba.HV = hv_d; ba.Dk = d_d; ba.Bk = b_d; ba.Pk = pk_d; ba.Hpp = h_d; ba.npts = n;
        SelinvArgs sa;
        sa.g = sg; sa.g.grid = n;
        sa.Dk = d_d; sa.Bk = b_d; sa.Pk = pk_d; sa.Hpp = h_d; sa.Skk = skk_d; sa.Snk = nullptr; sa.Spk = spk_d; sa.Spp = spp_d;
        sa.logdet = ld_d; sa.status = st_d; sa.ws = ws_d; sa.npts = n;
        UnpackArgs ua;
        ua.h = hg; ua.Skk = skk_d; ua.Spk = spk_d; ua.var_x = var_d; ua.cov_xx = cov_xx ? xx_d : nullptr; ua.cov_px = cov_px ? px_d : nullptr;
        ua.npts = n;
        if ((e = launch_hblocks(ba, h->stream)) != hipSuccess || (e = launch_selinv(sa, h->stream)) != hipSuccess
            || (e = launch_laplace_unpack(ua, h->stream)) != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);
            return fail(VA_EHIP, "k_hblocks / k_selinv / k_laplace_unpack launch: %s", hipGetErrorString(e));
        }
        HIPCHK(hipMemcpyAsync(var_x + (size_t)p0 * ND, var_d, sizeof(double) * n * ND, hipMemcpyDeviceToHost, h->stream));
        if (cov_xx) HIPCHK(hipMemcpyAsync(cov_xx + (size_t)p0 * ND * hd.D, xx_d, sizeof(double) * n * ND * hd.D, hipMemcpyDeviceToHost, h->stream));
        if (cov_px && NPe) HIPCHK(hipMemcpyAsync(cov_px + (size_t)p0 * NPe * ND, px_d, sizeof(double) * n * NPe * ND, hipMemcpyDeviceToHost, h->stream));
        if (cov_pp && NPe) HIPCHK(hipMemcpyAsync(cov_pp + (size_t)p0 * NPe * NPe, spp_d, sizeof(double) * n * NPe * NPe, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(logdet + p0, ld_d, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(status + p0, st_d, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));      // (the next chunk reuses the buffers; pageable destinations)
    }
    HIPCHK(hipGetLastError());
    return VA_OK;
}

int va_get_minpath(va_handle h, int32_t seed, int32_t beta_idx, double *out)
{
    if (!h || !out) return fail(VA_EINVAL, "null argument");
    const Dev &dv = h->dv;
    if (!dv.minpaths) return fail(VA_ESTATE, "problem was created with keep_paths=0");
    if (seed < 0 || seed >= dv.dm.B || beta_idx < 0 || beta_idx >= h->last_nbeta)
        return fail(VA_EINVAL, "seed/beta index out of range");
    HIPCHK(hipSetDevice(h->device));
    const size_t wide = dv.dm.ND + dv.dm.NP;
    HIPCHK(hipMemcpyAsync(out, dv.minpaths + ((size_t)seed * dv.max_beta + beta_idx) * wide,
                          sizeof(double) * wide, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return VA_OK;
}

namespace {
// The graph of `chunk` S1 evaluations va_eval_timed replays, built (or kept) OUTSIDE any timed region.  A host thread
// issues launches ~3.7 us apart, which would be the number measured for any kernel shorter than that (the kernel
// boundary is the same either way: MI355X_MICROARCH.md, "boundary: eager = hipGraph").  The kernels take the device
// image by value, so the graph is keyed on the bytes of h->dv / h->nn as run_eval(EPI_FINALIZE) leaves them.
int timed_chunk_of(int iters) { return iters < 250 ? iters : 250; }

bool timed_graph_current(va_handle h, int chunk)
{
    return h->timed_gexec && h->timed_chunk == chunk && h->tune_graph &&
           memcmp(&h->timed_dv, &h->dv, sizeof(Dev)) == 0 && memcmp(&h->timed_nn, &h->nn, sizeof(NnetDev)) == 0;
}

void timed_graph_drop(va_handle h)
{
    if (h->timed_gexec) { (void)hipGraphExecDestroy(h->timed_gexec); h->timed_gexec = nullptr; }
}

int timed_prepare(va_handle h, double rf_scale, int iters)
{
    Dev &dv = h->dv;
    if (h->timed_armed_rf != rf_scale) {
        launch_init_states(dv, PH_START, rf_scale, h->stream);
        h->timed_armed_rf = rf_scale;
    }
    if (!h->tune_graph || iters < 8) { timed_graph_drop(h); return VA_OK; }
    const int chunk = timed_chunk_of(iters);
    // (the fields run_eval writes, as it will leave them: the comparison below must not see a stale line-search launch)
    h->dv.lsrun = 0; h->dv.s1_rf = h->timed_armed_rf;
    h->dv.epi = (h->is_nnet ? !h->nn.small : !h->fold) ? EPI_NONE : EPI_FINALIZE;
    if (timed_graph_current(h, chunk)) return VA_OK;
    timed_graph_drop(h);
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        for (int i = 0; i < chunk; ++i) run_eval(h, EPI_FINALIZE);
        if (hipStreamEndCapture(h->stream, &g) != hipSuccess || !g ||
            hipGraphInstantiate(&h->timed_gexec, g, nullptr, nullptr, 0) != hipSuccess) h->timed_gexec = nullptr;
        if (g) (void)hipGraphDestroy(g);
    }
    if (!h->timed_gexec) { (void)hipGetLastError(); return VA_OK; }      // plain launches then
    h->timed_chunk = chunk;
    memcpy(&h->timed_dv, &h->dv, sizeof(Dev)); memcpy(&h->timed_nn, &h->nn, sizeof(NnetDev));
    (void)hipGraphUpload(h->timed_gexec, h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    return VA_OK;
}
}  // namespace

int va_eval_timed_prepare(va_handle h, double rf_scale, int32_t iters)
{
    if (!h || iters < 1 || !(rf_scale >= 0.0)) return fail(VA_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    return timed_prepare(h, rf_scale, iters);
}

int va_eval_timed(va_handle h, double rf_scale, int32_t iters, float *elapsed_ms)
{
    if (!h || !elapsed_ms || iters < 1 || !(rf_scale >= 0.0)) return fail(VA_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    Dev &dv = h->dv;
    // Each launch forms A, me, fe and the full gradient.  After va_eval_timed_prepare(h, rf_scale, iters) nothing
    // below but the launches themselves is issued: the seeds are armed and the chunk's graph is instantiated and
    // uploaded; without it (or after anything changed the handle) the same preparation happens here first.
    int rc = timed_prepare(h, rf_scale, iters);
    if (rc) return rc;
    const int chunk = timed_chunk_of(iters);
    hipGraphExec_t gexec = (iters >= 8 && timed_graph_current(h, chunk)) ? h->timed_gexec : nullptr;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    int done = 0;
    if (gexec)
        for (; done + chunk <= iters; done += chunk) HIPCHK(hipGraphLaunch(gexec, h->stream));
    for (; done < iters; ++done) run_eval(h, EPI_FINALIZE);
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    {
        // (polled: a blocking wait hands the thread to the kernel's scheduler, and its wake-up would be part of
        // whatever wall clock the caller keeps around this call)
        hipError_t q;
        while ((q = hipEventQuery(h->ev1)) == hipErrorNotReady) {}
        if (q != hipSuccess) return fail(VA_EHIP, "hipEventQuery: %s", hipGetErrorString(q));
    }
    HIPCHK(hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
    HIPCHK(hipGetLastError());
    h->n_eval_launch += iters; h->n_seed_evals += (int64_t)iters * dv.dm.B;
    h->n_seed_evals_direct += (int64_t)iters * dv.dm.B;
    return VA_OK;
}

int va_problem_tune(va_handle h, int32_t what, int32_t value)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    timed_graph_drop(h);      // (captured with the old settings)
    switch (what) {
    case VA_TUNE_FOLD:
        if (h->is_nnet) return fail(VA_EUNSUPPORTED, "the network action chooses its tail by the net's size");
        h->fold = value != 0; break;
    case VA_TUNE_GRAD_SC1: h->dv.gaux = value != 0 ? 1 : 0; break;
    case VA_TUNE_PRIO: break;       // (retired with the kernel's priority branches: accepted, nothing to set)
    case VA_TUNE_WIDE: {
        // 0: 4-wave workgroups; 1: the planner's width; 2, 3: that many row groups per workgroup, if the kernel has them
        if (h->is_nnet || h->dv.dm.emode != 4) {
            if (value > 1) return fail(VA_EUNSUPPORTED, "only the wave-private kernel k_eval4 has wide workgroups");
            break;
        }
        if (value < 0 || value > 3) return fail(VA_EINVAL, "wide = %d: 0, 1 (the planner's choice), 2 or 3 row groups per workgroup", value);
        HIPCHK(hipSetDevice(h->device));
        const int was = h->dv.wg4;
        set_eval4_groups(h->dv, value == 0 ? 1 : (value == 1 ? h->wg4_plan : value));
        EvalOp op{true, nullptr, hipSuccess};
        if (eval_lds_bytes(h->dv) > LDS_OPTIN_BYTES) op.err = hipErrorInvalidValue;
        else h->rt.eval(h->dv, op);         // (the wider kernel's own opt-in to its LDS; refuses a width the run length has no kernel for)
        if (op.err != hipSuccess) {
            set_eval4_groups(h->dv, was);
            (void)hipGetLastError();
            return fail(VA_EUNSUPPORTED, "k_eval4 at runs of %d rows has no workgroup of %d row groups (registers or LDS)", h->dv.dm.maxr, value);
        }
        break;
    }
    case VA_TUNE_GRAPH: h->tune_graph = value != 0; break;
    case VA_TUNE_NNET_FUSED:
        if (!h->is_nnet || !h->nn.Wf) return fail(VA_ESTATE, "not a network handle whose layers fit the fused kernel");
        // value 1: fused; value 2 + t: fused, the first workgroups' starts spread over t microseconds (measurement)
        h->nn.fused = value != 0 ? 1 : 0;
        h->nn.fb_stagger = value >= 2 ? (value - 2) * 100 : h->nn.fb_stagger; break;
    case VA_TUNE_PERSIST: h->tune_persist = value != 0; break;
    case VA_TUNE_PERSIST_ROWS: {
        if (!h->persist) return fail(VA_ESTATE, "the handle does not run the persistent kernel");
        int G = 0, T = 0;
        const Dims &dm = h->dv.dm;
        if (!persist_geometry(dm.N, dm.D, dm.L, dm.NP, dm.NPest, dm.m, dm.disc, PZ_LDS_BYTES, h->pz_maxG, value, &G, &T))
            return fail(VA_EINVAL, "%d rows per workgroup: not an admissible slice (>= 2 rows everywhere, even for SimpsonHermite, "
                                   "at most %d workgroups per seed, LDS)", value, h->pz_maxG);
        h->pz_G = G; h->pz_T = T;
        break;
    }
    default: return fail(VA_EINVAL, "unknown tuning knob %d", what);
    }
    return VA_OK;
}

// ---------------------------------------------------------------- the job's one collective (RCCL)
namespace {

typedef struct ncclComm *ncclComm_t;
struct NcclId { char internal[VA_COMM_ID_BYTES]; };
struct Rccl {
    void *dl = nullptr;
    int (*GetUniqueId)(NcclId *) = nullptr;
    int (*CommInitRank)(ncclComm_t *, int, NcclId, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, ncclComm_t, hipStream_t) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
std::mutex g_rccl_mutex;

int rccl_load()
{
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.dl) return VA_OK;
    void *dl = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!dl) dl = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!dl) return fail(VA_EUNSUPPORTED, "librccl.so not found: %s", dlerror());
    Rccl r;
    r.GetUniqueId = (int (*)(NcclId *))dlsym(dl, "ncclGetUniqueId");
    r.CommInitRank = (int (*)(ncclComm_t *, int, NcclId, int))dlsym(dl, "ncclCommInitRank");
    r.AllGather = (int (*)(const void *, void *, size_t, int, ncclComm_t, hipStream_t))dlsym(dl, "ncclAllGather");
    r.CommDestroy = (int (*)(ncclComm_t))dlsym(dl, "ncclCommDestroy");
    r.GetErrorString = (const char *(*)(int))dlsym(dl, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy || !r.GetErrorString)
        return fail(VA_EUNSUPPORTED, "librccl.so lacks an expected symbol");
    r.dl = dl;
    g_rccl = r;
    return VA_OK;
}

// [seed][step] rows of (A, me, fe, p_est..., status) in one buffer: what a rank contributes
__global__ void k_pack_results(const Dev dv, int nbeta, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int w = 4 + dv.dm.NPest;
    if (i >= dv.dm.B * nbeta) return;
    const int b = i / nbeta, k = i - b * nbeta;
    double *o = out + (size_t)i * w;
    const double *a = dv.ame + ((size_t)b * dv.max_beta + k) * 3;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
    for (int j = 0; j < dv.dm.NPest; ++j) o[3 + j] = dv.pest[((size_t)b * dv.max_beta + k) * dv.dm.NPest + j];
    o[3 + dv.dm.NPest] = (double)dv.status[(size_t)b * dv.max_beta + k];
}

}  // namespace

struct va_comm_s {
    ncclComm_t comm = nullptr;
    int world = 1, rank = 0, device = 0;
};

int va_comm_unique_id(char id[VA_COMM_ID_BYTES])
{
    if (!id) return fail(VA_EINVAL, "id is NULL");
    int rc = rccl_load();
    if (rc) return rc;
    NcclId nid;
    const int e = g_rccl.GetUniqueId(&nid);
    if (e) return fail(VA_EHIP, "ncclGetUniqueId: %s", g_rccl.GetErrorString(e));
    memcpy(id, nid.internal, VA_COMM_ID_BYTES);
    return VA_OK;
}

int va_comm_create(const char id[VA_COMM_ID_BYTES], int32_t world, int32_t rank, int32_t device, va_comm *out)
{
    if (!id || !out || world < 1 || rank < 0 || rank >= world) return fail(VA_EINVAL, "bad argument");
    *out = nullptr;
    int rc = rccl_load();
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    NcclId nid;
    memcpy(nid.internal, id, VA_COMM_ID_BYTES);
    va_comm c = new va_comm_s();
    c->world = world; c->rank = rank; c->device = device;
    const int e = g_rccl.CommInitRank(&c->comm, world, nid, rank);
    if (e) { delete c; return fail(VA_EHIP, "ncclCommInitRank: %s", g_rccl.GetErrorString(e)); }
    *out = c;
    return VA_OK;
}

void va_comm_destroy(va_comm c)
{
    if (!c) return;
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    delete c;
}

int va_gather_results(va_handle h, va_comm c, int32_t nbeta, double *table, int32_t *status)
{
    if (!h || !c || !table) return fail(VA_EINVAL, "null argument");
    const Dev &dv = h->dv;
    if (nbeta < 1 || nbeta > dv.max_beta) return fail(VA_EINVAL, "nbeta=%d outside [1, max_beta=%d]", nbeta, dv.max_beta);
    if (c->device != h->device) return fail(VA_EINVAL, "communicator lives on device %d, the problem on %d", c->device, h->device);
    HIPCHK(hipSetDevice(h->device));
    const int B = dv.dm.B, w = 4 + dv.dm.NPest;
    const size_t mine = (size_t)B * nbeta * w;
    double *send = nullptr, *recv = nullptr;
    HIPCHK(hipMalloc((void **)&send, sizeof(double) * mine));
    hipError_t e1 = hipMalloc((void **)&recv, sizeof(double) * mine * c->world);
    if (e1 != hipSuccess) { (void)hipFree(send); return fail(VA_ENOMEM, "hipMalloc: %s", hipGetErrorString(e1)); }
    hipLaunchKernelGGL(k_pack_results, dim3((B * nbeta + 255) / 256), dim3(256), 0, h->stream, dv, nbeta, send);
    const int e = g_rccl.AllGather(send, recv, mine, /* ncclFloat64 */ 8, c->comm, h->stream);      // the single collective
    std::vector<double> host(mine * c->world);
    hipError_t e2 = e ? hipSuccess : hipMemcpyAsync(host.data(), recv, sizeof(double) * host.size(), hipMemcpyDeviceToHost, h->stream);
    hipError_t e3 = hipStreamSynchronize(h->stream);
    (void)hipFree(send); (void)hipFree(recv);
    if (e) return fail(VA_EHIP, "ncclAllGather: %s", g_rccl.GetErrorString(e));
    if (e2 != hipSuccess || e3 != hipSuccess) return fail(VA_EHIP, "gather copy: %s", hipGetErrorString(e2 != hipSuccess ? e2 : e3));
    const size_t rows = (size_t)c->world * B * nbeta;
    for (size_t i = 0; i < rows; ++i) {
        memcpy(table + i * (w - 1), host.data() + i * w, sizeof(double) * (w - 1));
        if (status) status[i] = (int32_t)host[i * w + w - 1];
    }
    return VA_OK;
}

int va_lbfgs_timed(va_handle h, int32_t iters, float *ms_update, float *ms_direction)
{
    if (!h || !ms_update || !ms_direction || iters < 1) return fail(VA_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    Dev &dv = h->dv;
    // (a bounded handle's third launch is k_lbfgsb_dir, whose cost depends on the active set and the breakpoints
    // crossed: it has no "steady state" to arm -- profile it inside a real bounded ladder instead)
    if (dv.dm.bounded) return fail(VA_EUNSUPPORTED, "va_lbfgs_timed times k_direction; a bounded handle runs k_lbfgsb_dir");
    dv.sticky = 1;
    h->timed_armed_rf = -1.0;
    auto dir = [&]() { launch_direction(dv, h->stream); };
    launch_arm_full_history(dv, h->stream);
    launch_update(dv, h->stream); dir();           // warm-up
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < iters; ++i) launch_update(dv, h->stream);
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(ms_update, h->ev0, h->ev1));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < iters; ++i) dir();
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(ms_direction, h->ev0, h->ev1));
    dv.sticky = 0;
    launch_init_states(dv, PH_IDLE, 1.0, h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return VA_OK;
}

int va_eval_ls_timed(va_handle h, double rf_scale, int32_t iters, float *ms_eval)
{
    if (!h || !ms_eval || iters < 1) return fail(VA_EINVAL, "bad argument");
    if (h->is_nnet) return fail(VA_EUNSUPPORTED, "ODE problems only");
    HIPCHK(hipSetDevice(h->device));
    Dev &dv = h->dv;
    float both = 0.f, arm = 0.f;
    h->timed_armed_rf = -1.0;
    for (int pass = 0; pass < 2; ++pass) {
        launch_arm_ls(dv, rf_scale, h->stream);
        if (pass == 0) run_eval(h, EPI_LS);                                  // warm-up
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        for (int i = 0; i < iters; ++i) {
            launch_arm_ls(dv, rf_scale, h->stream);
            if (pass == 0) run_eval(h, EPI_LS);
        }
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipEventSynchronize(h->ev1));
        HIPCHK(hipEventElapsedTime(pass == 0 ? &both : &arm, h->ev0, h->ev1));
    }
    *ms_eval = both - arm;
    launch_init_states(dv, PH_IDLE, 1.0, h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return VA_OK;
}

int va_read_eval_outputs(va_handle h, double *A, double *me, double *fe, double *grad, int64_t ldg)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    const Dev &dv = h->dv;
    if (grad && ldg < dv.dm.ND + dv.dm.NPest) return fail(VA_EINVAL, "ldg < n_var");
    HIPCHK(hipSetDevice(h->device));
    const size_t nb = sizeof(double) * dv.dm.B;
    if (A) HIPCHK(hipMemcpyAsync(A, dv.outA, nb, hipMemcpyDeviceToHost, h->stream));
    if (me) HIPCHK(hipMemcpyAsync(me, dv.outme, nb, hipMemcpyDeviceToHost, h->stream));
    if (fe) HIPCHK(hipMemcpyAsync(fe, dv.outfe, nb, hipMemcpyDeviceToHost, h->stream));
    int rc;
    if (grad && (rc = copy_out(h, dv.gt, grad, ldg, VA_MEM_HOST))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return VA_OK;
}

int va_debug_read_partials(va_handle h, double *out, int64_t n)
{
    if (!h || !out || n < 0) return fail(VA_EINVAL, "bad argument");
    const Dev &dv = h->dv;
    const int64_t have = (int64_t)dv.dm.B * dv.dm.nchunks * dv.ups;
    if (n > have) return fail(VA_EINVAL, "n=%lld > %lld partials", (long long)n, (long long)have);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out, dv.upp, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return VA_OK;
}

int va_debug_read_persist(va_handle h, double *out, int64_t n)
{
    if (!h || !out || n < 0) return fail(VA_EINVAL, "bad argument");
    if (!h->dv.pz.stamps) return fail(VA_ESTATE, "the handle has no persistent-kernel buffers");
    if (n > PZ_NSTAMP) return fail(VA_EINVAL, "n > %d", PZ_NSTAMP);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out, h->dv.pz.stamps, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return VA_OK;
}

int va_get_counters(va_handle h, int64_t *eval_launches, int64_t *seed_evals, int64_t *cycles)
{
    if (!h) return fail(VA_EINVAL, "null handle");
    if (eval_launches) *eval_launches = h->n_eval_launch;
    if (seed_evals) *seed_evals = h->n_seed_evals;
    if (cycles) *cycles = h->n_cycles;
    return VA_OK;
}

}  // extern "C"
