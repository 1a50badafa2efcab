// rbsensor_probes.hip -- value-by-value probes of the per-pixel likelihood's device code.  TEST BUILD ONLY: rbsensor_capi.hip
// includes this file under RBS_TEST_HOOKS (librbsensor_mi355x_hooks.so, `make hooks`); the release library has none of it.
//
// Under __HIP_DEVICE_COMPILE__ rbs_math.h takes branches that no host build compiles (the Horner literals of exp_nonpos, the
// hex-coded constants and the classf test of log_f32, the reciprocal expansions div_f32 / rcp_f64, ocml exp / sqrt in
// frame_terms, the LDS copy of the tables), and the F32 pixel model exists on the device only.  Each probe runs ONE of those
// inline functions -- the function the raster kernels call, nothing copied -- over a host array, one thread per element, and
// hands every value back: tests/test_gpu_pixel_math.py compares them one by one.
//
// rbs_test_filter does the same for the particle filter's kernels (rbsensor_tracker.hip): it builds an rbt::TrackerDev from host
// arrays, launches a caller-chosen order of the frame's steps through the launch_* helpers rbs_tracker_submit itself uses
// (rbs_tracker_api.h: no kernel body and no launch geometry is restated here), and hands every array back:
// tests/test_gpu_filter_kernels.py.  rbs_test_posterior is the same for the posterior report's kernels (rbsensor_posterior.hip,
// launch_posterior): tests/test_gpu_tracker_posterior.py.
//
// rbs_test_find_* do the same for the object finder's kernels (rbsensor_find.hip), one entry point per launch helper
// (rbf::launch_*, the ones rbs_find_run itself calls): tests/test_gpu_finder_kernels.py.  Every output array there is IN and
// OUT and `tail` elements (rows) longer than the kernel may write: the caller fills it with a sentinel, the probe copies it to
// the device before the launch and back after it, so what the kernel left alone -- the tail included -- is seen.
// rbs_test_findfg_* are the same for step 1b's four launch helpers: tests/test_gpu_find_foreground_kernels.py.
// rbs_test_findr_* are the same for step 6b's launch helpers: tests/test_gpu_find_refinement_kernels.py.
// rbs_test_findc_evidence is the gate's evidence kernel alone, over a sensor's geometry: tests/test_gpu_find_gate_kernels.py.
// rbs_test_peer_scratch launches nothing: it hands back the scratch arrays the last rbs_peer_resample call on a handle left
// behind (rbsensor_peers.hip's per-tile cumulative weights, maxima and totals): tests/test_gpu_peer_kernels.py.
//
// rbs_test_prep does the same for the rectangles kernel (rbsensor_kernels.hip prep_particles): it builds a DevParams from host
// arrays -- no sensor handle, no mesh: the rectangle reads the vertices only -- and launches rbs_prep_kernel,
// rbs_prep_deltas_kernel or rbs_frame_prep_kernel through launch_prep, the helper enqueue_loglikes itself calls:
// tests/test_gpu_prep_kernels.py.
//
// Entry points (rbs_test_*): host arrays in, host arrays out, synchronous on the current device.  Null pointers and n < 0 (or
// n > kProbeMax) are RBS_ERR_INVALID_ARGUMENT, n == 0 is RBS_OK and touches nothing, a HIP failure is RBS_ERR_HIP.
namespace rbs {
namespace probe {

constexpr int64_t kProbeMax = int64_t(1) << 26;   // elements per call (the largest buffer, [n][4] doubles, is then 2 GB)
constexpr int kProbeTabErfc = rbsm::kErfcIntervals * rbsm::kErfcCoefs, kProbeTabLog = rbsm::kLogIntervals * 2;
static_assert(kMathTabDoubles == kProbeTabErfc + kProbeTabLog, "the probes' LDS copy is the raster kernel's");

__device__ inline size_t probe_index() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }

// The tables as the raster kernel's evaluation sees them.  LDS: the block's copy, filled by the raster kernel's own two loops
// (blocks of kBlock threads) and handed out as `tab` and `tab + ne`, as MathTabs is built there; else the constant tables.
// Every thread of the block calls this (it ends in a barrier).
template <bool LDS>
__device__ inline MathTabs probe_tabs(double* tab)
{
    if (!LDS) return MathTabs{rbsm::kErfcTab, rbsm::kLogTab, nullptr};
    constexpr int ne = kProbeTabErfc, nl = kProbeTabLog;
    for (int i = threadIdx.x; i < ne; i += kBlock) tab[i] = rbsm::kErfcTab[i];
    for (int i = threadIdx.x; i < nl; i += kBlock) tab[ne + i] = rbsm::kLogTab[i];
    __syncthreads();
    return MathTabs{tab, tab + ne, nullptr};
}

__global__ void __launch_bounds__(kBlock) exp_nonpos_kernel(const double* __restrict__ x, double* __restrict__ out, size_t n)
{
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::exp_nonpos(x[i], rbsm::kExpPoly);
}

template <bool LDS>
__global__ void __launch_bounds__(kBlock) erfc_pos_kernel(const double* __restrict__ z, double* __restrict__ out, size_t n)
{
    __shared__ alignas(16) double tab[kProbeTabErfc + kProbeTabLog];
    const MathTabs M = probe_tabs<LDS>(tab);
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::erfc_pos(z[i], M.erfc);
}

template <bool LDS>
__global__ void __launch_bounds__(kBlock) log_f32_kernel(const float* __restrict__ x, double* __restrict__ out, size_t n)
{
    __shared__ alignas(16) double tab[kProbeTabErfc + kProbeTabLog];
    const MathTabs M = probe_tabs<LDS>(tab);
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::log_f32(x[i], M.logt);
}

__global__ void __launch_bounds__(kBlock) div_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, size_t n)
{
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::div_f32(a[i], b[i]);
}

__global__ void __launch_bounds__(kBlock) rcp_f64_kernel(const double* __restrict__ x, double* __restrict__ out, size_t n)
{
    const size_t i = probe_index();
    if (i < n) out[i] = rbsm::rcp_f64(x[i]);
}

// The F64 pixel term as the raster kernel's batch evaluates it: pixel_loglik<false> on the aux entry frame_aux_kernel stored
// (P.aux, pixel i), the tables in LDS.
__global__ void __launch_bounds__(kBlock) pixel_f64_kernel(const DevParams P, const float* __restrict__ depth, const float* __restrict__ prior,
                                                           double* __restrict__ term, float* __restrict__ post, size_t n)
{
    __shared__ alignas(16) double tab[kProbeTabErfc + kProbeTabLog];
    const MathTabs M = probe_tabs<true>(tab);
    const size_t i = probe_index();
    if (i < n) {
        float q;
        term[i] = pixel_loglik<false>(P, M, (int)i, depth[i], prior[i], q);
        post[i] = q;
    }
}

__global__ void __launch_bounds__(kBlock) pixel_f32_kernel(const DevParams P, const float* __restrict__ obs, const float* __restrict__ depth,
                                                           const float* __restrict__ prior, double* __restrict__ term, float* __restrict__ post, size_t n)
{
    const size_t i = probe_index();
    if (i < n) {
        float q;
        term[i] = pixel_loglik_f32(P, depth[i], prior[i], obs[i], q);
        post[i] = q;
    }
}

// Device buffers of one call: freed on every way out.
struct Buffers {
    static constexpr int kMax = 32;
    void* p[kMax] = {};
    int k = 0;
    hipError_t err = hipSuccess;
    template <class T> T* make(size_t count, const T* from = nullptr)
    {
        void* d = nullptr;
        if (err == hipSuccess && k >= kMax) err = hipErrorOutOfMemory;
        if (err == hipSuccess) err = hipMalloc(&d, sizeof(T) * count);
        if (err != hipSuccess) return nullptr;
        p[k++] = d;
        if (from) err = hipMemcpy(d, from, sizeof(T) * count, hipMemcpyHostToDevice);
        return static_cast<T*>(d);
    }
    template <class T> void fetch(T* to, const T* d, size_t count)
    {
        if (err == hipSuccess) err = hipMemcpy(to, d, sizeof(T) * count, hipMemcpyDeviceToHost);
    }
    // after a launch: its launch error, then the kernel's own
    void ran()
    {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    int32_t status() const { return err == hipSuccess ? RBS_OK : RBS_ERR_HIP; }
    ~Buffers() { for (int i = 0; i < k; ++i) (void)hipFree(p[i]); }
};

inline dim3 probe_grid(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
inline bool probe_refused(int64_t n) { return n < 0 || n > kProbeMax; }

// the model parameters the pixel terms read, as rbs_create derives them
inline DevParams probe_params(double tw, double ms, double sf, double lam)
{
    DevParams P{};
    P.tw = tw; P.ms = ms; P.sf = sf; P.lambda = lam;
    P.cv0 = (1.0 - tw) / std::sqrt(M_PI);
    return P;
}

}  // namespace probe
}  // namespace rbs

// ---------------------------------------------------------------------------- the particle filter's kernels
// One call's arrays.  Every array is copied to the device before the first step and back after the last one, under the name
// it has THEN (RBS_TEST_STEP_SWAP exchanges an array with its gather target, as rbs_tracker_submit does after a sampling
// block), so the caller sees everything the kernels wrote and, by the values it put there, everything they left alone.
// normals [parts][n][6] and uniforms [parts][n] may be null: the device generator then draws them from (seed, frame).
struct rbs_test_filter_io {
    int32_t n, parts;
    double sigma[6];
    double vf, max_kl;
    uint64_t seed, frame;
    double* part_old; double* part_new; double* part_old2; double* part_new2;   // [n][parts * 12]
    double* noise; double* noise2;                                                // [n][parts][6]
    double* logw; double* ll; double* ll2; double* ll_new; double* cdf;          // [n]
    int32_t* idx; int32_t* idx2; int32_t* parents;                               // [n]
    double* deflt;                                                                // [parts * 12]
    double* mean;                                                                 // [parts * 12 + parts * 9]
    double* poses;                                                                // [n][parts][12]
    int32_t* flag;                                                                // [2]
    const double* normals; const double* uniforms;
    double* host_state;                                                           // [parts * 12]: publish_result's pinned target, in and out
    int32_t* host_flags;                                                          // [3]
};
enum {
    RBS_TEST_STEP_PROPAGATE = 0,        // b, recentre
    RBS_TEST_STEP_WEIGHTS = 1,          // updated
    RBS_TEST_STEP_RESAMPLE_GATHER = 2,  // b
    RBS_TEST_STEP_GATHER = 3,
    RBS_TEST_STEP_FILTER_TAIL = 4,      // b, updated
    RBS_TEST_STEP_FILTER_STEP = 5,      // b, updated, last
    RBS_TEST_STEP_MEAN = 6,
    RBS_TEST_STEP_RECENTRE = 7,         // part_new, in place
    RBS_TEST_STEP_SWAP = 8,             // no launch: swap_gathered
    RBS_TEST_STEP_COUNT = 9
};
struct rbs_test_filter_step { int32_t code, b, updated, last, recentre; };

extern "C" {

int32_t rbs_test_exp_nonpos(const double* x, double* out, int64_t n)
{
    namespace pr = rbs::probe;
    if (!x || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const double* dx = B.make<double>(n, x);
    double* dout = B.make<double>(n);
    if (B.err == hipSuccess) { hipLaunchKernelGGL(pr::exp_nonpos_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dx, dout, (size_t)n); B.ran(); }
    B.fetch(out, dout, n);
    return B.status();
}

int32_t rbs_test_erfc_pos(const double* z, double* out, int64_t n, int32_t lds_tables)
{
    namespace pr = rbs::probe;
    if (!z || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const double* dz = B.make<double>(n, z);
    double* dout = B.make<double>(n);
    if (B.err == hipSuccess) {
        if (lds_tables) hipLaunchKernelGGL(pr::erfc_pos_kernel<true>, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dz, dout, (size_t)n);
        else hipLaunchKernelGGL(pr::erfc_pos_kernel<false>, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dz, dout, (size_t)n);
        B.ran();
    }
    B.fetch(out, dout, n);
    return B.status();
}

int32_t rbs_test_log_f32(const float* x, double* out, int64_t n, int32_t lds_tables)
{
    namespace pr = rbs::probe;
    if (!x || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* dx = B.make<float>(n, x);
    double* dout = B.make<double>(n);
    if (B.err == hipSuccess) {
        if (lds_tables) hipLaunchKernelGGL(pr::log_f32_kernel<true>, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dx, dout, (size_t)n);
        else hipLaunchKernelGGL(pr::log_f32_kernel<false>, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dx, dout, (size_t)n);
        B.ran();
    }
    B.fetch(out, dout, n);
    return B.status();
}

int32_t rbs_test_div_f32(const float* a, const float* b, float* out, int64_t n)
{
    namespace pr = rbs::probe;
    if (!a || !b || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* da = B.make<float>(n, a);
    const float* db = B.make<float>(n, b);
    float* dout = B.make<float>(n);
    if (B.err == hipSuccess) { hipLaunchKernelGGL(pr::div_f32_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, da, db, dout, (size_t)n); B.ran(); }
    B.fetch(out, dout, n);
    return B.status();
}

int32_t rbs_test_rcp_f64(const double* x, double* out, int64_t n)
{
    namespace pr = rbs::probe;
    if (!x || !out || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const double* dx = B.make<double>(n, x);
    double* dout = B.make<double>(n);
    if (B.err == hipSuccess) { hipLaunchKernelGGL(pr::rcp_f64_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dx, dout, (size_t)n); B.ran(); }
    B.fetch(out, dout, n);
    return B.status();
}

// out4: [n][4], the aux entries {1/(sqrt2 sigma), k, o, e_o} as frame_aux_kernel (frame_aux_pixel) stores them
int32_t rbs_test_frame_terms(const float* obs, int64_t n, double tw, double ms, double sf, double lam, double* out4)
{
    namespace pr = rbs::probe;
    if (!obs || !out4 || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* dobs = B.make<float>(n, obs);
    double* daux = B.make<double>(4 * (size_t)n);
    if (B.err == hipSuccess) {
        hipLaunchKernelGGL(rbs::frame_aux_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dobs, daux, (float*)nullptr, (int)n, tw, ms, sf, lam,
                           (float*)nullptr);
        B.ran();
    }
    B.fetch(out4, daux, 4 * (size_t)n);
    return B.status();
}

// term[n], posterior[n] of (observation, rendered depth, prior)[n] in likelihood precision F64: frame_aux_kernel, then
// pixel_loglik<false> on the stored entries
int32_t rbs_test_pixel_f64(const float* obs, const float* depth, const float* prior, int64_t n, double tw, double ms, double sf, double lam,
                           double* term, float* posterior)
{
    namespace pr = rbs::probe;
    if (!obs || !depth || !prior || !term || !posterior || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* dobs = B.make<float>(n, obs);
    const float* ddepth = B.make<float>(n, depth);
    const float* dprior = B.make<float>(n, prior);
    double* daux = B.make<double>(4 * (size_t)n);
    double* dterm = B.make<double>(n);
    float* dpost = B.make<float>(n);
    if (B.err == hipSuccess) {
        DevParams P = pr::probe_params(tw, ms, sf, lam);
        P.npx = (int)n;
        P.aux = daux;
        hipLaunchKernelGGL(rbs::frame_aux_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, dobs, daux, (float*)nullptr, (int)n, tw, ms, sf, lam,
                           (float*)nullptr);
        hipLaunchKernelGGL(pr::pixel_f64_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, P, ddepth, dprior, dterm, dpost, (size_t)n);
        B.ran();
    }
    B.fetch(term, dterm, n);
    B.fetch(posterior, dpost, n);
    return B.status();
}

// ... in likelihood precision F32: pixel_loglik_f32
int32_t rbs_test_pixel_f32(const float* obs, const float* depth, const float* prior, int64_t n, double tw, double ms, double sf, double lam,
                           double* term, float* posterior)
{
    namespace pr = rbs::probe;
    if (!obs || !depth || !prior || !term || !posterior || pr::probe_refused(n)) return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    pr::Buffers B;
    const float* dobs = B.make<float>(n, obs);
    const float* ddepth = B.make<float>(n, depth);
    const float* dprior = B.make<float>(n, prior);
    double* dterm = B.make<double>(n);
    float* dpost = B.make<float>(n);
    if (B.err == hipSuccess) {
        const DevParams P = pr::probe_params(tw, ms, sf, lam);
        hipLaunchKernelGGL(pr::pixel_f32_kernel, pr::probe_grid(n), dim3(rbs::kBlock), 0, 0, P, dobs, ddepth, dprior, dterm, dpost, (size_t)n);
        B.ran();
    }
    B.fetch(term, dterm, n);
    B.fetch(posterior, dpost, n);
    return B.status();
}

}  // extern "C"

extern "C" int32_t rbs_test_filter(const rbs_test_filter_io* io, const rbs_test_filter_step* steps, int32_t n_steps)
{
    namespace pr = rbs::probe;
    constexpr int kMaxSteps = 16;
    if (!io || !steps || n_steps < 0 || n_steps > kMaxSteps) return RBS_ERR_INVALID_ARGUMENT;
    if (io->n < 1 || io->n > rbt::kRedBlocks * rbt::kChunk || io->parts < 1 || io->parts > rbs::kMaxBodies) return RBS_ERR_INVALID_ARGUMENT;
    if (!io->part_old || !io->part_new || !io->part_old2 || !io->part_new2 || !io->noise || !io->noise2 || !io->logw || !io->ll || !io->ll2 ||
        !io->ll_new || !io->cdf || !io->idx || !io->idx2 || !io->parents || !io->deflt || !io->mean || !io->poses || !io->flag ||
        !io->host_state || !io->host_flags)
        return RBS_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < n_steps; ++k)
        if (steps[k].code < 0 || steps[k].code >= RBS_TEST_STEP_COUNT || steps[k].b < 0 || steps[k].b >= io->parts) return RBS_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)io->n, parts = (size_t)io->parts, D = parts * rbt::kBody, P6 = parts * 6;
    pr::Buffers B;
    rbt::TrackerDev T{};
    T.n = io->n; T.parts = io->parts; T.D = (int)D;
    for (int k = 0; k < 6; ++k) T.sigma[k] = io->sigma[k];
    T.vf = io->vf; T.max_kl = io->max_kl; T.seed = io->seed; T.frame = io->frame;
    T.part_old = B.make<double>(n * D, io->part_old);    T.part_new = B.make<double>(n * D, io->part_new);
    T.part_old2 = B.make<double>(n * D, io->part_old2);  T.part_new2 = B.make<double>(n * D, io->part_new2);
    T.noise = B.make<double>(n * P6, io->noise);         T.noise2 = B.make<double>(n * P6, io->noise2);
    T.logw = B.make<double>(n, io->logw);                T.ll = B.make<double>(n, io->ll);
    T.ll2 = B.make<double>(n, io->ll2);                  T.ll_new = B.make<double>(n, io->ll_new);
    T.cdf = B.make<double>(n, io->cdf);
    T.idx = B.make<int>(n, io->idx);                     T.idx2 = B.make<int>(n, io->idx2);
    T.parents = B.make<int>(n, io->parents);
    T.deflt = B.make<double>(D, io->deflt);              T.mean = B.make<double>(D + parts * 9, io->mean);
    T.poses = B.make<double>(n * parts * 12, io->poses); T.flag = B.make<int>(2, io->flag);
    T.red = B.make<double>((size_t)rbt::kRedBlocks * (3 + D));
    if (io->normals) T.normals = B.make<double>(n * P6, io->normals);
    if (io->uniforms) T.uniforms = B.make<double>(n * parts, io->uniforms);
    // publish_result's target: pinned host memory of this call's own, as rbs_tracker_create maps the tracker's
    double* h_state = nullptr;
    int* h_flags = nullptr;
    if (B.err == hipSuccess) B.err = hipHostMalloc(&h_state, sizeof(double) * D, hipHostMallocDefault);
    if (B.err == hipSuccess) B.err = hipHostMalloc(&h_flags, sizeof(int) * 4, hipHostMallocDefault);
    if (B.err == hipSuccess) {
        std::memcpy(h_state, io->host_state, sizeof(double) * D);
        for (int k = 0; k < 3; ++k) h_flags[k] = io->host_flags[k];
        B.err = hipHostGetDevicePointer(reinterpret_cast<void**>(&T.host_state), h_state, 0);
    }
    if (B.err == hipSuccess) B.err = hipHostGetDevicePointer(reinterpret_cast<void**>(&T.host_flags), h_flags, 0);
    if (B.err == hipSuccess) B.err = hipMemset(T.red, 0, sizeof(double) * (size_t)rbt::kRedBlocks * (3 + D));
    if (B.err == hipSuccess) {
        hipStream_t s = nullptr;
        for (int k = 0; k < n_steps; ++k) {
            const rbs_test_filter_step& q = steps[k];
            switch (q.code) {
            case RBS_TEST_STEP_PROPAGATE: launch_propagate(T, q.b, q.recentre ? 1 : 0, s); break;
            case RBS_TEST_STEP_WEIGHTS: launch_weights(T, q.updated ? 1 : 0, s); break;
            case RBS_TEST_STEP_RESAMPLE_GATHER: launch_resample_gather(T, q.b, s); break;
            case RBS_TEST_STEP_GATHER: launch_gather(T, s); break;
            case RBS_TEST_STEP_FILTER_TAIL: launch_filter_tail(T, q.b, q.updated ? 1 : 0, s); break;
            case RBS_TEST_STEP_FILTER_STEP: launch_filter_step(T, q.b, q.updated ? 1 : 0, q.last ? 1 : 0, s); break;
            case RBS_TEST_STEP_MEAN: launch_mean(T, s); break;
            case RBS_TEST_STEP_RECENTRE: launch_recentre(T, T.part_new, s); break;
            default: swap_gathered(T); break;
            }
        }
        B.ran();
    }
    B.fetch(io->part_old, T.part_old, n * D);    B.fetch(io->part_new, T.part_new, n * D);
    B.fetch(io->part_old2, T.part_old2, n * D);  B.fetch(io->part_new2, T.part_new2, n * D);
    B.fetch(io->noise, T.noise, n * P6);         B.fetch(io->noise2, T.noise2, n * P6);
    B.fetch(io->logw, T.logw, n);                B.fetch(io->ll, T.ll, n);
    B.fetch(io->ll2, T.ll2, n);                  B.fetch(io->cdf, T.cdf, n);
    B.fetch(io->idx, T.idx, n);                  B.fetch(io->idx2, T.idx2, n);
    B.fetch(io->parents, T.parents, n);
    B.fetch(io->deflt, T.deflt, D);              B.fetch(io->mean, T.mean, D + parts * 9);
    B.fetch(io->poses, T.poses, n * parts * 12); B.fetch(io->flag, T.flag, 2);
    if (B.err == hipSuccess) {
        std::memcpy(io->host_state, h_state, sizeof(double) * D);
        for (int k = 0; k < 3; ++k) io->host_flags[k] = h_flags[k];
    }
    if (h_state) (void)hipHostFree(h_state);
    if (h_flags) (void)hipHostFree(h_flags);
    return B.status();
}

// ---------------------------------------------------------------------------- the posterior report's kernels
// Planted particles [n][parts * 12], log-weights [n], slot map [n], the mean rows and transposed mean rotations
// [parts * 12 + parts * 9] recentre_body reads, and the re-centred flag, through launch_posterior -- the helper
// rbs_tracker_submit itself calls: out [1 + D + D D] := ess, mean, cov; out_i [4] := n, survivors, resampled, frame + 1.
// particles, logw and idx come back as the device holds them afterwards (the kernels must have left them alone).
extern "C" int32_t rbs_test_posterior(int32_t n, int32_t parts, double* particles, double* logw, int32_t* idx, const double* mean,
                                      int32_t recentred, int32_t resampled, uint64_t frame, double* out, int32_t* out_i)
{
    namespace pr = rbs::probe;
    if (n < 1 || n > rbt::kRedBlocks * rbt::kChunk || parts < 1 || parts > rbs::kMaxBodies) return RBS_ERR_INVALID_ARGUMENT;
    if (!particles || !logw || !idx || !mean || !out || !out_i) return RBS_ERR_INVALID_ARGUMENT;
    const size_t N = (size_t)n, D = (size_t)parts * rbt::kBody, nd = rbt::post_out_doubles((int)D);
    const int flags[2] = {resampled ? 1 : 0, 0};
    pr::Buffers B;
    rbt::TrackerDev T{};
    T.n = n; T.parts = parts; T.D = (int)D; T.frame = frame;
    double* part = B.make<double>(N * D, particles);
    T.logw = B.make<double>(N, logw);
    T.idx = B.make<int>(N, idx);
    T.mean = B.make<double>(D + (size_t)parts * 9, mean);
    T.flag = B.make<int>(2, flags);
    rbt::PostDev P{};
    P.pose = B.make<double>(N * parts * 6);
    P.e = B.make<double>(N);
    P.partials = B.make<double>(rbt::post_partials_doubles(n, (int)D));
    P.bitmap = B.make<unsigned>((N + 31) / 32);
    P.out = B.make<double>(nd);
    P.out_i = B.make<int>(4);
    if (B.err == hipSuccess) B.err = hipMemset(P.out, 0xff, sizeof(double) * nd);
    if (B.err == hipSuccess) B.err = hipMemset(P.bitmap, 0xff, sizeof(unsigned) * ((N + 31) / 32));   // (the kernels clear it themselves)
    if (B.err == hipSuccess) {
        launch_posterior(T, P, part, recentred ? 1 : 0, nullptr);
        B.ran();
    }
    B.fetch(out, P.out, nd);
    B.fetch(out_i, P.out_i, 4);
    B.fetch(particles, part, N * D);
    B.fetch(logw, T.logw, N);
    B.fetch(idx, T.idx, N);
    return B.status();
}

// ---------------------------------------------------------------------------- the object finder's kernels
extern "C" {

// dst [(rows / f) * (cols / f) + tail]
int32_t rbs_test_find_subsample(const float* src, int32_t rows, int32_t cols, int32_t f, float* dst, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!src || !dst || rows < 0 || cols < 0 || f < 1 || tail < 0 || pr::probe_refused((int64_t)rows * cols) || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    const int cr = rows / f, cc = cols / f;
    if ((int64_t)cr * cc == 0) return RBS_OK;
    const size_t n = (size_t)rows * cols, m = (size_t)cr * cc + (size_t)tail;
    pr::Buffers B;
    const float* dsrc = B.make<float>(n, src);
    float* ddst = B.make<float>(m, dst);
    if (B.err == hipSuccess) { rbf::launch_subsample(nullptr, dsrc, cols, ddst, cr, cc, f); B.ran(); }
    B.fetch(dst, ddst, m);
    return B.status();
}

// cells [ceil(rows / stride) * ceil(cols / stride) + tail], seeds [min(max_seeds, cells) + tail][4], info [2 + tail]
int32_t rbs_test_find_seeds(const float* frame, int32_t rows, int32_t cols, int32_t stride, double dmin, double dmax, int32_t max_seeds,
                            int32_t* cells, double* seeds, int32_t* info, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!frame || !cells || !seeds || !info || rows < 0 || cols < 0 || stride < 1 || max_seeds < 1 || tail < 0 ||
        pr::probe_refused((int64_t)rows * cols) || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if ((int64_t)rows * cols == 0) return RBS_OK;
    const size_t n = (size_t)rows * cols, nc = rbf::seed_cells(rows, cols, stride), ns = std::min<size_t>((size_t)max_seeds, nc);
    pr::Buffers B;
    const float* dframe = B.make<float>(n, frame);
    int* dcells = B.make<int>(nc + (size_t)tail, cells);
    double* dseeds = B.make<double>(4 * (ns + (size_t)tail), seeds);
    int* dinfo = B.make<int>(2 + (size_t)tail, info);
    if (B.err == hipSuccess) { rbf::launch_seeds(nullptr, dframe, rows, cols, stride, dmin, dmax, max_seeds, dcells, dseeds, dinfo); B.ran(); }
    B.fetch(cells, dcells, nc + (size_t)tail);
    B.fetch(seeds, dseeds, 4 * (ns + (size_t)tail));
    B.fetch(info, dinfo, 2 + (size_t)tail);
    return B.status();
}

// idx == NULL: rbs_find_hyp_kernel over hypotheses h0 .. h0 + n - 1; else rbs_find_gather_kernel over idx [n].  Every
// hypothesis must lie in [0, n_seeds * n_rot).  poses [n + tail][12]
int32_t rbs_test_find_hyp(const double* seeds, int32_t n_seeds, int32_t n_rot, double fx, double fy, double cx, double cy, double offset,
                          int64_t h0, const int64_t* idx, int32_t n, double* poses, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!seeds || !poses || n_seeds < 1 || n_rot < 1 || n < 0 || tail < 0 || pr::probe_refused(n) || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    const int64_t H = (int64_t)n_seeds * n_rot;
    if (idx) {
        for (int32_t i = 0; i < n; ++i)
            if (idx[i] < 0 || idx[i] >= H) return RBS_ERR_INVALID_ARGUMENT;
    } else if (h0 < 0 || h0 + n > H) {
        return RBS_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return RBS_OK;
    const size_t m = 12 * ((size_t)n + (size_t)tail);
    pr::Buffers B;
    rbf::HypParams HP;
    HP.seeds = B.make<double>(4 * (size_t)n_seeds, seeds);
    HP.n_rot = n_rot;
    HP.fx = fx; HP.fy = fy; HP.cx = cx; HP.cy = cy;
    HP.offset = offset;
    const long long* didx = idx ? B.make<long long>((size_t)n, reinterpret_cast<const long long*>(idx)) : nullptr;
    double* dposes = B.make<double>(m, poses);
    if (B.err == hipSuccess) {
        if (idx) rbf::launch_gather(nullptr, HP, didx, n, dposes);
        else rbf::launch_hyp(nullptr, HP, (long)h0, n, dposes);
        B.ran();
    }
    B.fetch(poses, dposes, m);
    return B.status();
}

// The best k of (score, idx) [n] (idx may be NULL: positions) through rbf::launch_topk's own loop of passes, its ping-pong
// buffers rbf::topk_items(n, k) + tail items each; tail_s / tail_i [2][tail]: those buffers' tails, in and out.
// out_score / out_idx [k]; *passes (may be NULL) := the launches it took.
int32_t rbs_test_find_topk(const double* score, const int64_t* idx, int64_t n, int32_t k, double* out_score, int64_t* out_idx,
                           double* tail_s, int64_t* tail_i, int64_t tail, int32_t* passes)
{
    namespace pr = rbs::probe;
    if (!score || !out_score || !out_idx || !tail_s || !tail_i || k < 1 || k > rbf::kMaxCandidates || tail < 0 || pr::probe_refused(n) ||
        pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    const size_t cap = rbf::topk_items(n, k), T = (size_t)tail;
    pr::Buffers B;
    const double* dscore = B.make<double>((size_t)n, score);
    const long long* didx = idx ? B.make<long long>((size_t)n, reinterpret_cast<const long long*>(idx)) : nullptr;
    double* tk_s[2] = {B.make<double>(cap + T), B.make<double>(cap + T)};
    long long* tk_i[2] = {B.make<long long>(cap + T), B.make<long long>(cap + T)};
    for (int b = 0; b < 2 && T > 0; ++b) {
        if (B.err == hipSuccess) B.err = hipMemcpy(tk_s[b] + cap, tail_s + b * T, sizeof(double) * T, hipMemcpyHostToDevice);
        if (B.err == hipSuccess) B.err = hipMemcpy(tk_i[b] + cap, tail_i + b * T, sizeof(long long) * T, hipMemcpyHostToDevice);
    }
    const double* rs = nullptr;
    const long long* ri = nullptr;
    if (B.err == hipSuccess) { B.err = rbf::launch_topk(nullptr, dscore, didx, (long)n, k, tk_s, tk_i, &rs, &ri); B.ran(); }
    if (B.err == hipSuccess) {
        B.fetch(out_score, rs, (size_t)k);
        B.fetch(reinterpret_cast<long long*>(out_idx), ri, (size_t)k);
        for (int b = 0; b < 2 && T > 0; ++b) {
            B.fetch(tail_s + b * T, tk_s[b] + cap, T);
            B.fetch(reinterpret_cast<long long*>(tail_i) + b * T, tk_i[b] + cap, T);
        }
        if (passes) {
            int32_t np = 0;
            for (long m = (long)n;;) { const long blocks = (m + rbf::kTopC - 1) / rbf::kTopC; ++np; if (blocks == 1) break; m = blocks * k; }
            *passes = np;
        }
    }
    return B.status();
}

// The suppression and the keep kernel over candidates [n] in order, the thresholds from (nms_translation, nms_angle) as
// rbs_find_create derives them.  kept [64 + tail], count [1 + tail], surv [max_keep + tail][12], surv_score / surv_idx
// [max_keep + tail]
int32_t rbs_test_find_nms(const double* poses, const double* score, const int64_t* idx, int32_t n, double nms_translation, double nms_angle,
                          int32_t max_keep, int32_t* kept, int32_t* count, double* surv, double* surv_score, int64_t* surv_idx, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!poses || !score || !idx || !kept || !count || !surv || !surv_score || !surv_idx || n < 0 || max_keep < 1 ||
        max_keep > rbf::kMaxSurvivors || tail < 0 || pr::probe_refused(n) || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    const size_t T = (size_t)tail, K = (size_t)max_keep + T;
    double t2, trace_min;
    rbf::nms_thresholds(nms_translation, nms_angle, &t2, &trace_min);
    pr::Buffers B;
    const double* dposes = B.make<double>(12 * (size_t)n, poses);
    const double* dscore = B.make<double>((size_t)n, score);
    const long long* didx = B.make<long long>((size_t)n, reinterpret_cast<const long long*>(idx));
    int* dkept = B.make<int>(rbf::kMaxSurvivors + T, kept);
    int* dcount = B.make<int>(1 + T, count);
    double* dsurv = B.make<double>(12 * K, surv);
    double* dsurv_score = B.make<double>(K, surv_score);
    long long* dsurv_idx = B.make<long long>(K, reinterpret_cast<const long long*>(surv_idx));
    if (B.err == hipSuccess) {
        rbf::launch_nms_keep(nullptr, dposes, dscore, didx, n, t2, trace_min, max_keep, dkept, dcount, dsurv, dsurv_score, dsurv_idx);
        B.ran();
    }
    B.fetch(kept, dkept, rbf::kMaxSurvivors + T);
    B.fetch(count, dcount, 1 + T);
    B.fetch(surv, dsurv, 12 * K);
    B.fetch(surv_score, dsurv_score, K);
    B.fetch(reinterpret_cast<long long*>(surv_idx), dsurv_idx, K);
    return B.status();
}

// out [S * children + tail][12]
int32_t rbs_test_find_children(const double* surv, int32_t S, int32_t children, int32_t round, uint64_t seed, double sigma_t, double sigma_a,
                               double* out, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!surv || !out || S < 0 || S > rbf::kMaxSurvivors || children < 1 || children > 4096 || round < 0 || round > 63 || tail < 0 ||
        pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if (S == 0) return RBS_OK;
    const size_t m = 12 * ((size_t)S * children + (size_t)tail);
    pr::Buffers B;
    const double* dsurv = B.make<double>(12 * (size_t)S, surv);
    double* dout = B.make<double>(m, out);
    if (B.err == hipSuccess) { rbf::launch_children(nullptr, dsurv, S, children, round, (unsigned long long)seed, sigma_t, sigma_a, dout); B.ran(); }
    B.fetch(out, dout, m);
    return B.status();
}

// child [S * children][12], child_score [S * children] -> surv [S + tail][12], surv_score [S + tail]
int32_t rbs_test_find_select(const double* child, const double* child_score, int32_t S, int32_t children, double* surv, double* surv_score,
                             int64_t tail)
{
    namespace pr = rbs::probe;
    if (!child || !child_score || !surv || !surv_score || S < 0 || S > rbf::kMaxSurvivors || children < 1 || children > 4096 || tail < 0 ||
        pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if (S == 0) return RBS_OK;
    const size_t nch = (size_t)S * children, K = (size_t)S + (size_t)tail;
    pr::Buffers B;
    const double* dchild = B.make<double>(12 * nch, child);
    const double* dscore = B.make<double>(nch, child_score);
    double* dsurv = B.make<double>(12 * K, surv);
    double* dsurv_score = B.make<double>(K, surv_score);
    if (B.err == hipSuccess) { rbf::launch_select(nullptr, dchild, dscore, S, children, dsurv, dsurv_score); B.ran(); }
    B.fetch(surv, dsurv, 12 * K);
    B.fetch(surv_score, dsurv_score, K);
    return B.status();
}

// surv [S][12], surv_score [S], order [S] (each in 0 .. S - 1) -> out_pose [S + tail][12], out_score [S + tail]
int32_t rbs_test_find_order(const double* surv, const double* surv_score, const int64_t* order, int32_t S, double* out_pose, double* out_score,
                            int64_t tail)
{
    namespace pr = rbs::probe;
    if (!surv || !surv_score || !order || !out_pose || !out_score || S < 0 || S > rbf::kMaxSurvivors || tail < 0 || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    for (int32_t i = 0; i < S; ++i)
        if (order[i] < 0 || order[i] >= S) return RBS_ERR_INVALID_ARGUMENT;
    if (S == 0) return RBS_OK;
    const size_t K = (size_t)S + (size_t)tail;
    pr::Buffers B;
    const double* dsurv = B.make<double>(12 * (size_t)S, surv);
    const double* dscore = B.make<double>((size_t)S, surv_score);
    const long long* dorder = B.make<long long>((size_t)S, reinterpret_cast<const long long*>(order));
    double* dout = B.make<double>(12 * K, out_pose);
    double* dout_score = B.make<double>(K, out_score);
    if (B.err == hipSuccess) { rbf::launch_order(nullptr, dsurv, dscore, dorder, S, dout, dout_score); B.ran(); }
    B.fetch(out_pose, dout, 12 * K);
    B.fetch(out_score, dout_score, K);
    return B.status();
}

// ---- step 1b, the foreground (rbs_findfg_*_kernel): tests/find_fg_probes.py, tests/test_gpu_find_foreground_kernels.py
// planes [trials + tail][4]
int32_t rbs_test_findfg_trials(const float* frame, int32_t rows, int32_t cols, double dmin, double dmax, uint64_t seed, int32_t trials,
                               double* planes, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!frame || !planes || rows < 0 || cols < 0 || trials < 0 || trials > rbf::kFgMaxTrials || tail < 0 ||
        pr::probe_refused((int64_t)rows * cols) || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if ((int64_t)rows * cols == 0 || trials == 0) return RBS_OK;
    const size_t m = 4 * ((size_t)trials + (size_t)tail);
    pr::Buffers B;
    const float* dframe = B.make<float>((size_t)rows * cols, frame);
    double* dplanes = B.make<double>(m, planes);
    const rbf::FgModel M{dmin, dmax, 0.0, 0.0};
    if (B.err == hipSuccess) { rbf::launch_plane_trials(nullptr, dframe, rows, cols, M, (unsigned long long)seed, trials, dplanes); B.ran(); }
    B.fetch(planes, dplanes, m);
    return B.status();
}

// planes [trials][4]; counts [trials + 1 + tail].  trials == 0: the valid pixels alone (planes may be NULL)
int32_t rbs_test_findfg_count(const float* frame, int32_t rows, int32_t cols, double dmin, double dmax, double model_sigma,
                              double sigma_factor, const double* planes, int32_t trials, double ransac_sigmas, int32_t* counts, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!frame || !counts || (trials > 0 && !planes) || rows < 0 || cols < 0 || trials < 0 || trials > rbf::kFgMaxTrials || tail < 0 ||
        pr::probe_refused((int64_t)rows * cols) || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if ((int64_t)rows * cols == 0) return RBS_OK;
    const size_t m = (size_t)trials + 1 + (size_t)tail;
    pr::Buffers B;
    const float* dframe = B.make<float>((size_t)rows * cols, frame);
    const double* dplanes = trials > 0 ? B.make<double>(4 * (size_t)trials, planes) : nullptr;
    int* dcounts = B.make<int>(m, counts);
    const rbf::FgModel M{dmin, dmax, model_sigma, sigma_factor};
    if (B.err == hipSuccess) { rbf::launch_plane_count(nullptr, dframe, rows, cols, M, dplanes, trials, ransac_sigmas, dcounts); B.ran(); }
    B.fetch(counts, dcounts, m);
    return B.status();
}

// planes [trials][4], counts [trials + 1]; rec [8 + tail]
int32_t rbs_test_findfg_best(const double* planes, const int32_t* counts, int32_t trials, double min_inlier_fraction, double* rec, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!planes || !counts || !rec || trials < 0 || trials > rbf::kFgMaxTrials || tail < 0 || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if (trials == 0) return RBS_OK;
    const size_t m = (size_t)rbf::kFgRecord + (size_t)tail;
    pr::Buffers B;
    const double* dplanes = B.make<double>(4 * (size_t)trials, planes);
    const int* dcounts = B.make<int>((size_t)trials + 1, counts);
    double* drec = B.make<double>(m, rec);
    if (B.err == hipSuccess) { rbf::launch_plane_best(nullptr, dplanes, dcounts, trials, min_inlier_fraction, drec); B.ran(); }
    B.fetch(rec, drec, m);
    return B.status();
}

// rec [8]; out [rows * cols + tail]
int32_t rbs_test_findfg_mask(const float* frame, int32_t rows, int32_t cols, double model_sigma, double sigma_factor, const double* rec,
                             double mask_sigmas, float* out, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!frame || !rec || !out || rows < 0 || cols < 0 || tail < 0 || pr::probe_refused((int64_t)rows * cols) || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if ((int64_t)rows * cols == 0) return RBS_OK;
    const size_t n = (size_t)rows * cols, m = n + (size_t)tail;
    pr::Buffers B;
    const float* dframe = B.make<float>(n, frame);
    const double* drec = B.make<double>((size_t)rbf::kFgRecord, rec);
    float* dout = B.make<float>(m, out);
    const rbf::FgModel M{0.0, 0.0, model_sigma, sigma_factor};
    if (B.err == hipSuccess) { rbf::launch_mask(nullptr, dframe, rows, cols, M, drec, mask_sigmas, dout); B.ran(); }
    B.fetch(out, dout, m);
    return B.status();
}

// ---- step 6b, the adaptive refinement (rbs_findr_*_kernel): tests/find_refine_probes.py, tests/test_gpu_find_refinement_kernels.py
// fac == NULL: rbf::launch_refine_init makes the factors of diag(sigma_a^2 x 3, sigma_t^2 x 3) first (cov [S + tail][36] is then
// written too); else fac [S][36] is read.  out [S * children + tail][12], dd [S * children + tail][6]
int32_t rbs_test_findr_children(const double* surv, const double* fac, int32_t S, int32_t children, int32_t round, uint64_t seed,
                                double sigma_a, double sigma_t, double jitter, double* cov, double* out, double* dd, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!surv || !out || !dd || (!fac && !cov) || S < 0 || S > rbf::kMaxSurvivors || children < 1 || children > 4096 || round < 0 ||
        round > 63 || tail < 0 || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if (S == 0) return RBS_OK;
    const size_t nch = (size_t)S * children + (size_t)tail, K = (size_t)S + (size_t)tail;
    pr::Buffers B;
    const double* dsurv = B.make<double>(12 * (size_t)S, surv);
    double* dfac = fac ? B.make<double>(36 * (size_t)S, fac) : B.make<double>(36 * (size_t)S, (const double*)nullptr);
    double* dcov = fac ? nullptr : B.make<double>(36 * K, cov);
    double* dout = B.make<double>(12 * nch, out);
    double* ddd = B.make<double>(6 * nch, dd);
    if (B.err == hipSuccess) {
        if (!fac) rbf::launch_refine_init(nullptr, S, sigma_a, sigma_t, jitter, dcov, dfac);
        rbf::launch_refine_children(nullptr, dsurv, dfac, S, children, round, (unsigned long long)seed, dout, ddd);
        B.ran();
    }
    if (!fac) B.fetch(cov, dcov, 36 * K);
    B.fetch(out, dout, 12 * nch);
    B.fetch(dd, ddd, 6 * nch);
    return B.status();
}

// child_score [S * children], dd [S * children][6], cov [S + tail][36] IN and OUT (updated in place), fac [S + tail][36] OUT
int32_t rbs_test_findr_update(const double* child_score, const double* dd, int32_t S, int32_t children, int32_t elite, double mix,
                              double shrink, double jitter, double* cov, double* fac, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!child_score || !dd || !cov || !fac || S < 0 || S > rbf::kMaxSurvivors || children < 1 || children > 4096 || elite < 1 ||
        elite > rbf::kRefMaxElite || elite > children || tail < 0 || pr::probe_refused(tail))
        return RBS_ERR_INVALID_ARGUMENT;
    if (S == 0) return RBS_OK;
    const size_t nch = (size_t)S * children, K = (size_t)S + (size_t)tail;
    pr::Buffers B;
    const double* dscore = B.make<double>(nch, child_score);
    const double* ddd = B.make<double>(6 * nch, dd);
    double* dcov = B.make<double>(36 * K, cov);
    double* dfac = B.make<double>(36 * K, fac);
    const rbf::RefineRule U{elite, mix, shrink, jitter};
    if (B.err == hipSuccess) { rbf::launch_refine_update(nullptr, dscore, ddd, S, children, U, dcov, dcov, dfac); B.ran(); }
    B.fetch(cov, dcov, 36 * K);
    B.fetch(fac, dfac, 36 * K);
    return B.status();
}

// ---- the gate (rbs_findc_evidence_kernel): tests/test_gpu_find_gate_kernels.py
// The evidence of poses [n][12] against frame [rows * cols] through the one-body sensor h's geometry, alone on the null stream:
// rec [n + tail][10] and cls [n + tail] IN and OUT.  g: the rule (checked as rbs_find_set_gate checks it).
int32_t rbs_test_findc_evidence(rbs_handle* h, const rbs_find_gate* g, const float* frame, const double* poses, int32_t n, int32_t* rec,
                                int32_t* cls, int64_t tail)
{
    namespace pr = rbs::probe;
    if (!h || !g || !frame || !poses || !rec || !cls || n < 0 || tail < 0 || pr::probe_refused(n) || pr::probe_refused(tail) ||
        h->n_bodies != 1 || !h->shards.empty() || h->group || h->peer_world > 1 || gate_check(g))
        return RBS_ERR_INVALID_ARGUMENT;
    if (n == 0) return RBS_OK;
    if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return RBS_ERR_HIP;
    const size_t K = (size_t)n + (size_t)tail;
    pr::Buffers B;
    const float* dframe = B.make<float>((size_t)h->npx, frame);
    const double* dposes = B.make<double>(12 * (size_t)n, poses);
    int* drec = B.make<int>(rbf::kEvFields * K, rec);
    int* dcls = B.make<int>(K, cls);
    if (B.err == hipSuccess) { rbf::launch_evidence(nullptr, h, *g, dframe, dposes, n, drec, dcls); B.ran(); }
    B.fetch(rec, drec, rbf::kEvFields * K);
    B.fetch(cls, dcls, K);
    return B.status();
}

// ---- resampling across processes (rbsensor_peers.hip): tests/peer_probes.py, tests/test_gpu_peer_kernels.py
// What the LAST rbs_peer_resample call on h left in the handle's scratch block, after its stream has drained: cdf [N] (cumulative
// weights within each tile), tile_total [tiles], mine [n] -- and tile_max [tiles] where peer_max_kernel ran (large jobs only), else
// the caller's array is left alone.  Returns 1 / 0 (RBS_OK): tile_max was / was not written; < 0: an error.  Nothing is launched.
int32_t rbs_test_peer_scratch(rbs_handle* h, double* cdf, double* tile_max, double* tile_total, int32_t* mine)
{
    if (!h || !cdf || !tile_max || !tile_total || !mine || h->peer_last.N < 1 || !h->d_peer_scratch) return RBS_ERR_INVALID_ARGUMENT;
    const rbp::PeerPlan& Q = h->peer_last;
    const size_t N = (size_t)Q.N, tiles = (N + rbp::kTile - 1) / rbp::kTile;
    if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->peer_last_stream) != hipSuccess) return RBS_ERR_HIP;
    rbs::probe::Buffers B;   // (none of its own: the fetches and the status)
    B.fetch(cdf, Q.cdf, N);
    B.fetch(tile_total, Q.tile_total, tiles);
    if (h->peer_last_max) B.fetch(tile_max, Q.tile_max, tiles);
    B.fetch(mine, Q.mine, (size_t)Q.n);
    return B.err == hipSuccess ? (h->peer_last_max ? 1 : 0) : RBS_ERR_HIP;
}

}  // extern "C"

// ---------------------------------------------------------------------------- the rectangles kernel
// One call's arrays.  Inputs are const; every output is IN and OUT, `tail` elements (rows) longer than the kernel may write, and
// filled by the caller (sentinels; ctr_this, err and area_sum with the values the call starts from).
//   route 0: poses_in [n][bodies][12] is copied to the device array `poses`
//   route 1: ... to pinned host memory the kernel pulls it from (DevParams::poses_src)
//   route 2: poses_in is [n + 1][bodies][6], the state deltas followed by the default poses, pinned (DevParams::deltas_src)
// frame != null: the frame launch, whose other blocks write aux [rows * cols][4] (null: none) and keep [rows * cols] (null: none).
// groups / strips / area_sum null: not allocated (DevParams::groups / strips / area_sum null).
struct rbs_test_prep_io {
    int32_t rows, cols, n_bodies, n;
    double fx, fy, cx, cy;
    const int32_t* vtx_begin;       // [n_bodies + 1]
    const float* vtx;               // [vtx_begin[n_bodies]][4]
    int32_t rect_align, tile_w, tile_h, tile_px;
    int32_t windowed, slab_px, slots, update;
    const int32_t* win_src;         // [slots][4]
    const int32_t* rebase_box;      // [4] or null
    int32_t route, pad0;
    const double* poses_in;
    const int32_t* indices;         // [n]
    const float* frame;             // [rows * cols] or null
    double tw, ms, sf, lam;
    int64_t tail;
    double* poses;                  // [n * bodies * 12 + tail]
    int32_t* rects;                 // [n + tail][4]
    int32_t* groups;                // [n + tail][sizeof(Groups) / 4] or null
    int32_t* strips;                // [n + tail][sizeof(Strips) / 4] or null
    int32_t* parents;               // [n + tail]
    int32_t* item_range;            // [n + tail][2]
    int32_t* item_particle;         // [n * tiles_ub * (groups ? kMaxGroups : 1) + tail]: as enqueue_loglikes sizes it
    int32_t* ctr_this;              // [2 + tail]
    int32_t* done;                  // [n + tail]
    int32_t* win_used;              // [n + tail][4]
    int32_t* win_dst;               // [n + tail][4]
    int32_t* reg_dst;               // [n + tail][4]
    int32_t* err;                   // [2 + tail]
    uint64_t* area_sum;             // [1] or null
    double* aux;                    // [rows * cols + tail][4] or null
    float* keep;                    // [rows * cols + tail] or null
};

extern "C" {

// {sizeof(Groups), sizeof(Strips), kMaxGroups, kMaxStrips, kPrepPerBlock, kMaxBodies}: what the caller's view of the arrays rests on
int32_t rbs_test_prep_layout(int32_t* out6)
{
    if (!out6) return RBS_ERR_INVALID_ARGUMENT;
    out6[0] = (int32_t)sizeof(rbs::Groups); out6[1] = (int32_t)sizeof(rbs::Strips); out6[2] = rbs::kMaxGroups; out6[3] = rbs::kMaxStrips;
    out6[4] = rbs::kPrepPerBlock; out6[5] = rbs::kMaxBodies;
    return RBS_OK;
}

// tiles_upper_bound(cols, rows, tile_w, min(tile_w * tile_h, tile_px)) as enqueue_loglikes computes it (host only)
int64_t rbs_test_prep_tiles_ub(int32_t cols, int32_t rows, int32_t tile_w, int32_t tile_h, int32_t tile_px)
{
    if (cols < 1 || rows < 1 || tile_w < 16 || tile_h < 1 || tile_px < 1) return -1;
    return (int64_t)tiles_upper_bound(cols, rows, tile_w, std::min(tile_w * tile_h, tile_px));
}

int32_t rbs_test_prep(const rbs_test_prep_io* io)
{
    namespace pr = rbs::probe;
    if (!io) return RBS_ERR_INVALID_ARGUMENT;
    // (columns and rows <= 8 192: Strips::box; whole float4 columns: the strips' cells)
    if (io->rows < 1 || io->rows > 8192 || io->cols < 4 || io->cols > 8192 || (io->cols & 3) || io->n < 1 || io->n > (1 << 16) ||
        io->n_bodies < 1 || io->n_bodies > rbs::kMaxBodies || io->tail < 0 || io->tail > 4096 || io->slots < 0 || io->slab_px < 0)
        return RBS_ERR_INVALID_ARGUMENT;
    if (io->rect_align < 4 || (io->rect_align & (io->rect_align - 1)) || io->tile_w < 16 || (io->tile_w & 15) || io->tile_h < 1 || io->tile_px < 1 ||
        io->tile_w > 8192 || io->tile_h > 8192 || io->route < 0 || io->route > 2 || (io->frame && io->route != 0))
        return RBS_ERR_INVALID_ARGUMENT;
    if (!io->vtx_begin || !io->vtx || !io->poses_in || !io->indices || !io->poses || !io->rects || !io->parents || !io->item_range ||
        !io->item_particle || !io->ctr_this || !io->done || !io->win_used || !io->win_dst || !io->reg_dst || !io->err || (io->slots && !io->win_src) ||
        (io->strips && !io->groups))
        return RBS_ERR_INVALID_ARGUMENT;
    if (io->vtx_begin[0] != 0) return RBS_ERR_INVALID_ARGUMENT;
    for (int b = 0; b < io->n_bodies; ++b)
        if (io->vtx_begin[b + 1] < io->vtx_begin[b]) return RBS_ERR_INVALID_ARGUMENT;
    const size_t nv = (size_t)io->vtx_begin[io->n_bodies];
    if (nv < 1 || pr::probe_refused((int64_t)nv)) return RBS_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)io->n, B_ = (size_t)io->n_bodies, tail = (size_t)io->tail, npx = (size_t)io->rows * io->cols;
    constexpr size_t kG = sizeof(rbs::Groups) / 4, kS = sizeof(rbs::Strips) / 4;
    DevParams P = pr::probe_params(io->tw, io->ms, io->sf, io->lam);
    P.rows = io->rows; P.cols = io->cols; P.npx = (int)npx;
    P.n_bodies = io->n_bodies;
    for (int b = 0; b <= io->n_bodies; ++b) P.vtx_begin[b] = io->vtx_begin[b];
    P.rect_align = io->rect_align; P.tile_w = io->tile_w; P.tile_h = io->tile_h; P.tile_px = io->tile_px;
    P.fx = io->fx; P.fy = io->fy; P.cx = io->cx; P.cy = io->cy;
    P.windowed = io->windowed; P.slab_px = io->slab_px; P.plane_stride = io->slab_px ? io->slab_px : (int)npx; P.slots = io->slots;
    P.n = io->n;
    const size_t tiles_max = tiles_upper_bound(io->cols, io->rows, P.tile_w, std::min(P.tile_w * P.tile_h, P.tile_px));
    const size_t items = n * tiles_max * (io->groups ? rbs::kMaxGroups : 1);   // (enqueue_loglikes: `need`)
    if (pr::probe_refused((int64_t)items)) return RBS_ERR_INVALID_ARGUMENT;
    pr::Buffers B;
    P.vtx = reinterpret_cast<const rbs::floatx4*>(B.make<float>(4 * nv, io->vtx));
    if (io->slots) P.win_src = reinterpret_cast<const int4*>(B.make<int>(4 * (size_t)io->slots, io->win_src));
    if (io->rebase_box) P.rebase_box = reinterpret_cast<const int4*>(B.make<int>(4, io->rebase_box));
    P.indices = B.make<int>(n, io->indices);
    double* dposes = B.make<double>(n * B_ * 12 + tail, io->poses);
    P.poses = dposes;
    // the host-pointer routes: pinned memory of this call's own, as the handle maps its staging buffers
    double* h_src = nullptr;
    const size_t n_src = io->route == 2 ? (n + 1) * B_ * 6 : n * B_ * 12;
    if (io->route == 0) {
        if (B.err == hipSuccess) B.err = hipMemcpy(dposes, io->poses_in, sizeof(double) * n_src, hipMemcpyHostToDevice);
    } else {
        const double* d_src = nullptr;
        if (B.err == hipSuccess) B.err = hipHostMalloc(&h_src, sizeof(double) * n_src, hipHostMallocDefault);
        if (B.err == hipSuccess) {
            std::memcpy(h_src, io->poses_in, sizeof(double) * n_src);
            B.err = hipHostGetDevicePointer(reinterpret_cast<void**>(const_cast<double**>(&d_src)), h_src, 0);
        }
        if (io->route == 1) P.poses_src = d_src; else P.deltas_src = d_src;
    }
    int* drects = B.make<int>(4 * (n + tail), io->rects);
    P.rects = drects;
    int* dgroups = io->groups ? B.make<int>(kG * (n + tail), io->groups) : nullptr;
    int* dstrips = io->strips ? B.make<int>(kS * (n + tail), io->strips) : nullptr;
    P.groups = reinterpret_cast<rbs::Groups*>(dgroups);
    P.strips = reinterpret_cast<rbs::Strips*>(dstrips);
    P.parents = B.make<int>(n + tail, io->parents);
    int* drange = B.make<int>(2 * (n + tail), io->item_range);
    P.item_range = reinterpret_cast<int2*>(drange);
    // (device side only: room behind the tail, so that a particle whose items exceeded the host's bound -- what the test is there
    // to find -- would overwrite the tail's sentinels and nobody else's memory)
    const size_t guard = n * 64;
    P.item_particle = B.make<int>(items + tail + guard);
    if (B.err == hipSuccess) B.err = hipMemcpy(P.item_particle, io->item_particle, sizeof(int) * (items + tail), hipMemcpyHostToDevice);
    P.ctr_this = B.make<int>(2 + tail, io->ctr_this);
    P.done = B.make<int>(n + tail, io->done);
    int* dused = B.make<int>(4 * (n + tail), io->win_used);
    int* dwdst = B.make<int>(4 * (n + tail), io->win_dst);
    int* drdst = B.make<int>(4 * (n + tail), io->reg_dst);
    P.win_used = reinterpret_cast<int4*>(dused); P.win_dst = reinterpret_cast<int4*>(dwdst); P.reg_dst = reinterpret_cast<int4*>(drdst);
    P.err = B.make<int>(2 + tail, io->err);
    unsigned long long* darea = io->area_sum ? B.make<unsigned long long>(1, reinterpret_cast<const unsigned long long*>(io->area_sum)) : nullptr;
    P.area_sum = darea;
    const float* dframe = io->frame ? B.make<float>(npx, io->frame) : nullptr;
    double* daux = io->frame && io->aux ? B.make<double>(4 * (npx + tail), io->aux) : nullptr;
    float* dkeep = io->frame && io->keep ? B.make<float>(npx + tail, io->keep) : nullptr;
    if (B.err == hipSuccess) {
        launch_prep(P, drects, io->update ? 1 : 0, io->route == 2, dframe, daux, nullptr, dkeep, nullptr);
        B.ran();
    }
    B.fetch(io->poses, dposes, n * B_ * 12 + tail);
    B.fetch(io->rects, drects, 4 * (n + tail));
    if (dgroups) B.fetch(io->groups, dgroups, kG * (n + tail));
    if (dstrips) B.fetch(io->strips, dstrips, kS * (n + tail));
    B.fetch(io->parents, P.parents, n + tail);
    B.fetch(io->item_range, drange, 2 * (n + tail));
    B.fetch(io->item_particle, P.item_particle, items + tail);
    B.fetch(io->ctr_this, P.ctr_this, 2 + tail);
    B.fetch(io->done, P.done, n + tail);
    B.fetch(io->win_used, dused, 4 * (n + tail));
    B.fetch(io->win_dst, dwdst, 4 * (n + tail));
    B.fetch(io->reg_dst, drdst, 4 * (n + tail));
    B.fetch(io->err, P.err, 2 + tail);
    if (darea) B.fetch(reinterpret_cast<unsigned long long*>(io->area_sum), darea, 1);
    if (daux) B.fetch(io->aux, daux, 4 * (npx + tail));
    if (dkeep) B.fetch(io->keep, dkeep, npx + tail);
    if (h_src) (void)hipHostFree(h_src);
    return B.status();
}

}  // extern "C"
